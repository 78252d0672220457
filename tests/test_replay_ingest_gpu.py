"""Finished games go from the device history to the replay ring in HIP (gmz_replay_ingest): the ring must hold,
bit for bit, what GameHistory.harvest + replay.slices_from_game + ReplayBuffer.add_arrays put there."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 5
DISCOUNT = 0.997


def _tcfg(H, n_steps, N, per):
    from datou_gomoku_muzero_amd import trainer as T
    return T.TrainConfig(BOARD_SIZE=H, NUM_RES_BLOCKS=1, NUM_UNROLL_STEPS=U, N_STEPS=n_steps, DISCOUNT=DISCOUNT,
                         TRAIN_BUFFER_SIZE=N, ENABLE_PER=per)


def _random_history(G, A, rs):
    """A GameHistory whose every row, recorded or not, holds random data: a read outside a game's rows shows."""
    from datou_gomoku_muzero_amd.worker import GameHistory
    h = GameHistory(G, A, torch.device("cuda"))
    dev = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    h.board.copy_(dev(rs.randint(-1, 2, (2, G, A, A)).astype(np.int8)))
    h.player.copy_(dev(rs.choice([-1, 1], (2, G, A)).astype(np.int8)))
    h.last.copy_(dev(rs.randint(-1, A, (2, G, A)).astype(np.int32)))
    h.pol.copy_(dev(rs.dirichlet(np.full(A, 0.3), (2, G, A))))
    h.val.copy_(dev(rs.uniform(-1, 1, (2, G, A)).astype(np.float32)))
    h.act.copy_(dev(rs.randint(0, A, (2, G, A)).astype(np.int32)))
    return h


def _snapshot(h, games):
    """The snapshot of a move at which ``games`` = {slot: (bank, start row, n_moves, winner, abandoned)} ended and
    every other slot plays on, made by GameHistory.after_play itself."""
    G = h.G
    status = np.full(G, 2, np.int8)
    mc, act = np.zeros(G, np.int32), np.full(G, 3, np.int32)
    bank = np.zeros(G, np.int64)
    for g, (bk, s0, n, winner, abandoned) in games.items():
        status[g], mc[g], bank[g] = winner, s0 + n - 1, bk
        h.start[bk, g] = s0
        if abandoned:
            act[g] = -1
    dev = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    h.bank.copy_(dev(bank))
    mf, mt = dev(np.arange(G, dtype=np.int32)), dev(np.arange(G, dtype=np.int32) + 10)
    return h.after_play(dev(status), dev(mc), dev(act), mf, mt)


def _both_paths(h, sn, rb_host, rb_dev):
    """One snapshot's finished games through the host path into ``rb_host`` and the device path into ``rb_dev``."""
    from datou_gomoku_muzero_amd.replay import slices_from_game
    c = rb_host.cfg
    fin = h.finished(sn)
    done = h.harvest(sn, games=fin)
    for (g, winner, n, mf, mt, boards, players, lasts, pols, vals, acts) in done:
        rb_host.add_arrays(*slices_from_game(boards, players, lasts, pols, vals, acts, winner, c.BOARD_SIZE, c.DISCOUNT,
                                             c.N_STEPS, c.NUM_UNROLL_STEPS))
    got = rb_dev.ingest_history(h, sn, games=fin)
    assert got == [x[:5] for x in done]
    return len(done)


def _assert_rings_equal(a, b):
    torch.cuda.synchronize()
    assert (a.ptr, a.count) == (b.ptr, b.count)
    for name in ("obs", "act", "rew", "pol", "val", "prio"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x, y), "%s differs in %d ring rows" % (
            name, int((x.reshape(a.N, -1) != y.reshape(a.N, -1)).any(1).sum()))


def _rings(H, n_steps, N, per):
    from datou_gomoku_muzero_amd import replay as RP, trainer as T
    out = []
    for _ in range(2):
        rb = RP.ReplayBuffer(_tcfg(H, n_steps, N, per), device="cuda")
        if per:  # the admission priority after an update_priorities: a device scalar
            rb.max_priority = torch.tensor(2.5, dtype=torch.float32, device="cuda")
        if N == 37:  # a full ring whose pointer is about to wrap
            rb.ptr, rb.count = 30, 37
        out.append(rb)
    return out


@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("N", [256, 37])
@pytest.mark.parametrize("n_steps", [3, 10])
def test_kernel_equals_host_path_on_synthetic_games_5x5(n_steps, N, per):
    """A = 25 (less than a wave).  Lengths 1, 2, U, U+1, n_steps, n_steps+1 and A; winners -1, 0, 1; games on bank 1;
    start rows > 0; an abandoned game; two launches, the second through the other job table.  N = 37: the pointer
    wraps and the second launch's games overwrite each other's slices (4+25+7+9 or 11+25+7+9 > 37)."""
    H, A, G = 5, 25, 6
    h = _random_history(G, A, np.random.RandomState(n_steps))
    rb_host, rb_dev = _rings(H, n_steps, N, per)
    first = {0: (0, 0, 1, 1, False), 1: (1, 3, 2, -1, False), 2: (0, 0, U, 0, False), 3: (0, 7, U + 1, -1, False),
             4: (1, 0, n_steps, 1, False), 5: (0, 0, 6, 0, True)}
    assert _both_paths(h, _snapshot(h, first), rb_host, rb_dev) == 5
    _assert_rings_equal(rb_host, rb_dev)
    second = {0: (1, 2, n_steps + 1, -1, False), 1: (0, 0, A, 1, False), 2: (1, 0, 7, 1, False), 3: (1, 2, 9, 0, False)}
    assert _both_paths(h, _snapshot(h, second), rb_host, rb_dev) == 4
    _assert_rings_equal(rb_host, rb_dev)
    assert rb_dev.count == min(N, (37 if N == 37 else 0) + 56 + 2 * n_steps)
    assert float(rb_dev.prio[rb_dev.ptr - 1]) == (2.5 if per else 1.0)


@pytest.mark.parametrize("n_steps,N,per", [(10, 37, True), (3, 512, False)])
def test_kernel_equals_host_path_on_synthetic_games_15x15(n_steps, N, per):
    """A = 225: more than a wave, more than a 128- or 192-thread workgroup and a multiple of neither.  Two games in
    two slots: a full board of 225 moves (longer than the ring at N = 37) and a short one on bank 1 from row 4."""
    H, A, G = 15, 225, 2
    h = _random_history(G, A, np.random.RandomState(15))
    rb_host, rb_dev = _rings(H, n_steps, N, per)
    games = {0: (0, 0, A, -1, False), 1: (1, 4, n_steps + 2, 1, False)}
    assert _both_paths(h, _snapshot(h, games), rb_host, rb_dev) == 2
    _assert_rings_equal(rb_host, rb_dev)


def test_real_engine_games_through_both_paths():
    """SelfPlay at 6x6 (16 simulations, 1 block, 32 games, 40 moves): every snapshot's finished games go through
    harvest + the host path into ring A and through the device path into ring B; the rings are equal bit for bit.
    The ring of 300 slices wraps several times."""
    from datou_gomoku_muzero_amd import loop as LP, weights as W
    from datou_gomoku_muzero_amd.config import GmzConfig
    cfg = GmzConfig(BOARD_SIZE=6, NUM_SIMULATIONS=16, NUM_RES_BLOCKS=1)
    sp = LP.SelfPlay(cfg, 32, W.synthetic_state_dict(cfg, seed=1, with_projection=False), seed=3)
    rb_host, rb_dev = _rings(6, cfg.N_STEPS, 300, True)
    assert (rb_host.cfg.DISCOUNT, rb_host.cfg.NUM_UNROLL_STEPS) == (cfg.DISCOUNT, cfg.NUM_UNROLL_STEPS)
    e, h = sp.eng, sp.hist
    pending, games = None, 0
    for _ in range(40):
        b, p, lm, mc = e.game_state()
        pol, val, act = e.search()
        e.winning_scan(b, p, act, counters=sp.missed)
        h.record(b, p, lm, mc, pol, val, act)
        status = e.play(reset_finished=True)
        sn = h.after_play(status, mc, act, *sp.missed)
        if pending is not None:
            games += _both_paths(h, pending, rb_host, rb_dev)
        pending = sn
    games += _both_paths(h, pending, rb_host, rb_dev)
    assert games > 0, "no game finished in 40 moves"
    _assert_rings_equal(rb_host, rb_dev)
    assert rb_dev.count == 300 and float(rb_dev.pol.sum()) > 0
    sp.close()


@pytest.mark.parametrize("concurrent", [False, True])
def test_c4_loop_with_device_ingest(concurrent):
    """loop.C4Loop(device_ingest=True) at the shapes of test_pipeline_gpu.py's loop tests, time-sliced and with the
    trainer on its own stream: every finished game's slices are in the shard, the trainer steps, the pushes follow
    the steps, and the engine reports no error."""
    from datou_gomoku_muzero_amd import loop as LP, replay as RP, trainer as T
    from datou_gomoku_muzero_amd.config import GmzConfig
    cfg = GmzConfig(BOARD_SIZE=6, NUM_SIMULATIONS=16, NUM_RES_BLOCKS=1)
    tcfg = T.TrainConfig(BOARD_SIZE=6, NUM_RES_BLOCKS=1, PHYSICAL_BATCH_SIZE=16, TRAIN_BUFFER_SIZE=4096, ENABLE_PER=True)
    tr = T.Trainer(tcfg, device="cuda") if concurrent else T.Trainer(tcfg, device="cuda", graph=False)
    sp = LP.SelfPlay(cfg, 32, tr.state_dict_cpu(), seed=3)
    rb = RP.ReplayBuffer(tcfg, device="cuda")
    lp = LP.C4Loop(sp, tr, rb, tcfg, 16, moves_per_iter=2, train_steps_per_iter=1, model_update_interval=2,
                   concurrent=concurrent, device_ingest=True)
    assert lp.device_ingest and lp.concurrent == concurrent and sp.ingest_buffer is rb
    st = lp.run(40)
    torch.cuda.synchronize()
    assert st["games"] > 0 and st["games"] == len(lp.game_lengths) and st["slices"] == sum(lp.game_lengths)
    assert st["slices"] == len(rb) and st["train_steps"] > 0
    assert st["weight_pushes"] == st["train_steps"] // 2 >= 1
    assert torch.isfinite(lp.last_logs).all()
    n = len(rb)
    assert float(rb.prio[:n].min()) > 0 and float(rb.prio[n:].abs().max()) == 0  # admitted slices, and only they
    assert bool((rb.pol[:n, 0].sum(1) > 0.5).all())  # every slice starts at a searched position's policy
    for eng in getattr(sp.eng, "engines", [sp.eng]):
        assert eng.errors() == 0
    sp.close()
