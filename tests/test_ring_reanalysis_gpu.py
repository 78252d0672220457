"""Re-analysis of the games in the device replay ring (reanalysis.RingReanalyser): gmz_replay_positions must decode
ring slices into exactly the positions that were played, gmz_replay_rewrite must leave the ring as
ReplayBuffer.rewrite_games_host leaves it, a whole pass must equal Reanalyser.search_positions followed by the host
rewrite, and the composed loop must run with it in both stream settings.  Every comparison is bit for bit; every ring
is filled with random bytes first, so that a stray write shows."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 5
DISCOUNT = 0.997
RING = ("obs", "act", "rew", "pol", "val", "prio")


def _tcfg(H, n_steps, N):
    from datou_gomoku_muzero_amd import trainer as T
    return T.TrainConfig(BOARD_SIZE=H, NUM_RES_BLOCKS=1, NUM_UNROLL_STEPS=U, N_STEPS=n_steps, DISCOUNT=DISCOUNT,
                         TRAIN_BUFFER_SIZE=N, ENABLE_PER=True)


def _play(rs, H, start, n, winner):
    """A game by random legal moves: ``start`` opening stones (black first), then ``n`` recorded moves; the arrays
    GameHistory.harvest returns, plus the move counts."""
    A = H * H
    assert start + n <= A
    cells = rs.permutation(A)[:start + n]
    board = np.zeros(A, np.int8)
    for i in range(start):
        board[cells[i]] = 1 if i % 2 == 0 else -1
    boards, players, lasts = [], [], []
    last = int(cells[start - 1]) if start else -1
    for i in range(start, start + n):
        p = 1 if i % 2 == 0 else -1
        boards.append(board.copy())
        players.append(p)
        lasts.append(last)
        board[cells[i]] = p
        last = int(cells[i])
    return dict(boards=np.array(boards, np.int8), players=np.array(players, np.int8), lasts=np.array(lasts, np.int32),
                mcs=np.arange(start, start + n, dtype=np.int32), pols=rs.dirichlet(np.full(A, 0.3), n),
                vals=rs.uniform(-1, 1, n).astype(np.float32), acts=cells[start:].astype(np.int32), winner=winner,
                start=start, n=n)


def _random_ring(H, n_steps, N, ptr=0, seed=0):
    """A device ring whose every byte is random (a write outside a game's targets shows), at ``ptr``."""
    from datou_gomoku_muzero_amd import replay as RP, trainer as T
    rb = RP.ReplayBuffer(_tcfg(H, n_steps, N), device="cuda")
    g = torch.Generator().manual_seed(seed)
    rb.obs.copy_(torch.randint(0, 256, rb.obs.shape, dtype=torch.uint8, generator=g))
    rb.act.copy_(torch.randint(-1, H * H, rb.act.shape, dtype=torch.int32, generator=g))
    for t in (rb.rew, rb.pol, rb.val, rb.prio):
        t.copy_(torch.rand(t.shape, generator=g) * 2 - 1)
    if ptr:
        rb.ptr, rb.count = ptr, N
    return rb


def _add(rb, game, pols=None, vals=None):
    from datou_gomoku_muzero_amd.replay import slices_from_game
    c, g = rb.cfg, game
    rb.add_arrays(*slices_from_game(g["boards"], g["players"], g["lasts"], g["pols"] if pols is None else pols,
                                    g["vals"] if vals is None else vals, g["acts"], g["winner"], c.BOARD_SIZE, c.DISCOUNT,
                                    c.N_STEPS, c.NUM_UNROLL_STEPS), game=(g["winner"], g["start"], 0))


def _snap(rb):
    torch.cuda.synchronize()
    return {k: getattr(rb, k).clone() for k in RING}


def _assert_ring(rb, want, what):
    torch.cuda.synchronize()
    for k in RING:
        x, y = getattr(rb, k), want[k] if isinstance(want, dict) else getattr(want, k)
        assert torch.equal(x, y), "%s: %s differs in %d ring rows" % (
            what, k, int((x.reshape(rb.N, -1) != y.reshape(rb.N, -1)).any(1).sum()))


# ---------------------------------------------------------------------------------------------- positions kernel
@pytest.mark.parametrize("H,N,ptr,G,shape", [
    # 5x5, A = 25 (less than a wave).  N = 37 at ptr 30: the first game's slots wrap the ring's end and the last game
    # takes its oldest 9 slices (drop 9), wrapping itself; odd starts (player -1 first); the last game starts from
    # the empty board (no last move); 3 + 20 + 5 + 9 = 37 positions in chunks of 16, 16 and 5 (P < G)
    (5, 37, 30, 16, [(0, 12), (3, 20), (1, 5), (0, 9)]),
    # 15x15, A = 225 (more than a wave, a multiple of neither 64 nor 256): a game longer than the ring (drop 23, its 37
    # slices fill the ring from slot 30 round to 29), from an odd start; one chunk with P = 37 < G = 48
    (15, 37, 30, 48, [(7, 60)]),
    # 15x15, two games, the first from the empty board; 51 positions in chunks of 48 and 3
    (15, 80, 0, 48, [(0, 30), (11, 21)]),
])
def test_positions_kernel_decodes_every_surviving_slice(H, N, ptr, G, shape):
    from datou_gomoku_muzero_amd import replay as RP
    A = H * H
    rs = np.random.RandomState(H + N)
    rb = _random_ring(H, 10, N, ptr)
    games = [_play(rs, H, start, n, (-1, 0, 1)[i % 3]) for i, (start, n) in enumerate(shape)]
    for g in games:
        _add(rb, g)
    if N == 37:
        assert any(e.drop > 0 for e in rb.games) and any(e.slot + e.kept > N for e in rb.games)
    assert any(g["start"] % 2 == 1 for g in games)  # a first position with player -1
    if len(games) > 1:  # a surviving first position with no last move
        assert any(games[e.seq]["start"] == 0 and e.drop == 0 for e in rb.games)
    want = [np.concatenate([games[e.seq][k][e.drop:] for e in rb.games]) for k in ("boards", "players", "lasts", "mcs")]
    rows = RP.ring_rows(rb.games, N)
    P = len(rows)
    assert P == sum(e.kept for e in rb.games) == len(want[0]) and P % G != 0
    pin = torch.from_numpy(rows).pin_memory()
    dev = pin.cuda()
    got = [[], [], [], []]
    for lo in range(0, P, G):
        n = min(G, P - lo)
        out = (torch.full((G, A), 7, dtype=torch.int8, device="cuda"), torch.full((G,), 7, dtype=torch.int8, device="cuda"),
               torch.full((G,), 7, dtype=torch.int32, device="cuda"), torch.full((G,), 7, dtype=torch.int32, device="cuda"))
        rb.decode_positions(pin[lo:lo + n], dev[lo:lo + n], n, *out)
        torch.cuda.synchronize()
        for k, t in enumerate(out):
            got[k].append(t[:n].cpu())
        if n < G:  # padding rows: empty boards, player +1, no last move, count 0
            pad = (torch.zeros(G - n, A, dtype=torch.int8), torch.ones(G - n, dtype=torch.int8),
                   torch.full((G - n,), -1, dtype=torch.int32), torch.zeros(G - n, dtype=torch.int32))
            for t, w in zip(out, pad):
                assert torch.equal(t[n:].cpu(), w)
    for k, name in enumerate(("board", "player", "last move", "move count")):
        assert torch.equal(torch.cat(got[k]), torch.from_numpy(want[k])), name
    host = RP.ring_positions_host(rb, rows)  # the host path's decode is the same function of the ring
    for k in range(4):
        assert np.array_equal(host[k].reshape(want[k].shape), want[k])


# ---------------------------------------------------------------------------------------------- rewrite kernel
def _tables(entries, overrides=None):
    kept = np.array([e.kept for e in entries], np.int64)
    jobs = np.array([[e.slot, e.kept, e.n, e.drop, e.winner, 0] for e in entries], np.int32).reshape(-1, 6)
    jobs[:, 5] = np.cumsum(kept) - kept
    for (i, col), v in (overrides or {}).items():
        jobs[i, col] = v
    pin = torch.from_numpy(jobs).pin_memory()
    return pin, pin.cuda()


def _staged(entries, new):
    pol = np.concatenate([new[e.seq][0][e.drop:] for e in entries])
    val = np.concatenate([new[e.seq][1][e.drop:] for e in entries])
    return pol, val


def _twin_rings(H, n_steps, N, ptr, shape, seed):
    rs = np.random.RandomState(seed)
    games = [_play(rs, H, start, n, (-1, 0, 1)[i % 3]) for i, (start, n) in enumerate(shape)]
    new = [(rs.dirichlet(np.full(H * H, 0.3), g["n"]), rs.uniform(-1, 1, g["n"]).astype(np.float32)) for g in games]
    rings = []
    for _ in range(2):
        rb = _random_ring(H, n_steps, N, ptr, seed)
        for g in games:
            _add(rb, g)
        rings.append(rb)
    _assert_ring(rings[0], rings[1], "the twin rings before the rewrite")
    return rings[0], rings[1], new


@pytest.mark.parametrize("n_steps", [3, 10])
@pytest.mark.parametrize("layout", ["lengths", "wrap", "15x15"])
def test_rewrite_kernel_equals_host_rewrite(n_steps, layout):
    """lengths: 5x5, games of 1, 2, U, U+1, n_steps, n_steps+1 and A moves, winners -1, 0 and 1, and a resident game
    of 8 moves that is not in the job table.  wrap: N = 37 at ptr 30, the first game trimmed to its last 3 slices,
    the last one wrapping the ring's end, three games in one launch and a resident one left out.  15x15: A = 225."""
    H, N, ptr, shape, skip = {
        "lengths": (5, 256, 0, [(0, 1), (1, 2), (0, U), (2, 8), (3, U + 1), (0, n_steps), (1, n_steps + 1), (0, 25)], 3),
        "wrap": (5, 37, 30, [(0, 12), (3, 20), (1, 5), (0, 9)], 1),
        "15x15": (15, 256, 0, [(0, 225), (4, 7), (1, n_steps + 1)], 1)}[layout]
    dev, host, new = _twin_rings(H, n_steps, N, ptr, shape, 7 * n_steps + H)
    if layout == "wrap":
        assert [(e.slot, e.kept, e.drop) for e in dev.games] == [(2, 3, 9), (5, 20, 0), (25, 5, 0), (30, 9, 0)]
    entries = [e for e in dev.games if e.seq != skip]
    assert len(entries) == len(shape) - 1 >= 2 and (layout != "lengths" or {e.winner for e in entries} == {-1, 0, 1})
    pol, val = _staged(entries, new)
    P = len(val)
    pin, tab = _tables(entries)
    before = _snap(dev)
    dev.rewrite_games(torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda(), P, pin, tab, len(entries))
    host.rewrite_games_host([e for e in host.games if e.seq != skip], pol, val)
    _assert_ring(dev, host, layout)
    for k in ("obs", "act", "rew", "prio"):
        assert torch.equal(getattr(dev, k), before[k]), k
    e = [e for e in dev.games if e.seq == skip][0]  # the resident game outside the table: not a bit of it changed
    idx = ((torch.arange(e.kept) + e.slot) % N).cuda()
    assert torch.equal(dev.pol[idx], before["pol"][idx]) and torch.equal(dev.val[idx], before["val"][idx])
    # every policy is new; the value targets change where a surviving position bootstraps from a new value
    assert not torch.equal(dev.pol, before["pol"])
    assert torch.equal(dev.val, before["val"]) != any(e.n - n_steps > e.drop for e in entries)


def test_rewrite_kernel_refusals_leave_the_ring_unchanged():
    from datou_gomoku_muzero_amd import _lib as L
    dev, _, new = _twin_rings(5, 10, 37, 30, [(0, 12), (3, 20)], 3)
    entries = list(dev.games)
    pol, val = _staged(entries, new)
    P = len(val)
    pol_d, val_d = torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda()
    before = _snap(dev)
    pin, tab = _tables(entries)
    cases = {
        "overlap": lambda: dev.rewrite_games(pol_d, val_d, P, *_tables(entries, {(1, 0): 3}), 2),  # 30..4 and 3..22
        "staged row": lambda: dev.rewrite_games(pol_d, val_d, P - 1, pin, tab, 2),
        "pol_new": lambda: dev.rewrite_games(pol_d[:P - 1], val_d, P, pin, tab, 2),
        "val_new": lambda: dev.rewrite_games(pol_d, val_d[:P - 1], P, pin, tab, 2),
        "job table": lambda: dev.rewrite_games(pol_d, val_d, P, pin, tab[:1], 2),
        "kept": lambda: dev.rewrite_games(pol_d, val_d, P, *_tables(entries, {(1, 1): 38, (1, 2): 38}), 2),  # > N
    }
    for word, call in cases.items():
        with pytest.raises(L.GmzError, match=word):
            call()
        _assert_ring(dev, before, "after the refusal of a bad %s" % word)
    dev.rewrite_games(pol_d, val_d, P, pin, tab, 2)  # and the good call goes through
    torch.cuda.synchronize()
    assert not torch.equal(dev.pol, before["pol"])


# ---------------------------------------------------------------------------------------------- a whole pass
def _ingest_games(rings, H, games, rs):
    """``games`` through a device history and ReplayBuffer.ingest_history into every ring of ``rings``."""
    from test_replay_ingest_gpu import _random_history, _snapshot
    A = H * H
    h = _random_history(len(games), A, rs)
    fin = {}
    for g, game in enumerate(games):
        bk, s0, n = g & 1, game["start"], game["n"]
        for name, key in (("board", "boards"), ("player", "players"), ("last", "lasts"), ("pol", "pols"), ("val", "vals"),
                          ("act", "acts")):
            getattr(h, name)[bk, g, s0:s0 + n] = torch.from_numpy(game[key]).cuda()
        fin[g] = (bk, s0, n, game["winner"], False)
    sn = _snapshot(h, fin)
    done = h.finished(sn)
    for rb in rings:
        assert len(rb.ingest_history(h, sn, games=done)) == len(games)
    return h


def test_pass_equals_search_positions_then_host_rewrite():
    """9x9 MuZero, 50 simulations, 16 engine slots, the hash backend (tests/test_reanalysis_gpu.py's engine); three
    ingested games of 9 + 12 + 7 = 28 positions, so the second game spans two search chunks and the second chunk is
    padded; one game from an odd start.  With the same Gumbel noise the pass leaves the ring as
    Reanalyser.search_positions + rewrite_games_host leave its twin; so does the pass through the host; a second pass
    at the same step finds nothing old enough."""
    from datou_gomoku_muzero_amd import engine as E, reanalysis as RA
    from datou_gomoku_muzero_amd.config import GmzConfig
    H, A = 9, 81
    rs = np.random.RandomState(11)
    games = [_play(rs, H, start, n, w) for (start, n, w) in ((0, 9, 1), (3, 12, -1), (0, 7, 0))]
    rings = [_random_ring(H, 10, 64, 50, seed=5) for _ in range(3)]
    _ingest_games(rings, H, games, rs)
    dev, twin, via_host = rings
    _assert_ring(dev, twin, "the rings after the ingest")
    assert [(e.n, e.start, e.winner, e.version) for e in dev.games] == [(9, 0, 1, 0), (12, 3, -1, 0), (7, 0, 0, 0)]
    P = 28
    gumbel = rs.gumbel(0, 1, (P, A))
    cfg = GmzConfig(BOARD_SIZE=H, NUM_SIMULATIONS=50)
    before = _snap(dev)
    ra = RA.RingReanalyser(cfg, dev, None, num_games=16, max_positions=A, seed=1)
    assert ra.pass_(2, age=3, gumbel=gumbel) == (0, 0)  # version 0 > 2 - 3: too young
    assert ra.pass_(5, age=3, gumbel=gumbel) == (3, P)
    torch.cuda.synchronize()
    assert [e.version for e in dev.games] == [5, 5, 5] and ra.eng.errors() == 0
    # the twin: the original positions through the batched host-side search, then the host rewrite
    eng = E.BatchedSelfPlayEngine(None, num_games=16, BOARD_SIZE=H, NUM_SIMULATIONS=50, MCTS_IMPLEMENTATION="MuZero")
    pos = [np.concatenate([g[k] for g in games]) for k in ("boards", "players", "lasts", "mcs")]
    pol, val, act, _ = RA.Reanalyser(eng).search_positions(pos[0].reshape(P, H, H), *pos[1:], gumbel=gumbel)
    assert (act >= 0).all()
    twin.rewrite_games_host(twin.eligible(5, 3), pol, val)
    _assert_ring(dev, twin, "the device pass against search_positions + rewrite_games_host")
    assert torch.equal(ra.pol_new[:P].cpu(), torch.from_numpy(pol)) and torch.equal(ra.val_new[:P].cpu(), torch.from_numpy(val))
    for k in ("obs", "act", "rew", "prio"):
        assert torch.equal(getattr(dev, k), before[k]), k
    assert not torch.equal(dev.pol, before["pol"]) and not torch.equal(dev.val, before["val"])
    after = _snap(dev)
    assert ra.pass_(5, age=3, gumbel=gumbel) == (0, 0)
    _assert_ring(dev, after, "a second pass at the same step")
    # the same pass through host memory (the path of a CPU ring and of the A/B)
    rh = RA.RingReanalyser(cfg, via_host, None, num_games=16, max_positions=A, seed=1)
    rh.host = True
    assert rh.pass_(5, age=3, gumbel=gumbel) == (3, P)
    _assert_ring(via_host, dev, "the host pass against the device pass")
    # a pass with the engine's own noise must not block the host: every torch operation that
    # synchronises (a pageable upload, a read-back) raises in this mode; the last chunk is padded (12 of 16 rows)
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert ra.pass_(9, age=3) == (3, P)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert [e.version for e in dev.games] == [9, 9, 9] and ra.eng.errors() == 0
    for r in (ra, rh):
        r.close()
    eng.close()


# ---------------------------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("concurrent", [False, True])
def test_c4_loop_reanalyses_its_shard(concurrent):
    """C4Loop(device_ingest=True, reanalyse_per_iter=1) with age 0 on a 6x6 one-block network, time-sliced and with
    the trainer on its own stream.  The staging holds the whole ring of 256 slices, so every pass re-searches every
    game in it: afterwards every entry carries the last pass's step, and every game's ring targets are the n-step
    returns of the values (and the policies) that pass staged."""
    from datou_gomoku_muzero_amd import loop as LP, records as R, reanalysis as RA, replay as RP, trainer as T
    from datou_gomoku_muzero_amd.config import GmzConfig
    N = 256
    cfg = GmzConfig(BOARD_SIZE=6, NUM_SIMULATIONS=16, NUM_RES_BLOCKS=1, REANALYSIS_AGE_THRESHOLD=0)
    tcfg = T.TrainConfig(BOARD_SIZE=6, NUM_RES_BLOCKS=1, PHYSICAL_BATCH_SIZE=16, TRAIN_BUFFER_SIZE=N, ENABLE_PER=True)
    tr = T.Trainer(tcfg, device="cuda") if concurrent else T.Trainer(tcfg, device="cuda", graph=False)
    sp = LP.SelfPlay(cfg, 32, tr.state_dict_cpu(), seed=3)
    rb = RP.ReplayBuffer(tcfg, device="cuda")
    ra = RA.RingReanalyser(cfg, rb, tr.state_dict_cpu(), num_games=64, max_positions=N, seed=5)
    lp = LP.C4Loop(sp, tr, rb, tcfg, 16, moves_per_iter=2, train_steps_per_iter=1, model_update_interval=2,
                   concurrent=concurrent, device_ingest=True, reanalyser=ra, reanalyse_per_iter=1)
    assert lp.concurrent == concurrent and (ra.ring_stream is lp.train_stream) and not ra.host
    st = lp.run(24)
    torch.cuda.synchronize()
    assert st["games"] > 0 and st["train_steps"] >= 5 and st["weight_pushes"] == st["train_steps"] // 2
    assert st["reanalysed_games"] == ra.games > 0 and st["reanalysed_positions"] == ra.positions > 0
    assert torch.isfinite(lp.last_logs).all()
    last_step = st["train_steps"] if concurrent else st["train_steps"] - 1  # the last pass ran before the last step
    assert len(rb.games) > 0 and sum(e.kept for e in rb.games) == len(rb)
    assert [e.version for e in rb.games] == [last_step] * len(rb.games)
    take, P = ra.last_pass
    assert [e.seq for e in take] == [e.seq for e in rb.games] and P == len(rb)
    pols, vals = ra.pol_new[:P].float().cpu(), ra.val_new[:P].cpu().numpy()
    U1, first = tcfg.NUM_UNROLL_STEPS + 1, 0
    for e in take:
        full = np.zeros(e.n, np.float32)
        full[e.drop:] = vals[first:first + e.kept]
        vt = np.asarray(R.compute_n_step_returns(R.final_rewards(e.n, e.winner).tolist(), list(full), tcfg.DISCOUNT,
                                                 tcfg.N_STEPS), np.float32)
        want = np.zeros((e.kept, U1), np.float32)
        for k in range(e.kept):
            m = min(U1, e.n - e.drop - k)
            want[k, :m] = vt[e.drop + k:e.drop + k + m]
        idx = ((torch.arange(e.kept) + e.slot) % N).cuda()
        assert torch.equal(rb.val[idx].cpu(), torch.from_numpy(want)), e
        assert torch.equal(rb.pol[idx, 0].cpu(), pols[first:first + e.kept]), e
        first += e.kept
    for eng in list(getattr(sp.eng, "engines", [sp.eng])) + [ra.eng]:
        assert eng.errors() == 0
    sp.close()
    ra.close()
