"""Re-analysis of the games in the replay ring, without a GPU: the ring's game directory against a brute-force model
of the ring, the selection of games to re-analyse, the host rewrite of a game's targets against a ring rebuilt from
scratch, the composed loop's bookkeeping with a scripted re-analyser, and the refusals of the two new entry points
(fake pointers: every call must stop at a check before any launch)."""
import ctypes

import numpy as np
import pytest

from test_loop import _ScriptedSelfPlay, _random_game

torch = pytest.importorskip("torch")

H, A, U = 6, 36, 5


def _tcfg(N, **kw):
    from datou_gomoku_muzero_amd import trainer as T
    return T.TrainConfig(BOARD_SIZE=H, NUM_RES_BLOCKS=1, NUM_FILTERS=16, NUM_UNROLL_STEPS=U, TRAIN_BUFFER_SIZE=N, **kw)


def _blank_slices(n):
    return (np.zeros((n, U + 1, 3, H, H), np.uint8), np.zeros((n, U), np.int32), np.zeros((n, U), np.float32),
            np.zeros((n, U + 1, A), np.float32), np.zeros((n, U + 1), np.float32))


def _model_append(model, ptr, n, seq, N):
    """ReplayBuffer.add_arrays of an n-slice game on the model: slot -> (seq, slice index), None for no game."""
    first = max(0, n - N)
    for i in range(n - first):
        model[(ptr + i) % N] = None if seq is None else (seq, first + i)
    return (ptr + n - first) % N


def _assert_directory_equals_model(rb, model):
    N = rb.N
    owners = {}
    for slot, own in enumerate(model):
        if own is not None:
            owners.setdefault(own[0], {})[own[1]] = slot
    assert sorted(e.seq for e in rb.games) == sorted(owners), "an entry is missing or extra"
    assert [e.seq for e in rb.games] == sorted(owners), "entries out of append order"
    for e in rb.games:
        ts = owners[e.seq]
        assert (e.kept, e.drop, e.slot) == (len(ts), min(ts), ts[min(ts)]), e
        assert e.drop + e.kept == e.n  # what survives is the game's newest slices
        assert all(ts[e.drop + k] == (e.slot + k) % N for k in range(e.kept)), e


def test_directory_equals_a_brute_force_model_of_the_ring():
    """N = 37; 300 random appends of games of 1..40 moves (some longer than the ring): add_arrays with ``game=``,
    add_arrays without it, and the job tables of whole snapshots (replay.replay_jobs + note_jobs, what
    ReplayBuffer.ingest_history does).  After every append each entry's (slot, kept, drop) is what the model's slots say."""
    from datou_gomoku_muzero_amd import replay as RP, trainer as T
    from datou_gomoku_muzero_amd.replay import replay_jobs
    N = 37
    rb = RP.ReplayBuffer(_tcfg(N), device="cpu")
    rs = np.random.RandomState(0)
    model, seq, kinds = [None] * N, 0, [0, 0, 0]
    for step in range(300):
        kind = int(rs.randint(3))
        kinds[kind] += 1
        if kind < 2:
            n = int(rs.randint(1, 41))
            ptr = rb.ptr
            if kind == 0:
                rb.add_arrays(*_blank_slices(n), game=(int(rs.randint(-1, 2)), int(rs.randint(0, 5)), step))
                e = rb.games[-1]
                assert (e.n, e.version, e.seq) == (n, step, seq)
            else:
                rb.add_arrays(*_blank_slices(n))
            assert rb.ptr == _model_append(model, ptr, n, seq if kind == 0 else None, N)
            seq += kind == 0
        else:  # one snapshot's finished games through the ingest's job table
            lens = [int(x) for x in rs.randint(1, 41, rs.randint(1, 5))]
            games = [(g, g & 1, int(rs.randint(0, 4)), n, int(rs.randint(-1, 2))) for g, n in enumerate(lens)]
            jobs, new_ptr, new_count = replay_jobs(games, rb.ptr, rb.count, N)
            rb.step = step
            rb.note_jobs(jobs, sum(min(n, N) for n in lens))
            ptr, in_table, seq0 = rb.ptr, set(jobs[:, 0].tolist()), seq
            for g, n in enumerate(lens):  # a game the table leaves out is overwritten whole by the ones after it
                ptr = _model_append(model, ptr, n, seq if g in in_table else None, N)
                seq += g in in_table
            assert ptr == new_ptr
            rb.ptr, rb.count = new_ptr, new_count
            made = [e for e in rb.games if e.seq >= seq0]
            assert [(e.n, e.winner, e.start, e.version) for e in made] == \
                [(n, w, row0, step) for (g, _, row0, n, w) in games if g in in_table]
        _assert_directory_equals_model(rb, model)
    assert min(kinds) > 50 and len(rb.games) > 0


def test_eligible_orders_by_version_then_append_order_and_cuts_by_age():
    from datou_gomoku_muzero_amd import replay as RP, trainer as T
    rb = RP.ReplayBuffer(_tcfg(200), device="cpu")
    for v in (7, 3, 9, 3, 0, 12):
        rb.add_arrays(*_blank_slices(4), game=(1, 0, v))
    key = lambda es: [(e.version, e.seq) for e in es]  # noqa: E731
    assert key(rb.eligible(12, 0)) == [(0, 4), (3, 1), (3, 3), (7, 0), (9, 2), (12, 5)]
    assert key(rb.eligible(12, 3)) == [(0, 4), (3, 1), (3, 3), (7, 0), (9, 2)]
    assert key(rb.eligible(12, 5)) == [(0, 4), (3, 1), (3, 3), (7, 0)]
    assert key(rb.eligible(12, 900)) == [] and key(rb.eligible(2, 0)) == [(0, 4)]
    rb.eligible(12, 0)[0].version = 12  # a re-analysed game goes to the back of the queue
    assert key(rb.eligible(12, 0))[0] == (3, 1) and key(rb.eligible(12, 1)) == [(3, 1), (3, 3), (7, 0), (9, 2)]


def _game_of(rs, n):
    """test_loop's random game with exactly ``n`` moves."""
    while True:
        g = _random_game(rs)
        if g[2] >= n:
            return tuple([g[0], g[1], n, 0, 0] + [x[:n] for x in g[5:]])


def _ring_of(games, pols, vals, N, ptr, extra):
    """A CPU ring at ``ptr`` holding ``extra`` slices of no game and then ``games`` with the given policies/values."""
    from datou_gomoku_muzero_amd import loop as LP, replay as RP, trainer as T
    cfg = _tcfg(N)
    rb = RP.ReplayBuffer(cfg, device="cpu")
    rb.ptr, rb.count = ptr, (N if ptr else 0)
    rs = np.random.RandomState(99)
    rb.add_arrays(rs.randint(0, 2, (extra, U + 1, 3, H, H)).astype(np.uint8), rs.randint(0, A, (extra, U)),
                  rs.uniform(-1, 1, (extra, U)), rs.dirichlet(np.ones(A), (extra, U + 1)),
                  rs.uniform(-1, 1, (extra, U + 1)))
    for (g, p, v) in zip(games, pols, vals):
        _, winner, n, _, _, boards, players, lasts, _, _, acts = g
        arrs = RP.slices_from_game(boards, players, lasts, p, v, acts, winner, H, cfg.DISCOUNT, cfg.N_STEPS, U)
        rb.add_arrays(*arrs, game=(winner, 0, 0))
    return rb


@pytest.mark.parametrize("N,ptr", [(400, 0), (37, 30)])
def test_rewrite_games_host_equals_a_ring_rebuilt_from_the_new_targets(N, ptr):
    """Ring A holds games with their self-play targets and is rewritten by rewrite_games_host; ring B is built from
    scratch by add_arrays of slices_from_game with the new policies and values.  N = 37: the pointer wraps inside a
    game and the oldest game has lost slices from the front."""
    rs = np.random.RandomState(N)
    # N = 37 at ptr 30: 3 + 20 + 12 + 12 slices, so the last game wraps and takes the first game's oldest 7 slices
    games = [_game_of(rs, n) for n in ((20, 12, 12) if N == 37 else (1, 2, 7, A, 13))]
    old_p, old_v = [g[8] for g in games], [g[9] for g in games]
    new_p = [rs.dirichlet(np.full(A, 0.3), g[2]) for g in games]
    new_v = [rs.uniform(-1, 1, g[2]).astype(np.float32) for g in games]
    a = _ring_of(games, old_p, old_v, N, ptr, 3)
    b = _ring_of(games, new_p, new_v, N, ptr, 3)
    assert not torch.equal(a.pol, b.pol) and not torch.equal(a.val, b.val)
    if N == 37:
        assert [(e.slot, e.kept, e.drop) for e in a.games] == [(3, 13, 7), (16, 12, 0), (28, 12, 0)]
    entries = a.eligible(0, 0)
    by_seq = dict(zip(range(len(games)), zip(new_p, new_v)))
    pol = np.concatenate([by_seq[e.seq][0][e.drop:] for e in entries])
    val = np.concatenate([by_seq[e.seq][1][e.drop:] for e in entries])
    a.rewrite_games_host(entries, pol, val)
    for name in ("obs", "act", "rew", "pol", "val", "prio"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert [(e.slot, e.kept, e.n, e.winner) for e in a.games] == [(e.slot, e.kept, e.n, e.winner) for e in b.games]


class _ScriptedReanalyser:
    """Stand-in for reanalysis.RingReanalyser: counts its passes and records the pushed weights."""

    def __init__(self):
        self.steps, self.loaded, self.ring_stream = [], [], "unset"

    def pass_(self, step):
        self.steps.append(step)
        return 2, 11

    def load_weights(self, sd):
        self.loaded.append(sorted(sd))


def test_c4_loop_runs_the_passes_and_pushes_weights_to_the_reanalyser():
    from datou_gomoku_muzero_amd import loop as LP, replay as RP, trainer as T
    cfg = _tcfg(4096, PHYSICAL_BATCH_SIZE=8, ENABLE_PER=True)
    tr = T.Trainer(cfg, device="cpu")
    rb = RP.ReplayBuffer(cfg, device="cpu")
    sp, ra = _ScriptedSelfPlay(5), _ScriptedReanalyser()
    lp = LP.C4Loop(sp, tr, rb, cfg, 8, moves_per_iter=2, train_steps_per_iter=1, model_update_interval=2, seed=7,
                   device="cpu", reanalyser=ra, reanalyse_per_iter=3)
    assert ra.ring_stream is None  # no train stream on the CPU: ring work on the current one
    st = lp.run(6)
    assert st["reanalysed_games"] == 2 * 18 and st["reanalysed_positions"] == 11 * 18 and len(ra.steps) == 18
    assert ra.steps == sorted(ra.steps) and ra.steps[-1] == st["train_steps"] - 1  # the pass before the last step
    assert st["weight_pushes"] == st["train_steps"] // 2 >= 1
    assert len(ra.loaded) == len(sp.loaded) == st["weight_pushes"] and ra.loaded[0] == sorted(sp.loaded[0])
    # the host path gave every game a directory entry at the step it was added
    assert len(rb.games) == st["games"] > 0 and sum(e.kept for e in rb.games) == len(rb) == st["slices"]
    assert all(e.drop == 0 and e.start == 0 and 0 <= e.version <= st["train_steps"] for e in rb.games)
    # off by default: no re-analyser, no passes, the counters stay in stats()
    off = LP.C4Loop(_ScriptedSelfPlay(5), tr, RP.ReplayBuffer(cfg, device="cpu"), cfg, 8, device="cpu")
    off.run(2)
    assert (off.stats()["reanalysed_games"], off.stats()["reanalysed_positions"], off.reanalyse_per_iter) == (0, 0, 0)


FAKE = ctypes.c_void_p(1 << 20)


def _positions(lib, rows, H=6, U=5, N=100, G=16, P=None, short=None):
    tab = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
    A = H * H
    caps = dict(ring=N * (U + 1) * 3 * A, rows=tab.nbytes, board=G * A, player=G, last=4 * G, count=4 * G)
    if short:
        caps[short] -= 1
    return lib.gmz_replay_positions(H, U, N, FAKE, caps["ring"], ctypes.c_void_p(tab.ctypes.data),
                                    len(tab) if P is None else P, FAKE, caps["rows"], G, FAKE, caps["board"], FAKE,
                                    caps["player"], FAKE, caps["last"], FAKE, caps["count"], None)


def _rewrite(lib, jobs, H=6, U=5, n_steps=10, N=100, P=50, short=None):
    tab = np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 6))
    A = H * H
    caps = dict(ring_pol=N * (U + 1) * A * 4, ring_val=N * (U + 1) * 4, pol_new=P * A * 8, val_new=P * 4, jobs=tab.nbytes)
    if short:
        caps[short] -= 1
    pw = (ctypes.c_double * 34)(*[0.997 ** i for i in range(34)])
    return lib.gmz_replay_rewrite(H, U, n_steps, N, FAKE, caps["ring_pol"], FAKE, caps["ring_val"], FAKE,
                                  caps["pol_new"], FAKE, caps["val_new"], P, ctypes.c_void_p(tab.ctypes.data), len(tab),
                                  FAKE, caps["jobs"], pw, None)


def test_positions_refuses_every_bad_argument_before_launching():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    err = lambda: lib.gmz_last_error().decode()  # noqa: E731
    good = [[3, 0], [99, 35]]
    for bad_h in (4, 23):
        assert _positions(lib, good, H=bad_h) < 0 and "board_size" in err()
    assert _positions(lib, good, U=0) < 0 and "unroll" in err()
    assert _positions(lib, good, P=0) < 0 and "P 0" in err()
    assert _positions(lib, [[0, 0]] * 17, G=16) < 0 and "P 17" in err()
    assert _positions(lib, [[100, 0]]) < 0 and "ring slot 100" in err()
    assert _positions(lib, [[-1, 0]]) < 0 and "ring slot -1" in err()
    assert _positions(lib, [[0, 36]]) < 0 and "move count 36" in err()  # a full board has no move to search
    assert _positions(lib, [[0, -1]]) < 0 and "move count -1" in err()
    for name, word in (("ring", "ring_obs"), ("rows", "row table"), ("board", "board_out"), ("player", "player_out"),
                       ("last", "last_out"), ("count", "count_out")):
        assert _positions(lib, good, short=name) < 0 and word in err() and "short" in err()


def test_rewrite_refuses_every_bad_argument_before_launching():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    err = lambda: lib.gmz_last_error().decode()  # noqa: E731
    good = [5, 9, 9, 0, 1, 0]  # slot, kept, n, drop, winner, first
    assert _rewrite(lib, np.zeros((0, 6), np.int32)) == 0  # an empty table is no error and launches nothing
    for bad_h in (4, 23):
        assert _rewrite(lib, [good], H=bad_h) < 0 and "board_size" in err()
    assert _rewrite(lib, [good], U=0) < 0 and "unroll" in err()
    assert _rewrite(lib, [good], n_steps=33) < 0 and "n_steps" in err()
    assert _rewrite(lib, [[100, 9, 9, 0, 1, 0]]) < 0 and "ring slot 100" in err()
    assert _rewrite(lib, [[5, 0, 9, 9, 1, 0]]) < 0 and "kept 0" in err()
    assert _rewrite(lib, [[5, 21, 30, 9, 1, 0]], N=20) < 0 and "kept 21" in err()  # kept > N
    assert _rewrite(lib, [[5, 9, 12, 2, 1, 0]]) < 0 and "n - kept" in err()
    assert _rewrite(lib, [[5, 9, 9, 0, 2, 0]]) < 0 and "winner" in err()
    assert _rewrite(lib, [good, [20, 4, 4, 0, 0, 8]]) < 0 and "first" in err()
    # a staged row outside 0..P-1: 9 + 4 rows against P = 12
    assert _rewrite(lib, [good, [20, 4, 4, 0, 0, 9]], P=12) < 0 and "staged row 12" in err()
    # jobs whose slot runs overlap: 5..13 against 13..16, and a run that wraps (95..99, 0..3) against 3..6
    assert _rewrite(lib, [good, [13, 4, 4, 0, 0, 9]]) < 0 and "overlap at ring slot 13" in err()
    assert _rewrite(lib, [[95, 9, 11, 2, -1, 0], [3, 4, 4, 0, 0, 9]]) < 0 and "overlap at ring slot 3" in err()
    for name, word in (("ring_pol", "ring_pol"), ("ring_val", "ring_val"), ("pol_new", "pol_new"),
                       ("val_new", "val_new"), ("jobs", "job table")):
        assert _rewrite(lib, [good], short=name) < 0 and word in err() and "short" in err()
