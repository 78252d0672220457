"""gmz_replay_ingest without a GPU: the refusals that keep a wrong index from ever reaching a launch, the job-table
builder against a plain simulation of sequential ReplayBuffer.add_arrays, and the kernel's n-step model against
records.compute_n_step_returns."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO

torch = pytest.importorskip("torch")

MAX_N_STEPS = 32  # GMZ_REPLAY_MAX_N_STEPS (include/gmz.h)


def _call(lib, jobs, H=6, U=5, n_steps=10, G=4, L=36, N=100, dev_bytes=None):
    """gmz_replay_ingest with fake device pointers: every call here must stop at a check (no GPU, nothing launched)."""
    fake = ctypes.c_void_p(1 << 20)
    tab = np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 8))
    pw = (ctypes.c_double * (MAX_N_STEPS + 2))(*[0.997 ** i for i in range(MAX_N_STEPS + 2)])
    nb = tab.nbytes if dev_bytes is None else dev_bytes
    return lib.gmz_replay_ingest(H, U, n_steps, G, L, fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, fake,
                                 fake, N, ctypes.c_void_p(tab.ctypes.data), len(tab), fake, nb, pw, None, None)


def test_ingest_refuses_every_bad_argument_before_launching():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    err = lambda: lib.gmz_last_error().decode()  # noqa: E731
    hdr = open(os.path.join(REPO, "include", "gmz.h")).read()
    assert "#define GMZ_REPLAY_MAX_N_STEPS %d" % MAX_N_STEPS in hdr
    good = [0, 0, 0, 9, 1, 0, 0, 0]  # game, bank, row0, n, winner, drop, slot, first
    for H in (4, 23):
        assert _call(lib, [good], H=H) < 0 and "board_size" in err()
    assert _call(lib, [good], n_steps=MAX_N_STEPS + 1) < 0 and "n_steps" in err()
    assert _call(lib, [good], U=0) < 0 and "unroll" in err()
    assert _call(lib, [good, [1, 0, 0, 9, 1, 0, 9, 9]], dev_bytes=2 * 32 - 32) < 0 and "device job table" in err()
    assert _call(lib, [[4, 0, 0, 9, 1, 0, 0, 0]], G=4) < 0 and "game 4" in err()
    assert _call(lib, [[0, 2, 0, 9, 1, 0, 0, 0]]) < 0 and "bank 2" in err()
    assert _call(lib, [[0, 0, 30, 7, 1, 0, 0, 0]], L=36) < 0 and "rows" in err() and "L = 36" in err()
    assert _call(lib, [[0, 0, 0, 9, 1, 0, 100, 0]], N=100) < 0 and "ring slot 100" in err()
    # two jobs whose kept slices share ring slots 5..8 (the second wraps: 95..99, 0..8 against 5..13)
    assert _call(lib, [[0, 0, 0, 9, 1, 0, 5, 0], [1, 0, 0, 14, 1, 0, 95, 9]], N=100) < 0 and "overlap" in err()
    assert _call(lib, [[0, 0, 0, 9, 1, 0, 5, 0], [1, 0, 0, 9, 1, 0, 13, 9]], N=100) < 0 and "overlap" in err()
    # more kept slices than the ring holds, a wrong prefix, a drop that leaves nothing
    assert _call(lib, [[0, 0, 0, 30, 1, 0, 0, 0], [1, 0, 0, 30, 1, 0, 30, 30]], N=50) < 0 and "more than" in err()
    assert _call(lib, [good, [1, 0, 0, 9, 1, 0, 9, 8]]) < 0 and "first" in err()
    assert _call(lib, [[0, 0, 0, 9, 1, 9, 0, 0]]) < 0 and "drop" in err()
    # an empty table is no error and launches nothing
    assert _call(lib, np.zeros((0, 8), np.int32)) == 0


def _simulate(games, ptr, count, N):
    """Sequential ReplayBuffer.add_arrays of each game's n slices, as written in trainer.py: owner[slot] = (game
    index in the list, slice index in the game) of the slice a slot holds at the end (None: untouched)."""
    owner = [None] * N
    for j, n in enumerate(games):
        first = 0
        if n > N:  # only the newest N survive the ring
            first, n = n - N, N
        for i in range(n):
            owner[(ptr + i) % N] = (j, first + i)
        ptr = (ptr + n) % N
        count = min(N, count + n)
    return owner, ptr, count


@pytest.mark.parametrize("name,N,ptr,count,lens", [
    ("empty ring", 50, 0, 0, [9, 12, 1]),
    ("wrapping ptr", 50, 44, 50, [9, 12]),
    ("one game longer than the ring", 20, 7, 11, [36]),
    ("games whose total exceeds the ring", 37, 30, 37, [5, 1, 2, 6, 11, 10, 25]),
    ("a long game between short ones", 20, 3, 20, [4, 25, 6, 9]),
    ("exactly the ring", 16, 5, 2, [16, 3]),
])
def test_job_table_equals_sequential_add_arrays(name, N, ptr, count, lens):
    from datou_gomoku_muzero_amd.replay import replay_jobs
    games = [(10 + j, j & 1, 3 * (j % 2), n, (-1, 0, 1)[j % 3]) for j, n in enumerate(lens)]
    jobs, new_ptr, new_count = replay_jobs(games, ptr, count, N)
    owner, want_ptr, want_count = _simulate(lens, ptr, count, N)
    assert (new_ptr, new_count) == (want_ptr, want_count), name
    assert jobs.dtype == np.int32 and jobs.shape[1] == 8
    got = [None] * N
    first = 0
    for (g, bk, s0, n, w, drop, slot, fst) in jobs.tolist():
        j = g - 10
        assert games[j] == (g, bk, s0, n, w) and 0 <= drop < n and fst == first
        for k in range(n - drop):
            s = (slot + k) % N
            assert got[s] is None, "%s: two kept slices share ring slot %d" % (name, s)
            got[s] = (j, drop + k)
        first += n - drop
    assert got == owner, name
    assert first <= N


def test_job_table_of_nothing_changes_nothing():
    from datou_gomoku_muzero_amd.replay import replay_jobs
    jobs, ptr, count = replay_jobs([], 7, 9, 20)
    assert jobs.shape == (0, 8) and (ptr, count) == (7, 9)


def test_abandoned_game_contributes_nothing():
    """GameHistory.finished leaves an abandoned game (action -1) out, so it never reaches the table; its bank's
    start row is reset all the same.  Checked on the class without its device tensors."""
    from datou_gomoku_muzero_amd.replay import replay_jobs
    from datou_gomoku_muzero_amd.worker import GameHistory

    class _Ev:
        def synchronize(self):
            pass
    h = GameHistory.__new__(GameHistory)
    h.start = np.array([[0, 4, 0, 2], [0, 0, 0, 0]], dtype=np.int64)
    t = lambda x, dt: torch.tensor(x, dtype=dt)  # noqa: E731
    sn = dict(status=t([2, 1, -1, 0], torch.int8), mc=t([5, 12, 8, 35], torch.int32), bank=t([0, 0, 1, 0], torch.int64),
              mf=t([0, 1, 2, 3], torch.int32), mt=t([0, 4, 5, 6], torch.int32), act=t([3, 7, 9, -1], torch.int32), ev=_Ev())
    fin = h.finished(sn)
    assert fin == [(1, 0, 4, 9, 1, 1, 4), (2, 1, 0, 9, -1, 2, 5)]
    assert h.start.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]  # slot 3 (abandoned) reset too
    jobs, ptr, count = replay_jobs([x[:5] for x in fin], 0, 0, 100)
    assert jobs[:, 0].tolist() == [1, 2] and (ptr, count) == (18, 18)
    assert h.finished(None) == [] and h.finished(dict(ev=None)) == []


def _n_step_model(rew32, val32, discount, n_steps):
    """The kernel's value targets (csrc/gmz_replay.hip): f64 running sum of pw[i] * r in order, rounded to f32,
    then one f32 multiply and one f32 add for the bootstrap."""
    n = len(rew32)
    pw = [discount ** i for i in range(n_steps + 1)]  # python floats: the table the host hands to the kernel
    out = np.zeros(n, dtype=np.float32)
    for t in range(n):
        s = np.float64(0.0)
        for i in range(n_steps):
            if t + i < n:
                s = s + np.float64(pw[i]) * np.float64(rew32[t + i])
        o = np.float32(s)
        if t + n_steps < n:
            o = np.float32(o + np.float32(val32[t + n_steps]) * np.float32(pw[n_steps]))
        out[t] = o
    return out


def test_n_step_model_equals_compute_n_step_returns_bit_for_bit():
    from datou_gomoku_muzero_amd import records as R
    rs = np.random.RandomState(5)
    mismatches = games = 0
    for _ in range(300):
        n = int(rs.randint(1, 60))
        winner = int(rs.choice([-1, 0, 1]))
        rew = R.final_rewards(n, winner)
        # the kernel's closed form of final_rewards, quirk included
        d = n - 1 - np.arange(n)
        assert np.array_equal(rew, np.where(winner == 0, 0.0, np.where((d % 4 == 0) | (d % 4 == 3), 1.0, -1.0)))
        vals = rs.uniform(-1, 1, n).astype(np.float32)
        for n_steps in (1, 3, 10):
            for discount in (0.9, 0.997, 1.0):
                want = np.asarray(R.compute_n_step_returns(rew.tolist(), list(vals), discount, n_steps), np.float32)
                got = _n_step_model(rew, vals, discount, n_steps)
                mismatches += int((want.view(np.uint32) != got.view(np.uint32)).sum())
                games += 1
    assert games == 2700 and mismatches == 0, mismatches


def test_device_ingest_needs_a_device_history_and_a_device_ring():
    from datou_gomoku_muzero_amd import loop as LP, replay as RP, trainer as T
    cfg = T.TrainConfig(BOARD_SIZE=6, NUM_RES_BLOCKS=1, PHYSICAL_BATCH_SIZE=8, TRAIN_BUFFER_SIZE=64)
    rb = RP.ReplayBuffer(cfg, device="cpu")

    class _Scripted:  # a self-play source without a device history, as tests/test_loop.py's stand-in
        moves = 0
    with pytest.raises(ValueError, match="device history"):
        LP.C4Loop(_Scripted(), None, rb, cfg, 8, device="cpu", device_ingest=True)
    lp = LP.C4Loop(_Scripted(), None, rb, cfg, 8, device="cpu")  # the default stays the host path
    assert lp.device_ingest is False

    class _Hist:
        A = 36
    with pytest.raises(ValueError, match="device-resident"):
        rb.ingest_history(_Hist(), None)
