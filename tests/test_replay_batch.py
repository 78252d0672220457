"""gmz_replay_gather and gmz_replay_per_sample without a GPU: every refusal stops before a launch (fake pointers), the
numpy restatement of the draw's summation order equals ReplayBuffer.sample's PER branch where every partial sum is
exact, and ReplayBuffer.sample_indices is the index and weight half of sample, RNG stream included."""
import ctypes

import numpy as np
import pytest

import replay_batch_ref as REF

torch = pytest.importorskip("torch")

FAKE = ctypes.c_void_p(1 << 20)


def _gather(lib, H=6, U=5, N=100, count=50, B=7, k=1, flip=1, ring=(FAKE,) * 5, idx=FAKE, w=None, outs=(FAKE,) * 7,
            short=None):
    """gmz_replay_gather with fake device pointers: every call here must stop at a check (no GPU, nothing launched).
    ``short``: the output whose capacity is one byte short."""
    A = H * H
    need = [B * (U + 1) * 3 * A * 4, B * U * 8, B * U * 4, B * (U + 1) * A * 4, B * (U + 1) * 4, B * U * 8, B * 4]
    sized = []
    for i, (p, n) in enumerate(zip(outs, need)):
        sized += [p, max(n, 0) - (1 if i == short else 0)]
    return lib.gmz_replay_gather(H, U, N, count, B, *ring, idx, w, k, flip, *sized, None)


def test_gather_refuses_every_bad_argument_before_launching():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    err = lambda: lib.gmz_last_error().decode()  # noqa: E731
    for H in (4, 23):
        assert _gather(lib, H=H) < 0 and "board_size" in err()
    assert _gather(lib, U=0) < 0 and "unroll" in err()
    for B in (0, -3):
        assert _gather(lib, B=B) < 0 and "B " in err()
    assert _gather(lib, N=0, count=0) < 0 and "N " in err()
    for count in (0, 101, -1):
        assert _gather(lib, N=100, count=count) < 0 and "count" in err()
    for k in (-1, 4):
        assert _gather(lib, k=k) < 0 and "k " in err()
    for flip in (-1, 2):
        assert _gather(lib, flip=flip) < 0 and "flip" in err()
    for i in range(5):
        ring = tuple(None if j == i else FAKE for j in range(5))
        assert _gather(lib, ring=ring) < 0 and "ring" in err()
    assert _gather(lib, idx=None) < 0 and "idx" in err()
    for i in range(7):
        outs = tuple(None if j == i else FAKE for j in range(7))
        assert _gather(lib, outs=outs) < 0 and "output" in err()
    for i, name in enumerate(("obs_out", "act_out", "rew_out", "pol_out", "val_out", "act_aug_out", "w_out")):
        assert _gather(lib, short=i) < 0 and name in err() and "short" in err()


def _draw(lib, count=1000, B=7, prio=FAKE, r=FAKE, idx=FAKE, prob=FAKE, ws=FAKE, ws_short=0, idx_short=0, prob_short=0):
    need = ctypes.c_size_t()
    assert lib.gmz_replay_per_sample_workspace_bytes(max(count, 1), max(B, 1), ctypes.byref(need)) == 0
    return lib.gmz_replay_per_sample(prio, r, count, B, idx, max(B, 0) * 8 - idx_short, prob, max(B, 0) * 8 - prob_short,
                                     ws, need.value - ws_short, None)


def test_per_sample_refuses_every_bad_argument_before_launching():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    err = lambda: lib.gmz_last_error().decode()  # noqa: E731
    need = ctypes.c_size_t()
    for count in (0, -5):
        assert _draw(lib, count=count) < 0 and "count" in err()
        assert lib.gmz_replay_per_sample_workspace_bytes(count, 7, ctypes.byref(need)) < 0 and "count" in err()
    for B in (0, -1):
        assert _draw(lib, B=B) < 0 and "B " in err()
        assert lib.gmz_replay_per_sample_workspace_bytes(10, B, ctypes.byref(need)) < 0 and "B " in err()
    assert lib.gmz_replay_per_sample_workspace_bytes(10, 7, None) < 0 and "out" in err()
    for name in ("prio", "r", "idx", "prob", "ws"):
        assert _draw(lib, **{name: None}) < 0 and ("workspace" if name == "ws" else name + "_dev") in err()
    assert _draw(lib, ws_short=8) < 0 and "workspace" in err() and "short" in err()
    assert _draw(lib, idx_short=1) < 0 and "idx" in err() and "short" in err()
    assert _draw(lib, prob_short=1) < 0 and "prob" in err() and "short" in err()
    # the need grows with count (a workspace sized for the full ring serves every fill level): l per 16, T per 1024
    for count, want in ((1, 2), (16, 2), (17, 3), (1024, 65), (1025, 67), (70001, 4376 + 69)):
        assert lib.gmz_replay_per_sample_workspace_bytes(count, 360, ctypes.byref(need)) == 0
        assert need.value == 8 * want, (count, need.value)


def _ring(count, prio, per=True, N=None):
    from datou_gomoku_muzero_amd import replay as RP, trainer as T
    cfg = T.TrainConfig(BOARD_SIZE=5, NUM_UNROLL_STEPS=1, PHYSICAL_BATCH_SIZE=8, TRAIN_BUFFER_SIZE=N or count,
                        ENABLE_PER=per)
    rb = RP.ReplayBuffer(cfg, device="cpu")
    rb.count = count
    rb.prio[:count] = torch.from_numpy(np.asarray(prio, np.float32))
    return rb


@pytest.mark.parametrize("count", [1, 23, 70001])
def test_restatement_equals_sample_where_every_sum_is_exact(count):
    """Multiples of 2^-8 below 64: every f64 partial sum is exact in any order, so the stated order and torch's
    cumsum give the same cum, the same idx and the same weights, bit for bit."""
    rs = np.random.RandomState(count)
    prio = REF.dyadic_priorities(count, rs)
    rb = _ring(count, prio)
    cum, total = REF.per_cum(prio)
    assert np.array_equal(cum, np.cumsum(prio.astype(np.float64))) and total == cum[-1]
    for B in (1, 7, 360):
        if B > count:
            continue
        _, idx, w = rb.sample(B, np.random.RandomState(100 + B))
        r = np.random.RandomState(100 + B).random_sample(B)
        ridx, prob = REF.per_sample(prio, r, B)
        assert np.array_equal(ridx, idx.numpy())
        wr = (float(count) * torch.from_numpy(prob)) ** (-rb.cfg.PER_BETA)  # sample's own weight lines
        assert torch.equal((wr / wr.max()).float(), w)


def test_restatement_edges_clamp_and_first_of_equals():
    """r = 0 picks the first element whose cum reaches the segment's start (searchsorted's left side); a uniform of
    1 - 2^-53 in the last segment rounds u up to the total or past it and the clamp keeps count - 1."""
    prio = np.array([0.5, 0.25, 0.25, 1.0, 2.0], np.float32)
    idx, prob = REF.per_sample(prio, np.zeros(4), 4)     # u = 0, 1, 2, 3; cum = .5 .75 1 2 4
    assert idx.tolist() == [0, 2, 3, 4] and prob.tolist() == [0.125, 0.0625, 0.25, 0.5]
    r = np.array([0.0, 0.0, 1.0 - 2.0 ** -53])
    idx, _ = REF.per_sample(np.full(7, 0.1, np.float32), r, 3)
    assert idx.tolist()[0] == 0 and idx.tolist()[2] == 6


@pytest.mark.parametrize("per", [True, False])
def test_sample_indices_is_the_index_and_weight_half_of_sample(per):
    rs = np.random.RandomState(3)
    rb = _ring(500, rs.uniform(0.01, 3.0, 500), per=per, N=600)
    for B, seed in ((1, 0), (8, 1), (64, 2)):
        r1, r2 = np.random.RandomState(seed), np.random.RandomState(seed)
        _, idx, w = rb.sample(B, r1)
        got = rb.sample_indices(B, r2)
        assert torch.equal(got[0], idx) and got[0].dtype == torch.int64
        assert torch.equal(got[1], w) and got[1].dtype == torch.float32
        s1, s2 = r1.get_state(), r2.get_state()
        assert np.array_equal(s1[1], s2[1]) and s1[2:] == s2[2:]
    assert rb.sample_indices(501, np.random.RandomState(0)) is None
    assert rb.sample(501, np.random.RandomState(0)) is None


def test_hip_paths_refuse_a_cpu_ring():
    from datou_gomoku_muzero_amd import loop as LP, replay as RP, trainer as T
    rb = _ring(50, np.ones(50))
    with pytest.raises(ValueError, match="device-resident"):
        rb.sample_indices(8, np.random.RandomState(0), hip=True)
    with pytest.raises(ValueError, match="device-resident"):
        rb.sample_indices(80, np.random.RandomState(0), hip=True)  # before the "no batch yet" answer, too
    with pytest.raises(ValueError, match="device-resident"):
        rb.gather_into((None,) * 7, torch.zeros(8, dtype=torch.int64), None, 0, False)

    class _Scripted:
        moves = 0
    with pytest.raises(ValueError, match="device_batches needs the loop on a GPU"):
        LP.C4Loop(_Scripted(), None, rb, rb.cfg, 8, device="cpu", device_batches=True)
    assert LP.C4Loop(_Scripted(), None, rb, rb.cfg, 8, device="cpu").device_batches is False  # the default stays
    assert RP.ReplayBuffer.sample_indices.__defaults__[-1] is False
