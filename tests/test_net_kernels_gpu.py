"""The inference network's kernels (csrc/gmz_net.hip: k_tower3, k_head_gemm, k_head_finish) against tests/net_ref.py,
the float64 model of the gmz_net_* contract of include/gmz.h, bit for bit, through GomokuNetHip, at every board size
5..19 in f16 and bf16, for the initial and the recurrent pass.

With 16-bit operands every product is exact in f32; the data of tests/net_cases.py keep every layer's terms multiples
of a quantum q with sum |terms| < 2^24 q (asserted on the CPU in tests/test_net_ref.py), so every partial sum in any
order is exact in f32, fused or not, and each stored activation is ONE rounding of the exact sum: the hidden states'
16-bit patterns, the logits' f32 bits and (through the logits) the head planes are determined.  The support logits
are exact too; the value and reward scalars then differ from float64 by support3's f32 arithmetic alone: three expf
at 1 ulp, two additions and three divisions give 8 * 2^-24, asserted as 16 * 2^-24 (an expf of up to 3 ulp).

Rules every test here follows
  * 13 rows: odd and no multiple of 2 or 5, so a packed workgroup repeats its partner; two rows are skipped (slot
    -1): rows (4, 9) on the full grid, (5, 10) with max_grid = 1, where one workgroup walks every board (bias slot
    parity, weight ring wrap, next-board input DMA).  Every row is live in one of the two runs;
  * the pool is filled with a NaN pattern; output slots have unnamed slots before, between and after them, which
    must keep the pattern; the recurrent pass's input states are the MODEL's, written straight into the pool, and
    must be unchanged afterwards;
  * logits, value and reward are pre-filled with NaN: live rows end finite, skipped rows untouched.

Tier A  one weight per output channel (tests/net_cases.py tap_targets): every tap in every layer, nothing rounds; one
        tap offset on the full grid, another with max_grid = 1.
Tier B  dense exact data whose final roundings bite (inexact / tie / negative shares asserted on the CPU), on both grids.
Tiers A and B run at every size with 2 blocks and at 5, 8, 13, 17 with 1 block, in f16 and bf16.  The f16 saturation
and subnormal cases run at every size on the full grid, saturation with 2 blocks (initial pass), subnormal stores
with 1 block (both passes); the one-call entry points at 9 and 15.
The shares, the largest scalar error over its bound and the mutants these tests were shown to catch are in
profiles/net_kernel_tests.txt.
"""
import ctypes

import numpy as np
import pytest

import net_cases as K
import net_ref as M

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROWS = K.ROWS
SENT = 0xFFA5  # a NaN in f16 and in bf16
OUT_I = 1 + 2 * np.arange(ROWS)          # initial pass: output slots, every other slot from 1
IN_R = 28 + np.arange(ROWS)              # recurrent pass: input states
OUT_R = 43 + 2 * np.arange(ROWS)         # recurrent pass: output slots
NS = 70
SKIPS = {0: K.SKIP, 1: (5, 10)}          # by max_grid
SCALAR_BOUND = 16 * 2.0 ** -24
DN = {1: "f16", 2: "bf16"}


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from datou_gomoku_muzero_amd import network as N, _lib
    from datou_gomoku_muzero_amd.config import GmzConfig
    return N, _lib, GmzConfig


def make_net(mods, case, size, dtype, max_grid=0):
    N, _, GmzConfig = mods
    cfg = GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=case["model"].blocks)
    net = N.GomokuNetHip(case["sd"], cfg, num_slots=NS, max_rows=ROWS, precision=K.PREC[dtype])
    net.w.max_grid = max_grid
    return net


def pool_bits(net):
    return net.pool.cpu().numpy().view(np.uint16).reshape(NS, net.A, 128)


def where(idx, H):
    r, p, ch = (int(i) for i in idx)
    return "row %d cell (%d, %d) channel %d" % (r, p // H, p % H, ch)


def assert_hidden(name, got, want, dtype, H, rows, taps=None):
    """16-bit patterns of the live rows against the model's stored values; the first difference names its cell."""
    wb = M.bits16(want, dtype)
    assert np.array_equal(M.from_bits16(wb, dtype), want)
    bad = got[rows] != wb[rows]
    if bad.any():
        i = np.argwhere(bad)[0]
        r, ch = rows[i[0]], int(i[2])
        chain = "" if taps is None else "; taps from the last layer back along the channel rotation: %s" % [
            int(t[(ch + 17 * k) % 128]) for k, t in enumerate(reversed(taps))]
        raise AssertionError("%s: %d of %d values differ, first at %s: got %r want %r%s" % (
            name, bad.sum(), bad.size, where((r, i[1], ch), H), M.from_bits16(got[r, i[1], ch], dtype),
            want[r, i[1], ch], chain))


def assert_f32(name, got, want, rows):
    w32 = np.asarray(want, np.float32)
    assert np.array_equal(w32.astype(np.float64), want), name + ": the model's value is not a float32"
    bad = got[rows].view(np.uint32) != w32[rows].view(np.uint32)
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d differ, first at row %d column %d: got %r want %r" % (
            name, bad.sum(), bad.size, rows[i[0]], i[1], got[rows][tuple(i)], w32[rows][tuple(i)]))


def assert_scalar(name, got, want, rows):
    """Prints the error over its bound (pytest -s): profiles/net_kernel_tests.txt quotes the largest of a run."""
    err = np.abs(got[rows].astype(np.float64) - want[rows])
    print("%s: max |error| %.3g = %.3f of the bound" % (name, err.max(), err.max() / SCALAR_BOUND))
    assert (err <= SCALAR_BOUND).all(), (name, err.max())


def outputs(net, n, reward):
    dev = net.device
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    return (nan(n, net.A), nan(n)) + ((nan(n),) if reward else ())


def check_guards(name, net, before, out, slots, outs, refused=False):
    """Everything the pass was not told to write is what it was; live rows are finite.  A refused call writes nothing."""
    live = (slots >= 0) & (not refused)
    after = pool_bits(net)
    keep = np.ones(NS, bool)
    keep[out[live]] = False
    assert np.array_equal(after[keep], before[keep]), name + ": a slot that was not named changed"
    for o in outs:
        o = o.cpu().numpy()
        assert np.isfinite(o[live]).all(), name + ": a live row is not finite"
        assert np.isnan(o[~live]).all(), name + ": a skipped row was written"
    return after


def run_initial(mods, net, obs, skip, call=None, refused=False):
    _, _lib, _ = mods
    slots = OUT_I.copy()
    slots[list(skip)] = -1
    net.pool.fill_(np.array(SENT, np.uint16).view(np.int16).item())
    before = pool_bits(net)
    ot = torch.from_numpy(obs).to(net.device)
    st = torch.from_numpy(slots.astype(np.int32)).to(net.device)
    lg, v = outputs(net, ROWS, False)
    (call or net.initial)(ot, st, lg, v, _lib.stream_ptr())
    torch.cuda.synchronize()
    after = check_guards("initial", net, before, OUT_I, slots, (lg, v), refused)
    return after[OUT_I], lg.cpu().numpy(), v.cpu().numpy(), np.flatnonzero(slots >= 0)


def run_recurrent(mods, net, states, actions, skip, dtype, call=None, refused=False):
    _, _lib, _ = mods
    slots = OUT_R.copy()
    slots[list(skip)] = -1
    net.pool.fill_(np.array(SENT, np.uint16).view(np.int16).item())
    sb = M.bits16(states, dtype)
    assert np.array_equal(M.from_bits16(sb, dtype), states)
    net.pool.view(NS, net.A, 128)[torch.from_numpy(IN_R).to(net.device)] = torch.from_numpy(sb.view(np.int16)).to(net.device)
    before = pool_bits(net)
    dev = net.device
    it, at, st = (torch.from_numpy(np.asarray(a, np.int32)).to(dev) for a in (IN_R, actions, slots))
    lg, v, r = outputs(net, ROWS, True)
    (call or net.recurrent)(it, at, st, lg, v, r, _lib.stream_ptr())
    torch.cuda.synchronize()
    after = check_guards("recurrent", net, before, OUT_R, slots, (lg, v, r), refused)
    return after[OUT_R], lg.cpu().numpy(), v.cpu().numpy(), r.cpu().numpy(), np.flatnonzero(slots >= 0)


def check_initial(mods, net, case, dtype, skip, what, taps=None, call=None):
    H, want = net.cfg.BOARD_SIZE, case["init"]
    hid, lg, v, rows = run_initial(mods, net, case["obs"], skip, call)
    assert_hidden(what + " initial hidden", hid, want["hidden"], dtype, H, rows, taps)
    assert_f32(what + " initial logits", lg, want["logits"], rows)
    assert_scalar(what + " initial value", v, want["value"], rows)
    return hid, lg, v


def check_recurrent(mods, net, case, dtype, skip, what, taps=None, call=None):
    H, want = net.cfg.BOARD_SIZE, case["rec"]
    hid, lg, v, r, rows = run_recurrent(mods, net, case["states"], case["actions"], skip, dtype, call)
    assert_hidden(what + " recurrent hidden", hid, want["hidden"], dtype, H, rows, taps)
    assert_f32(what + " recurrent logits", lg, want["logits"], rows)
    assert_scalar(what + " recurrent value", v, want["value"], rows)
    assert_scalar(what + " recurrent reward", r, want["reward"], rows)
    return hid, lg, v, r


# ---------------------------------------------------------------- Tier A
@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("size,blocks", K.CASES)
def test_tier_a_single_taps(mods, size, blocks, dtype):
    """A shifted, clipped copy per layer: tap offset 0 on the full grid, tap offset 5 with one workgroup walking every
    board.  The second network then goes through initial_inference, recurrent_inference and hidden, the convenience
    calls, on slots of their own choosing."""
    for t0, max_grid in zip(K.TAP_OFFSETS, (0, 1)):
        case = K.tap_case(size, dtype, t0, blocks)
        net = make_net(mods, case, size, dtype, max_grid)
        what = "taps+%d %dx%d %d blocks %s grid %d" % (t0, size, size, blocks, DN[dtype], max_grid)
        check_initial(mods, net, case, dtype, SKIPS[max_grid], what, taps=case["taps"]["repr"])
        check_recurrent(mods, net, case, dtype, SKIPS[max_grid], what, taps=case["taps"]["dyn"])
    check_convenience_calls(net, case, dtype, what)


def check_convenience_calls(net, case, dtype, what):
    net.w.max_grid = 0
    init = case["init"]
    lg, v, slots = net.initial_inference(case["obs"])
    lg2, v2, r2 = net.recurrent_inference(np.arange(ROWS), case["actions"], np.arange(ROWS, 2 * ROWS))
    torch.cuda.synchronize()
    rows = np.arange(ROWS)
    nhwc = lambda h: h.cpu().numpy().reshape(ROWS, 128, -1).transpose(0, 2, 1).astype(np.float64)
    assert np.array_equal(slots.cpu().numpy(), rows)
    assert np.array_equal(nhwc(net.hidden(rows)), init["hidden"])
    assert_f32(what + " initial_inference", lg.cpu().numpy(), init["logits"], rows)
    assert_scalar(what + " initial_inference value", v.cpu().numpy(), init["value"], rows)
    again = case["model"].recurrent(init["hidden"], case["actions"])
    assert np.array_equal(nhwc(net.hidden(np.arange(ROWS, 2 * ROWS))), again["hidden"])
    assert_f32(what + " recurrent_inference", lg2.cpu().numpy(), again["logits"], rows)
    assert_scalar(what + " recurrent_inference value", v2.cpu().numpy(), again["value"], rows)
    assert_scalar(what + " recurrent_inference reward", r2.cpu().numpy(), again["reward"], rows)


# ---------------------------------------------------------------- Tier B
# a case's two grids run one after the other, so its model (net_cases.dense_case keeps the last two) is built once
@pytest.mark.parametrize("size,blocks,dtype,max_grid", [(s, b, dt, g) for s, b in K.CASES for dt in (1, 2) for g in (0, 1)])
def test_tier_b_dense_exact(mods, size, blocks, dtype, max_grid):
    case = K.dense_case(size, blocks, dtype)
    net = make_net(mods, case, size, dtype, max_grid)
    what = "dense %dx%d %d blocks %s grid %d" % (size, size, blocks, DN[dtype], max_grid)
    check_initial(mods, net, case, dtype, SKIPS[max_grid], what)
    check_recurrent(mods, net, case, dtype, SKIPS[max_grid], what)


@pytest.mark.parametrize("size", K.SIZES)
def test_f16_stores_saturate_at_65504(mods, size):
    """Sums past 65504 are stored as 65504, never inf: by the convs' store (the last representation conv scaled up; the
    recurrent pass of the dense tier holds such sums too) and by the stem's, which has a clamp of its own."""
    live = np.setdiff1d(np.arange(ROWS), K.SKIP)
    case = K.variant_case(size, 2, "saturate")
    net = make_net(mods, case, size, 1)
    hid, _, _ = check_initial(mods, net, case, 1, K.SKIP, "saturate %d" % size)
    assert (hid[live] == 0x7BFF).mean() >= 0.005 and not (hid[live] == 0x7C00).any()
    case = K.variant_case(size, 2, "saturate_stem")
    net.load_state_dict(case["sd"])
    hid, _, _ = check_initial(mods, net, case, 1, K.SKIP, "saturate_stem %d" % size)
    assert not (hid[live] == 0x7C00).any()


@pytest.mark.parametrize("size", K.SIZES)
def test_f16_subnormal_stores(mods, size):
    """Hidden states in [2^-24, 2^-14): the conversion of a store keeps subnormals (net_ref.FLUSH_SUBNORMAL_STORES),
    and the next layer's MFMA and the heads read them as they are.  One block: see test_net_ref.test_subnormal_cases."""
    case = K.variant_case(size, 1, "subnormal24")
    net = make_net(mods, case, size, 1)
    hid, _, _ = check_initial(mods, net, case, 1, K.SKIP, "subnormal %d" % size)
    live = np.setdiff1d(np.arange(ROWS), K.SKIP)
    assert ((hid[live] > 0) & (hid[live] < 0x0400)).mean() >= 0.25
    case = K.variant_case(size, 1, "subnormal31")
    net.load_state_dict(case["sd"])
    check_recurrent(mods, net, case, 1, K.SKIP, "subnormal %d" % size)


# ---------------------------------------------------------------- one-call entry points
def raw_calls(mods, net, workspace_bytes=None):
    """gmz_net_initial / gmz_net_recurrent with net.initial's / net.recurrent's arguments."""
    _, _lib, _ = mods
    lib, ptr = net.lib, _lib.ptr
    wsb = net.workspace.numel() if workspace_bytes is None else workspace_bytes

    def initial(obs, slot, lg, v, stream):
        return lib.gmz_net_initial(ctypes.byref(net.w), ptr(obs), obs.shape[0], ptr(slot), ptr(net.pool), ptr(lg), ptr(v),
                                   ptr(net.workspace), wsb, stream)

    def recurrent(ins, act, slot, lg, v, r, stream):
        return lib.gmz_net_recurrent(ctypes.byref(net.w), ptr(net.pool), ptr(ins), ptr(act), ptr(slot), ins.shape[0],
                                     ptr(lg), ptr(v), ptr(r), ptr(net.workspace), wsb, stream)
    return initial, recurrent


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("size", [9, 15])
def test_one_call_entry_points(mods, size, dtype):
    """gmz_net_initial and gmz_net_recurrent equal the tower + heads pair and the model, bit for bit."""
    _, _lib, _ = mods
    case = K.dense_case(size, 2, dtype)
    net = make_net(mods, case, size, dtype)
    what = "one call %dx%d %s" % (size, size, DN[dtype])
    initial, recurrent = raw_calls(mods, net)
    ok = lambda f: (lambda *a: _lib.check(f(*a)))
    one = check_initial(mods, net, case, dtype, K.SKIP, what, call=ok(initial))
    one += check_recurrent(mods, net, case, dtype, K.SKIP, what, call=ok(recurrent))
    pair = check_initial(mods, net, case, dtype, K.SKIP, what) + check_recurrent(mods, net, case, dtype, K.SKIP, what)
    live = np.setdiff1d(np.arange(ROWS), K.SKIP)
    for a, b in zip(one, pair):
        assert np.array_equal(a[live].view(np.uint16 if a.dtype == np.uint16 else np.uint32),
                              b[live].view(np.uint16 if b.dtype == np.uint16 else np.uint32))


def test_one_call_entry_points_refuse_a_short_workspace(mods):
    """workspace_bytes one short of gmz_net_workspace_bytes: refused before any launch, nothing written."""
    _, _lib, _ = mods
    case = K.dense_case(9, 2, 1)
    net = make_net(mods, case, 9, 1)
    need = ctypes.c_size_t()
    _lib.check(net.lib.gmz_net_workspace_bytes(ctypes.byref(net.w), ROWS, ctypes.byref(need)))
    assert net.workspace.numel() == need.value
    initial, recurrent = raw_calls(mods, net, need.value - 1)
    seen = []

    def refused(f):
        def call(*a):
            seen.append(f(*a))
            assert seen[-1] != 0 and b"workspace" in net.lib.gmz_last_error()
        return call
    run_initial(mods, net, case["obs"], K.SKIP, call=refused(initial), refused=True)
    run_recurrent(mods, net, case["states"], case["actions"], K.SKIP, 1, call=refused(recurrent), refused=True)
    assert len(seen) == 2
