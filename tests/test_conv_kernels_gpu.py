"""Every f16/bf16 gmz_conv3x3_* entry point of include/gmz.h (csrc/gmz_conv.hip: k_pack_conv, k_pack_many, k_conv3,
k_conv3_wgrad, k_conv3_wgrad_reduce) against tests/conv_ref.py, the float64 model of its documented arithmetic,
element by element, through raw ``_lib.call``.

Rules every GPU test here follows
  * every output (y, bn_y, stats, dW, packed weights) is a slice of a larger byte buffer: PAD sentinel bytes (0xA5)
    on both sides, the slice itself pre-filled with 0xFF bytes (a NaN in f16, bf16, f32 and f64) or, for the packed
    weights, with 0xA5 and then 0x5A (the two results must agree).  Afterwards every element is finite and the
    sentinels are intact; a strided dW is a view whose gaps must still be NaN;
  * the weight-gradient workspace is exactly gmz_conv3x3_wgrad_workspace_bytes(N) long and the statistics buffer
    exactly gmz_conv3x3_stats_slots(N) (or N) slots, between sentinels;
  * inputs are the model's, never another kernel's output, except the packed weights (a private layout);
  * no CU count is written here: multi_processor_count and the public grid rules (forward: at most 4 * CUs
    workgroups, rounded down to a multiple of 16, two per board; weight gradient: CUs / 24 * 8 chunks) give the
    shapes with more boards than the grid.

Tier A  one-hot boards, arbitrary float32 weights (some forced onto f16 / bf16 ties): each product is exact and
        each output one product, so y is the ROUNDED weight stamped around the cell, +0.0 elsewhere, bit for bit.
Tier B  dense integer x in [-4, 4], weights k / 1024 with |k| <= 128, addends and stamp tables on the 2^-10 grid:
        every product is a multiple of 2^-10 and every partial sum of any subset of a position's terms is below
        2^10 in magnitude (ASSERTED on the model's absolute-value sums), so every intermediate spans at most 20
        bits and is exact in f32 whatever the order of summation: y = round_to(float64 sum) bit for bit.  The
        weight gradient likewise on integers below 2^24.  The model's outputs must be inexact / exact ties often
        enough (asserted) for the final rounding to matter.
Tier C  production-like data, per-element bound with no constant taken from the kernels' error.  Products of two
        16-bit operands are exact in f32.  The guides' MFMA table documents the f32-input MFMA as a chain of fmaf
        (MI355X_MICROARCH.md, matrix-core table, row "F32 (f32 in)": "exact f32 (= fmaf chain, bitwise)") and is
        silent on how the f16 / bf16 forms round inside their 32-term accumulation, so each of the K - 1 additions
        is charged e = 2^-23 (a truncating adder), not 2^-24:
          D = K e sum|x w|,     |dy| <= D + uT (|y| + D) + tT
        K = 1,152 for the convolution; K = N H^2 + chunks (the reduction's additions) for dW, stored in f32;
        uT = 2^-11 / 2^-8 (f16 / bf16), 2^-24 (f32), tT = half the smallest subnormal of the storage type.
        forward_add: one more f32 addition, K + 1 over sum|x w| + |addend|.
Statistics (f32 per lane and workgroup, then f64): a lane adds its ceil(ceil(H^2 / 16) / 2) positions of each of
        its ceil(N / slots) boards, then 4 shuffle steps: n f32 additions a chain, so per channel
        |d sum| <= n u sum|v| (u = 2^-24; v * v is exact in f32 and fused into its addition); where sum|y| < 2^14
        on the 2^-10 grid (Tier B at small N) the f32 sums of y are exact and compared exactly.  Backward sums:
        xhat = (x - mean) * invstd adds two roundings a term: (n + 2) u sum|dz xhat|.
The largest error / bound ratios, the inexact / tie shares and the mutants the tests were shown to catch are in
profiles/conv_kernel_tests.txt.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import bn_ref
import conv_ref as R
from conftest import REPO

gpu = pytest.mark.gpu
CC = 128
SIZES = [6, 9, 15, 19]
AB_SIZES = [9, 15]  # gmz_conv3x3_forward_stamp / _forward_bwdstats
TD = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
DN = {0: "f32", 1: "f16", 2: "bf16"}
U = 2.0 ** -24
E_MFMA = 2.0 ** -23
UT = {0: 2.0 ** -24, 1: 2.0 ** -11, 2: 2.0 ** -8}
TINY = {0: 2.0 ** -150, 1: 2.0 ** -25, 2: 2.0 ** -134}
PAD = 4096  # sentinel bytes on both sides of every output
SENT = 0xA5
PACKED_BYTES = 294912
KB = 8  # base boards of the +-1 construction
MASKS = ["null", "ones", "zeros", "one", "first", "last", "ragged"]
SMALL_N = [1, 2, 7, 8, 9, 13]


def _lib():
    import datou_gomoku_muzero_amd._lib as L
    return L


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------ the public grid rules
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def grid_cap(n_cu):
    """forward workgroups: at most 4 per CU, rounded down to a multiple of 16; two per board"""
    return 4 * n_cu // 16 * 16


def slots_rule(N, n_cu):
    return min((2 * N + 15) // 16 * 16, grid_cap(n_cu)) // 2


def chunks_rule(N, n_cu):
    return min(n_cu // 24 * 8, (N + 7) // 8 * 8)


def stride_shapes(n_cu):
    """H = 6 only: more boards than forward workgroup pairs, so the stride loop runs once and twice more."""
    n = grid_cap(n_cu) // 2 + 5
    return [n, 2 * n]


def wgrad_big_shapes(n_cu):
    ch = n_cu // 24 * 8
    return [ch + 3, 8 * ch + 5]


def test_shape_rules_cover_the_stride_loops():
    for n_cu in (256, 304, 64):
        a, b = stride_shapes(n_cu)
        assert -(-a // slots_rule(a, n_cu)) == 2 and -(-b // slots_rule(b, n_cu)) == 3
        c, d = wgrad_big_shapes(n_cu)
        assert -(-c // chunks_rule(c, n_cu)) == 2 and -(-d // chunks_rule(d, n_cu)) == 9
        assert b * 36 * CC * 2 <= 12 << 20  # the largest activation tensor stays near 10 MB


# ------------------------------------------------------------------------------------------------ device plumbing
class Region:
    """``nbytes`` inside a larger byte allocation, PAD sentinel bytes on both sides, pre-filled with ``fill``."""

    def __init__(self, nbytes, fill=0xFF):
        assert nbytes % 16 == 0
        self.raw = torch.full((PAD + nbytes + PAD,), SENT, dtype=torch.uint8, device="cuda")
        self.b = self.raw[PAD:PAD + nbytes]
        self.b.fill_(fill)
        self.nbytes = nbytes

    def view(self, dtype):
        return self.b.view(dtype)

    def intact(self):
        return bool((self.raw[:PAD] == SENT).all()) and bool((self.raw[PAD + self.nbytes:] == SENT).all())


def act_in(a, dt):
    """float64 [N][A][128] (representable) -> the kernel's operand"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(TD[dt]).cuda()


def act_out(N, H, dt):
    r = Region(N * H * H * CC * 2)
    return r, r.view(TD[dt])


def mask_of(kind, N, seed=0):
    if kind == "null":
        return None
    m = np.zeros(N, np.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind == "one":
        m[N // 2] = 1
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[-1] = 3  # any nonzero byte counts
    elif kind == "ragged":
        m[:] = np.random.RandomState(seed + N).rand(N) < 0.6
        m[0], m[-1] = (1, 0) if N > 1 else (1, 1)
    return m


def assert_bits(name, got, want, dtype):
    """got (device tensor) == want (float64 numpy, representable in dtype) bit for bit; NaN = not written."""
    w = torch.from_numpy(np.ascontiguousarray(want)).to(dtype).reshape(got.shape)
    assert np.array_equal(w.double().numpy().reshape(-1), np.asarray(want, np.float64).reshape(-1)), name + ": want not representable"
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[w.element_size()]
    g = got.contiguous().cpu()
    nanc = int(torch.isnan(g).sum())
    assert nanc == 0, "%s: %d of %d elements not written" % (name, nanc, g.numel())
    bad = g.view(it) != w.contiguous().view(it)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError("%s: %d of %d elements differ bitwise; first at flat index %d: got %r, want %r" % (
            name, int(bad.sum()), bad.numel(), i, float(g.reshape(-1)[i]), float(w.reshape(-1)[i])))


def within(name, dt, got, want, bound):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "%s: %d elements not written" % (name, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    bound = np.broadcast_to(bound, err.shape)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    print("%s %s: max error / bound = %.3g (max error %.3g)" % (name, DN[dt], ratio, float(err.max())))
    i = int(np.argmax(err - bound))
    assert ratio <= 1.0, "%s: error %.3g > bound %.3g at flat index %d (got %r, want %r)" % (
        name, err.flat[i], bound.flat[i], i, got.flat[i], np.asarray(want).flat[i])


# weights handed to the pack in every stride pattern the trainer uses
def weight_views(W32):
    """{name: device view of the same [128][128][3][3] values}: contiguous, channels-last, and the [:, :128] slice of
    a [128][144][3][3] weight (the dynamics stem) whose other 16 planes hold NaN."""
    w = torch.from_numpy(W32).cuda()
    full = torch.full((CC, 144, 3, 3), float("nan"), device="cuda")
    full[:, :CC] = w
    return {"contiguous": w, "channels_last": w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), "slice144": full[:, :CC]}


def pack(wview, dt, transpose):
    """gmz_conv3x3_pack into two differently pre-filled guarded regions; the agreed result (int16, device)."""
    L = _lib()
    outs = []
    for fill in (SENT, 0x5A):
        r = Region(PACKED_BYTES, fill)
        L.call("gmz_conv3x3_pack", dt, wview, *wview.stride(), int(transpose), r.b, L.stream_ptr())
        torch.cuda.synchronize()
        assert r.intact(), "pack wrote outside its 294,912 bytes"
        outs.append(r)
    assert torch.equal(outs[0].b, outs[1].b), "pack left bytes of its output unwritten"
    return outs[0].view(torch.int16)


def pack_many(jobs, dt):
    """jobs: [(weight view, transpose)] -> their packed int16 tensors, from ONE gmz_conv3x3_pack_many launch."""
    L = _lib()
    rec = np.dtype([("w", "<u8"), ("s", "<i8", 4), ("out", "<u8"), ("transpose", "<i4"), ("pad", "<i4")])
    assert rec.itemsize == L.query("gmz_conv3x3_pack_job_bytes")
    res = []
    for fill in (SENT, 0x5A):
        regs = [Region(PACKED_BYTES, fill) for _ in jobs]
        tab = np.zeros(len(jobs), rec)
        for i, ((wv, tr), r) in enumerate(zip(jobs, regs)):
            tab[i] = (wv.data_ptr(), tuple(wv.stride()), r.b.data_ptr(), int(tr), 0)
        dev = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
        L.call("gmz_conv3x3_pack_many", dt, dev, len(jobs), L.stream_ptr())
        torch.cuda.synchronize()
        assert all(r.intact() for r in regs)
        res.append(regs)
    for a, b in zip(*res):
        assert torch.equal(a.b, b.b), "pack_many left bytes of an output unwritten"
    return [r.view(torch.int16) for r in res[0]]


def stats_region(slots):
    r = Region(CC * slots * 24)
    return r, r.view(torch.float64)


def read_stats(sr, slots):
    r, t = sr
    assert r.intact(), "statistics written outside [128][%d][3]" % slots
    a = t.cpu().numpy().reshape(CC, slots, 3)
    assert np.isfinite(a).all(), "%d statistics elements not written" % int((~np.isfinite(a)).sum())
    return a


def forward(entry, dt, H, x, packed, N, addend=None, mask=None, stats=False, actions=None, table=None, bn=None):
    """One call of a forward-family entry point on fresh guarded outputs.  Returns (y device tensor, stats numpy
    [128][slots][3] or None)."""
    L = _lib()
    yr, y = act_out(N, H, dt)
    md = None if mask is None else torch.from_numpy(mask).cuda()
    slots, sr = 0, None
    if stats:
        slots = N if entry == "gmz_conv3x3_forward_board_stats" else L.query("gmz_conv3x3_stats_slots", N, ctype=ctypes.c_int)
        assert entry == "gmz_conv3x3_forward_board_stats" or slots == slots_rule(N, cus())
        sr = stats_region(slots)
    sp = sr[1] if sr else None
    st = L.stream_ptr()
    if entry == "gmz_conv3x3_forward":
        L.call(entry, dt, H, x, packed, y, N, st)
    elif entry == "gmz_conv3x3_forward_add":
        L.call(entry, dt, H, x, packed, addend, y, N, st)
    elif entry in ("gmz_conv3x3_forward_stats", "gmz_conv3x3_forward_board_stats"):
        L.call(entry, dt, H, x, packed, y, N, md, sp, slots, st)
    elif entry == "gmz_conv3x3_forward_stamp":
        L.call(entry, dt, H, x, packed, y, N, md, sp, slots, actions, table, 0, table.numel() * 4, st)
    elif entry == "gmz_conv3x3_forward_bwdstats":
        L.call(entry, dt, H, x, packed, addend, y, N, md, bn["x"], bn["y"], bn["save"], int(bn["relu"]), sp, slots, st)
    else:
        raise AssertionError(entry)
    torch.cuda.synchronize()
    assert yr.intact(), entry + " wrote outside y"
    return y, (read_stats(sr, slots) if stats else None)


DW_LAYOUTS = ["contiguous", "channels_last", "slice144"]


class DwOut:
    """The f32 weight gradient as a view of a guarded, NaN-filled region: contiguous, channels-last, or the [:, :128]
    slice of a [128][144][3][3] buffer (whose other planes are gaps that must stay NaN)."""

    def __init__(self, layout, dw0=None):
        self.r = Region(CC * (144 if layout == "slice144" else CC) * 9 * 4)
        f = self.r.view(torch.float32)
        self.gaps = None
        if layout == "contiguous":
            self.t = f.view(CC, CC, 3, 3)
        elif layout == "channels_last":
            self.t = f.view(CC, 3, 3, CC).permute(0, 3, 1, 2)
        else:
            full = f.view(CC, 144, 3, 3)
            self.t, self.gaps = full[:, :CC], full[:, CC:]
        if dw0 is not None:
            self.t.copy_(torch.from_numpy(dw0).to(torch.float32).cuda())

    def check(self, name):
        assert self.r.intact(), name + ": dW written outside its buffer"
        if self.gaps is not None:
            assert bool(torch.isnan(self.gaps).all()), name + ": the gaps of the strided dW were written"


def workspace_for(N):
    nb = _lib().query("gmz_conv3x3_wgrad_workspace_bytes", N)
    assert nb == chunks_rule(N, cus()) * 9 * CC * CC * 4
    return Region(nb)


def wgrad(dt, H, x, dy, N, layout, dw0=None):
    L = _lib()
    out, ws = DwOut(layout, dw0), workspace_for(N)
    L.call("gmz_conv3x3_wgrad", dt, H, x, dy, N, out.t, *out.t.stride(), int(dw0 is not None), ws.b, ws.nbytes,
           L.stream_ptr())
    torch.cuda.synchronize()
    out.check("gmz_conv3x3_wgrad")
    assert ws.intact(), "the weight gradient's partials left gmz_conv3x3_wgrad_workspace_bytes(%d)" % N
    return out.t


def wgrad_segments(dt, H, xs, dys, nps, layout, dw0=None):
    L = _lib()
    nseg = len(xs)
    out, ws = DwOut(layout, dw0), workspace_for(nseg * nps)
    P = ctypes.c_void_p * nseg
    L.call("gmz_conv3x3_wgrad_segments", dt, H, P(*[t.data_ptr() for t in xs]), P(*[t.data_ptr() for t in dys]), nseg,
           nps, out.t, *out.t.stride(), int(dw0 is not None), ws.b, ws.nbytes, L.stream_ptr())
    torch.cuda.synchronize()
    out.check("gmz_conv3x3_wgrad_segments")
    assert ws.intact()
    return out.t


# ------------------------------------------------------------------------------------------------ Tier A: geometry
def tie_weights(seed):
    """float32 randn / 34 with 300 elements each forced onto exact f16 and bf16 ties (a representable value plus half
    an ulp), lower neighbours of both parities."""
    rs = np.random.RandomState(seed)
    W = (rs.randn(CC, CC, 3, 3) / 34).astype(np.float32)
    flat = W.reshape(-1)
    idx = rs.choice(flat.size, 600, replace=False)
    for d, ix in ((1, idx[:300]), (2, idx[300:])):
        lo, q = R.ulp_gap(flat[ix].astype(np.float64), d)
        t = np.sign(flat[ix]) * (lo + q / 2)
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t) and R.is_tie(t, d).all()
        par = np.rint(lo / q) % 2
        assert 100 <= par.sum() <= 200
        flat[ix] = t
    return W


def geometry_cells(H):
    A, m = H * H, H // 2
    cells = [0, H - 1, A - H, A - 1, m, m * H, m * H + H - 1, A - H + m, m * H + m]
    if H == 19:
        cells += list(range(9 * H, 11 * H))  # rows 9 and 10: where the weight gradient's two row bands meet
    cells += [(A - 1) // 16 * 16, A - 1]  # first and last cell of the last partial 16-position tile
    return cells


GEOM_CHANNELS = [0, 7, 8, 63, 64, 127] + [8 * k + (3 * k + 1) % 8 for k in range(16)]


@functools.lru_cache(maxsize=None)
def geometry_case(H):
    cells = geometry_cells(H)
    N = max(len(cells), len(GEOM_CHANNELS))
    spec = [(cells[n % len(cells)], GEOM_CHANNELS[(n + n // len(GEOM_CHANNELS)) % len(GEOM_CHANNELS)]) for n in range(N)]
    x = np.zeros((N, H * H, CC))
    for n, (p, c) in enumerate(spec):
        x[n, p, c] = 1.0
    return spec, x, tie_weights(100 + H)


def geometry_want(spec, Wq, H):
    """round_to(W_eff)[o][c][t] at q = cell - d(t), +0.0 elsewhere (and where a weight rounds to -0.0: the product
    is added to an accumulator that starts at +0.0)"""
    want = np.zeros((len(spec), H, H, CC))
    for n, (p, c) in enumerate(spec):
        py, px = divmod(p, H)
        for ky in range(3):
            for kx in range(3):
                qy, qx = py - (ky - 1), px - (kx - 1)
                if 0 <= qy < H and 0 <= qx < H:
                    want[n, qy, qx] = Wq[:, c, ky, kx]
    return want.reshape(len(spec), H * H, CC) + 0.0


def test_geometry_case_covers_what_it_claims():
    assert sorted(set(c // 8 for c in GEOM_CHANNELS)) == list(range(16)) and {0, 7, 8, 63, 64, 127} <= set(GEOM_CHANNELS)
    for H in SIZES:
        spec, x, W = geometry_case(H)
        assert set(geometry_cells(H)) == set(p for p, _ in spec) and set(GEOM_CHANNELS) == set(c for _, c in spec)
        assert (x.sum(axis=(1, 2)) == 1).all()
        for dt in (1, 2):
            Wq = R.round_to(R.w_eff(W.astype(np.float64), 1), dt)
            want = geometry_want(spec, Wq, H)
            assert not np.signbit(want[want == 0]).any()
            if H <= 9:  # the hand-built expectation is the model's convolution
                assert np.array_equal(want, R.conv(x, Wq, H))
            assert (R.round_to(W.astype(np.float64), dt) != W).mean() > 0.9  # the pack's rounding is exercised


@gpu
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", SIZES)
def test_tier_a_forward_geometry_bitwise(H, dt, transpose):
    """Strictly contains the geometry of test_trainer.test_hip_conv3x3_forward_and_input_grad (kept)."""
    _need_gpu()
    spec, x, W = geometry_case(H)
    views = weight_views(W)
    packed = {k: pack(v, dt, transpose) for k, v in views.items()}
    for k in ("channels_last", "slice144"):
        assert torch.equal(packed[k], packed["contiguous"]), "pack from %s strides differs" % k
    # the same through gmz_conv3x3_pack_many, both packings of every stride pattern, jobs in shuffled order
    jobs = [(v, tr) for v in views.values() for tr in (0, 1)]
    order = np.random.RandomState(H).permutation(len(jobs))
    many = pack_many([jobs[i] for i in order], dt)
    other = pack(views["contiguous"], dt, 1 - transpose)
    for i, pk in zip(order, many):
        assert torch.equal(pk, packed["contiguous"] if jobs[i][1] == transpose else other), "pack_many job %d" % i
    assert not torch.equal(other, packed["contiguous"])
    Wq = R.round_to(R.w_eff(W.astype(np.float64), transpose), dt)
    y, _ = forward("gmz_conv3x3_forward", dt, H, act_in(x, dt), packed["contiguous"], len(spec))
    assert_bits("y", y.view(len(spec), H * H, CC), geometry_want(spec, Wq, H), TD[dt])


@functools.lru_cache(maxsize=None)
def wgrad_geometry_case(H):
    """Boards of up to three (p, q, c, o): x one-hot at cell p, channel c; dy one-hot at cell q, channel o; every
    (o, c) of the launch distinct, so block dW[o][c] has exactly one 1.0, at the tap with d(t) = p - q, or nothing."""
    A, m = H * H, H // 2
    qs = [0, H - 1, A - H, A - 1, m * H + m, (A - 1) // 16 * 16]
    if H == 19:
        qs += [9 * H, 9 * H + 18, 10 * H, 10 * H + 9, 10 * H + 18]
    pairs = []
    for q in qs:
        for t in range(9):
            py, px = q // H + t // 3 - 1, q % H + t % 3 - 1
            if 0 <= py < H and 0 <= px < H:
                pairs.append((py * H + px, q, t))
    # not neighbours: two apart; neighbours only by wrapping across a row end (index distance 1 and H -+ 1)
    far = [(2 * H + 2, 0), (0, 2), (H - 1, H), (H, H - 1), (H - 1, 0), (2 * H, H - 1), (A - 1, A - 2 * H)]
    pairs += [(p, q, None) for p, q in far]
    assert len(pairs) <= 120
    quads = [(p, q, (29 * i + 3) % CC, (37 * i + 5) % CC, t) for i, (p, q, t) in enumerate(pairs)]
    assert len(set((o, c) for _, _, c, o, _ in quads)) == len(quads) and len(set(c // 8 for _, _, c, _, _ in quads)) == 16
    N = -(-len(quads) // 3) + 2
    x, dy = np.zeros((N, A, CC)), np.zeros((N, A, CC))
    for i, (p, q, c, o, t) in enumerate(quads):
        x[i // 3, p, c] = 1.0
        dy[i // 3, q, o] = 1.0
    # neighbours only across BOARDS: the last cell of one board and the first of the next
    x[N - 2, A - 1, 126], dy[N - 1, 0, 125] = 1.0, 1.0
    quads.append((None, None, 126, 125, None))
    return quads, x, dy


def test_wgrad_geometry_case_is_what_it_claims():
    for H in SIZES:
        quads, x, dy = wgrad_geometry_case(H)
        dw = R.wgrad(x, dy, H)
        assert set(np.unique(dw)) <= {0.0, 1.0, 2.0, 3.0}
        for p, q, c, o, t in quads:
            blk = dw[o, c].reshape(9)
            if t is None:
                assert not blk.any()
            else:
                assert blk[t] == 1.0 and np.count_nonzero(blk) == 1


@gpu
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", SIZES)
def test_tier_a_wgrad_geometry_bitwise(H, dt):
    _need_gpu()
    quads, x, dy = wgrad_geometry_case(H)
    want = R.wgrad(x, dy, H)
    got = wgrad(dt, H, act_in(x, dt), act_in(dy, dt), x.shape[0], "contiguous")
    g = got.cpu().numpy()
    for p, q, c, o, t in quads:  # the named entries first, for a readable failure
        blk = g[o, c].reshape(9)
        assert (t is None and not blk.any()) or (t is not None and blk[t] == 1.0 and np.count_nonzero(blk) == 1), (
            "x cell %r channel %d, dy cell %r channel %d: dW[o][c] = %r, expected tap %r" % (p, c, q, o, blk, t))
    assert_bits("dW", got, want, torch.float32)


# ------------------------------------------------------------------------------------------------ Tier B: exact data
def grid16(rs, shape):
    """values j 2^s / 1024 with |j| <= 128 and s = 0..3: on the 2^-10 grid, |v| <= 1, 8 significant bits, so
    representable in f16 and in bf16"""
    return rs.randint(-128, 129, size=shape) * (2.0 ** rs.randint(0, 4, size=shape)) / 1024.0


@functools.lru_cache(maxsize=None)
def _exact_base(H, transpose):
    rs = np.random.RandomState(1000 * H + transpose)
    A = H * H
    x = rs.randint(-4, 5, size=(KB, A, CC)).astype(np.float64)
    W = rs.randint(-128, 129, size=(CC, CC, 3, 3)) / 1024.0
    addend = grid16(rs, (KB, A, CC))
    table = rs.randint(-4096, 4097, size=(9, CC)) / 1024.0
    assert np.array_equal(x * 1024, np.rint(x * 1024)) and np.abs(table).max() <= 4 and np.abs(x).max() <= 4
    We = R.w_eff(W, transpose)
    pre = R.conv(x, We, H)
    mag = R.abs_conv(x, We, H) + np.abs(addend) + np.abs(table).max()  # one table entry a cell
    # every partial sum of any subset of a position's terms is a multiple of 2^-10 below 2^10: at most 20 bits
    assert mag.max() < 1024, mag.max()
    assert np.array_equal(pre * 1024, np.rint(pre * 1024))
    return dict(x=x, W=W.astype(np.float32), We=We, addend=addend, table=table.astype(np.float32), pre=pre)


def exact_case(H, dt, transpose):
    """KB base boards; the model's exact sums; the conditions that make f32 accumulation exact, asserted.  The data
    are representable in f16 and in bf16 (asserted), so both dtypes share one float64 model per (H, packing)."""
    k = _exact_base(H, transpose)
    for a in (k["x"], k["W"].astype(np.float64), k["addend"]):
        assert np.array_equal(R.round_to(a, dt), a)
    return k


def shares(pre, dt):
    return float((R.round_to(pre, dt) != pre).mean()), float(R.is_tie(pre, dt).mean())


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", [6, 19])
def test_tier_b_data_exercise_the_final_rounding(H, dt):
    """From the model alone (CPU): at least 40 % (f16) / 80 % (bf16) of the exact sums are not representable and at
    least 5 % are exact ties."""
    k = exact_case(H, dt, 0)
    for name, pre in (("conv", k["pre"]), ("conv+addend", k["pre"] + k["addend"])):
        inexact, ties = shares(pre, dt)
        print("%s H=%d %s: inexact %.3f ties %.3f" % (name, H, DN[dt], inexact, ties))
        assert inexact >= (0.4 if dt == 1 else 0.8) and ties >= 0.05, (name, inexact, ties)


def signs(N, seed):
    s = np.where(np.random.RandomState(seed).rand(N) < 0.5, -1.0, 1.0)
    s[0] = 1.0
    return s


def lane_chain(H, N, slots):
    """f32 additions in one statistics chain: a lane's positions of each of its boards, then 4 shuffle steps"""
    npt = (H * H + 15) // 16
    return (npt + 1) // 2 * ((N + slots - 1) // slots) + 4


def check_stats(name, dt, H, N, got, y, mask, per_board):
    """got [128][slots][3] against the model's sums of the stored y over the live boards."""
    live = R.live(mask, N)
    if per_board:
        want = R.board_stats(y, mask)
        assert np.array_equal(got[:, :, 2], want[:, :, 2]), name + ": per-board counts"
        assert not got[:, ~live].any(), name + ": a dead board's statistics are not (0, 0, 0)"
        n_add, sabs, sq = lane_chain(H, 1, 1), np.abs(y).sum(axis=1).T * live[None, :], want[:, :, 1]
        g1, g2, w1, w2 = got[:, :, 0], got[:, :, 1], want[:, :, 0], want[:, :, 1]
    else:
        want = R.stats(y, mask)
        assert np.array_equal(got[:, :, 2].sum(axis=1), want[:, 2]), name + ": counts"
        n_add = lane_chain(H, N, got.shape[1])
        sabs, sq = np.abs(y[live]).sum(axis=(0, 1)), want[:, 1]
        g1, g2, w1, w2 = got[:, :, 0].sum(axis=1), got[:, :, 1].sum(axis=1), want[:, 0], want[:, 1]
    r = n_add * U + 2.0 ** -50
    if float(np.max(sabs, initial=0.0)) < 2.0 ** 14 and np.array_equal(y * 1024, np.rint(y * 1024)):
        assert np.array_equal(g1, w1), name + ": the f32 sums of y are exact here"
    else:
        within(name + " sum", 0, g1, w1, r * sabs)
    within(name + " sumsq", 0, g2, w2, r * sq)


@gpu
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", SIZES)
def test_tier_b_forward_family_bitwise(H, dt, transpose):
    """gmz_conv3x3_forward, _forward_add, _forward_stats, _forward_board_stats (and _forward_stamp at 9 and 15) on
    board n = s_n * base[n % 8]: y = round_to(exact sum) at every element, at every N.  A masked-out board's y is
    still the convolution (k_conv3 stores every board; the mask only selects what the statistics count).
    Strictly contains test_conv_sizes_gpu.test_forward_input_grad_and_weight_grad's forward half (kept)."""
    _need_gpu()
    k = exact_case(H, dt, transpose)
    packed = pack(torch.from_numpy(k["W"]).cuda(), dt, transpose)
    table = torch.from_numpy(k["table"]).cuda()
    Ns = SMALL_N + (stride_shapes(cus()) if H == 6 else [])
    for N in Ns:
        s = signs(N, N)[:, None, None]
        idx = np.arange(N) % KB
        x = act_in(s * k["x"][idx], dt)
        pre = s * k["pre"][idx] + 0.0  # -1 * 0 = -0.0; an exact zero sum is +0.0
        add = s * k["addend"][idx]
        want = R.round_to(pre, dt)
        tag = "H=%d N=%d " % (H, N)
        y, _ = forward("gmz_conv3x3_forward", dt, H, x, packed, N)
        assert_bits(tag + "forward y", y.view(N, H * H, CC), want, TD[dt])
        y, _ = forward("gmz_conv3x3_forward_add", dt, H, x, packed, N, addend=act_in(add, dt))
        assert_bits(tag + "forward_add y", y.view(N, H * H, CC), R.round_to(pre + add, dt), TD[dt])
        # every kind at N = 1 and 13; past the grid also the masks whose one live board is reached in a workgroup's
        # second or third stride iteration
        for kind in (MASKS if N in (1, 13) else ["ragged", "null", "one", "last"] if N > 13 else ["ragged", "null"]):
            m = mask_of(kind, N)
            for entry in ("gmz_conv3x3_forward_stats", "gmz_conv3x3_forward_board_stats"):
                y, st = forward(entry, dt, H, x, packed, N, mask=m, stats=True)
                name = tag + entry[12:] + " mask=" + kind
                assert_bits(name + " y", y.view(N, H * H, CC), want, TD[dt])
                check_stats(name, dt, H, N, st, want, m, entry.endswith("board_stats"))
        if H in AB_SIZES:
            rs = np.random.RandomState(N)
            actions = rs.randint(0, H * H, size=N).astype(np.int32)
            actions[:4] = [0, H - 1, H * H - H, H * H - 1][:min(4, N)]
            m = mask_of("ragged", N)
            w2 = R.round_to(pre + R.stamp_terms(actions, k["table"].astype(np.float64), H), dt)
            y, st = forward("gmz_conv3x3_forward_stamp", dt, H, x, packed, N, mask=m, stats=True,
                            actions=torch.from_numpy(actions).cuda(), table=table)
            assert_bits(tag + "forward_stamp y", y.view(N, H * H, CC), w2, TD[dt])
            check_stats(tag + "forward_stamp", dt, H, N, st, w2, m, False)
            y, st = forward("gmz_conv3x3_forward_stamp", dt, H, x, packed, N, actions=torch.from_numpy(actions).cuda(),
                            table=table)
            assert_bits(tag + "forward_stamp (no statistics) y", y.view(N, H * H, CC), w2, TD[dt])


@gpu
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", AB_SIZES)
def test_tier_b_forward_bwdstats(H, dt):
    """gmz_conv3x3_forward_bwdstats: y bitwise (with and without the addend), the BatchNorm backward sums within
    (n + 2) u sum|dz xhat| and n u sum|dz|, counts exact, for every mask kind and both relu settings."""
    _need_gpu()
    k = exact_case(H, dt, 1)
    packed = pack(torch.from_numpy(k["W"]).cuda(), dt, 1)
    rs = np.random.RandomState(H + dt)
    for N in SMALL_N:
        s = signs(N, N)[:, None, None]
        idx = np.arange(N) % KB
        x, pre, add = act_in(s * k["x"][idx], dt), s * k["pre"][idx] + 0.0, s * k["addend"][idx]
        bn_x = R.round_to(rs.randn(N, H * H, CC) * 2 + 0.5, dt)
        bn_y = R.round_to(np.maximum(rs.randn(N, H * H, CC), 0), dt)
        save = np.stack([rs.randn(CC) * 0.5 + 0.5, rs.uniform(0.3, 2, CC)]).astype(np.float32)
        for j, kind in enumerate(MASKS):
            relu, use_add = j % 2 == 0, j % 3 != 0
            m = mask_of(kind, N)
            want = R.round_to(pre + add if use_add else pre, dt)
            bn = dict(x=act_in(bn_x, dt), y=act_in(bn_y, dt), save=torch.from_numpy(save).cuda(), relu=relu)
            y, st = forward("gmz_conv3x3_forward_bwdstats", dt, H, x, packed, N, addend=act_in(add, dt) if use_add else None,
                            mask=m, stats=True, bn=bn)
            name = "H=%d N=%d bwdstats mask=%s" % (H, N, kind)
            assert_bits(name + " y", y.view(N, H * H, CC), want, TD[dt])
            live = R.live(m, N)
            dz, dzx = R.bwd_terms(want, bn_x, bn_y, save[0].astype(np.float64), save[1].astype(np.float64), relu)
            ref = R.bwd_stats(want, bn_x, bn_y, save[0].astype(np.float64), save[1].astype(np.float64), relu, m)
            assert np.array_equal(st[:, :, 2].sum(axis=1), ref[:, 2]), name + ": counts"
            n_add = lane_chain(H, N, st.shape[1])
            within(name + " sum dz", 0, st[:, :, 0].sum(axis=1), ref[:, 0], (n_add * U + 2.0 ** -50) * np.abs(dz[live]).sum(axis=(0, 1)))
            within(name + " sum dz xhat", 0, st[:, :, 1].sum(axis=1), ref[:, 1],
                   ((n_add + 2) * U + 2.0 ** -50) * np.abs(dzx[live]).sum(axis=(0, 1)))


@functools.lru_cache(maxsize=None)
def exact_wgrad_case(H):
    rs = np.random.RandomState(77 + H)
    x = rs.randint(-4, 5, size=(KB, H * H, CC)).astype(np.float64)
    dy = rs.randint(-4, 5, size=(KB, H * H, CC)).astype(np.float64)
    dwk = np.stack([R.wgrad(x[i:i + 1], dy[i:i + 1], H) for i in range(KB)])
    dw0 = rs.randint(-2 ** 20, 2 ** 20 + 1, size=(CC, CC, 3, 3)).astype(np.float64)
    return x, dy, dwk, dw0


def signed_boards(H, N, seed):
    """board n = (sx_n x_base[n % 8], sd_n dy_base[n % 8]); dW = sum_k (sum_{n = k mod 8} sx_n sd_n) dW_k"""
    x, dy, dwk, dw0 = exact_wgrad_case(H)
    sx, sd = signs(N, seed), signs(N, seed + 1)
    idx = np.arange(N) % KB
    coef = np.bincount(idx, weights=sx * sd, minlength=KB)
    dw = np.tensordot(coef, dwk, axes=1) + 0.0
    assert 16 * N * H * H + 2 ** 20 < 2 ** 24  # every partial sum of integers stays exact in f32
    return sx[:, None, None] * x[idx], sd[:, None, None] * dy[idx], dw, dw0


@gpu
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", SIZES)
def test_tier_b_wgrad_bitwise(H, dt):
    """gmz_conv3x3_wgrad on integer boards: dW is the integer result bit for bit, written and accumulated, into a
    contiguous, a channels-last and a sliced dW, at every N.  Strictly contains the weight-gradient half of
    test_conv_sizes_gpu.test_forward_input_grad_and_weight_grad (kept)."""
    _need_gpu()
    for N in SMALL_N + (wgrad_big_shapes(cus()) if H == 6 else []):
        x, dy, dw, dw0 = signed_boards(H, N, 3 * N)
        xd, dyd = act_in(x, dt), act_in(dy, dt)
        for layout in DW_LAYOUTS:
            for acc in (None, dw0):
                got = wgrad(dt, H, xd, dyd, N, layout, acc)
                assert_bits("H=%d N=%d %s accumulate=%d dW" % (H, N, layout, acc is not None), got,
                            dw if acc is None else dw + acc, torch.float32)


@gpu
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", SIZES)
def test_tier_b_wgrad_segments_bitwise(H, dt):
    """gmz_conv3x3_wgrad_segments against the MODEL (test_conv_sizes_gpu.test_multi_segment_weight_gradient compares
    the kernel with itself): 1, 2, 5, 8 segments of 1 and 3 boards, each its own allocation, listed in an order
    unlike the address order."""
    _need_gpu()
    for nseg in (1, 2, 5, 8):
        for nps in (1, 3):
            N = nseg * nps
            x, dy, dw, dw0 = signed_boards(H, N, 5 * N + nps)
            # 2 nseg separate allocations, sorted by address, dealt to the segments in reverse and interleaved order
            bufs = sorted((torch.empty(nps * H * H * CC, dtype=TD[dt], device="cuda") for _ in range(2 * nseg)),
                          key=lambda t: t.data_ptr())
            xs, dys = bufs[::-2], bufs[-2::-2]
            for g in range(nseg):
                xs[g].copy_(act_in(x[g * nps:(g + 1) * nps], dt).reshape(-1))
                dys[g].copy_(act_in(dy[g * nps:(g + 1) * nps], dt).reshape(-1))
            ptrs = [t.data_ptr() for t in xs]
            assert len(set(ptrs)) == nseg and (nseg == 1 or ptrs != sorted(ptrs)) and all(p % 16 == 0 for p in ptrs)
            for layout, acc in (("contiguous", None), ("slice144", dw0), ("channels_last", dw0 if nps == 1 else None)):
                got = wgrad_segments(dt, H, xs, dys, nps, layout, acc)
                assert_bits("H=%d nseg=%d nps=%d %s dW" % (H, nseg, nps, layout), got, dw if acc is None else dw + acc,
                            torch.float32)


# ------------------------------------------------------------------------------------------------ Tier C: real data
@functools.lru_cache(maxsize=None)
def real_case(H, dt):
    rs = np.random.RandomState(500 + H + dt)
    scale = 10.0 ** rs.uniform(-1, 1, CC)
    x = R.round_to(np.maximum(rs.randn(KB, H * H, CC), 0) * scale[None, None, :], dt)
    dy = R.round_to(rs.randn(KB, H * H, CC) * 1e-3, dt)
    W = (rs.randn(CC, CC, 3, 3) / 34).astype(np.float32)
    Wq = [R.round_to(R.w_eff(W.astype(np.float64), tr), dt) for tr in (0, 1)]
    assert 0.4 <= (x == 0).mean() <= 0.6
    return dict(x=x, dy=dy, W=W, Wq=Wq, y=R.conv(x, Wq[0], H), ya=R.abs_conv(x, Wq[0], H), dx=R.conv(dy, Wq[1], H),
                dxa=R.abs_conv(dy, Wq[1], H), dwk=np.stack([R.wgrad(x[i:i + 1], dy[i:i + 1], H) for i in range(KB)]),
                dwa=np.stack([R.wgrad(np.abs(x[i:i + 1]), np.abs(dy[i:i + 1]), H) for i in range(KB)]))


def store_bound(D, y, dt):
    return D + UT[dt] * (np.abs(y) + D) + TINY[dt]


def real_shapes(H):
    return [5] + (stride_shapes(cus()) if H == 6 else [])


@gpu
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", SIZES)
def test_tier_c_forward_and_input_gradient_within_derived_bound(H, dt):
    """relu(randn) activations with per-channel scales over two decades, randn / 34 weights, randn * 1e-3 gradients:
    y, y + addend and dx within the bound of the module docstring, element by element."""
    _need_gpu()
    k = real_case(H, dt)
    w = torch.from_numpy(k["W"]).cuda()
    pk = [pack(w, dt, 0), pack(w, dt, 1)]
    for N in real_shapes(H):
        s = signs(N, 7 * N)[:, None, None]
        idx = np.arange(N) % KB
        y, _ = forward("gmz_conv3x3_forward", dt, H, act_in(s * k["x"][idx], dt), pk[0], N)
        yw, ya = s * k["y"][idx], k["ya"][idx]
        within("forward y", dt, y.double().cpu().numpy().reshape(yw.shape), yw, store_bound(1152 * E_MFMA * ya, yw, dt))
        y, _ = forward("gmz_conv3x3_forward", dt, H, act_in(s * k["dy"][idx], dt), pk[1], N)
        dw_, da = s * k["dx"][idx], k["dxa"][idx]
        within("input gradient dx", dt, y.double().cpu().numpy().reshape(dw_.shape), dw_, store_bound(1152 * E_MFMA * da, dw_, dt))
        add = s * k["x"][(idx + 1) % KB]  # an addend of the activations' size: the residual path's gradient
        y, _ = forward("gmz_conv3x3_forward_add", dt, H, act_in(s * k["x"][idx], dt), pk[0], N, addend=act_in(add, dt))
        within("forward_add y", dt, y.double().cpu().numpy().reshape(yw.shape), yw + add,
               store_bound(1153 * E_MFMA * (ya + np.abs(add)), yw + add, dt))


@gpu
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", SIZES)
def test_tier_c_weight_gradient_within_derived_bound(H, dt):
    _need_gpu()
    k = real_case(H, dt)
    for N in real_shapes(H):
        sx, sd = signs(N, N), signs(N, N + 1)
        idx = np.arange(N) % KB
        dw = np.tensordot(np.bincount(idx, weights=sx * sd, minlength=KB), k["dwk"], axes=1)
        dwa = np.tensordot(np.bincount(idx, minlength=KB).astype(np.float64), k["dwa"], axes=1)
        got = wgrad(dt, H, act_in(sx[:, None, None] * k["x"][idx], dt), act_in(sd[:, None, None] * k["dy"][idx], dt), N,
                    "contiguous")
        K = N * H * H + chunks_rule(N, cus())
        within("dW", dt, got.double().cpu().numpy(), dw, store_bound(K * E_MFMA * dwa, dw, 0))


@gpu
@pytest.mark.parametrize("dt", [1, 2])
def test_tier_c_forward_bnapply(dt):
    """gmz_conv3x3_forward_bnapply (its bit-identity with BatchNorm-then-conv: test_bn_apply_gpu.py): bn_y against
    bn_ref's apply within the elementwise bound of test_bn_kernels_gpu.py (mean and invstd are inputs here: only
    sc = gamma invstd is rounded), y against the model's conv of the MODEL's rounded bn_y, the bound widened by what
    bn_y's own bound lets through the weights: sum|W| dbn_y."""
    _need_gpu()
    L = _lib()
    H, N = 9, 5
    rs = np.random.RandomState(40 + dt)
    z = R.round_to(rs.randn(N, H * H, CC) * 2 + 0.5, dt)
    res = R.round_to(rs.randn(N, H * H, CC), dt)
    gamma, beta = rs.uniform(0.5, 1.5, CC).astype(np.float32), rs.uniform(-0.3, 0.3, CC).astype(np.float32)
    save = np.stack([rs.randn(CC) * 0.3 + 0.5, rs.uniform(0.3, 1.0, CC)]).astype(np.float32)
    W = (rs.randn(CC, CC, 3, 3) / 34).astype(np.float32)
    Wq = R.round_to(W.astype(np.float64), dt)
    g64, b64, mean, invstd = (a.astype(np.float64) for a in (gamma, beta, save[0], save[1]))
    t = lambda a: a.transpose(0, 2, 1)  # noqa: E731  (bn_ref: [B][C][S])
    _, bny = bn_ref.apply(t(z), mean, invstd, g64, b64, t(res), True)
    bny = t(bny)
    sc = np.abs(g64 * invstd)[None, None, :]
    d = np.abs(z - mean[None, None, :])
    D = d * U * sc + 4 * U * (d * sc + np.abs(b64)[None, None, :] + np.abs(res))
    bny_bound = store_bound(D, bny, dt)
    bny_q = R.round_to(bny, dt)
    yw = R.conv(bny_q, Wq, H)
    y_bound = store_bound(1152 * E_MFMA * R.abs_conv(bny_q, Wq, H) + R.conv(bny_bound, np.abs(Wq), H), yw, dt)
    packed = pack(torch.from_numpy(W).cuda(), dt, 0)
    (br, by), (yr, y) = act_out(N, H, dt), act_out(N, H, dt)
    slots = L.query("gmz_conv3x3_stats_slots", N, ctype=ctypes.c_int)
    sr = stats_region(slots)
    m = mask_of("ragged", N)
    L.call("gmz_conv3x3_forward_bnapply", dt, H, act_in(z, dt), act_in(res, dt), torch.from_numpy(gamma).cuda(),
           torch.from_numpy(beta).cuda(), torch.from_numpy(save).cuda(), 1, by, packed, y, N, torch.from_numpy(m).cuda(),
           sr[1], slots, L.stream_ptr())
    torch.cuda.synchronize()
    assert br.intact() and yr.intact()
    within("bnapply bn_y", dt, by.double().cpu().numpy().reshape(bny.shape), bny, bny_bound)
    yg = y.double().cpu().numpy().reshape(yw.shape)
    within("bnapply y", dt, yg, yw, y_bound)
    st = read_stats(sr, slots)
    assert np.array_equal(st[:, :, 2].sum(axis=1), np.full(CC, float(m.astype(bool).sum() * H * H)))
    # the statistics are those of the y the kernel stored
    yq = R.round_to(yg, dt)
    ref = R.stats(yq, m)
    r = lane_chain(H, N, slots) * U + 2.0 ** -50
    within("bnapply sum", 0, st[:, :, 0].sum(axis=1), ref[:, 0], r * np.abs(yq[R.live(m, N)]).sum(axis=(0, 1)))
    within("bnapply sumsq", 0, st[:, :, 1].sum(axis=1), ref[:, 1], r * ref[:, 1])


# ------------------------------------------------------------------------------------------------ refusals (CPU)
FAKE = 1 << 20


def _refused(rc, text):
    msg = _lib().load().gmz_last_error().decode()
    assert rc < 0 and text in msg, (rc, msg, text)


def _entry_calls(lib, dt, H, p=FAKE, N=4, slots=None, ws=None, ptrs=None):
    """{entry point: a call with fake pointers (never dereferenced: each must stop at a check)}.  ``ptrs`` overrides
    single operands by name."""
    ns = ctypes.c_int()
    assert lib.gmz_conv3x3_stats_slots(N, ctypes.byref(ns)) == 0
    need = ctypes.c_size_t()
    assert lib.gmz_conv3x3_wgrad_workspace_bytes(N, ctypes.byref(need)) == 0
    sl = ns.value if slots is None else slots
    wsb = need.value if ws is None else ws
    q = dict(x=p, pk=p + 4096, y=p + 8192, add=p + 12288, bnx=p + 16384, bny=p + 20480, st=p + 24576, dw=p + 28672,
             dy=p + 32768, ws=p + 36864, res=p + 40960)
    q.update(ptrs or {})
    v = {k_: ctypes.c_void_p(a) for k_, a in q.items()}
    segs = (ctypes.c_void_p * 2)(q["x"], q["x"] + 65536)
    dsegs = (ctypes.c_void_p * 2)(q["dy"], q["dy"] + 65536)
    return {
        "gmz_conv3x3_forward": lambda: lib.gmz_conv3x3_forward(dt, H, v["x"], v["pk"], v["y"], N, None),
        "gmz_conv3x3_forward_add": lambda: lib.gmz_conv3x3_forward_add(dt, H, v["x"], v["pk"], v["add"], v["y"], N, None),
        "gmz_conv3x3_forward_stats": lambda: lib.gmz_conv3x3_forward_stats(dt, H, v["x"], v["pk"], v["y"], N, None, v["st"], sl,
                                                                           None),
        "gmz_conv3x3_forward_board_stats": lambda: lib.gmz_conv3x3_forward_board_stats(
            dt, H, v["x"], v["pk"], v["y"], N, None, v["st"], N if slots is None else slots, None),
        "gmz_conv3x3_forward_stamp": lambda: lib.gmz_conv3x3_forward_stamp(dt, H, v["x"], v["pk"], v["y"], N, None, v["st"], sl,
                                                                           v["bnx"], v["bny"], 0, 4608, None),
        "gmz_conv3x3_forward_bwdstats": lambda: lib.gmz_conv3x3_forward_bwdstats(
            dt, H, v["x"], v["pk"], v["add"], v["y"], N, None, v["bnx"], v["bny"], v["res"], 1, v["st"], sl, None),
        "gmz_conv3x3_forward_bnapply": lambda: lib.gmz_conv3x3_forward_bnapply(
            dt, H, v["bnx"], v["res"], v["ws"], v["ws"], v["ws"], 1, v["bny"], v["pk"], v["y"], N, None, v["st"], sl, None),
        "gmz_conv3x3_wgrad": lambda: lib.gmz_conv3x3_wgrad(dt, H, v["x"], v["dy"], N, v["dw"], 1152, 9, 3, 1, 0, v["ws"], wsb,
                                                           None),
        "gmz_conv3x3_wgrad_segments": lambda: lib.gmz_conv3x3_wgrad_segments(dt, H, segs, dsegs, 2, N // 2, v["dw"], 1152, 9, 3,
                                                                             1, 0, v["ws"], wsb, None),
    }


AB_ENTRIES = ("gmz_conv3x3_forward_stamp", "gmz_conv3x3_forward_bwdstats")


def test_refusals_before_any_launch():
    """Fake pointers, no GPU needed (but a built libgmz.so, as tests/test_abi.py: the library is loaded, not built,
    here): every refusal returns < 0 with the documented text before anything is launched
    (beside the capacity refusals of tests/test_abi.py)."""
    lib = _lib().load()
    for dt in (1, 2):
        for H in (5, 7, 16, 20):
            for name, f in _entry_calls(lib, dt, H).items():
                _refused(f(), "board size must be 6, 9, 15 or 19")
        for H in (6, 19):  # the two off-by-default A/B entry points are built for 9 and 15 only
            for name in AB_ENTRIES:
                _refused(_entry_calls(lib, dt, H)[name](), "board sizes 9 and 15 only")
    for dt in (0, 3):
        for name, f in _entry_calls(lib, dt, 9).items():
            _refused(f(), "dtype must be 1 (f16) or 2 (bf16)")
        _refused(lib.gmz_conv3x3_pack(dt, ctypes.c_void_p(FAKE), 1152, 9, 3, 1, 0, ctypes.c_void_p(FAKE + 4096), None),
                 "dtype must be 1 (f16) or 2 (bf16)")
        _refused(lib.gmz_conv3x3_pack_many(dt, ctypes.c_void_p(FAKE), 2, None), "dtype must be 1 (f16) or 2 (bf16)")
    # operands 8 bytes off the 16-byte grid, one at a time
    mis = {"gmz_conv3x3_forward": "x pk y", "gmz_conv3x3_forward_add": "x pk y add", "gmz_conv3x3_forward_stats": "x pk y",
           "gmz_conv3x3_forward_board_stats": "x pk y", "gmz_conv3x3_forward_stamp": "x pk y",
           "gmz_conv3x3_forward_bwdstats": "x pk y add", "gmz_conv3x3_forward_bnapply": "bnx res bny pk y",
           "gmz_conv3x3_wgrad": "x dy", "gmz_conv3x3_wgrad_segments": "x dy"}
    base = _entry_calls(lib, 1, 9)
    assert set(mis) == set(base)
    q0 = dict(x=FAKE, pk=FAKE + 4096, y=FAKE + 8192, add=FAKE + 12288, bnx=FAKE + 16384, bny=FAKE + 20480, dy=FAKE + 32768,
              res=FAKE + 40960)
    for name, ops in mis.items():
        for op in ops.split():
            _refused(_entry_calls(lib, 1, 9, ptrs={op: q0[op] + 8})[name](), "16-B aligned")
    for op in ("bnx", "bny"):  # the BatchNorm operands of the backward-statistics variant: 8-byte alignment
        _refused(_entry_calls(lib, 1, 9, ptrs={op: q0[op] + 4})["gmz_conv3x3_forward_bwdstats"](), "8-B aligned")
    _refused(lib.gmz_conv3x3_pack(1, ctypes.c_void_p(FAKE), 1152, 9, 3, 1, 0, ctypes.c_void_p(FAKE + 4096 + 8), None),
             "16-B aligned")
    # a workspace one byte short; a wrong slot count
    need = ctypes.c_size_t()
    for N in (4, 10, 360):
        assert lib.gmz_conv3x3_wgrad_workspace_bytes(N, ctypes.byref(need)) == 0
        for name in ("gmz_conv3x3_wgrad", "gmz_conv3x3_wgrad_segments"):
            _refused(_entry_calls(lib, 1, 9, N=N, ws=need.value - 1)[name](), "workspace of %d bytes" % (need.value - 1))
    ns = ctypes.c_int()
    assert lib.gmz_conv3x3_stats_slots(4, ctypes.byref(ns)) == 0
    for bad in (ns.value - 1, ns.value + 1):
        for name in ("gmz_conv3x3_forward_stats", "gmz_conv3x3_forward_stamp", "gmz_conv3x3_forward_bwdstats",
                     "gmz_conv3x3_forward_bnapply"):
            _refused(_entry_calls(lib, 1, 9, slots=bad)[name](), "statistics buffer of %d slots" % bad)
    for bad in (3, 5, ns.value if ns.value != 4 else 8):
        _refused(_entry_calls(lib, 1, 9, slots=bad)["gmz_conv3x3_forward_board_stats"](), "one per board")


def test_every_f16_bf16_conv_entry_point_is_called_here():
    hdr = open(os.path.join(REPO, "include", "gmz.h")).read()
    names = set(re.findall(r"^int\s+(gmz_conv3x3_\w+)\(", hdr, re.M))
    names = set(n for n in names if "split" not in n)  # the float32 sibling: tests/test_conv_split_gpu.py
    assert len(names) >= 14
    src = open(os.path.abspath(__file__)).read()
    assert not [n for n in names if '"%s"' % n not in src and "lib.%s(" % n not in src]
