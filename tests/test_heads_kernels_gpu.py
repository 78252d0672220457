"""Every entry point of csrc/gmz_heads.hip (gmz_head_conv1x1_forward / _backward, gmz_seg_bn_forward / _backward and
their _small forms, the two *_workspace_bytes queries) against tests/heads_ref.py, the float64 model of what
include/gmz.h documents, element by element, through raw ``_lib.call``.

Rules (those of tests/test_bn_kernels_gpu.py and tests/test_conv_kernels_gpu.py)
  * every output is NaN-filled between NaN guards (dW, db, dgamma, dbeta too unless accumulating) and must be finite
    afterwards with the guards still NaN;
  * every workspace is exactly the bytes the library names, between byte sentinels that must survive, and starts as
    NaN; the stats buffer is exactly (3 nseg C + nseg) f32 between NaN guards;
  * the backwards run on the MODEL's statistics (rounded to f32), never on the forward kernel's output;
  * the bounds are per element, first order in u = 2^-24, from unit roundoffs, the summation lengths of the public
    launch rules and the model's magnitudes.  No constant was chosen by looking at the kernels' error.  The largest
    error / bound ratios and the mutants these tests catch are in profiles/heads_opt_kernel_tests.txt.

Head conv, bitwise tier.  x, dy = k / 8 with |k| <= 16, W = j / 16 with |j| <= 16, b = i / 128 with |i| <= 127, all
representable in f16 and bf16.  Every product is a multiple of q = 2^-7 (forward, dx) or 2^-6 (dW, db), and the
model asserts sum|terms| / q < 2^24: every partial sum, in ANY order, is then an integer below 2^24 times q, hence
exact in f32.  So y and dx must equal round_T(exact) and dW, db the exact sums, bit for bit.  The model also asserts
that some y land exactly on a rounding tie and that for some y round_T(round_T(sum) + b) != round_T(sum + b).

Head conv, bound tier (production-like random data).  uT = 2^-24 / 2^-11 / 2^-8: the store; tT: half the smallest
subnormal of the storage type.
  y         8 fused multiply-adds a thread, 4 shuffle adds, the bias add: D = 13u (sum_c |x W| + |b|);
            |y - exact| <= D + uT (|exact| + D) + tT, against the model's value BEFORE its rounding
  dx        at most 4 fused multiply-adds: D = 4u sum_o |dy W|, then the store as above
  dW, db    nb = min(ceil(P / 16), 512) workgroups; a thread adds L = ceil(P / (16 nb)) terms in sequence, the 16
            position groups are added in sequence, then the nb partials: ceil(nb / 256) in sequence and an 8-level
            tree.  (L + 16 + ceil(nb / 256) + 8) u sum_p |terms|, + u |result| (the accumulate add)

Segmented BatchNorm.  All sums are f64: r = (N + 4) 2^-53 with N = B S elements of a segment.
  mean      f32 input: u |mean| + r E|x|.  f16 input: the f64 sum of multiples of 2^-24 is exact in any order, so
            mean must BE float32(sum / n), bit for bit (asserted so)
  var       general (two passes, deviations from the f64 mean): r var — no cancellation.
            small (E[x^2] - mean^2): r (E[x^2] + 2 |mean| E|x| + mean^2) — carries E[x^2] / var
  invstd    1 / sqrt(var + eps) in f64, one rounding: invstd (dvar / (2 (var + eps)) + u + 2^-51)
  unb       dvar n / (n - 1) + (u + 2^-51) unb;  live rows: exact
  y         ((x - mean) invstd) gamma + beta in f32, 4 roundings:
            D = dmean |sc| + |x - mean| |gamma| dinvstd + 4u (|x - mean| |sc| + |beta|), sc = gamma invstd; + 2^-149
  running   each update rm (1 - m) + m mean with (1 - m) rounded: the error e becomes
            (1 - m) e + m dmean + 4u (|(1 - m) rm| + |m mean|), replayed over the model's update sequence
  G1, G2    xhat = (x - mean) invstd in f32 (2u): dG1 = r sum|dy|, dG2 = (2u + r) sum|dy xhat|
  c1, c2    G / n rounded to f32: dc = dG / n + u |c|
  dx        k1 (dy - w (c1 + xhat c2)), k1 = gamma invstd, at most 6 roundings touch a term:
            live rows D = |k1| (dc1 + |xhat| dc2 + 6u (|dy| + |c1| + |xhat c2|)), others D = 3u |k1 dy|;
            |ddx| <= D + uT (|dx| + D) + tT
  dgamma    sum_s dG2 + u |sum| (+ u |result| when accumulating); dbeta likewise with G1
"""
import functools
import json
import os
import re
import zlib

import numpy as np
import pytest
import torch

import conv_ref
import heads_ref as R
from conftest import REPO
from kernel_guards import DN, TD, TINY, U, UT, Buf, Workspace, f32_in, lib, need_gpu, same, within as _within

gpu = pytest.mark.gpu
EPS, MOM = float(np.float32(1e-4)), float(np.float32(0.1))  # what the C float arguments hold
NB0 = 5
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_report():
    yield
    path = os.environ.get("GMZ_HEADS_RATIOS")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(dict(sorted(RATIOS.items())), f, indent=1)


def within(name, dt, got, want, bound):
    _within(RATIOS, name, dt, got, want, bound)


def test_every_header_entry_point_is_called_here():
    hdr = open(os.path.join(REPO, "include", "gmz.h")).read()
    names = set(re.findall(r"^int\s+(gmz_(?:head_conv1x1|seg_bn)_\w+)\(", hdr, re.M))
    assert len(names) == 8
    src = open(os.path.abspath(__file__)).read()
    assert not [n for n in names if '"%s"' % n not in src]


def f32_bits_equal(buf, want):
    """A device f32 buffer equals float32(want) bit for bit."""
    return same(buf.t, torch.from_numpy(np.ascontiguousarray(want, np.float64).astype(np.float32).ravel()).cuda())


# ================================================================================================ head conv
# (P, O0, O1, bias, accumulate, NULL destination, operands one element off the 16-byte grid)
def _h(P, O0, O1, bias=True, acc=False, null=None, mis=False):
    return (P, O0, O1, bias, acc, null, mis)


HEAD = [
    _h(225, 1, 0), _h(225, 2, 0, bias=False, acc=True), _h(225, 2, 1, acc=True), _h(225, 1, 3, bias=False), _h(225, 2, 2),
    _h(1, 2, 1), _h(15, 1, 3, acc=True), _h(16, 2, 2, bias=False), _h(17, 2, 0), _h(17, 1, 0, bias=False, acc=True),
    _h(8193, 2, 1), _h(8193, 2, 1, acc=True),  # one position past 512 workgroups x 16 in the backward
    _h(17, 2, 1, null="dw0"), _h(17, 2, 1, null="db0", acc=True), _h(17, 2, 1, null="dw1"), _h(17, 2, 1, null="db1", acc=True),
    _h(225, 2, 1, mis=True), _h(225, 1, 3, bias=False, mis=True),
]
HEAD_ALL = [(d, c) for c in HEAD for d in (0, 1, 2)]
HEAD_IDS = ["%s-P%d-O%d+%d%s%s%s%s" % (DN[d], c[0], c[1], c[2], "" if c[3] else "-nobias", "-acc" if c[4] else "",
                                      "-null_" + c[5] if c[5] else "", "-mis" if c[6] else "") for d, c in HEAD_ALL]
BIG_P = 262144 + 17  # past the forward's grid cap of 4,096 workgroups x 64 positions


def head_blocks(P):
    return min(-(-P // 16), 512)


CACHE_ELEMS = 100000  # cases above this many elements are rebuilt by each test that needs them, not kept resident


def head_case(dt, spec, tier):
    """Inputs as stored and the model's results; tier "bits": provably exact f32 accumulation, "bound": random.
    Built once and shared, unchanged, except the large cases (at most two tests use each)."""
    return (_head_case_cached if spec[0] * 128 <= CACHE_ELEMS else _head_case)(dt, spec, tier)


def _head_case(dt, spec, tier):
    P, O0, O1, bias, acc, null, mis = spec
    O = O0 + O1
    rs = np.random.RandomState(zlib.crc32(repr((dt, spec, tier)).encode()))
    if tier == "bits":
        x = rs.randint(-16, 17, (P, 128)).astype(np.int8).astype(np.float64) / 8
        dy = rs.randint(-16, 17, (P, O)).astype(np.float64) / 8
        W = rs.randint(-16, 17, (O, 128)).astype(np.float64) / 16
        b = rs.randint(-127, 128, O).astype(np.float64) / 128
        dW0, db0 = rs.randint(-64, 65, (O, 128)).astype(np.float64) / 64, rs.randint(-64, 65, O).astype(np.float64) / 64
    else:
        x = R.round_to(np.maximum(rs.randn(P, 128), 0) * 1.5, dt)  # a hidden state after its ReLU
        dy = R.round_to(rs.randn(P, O) * 0.1, dt)
        W, b = rs.randn(O, 128) * 0.1, rs.randn(O) * 0.5
        dW0, db0 = rs.randn(O, 128), rs.randn(O)
    W, b, dW0, db0 = (a.astype(np.float32).astype(np.float64) for a in (W, b, dW0, db0))
    w1 = W[O0:] if O1 else None
    f = R.head_forward(x, W[:O0], b[:O0] if bias else None, w1, b[O0:] if bias and O1 else None, dt)
    bw = R.head_backward(x, dy, W[:O0], w1, dt, (dW0, db0) if acc else None) if P < BIG_P else None
    if tier == "bits":
        for a, q in ((x, 8), (dy, 8), (W, 16), (b, 128), (dW0, 64), (db0, 64)):
            assert np.array_equal(a * q, np.rint(a * q)) and np.array_equal(R.round_to(a, dt), a)
        assert f["sabs"].max() * 128 < 2 ** 24
        if bw:
            assert bw["sabs_dx"].max() * 128 < 2 ** 24
            assert (bw["sabs_dW"].max() + np.abs(dW0).max()) * 64 < 2 ** 24 and (bw["sabs_db"].max() + 2) * 64 < 2 ** 24
    return dict(spec=spec, dt=dt, x=x, dy=dy, W=W, b=b, dW0=dW0, db0=db0, f=f, bw=bw)


_head_case_cached = functools.lru_cache(maxsize=None)(_head_case)


def _ties_and_double_rounding(k):
    """(elements of y exactly on a tie, elements where rounding the sum and then adding the bias differs)."""
    dt, f = k["dt"], k["f"]
    two = R.round_to(R.round_to(f["exact"] - f["b"], dt) + f["b"], dt)
    return int(conv_ref.is_tie(f["exact"], dt).sum()), int((two != f["y"]).sum())


def test_bitwise_head_data_has_ties_and_a_telling_bias():
    """CPU: the conditions on the model alone."""
    for dt in (1, 2):
        ties, twice = _ties_and_double_rounding(head_case(dt, _h(225, 2, 1, acc=True), "bits"))
        assert ties >= 5 and twice >= 5, (dt, ties, twice)


def head_forward_run(k):
    L = lib()
    P, O0, O1, bias, acc, null, mis = k["spec"]
    dt, off = k["dt"], int(k["spec"][6])
    x = Buf(P * 128, TD[dt], fill=0.0, data=k["x"])
    y0, y1 = Buf(P * O0, TD[dt], off), (Buf(P * O1, TD[dt], off) if O1 else None)
    if mis:
        assert y0.t.data_ptr() % 16 and y0.t.data_ptr() % 2 == 0
    W, b = k["W"], k["b"]
    L.call("gmz_head_conv1x1_forward", dt, x.t, P, 128, f32_in(W[:O0]), f32_in(b[:O0]) if bias else None, O0,
           f32_in(W[O0:]) if O1 else None, f32_in(b[O0:]) if bias and O1 else None, O1, y0.t, y1.t if O1 else None,
           L.stream_ptr())
    torch.cuda.synchronize()
    assert y0.intact() and (y1 is None or y1.intact()) and x.intact()
    got = np.concatenate([y0.f64().reshape(P, O0)] + ([y1.f64().reshape(P, O1)] if O1 else []), axis=1)
    assert np.isfinite(got).all()
    return got


def head_backward_run(k):
    L = lib()
    P, O0, O1, bias, acc, null, mis = k["spec"]
    dt, O, off = k["dt"], O0 + O1, int(k["spec"][6])
    x = Buf(P * 128, TD[dt], fill=0.0, data=k["x"])
    dy0 = Buf(P * O0, TD[dt], off, fill=0.0, data=k["dy"][:, :O0])
    dy1 = Buf(P * O1, TD[dt], off, fill=0.0, data=k["dy"][:, O0:]) if O1 else None
    dx = Buf(P * 128, TD[dt])
    init = (lambda a: a) if acc else (lambda a: None)
    dst = dict(dw0=Buf(O0 * 128, torch.float32, data=init(k["dW0"][:O0])), db0=Buf(O0, torch.float32, data=init(k["db0"][:O0])),
               dw1=Buf(O1 * 128, torch.float32, data=init(k["dW0"][O0:])) if O1 else None,
               db1=Buf(O1, torch.float32, data=init(k["db0"][O0:])) if O1 else None)
    if null:
        dst[null] = None
    nbytes = L.query("gmz_head_conv1x1_workspace_bytes", P, O)
    assert nbytes == head_blocks(P) * O * 129 * 4
    ws = Workspace(nbytes)
    p = lambda b: b.t if b is not None else None
    L.call("gmz_head_conv1x1_backward", dt, x.t, P, 128, f32_in(k["W"][:O0]), O0, f32_in(k["W"][O0:]) if O1 else None, O1,
           dy0.t, p(dy1), dx.t, p(dst["dw0"]), p(dst["db0"]), p(dst["dw1"]), p(dst["db1"]), int(acc), ws.t, ws.nbytes,
           L.stream_ptr())
    torch.cuda.synchronize()
    assert ws.intact() and dx.intact() and all(b.intact() for b in dst.values() if b is not None)
    return dx, dst


def _dst_parts(k, dst, bw):
    """(name, device buffer, model value, sum|terms|) of each non-NULL destination."""
    O0 = k["spec"][1]
    out = [("dw0", bw["dW"][:O0], bw["sabs_dW"][:O0]), ("db0", bw["db"][:O0], bw["sabs_db"][:O0]),
           ("dw1", bw["dW"][O0:], bw["sabs_dW"][O0:]), ("db1", bw["db"][O0:], bw["sabs_db"][O0:])]
    return [(n, dst[n], w, s) for n, w, s in out if dst.get(n) is not None]


@gpu
@pytest.mark.parametrize("dt,spec", HEAD_ALL, ids=HEAD_IDS)
def test_head_conv_bitwise(dt, spec):
    """Exact f32 accumulation: y and dx are round_T(exact), dW and db the exact sums, bit for bit."""
    need_gpu()
    k = head_case(dt, spec, "bits")
    P, O0, O1, bias, acc, null, mis = spec
    got = head_forward_run(k)
    bad = np.flatnonzero(got.ravel() != k["f"]["y"].ravel())
    assert not bad.size, "y: %d wrong, first at %d: got %r, want %r (exact %r)" % (
        bad.size, bad[0], got.ravel()[bad[0]], k["f"]["y"].ravel()[bad[0]], k["f"]["exact"].ravel()[bad[0]])
    dx, dst = head_backward_run(k)
    bw = k["bw"]
    assert np.array_equal(dx.f64().reshape(P, 128), bw["dx"])
    for name, buf, want, _ in _dst_parts(k, dst, bw):
        assert f32_bits_equal(buf, want), name


@gpu
@pytest.mark.parametrize("dt,spec", HEAD_ALL, ids=HEAD_IDS)
def test_head_conv_within_bounds(dt, spec):
    """Production-like data against the derived per-element bounds.  At P = 8,193, with accumulate off and on, the
    backward runs twice on this order-sensitive data and dx and every destination must be bit-identical: the fixed
    reduction order the header promises (the bitwise tier cannot show it: its sums are exact in any order)."""
    need_gpu()
    k = head_case(dt, spec, "bound")
    P, O0, O1, bias, acc, null, mis = spec
    f, bw = k["f"], k["bw"]
    D = 13 * U * f["sabs"]
    # against the value BEFORE the model's own rounding: against round_T(exact) a correct kernel may be a whole ulp off
    within("head y", dt, head_forward_run(k), f["exact"], D + UT[dt] * (np.abs(f["exact"]) + D) + TINY[dt])
    dx, dst = head_backward_run(k)
    D = 4 * U * bw["sabs_dx"]
    within("head dx", dt, dx.f64().reshape(P, 128), bw["dx_exact"], D + UT[dt] * (np.abs(bw["dx_exact"]) + D) + TINY[dt])
    nb = head_blocks(P)
    depth = -(-P // (16 * nb)) + 16 + -(-nb // 256) + 8
    for name, buf, want, sabs in _dst_parts(k, dst, bw):
        within("head " + name[:2], dt, buf.f64().reshape(want.shape), want, depth * U * sabs + U * np.abs(want) + 2.0 ** -149)
    if P == 8193:  # order-sensitive data, all 512 workgroup partials: a second run must give the same bits
        dx2, dst2 = head_backward_run(k)
        assert same(dx.t, dx2.t), "dx differs between two runs"
        for n in dst:
            assert dst[n] is None or same(dst[n].t, dst2[n].t), "%s differs between two runs" % n


@gpu
def test_head_conv_forward_past_the_grid_cap():
    """P = 262,144 + 17 at f16 (64 MB of x): workgroups take a second step of 4,096 x 16 positions; bitwise."""
    need_gpu()
    k = head_case(1, _h(BIG_P, 2, 1), "bits")
    got = head_forward_run(k)
    assert np.array_equal(got, k["f"]["y"])


# ================================================================================================ segmented BatchNorm
# (nseg, B, S, C, mask, update, pre_stats, gamma/beta, num_batches, accumulate, dgamma/dbeta, offset data)
def _s(nseg, B, S, C, mask="ragged", update=True, pre=False, affine=True, nb=True, acc=False, dpar=True, offset=False):
    return (nseg, B, S, C, mask, update, pre, affine, nb, acc, dpar, offset)


SEG = [
    _s(1, 7, 1, 1, "null"), _s(6, 9, 25, 2, pre=True), _s(32, 3, 1, 3, "only_last", acc=True),
    _s(32, 2, 25, 8, "dead_mid", pre=True, nb=False), _s(6, 5, 225, 2, "dead_first", affine=False),
    _s(3, 2047, 1, 2, "dead_mid", update=False, dpar=False), _s(3, 2049, 1, 3, "dead_last", pre=True, acc=True),
    _s(2, 4097, 1, 1),  # K = 2, chunks of 2,048 and 2,049
    _s(2, 5, 1, 2, "one"), _s(2, 5, 25, 3, "one", pre=True), _s(3, 4, 5, 2, "zeros"), _s(3, 4, 5, 8, "zeros", pre=True),
    _s(6, 9, 25, 9, pre=True), _s(2, 5, 1, 512, acc=True), _s(6, 4, 1, 9, "dead_first", affine=False, nb=False),
]
SEG_LARGE = [
    _s(2, 360, 225, 2, "null"),  # B S = 81,000: K = 39
    _s(2, 131075, 1, 8),  # K at its cap of 64 with C = 8: the backward's partials end where its coefficients begin
]
SEG_ALL = [(d, c) for c in SEG + SEG_LARGE for d in (0, 1, 2)] + [
    (1, _s(2, 37, 36, 2, offset=True)),  # f16, mean 8, std 0.5
    (1, _s(2, 9325, 225, 1, "null", update=False)),  # 4,196,250 elements: past the elementwise grid's 4,096 x 1,024
]
SEG_IDS = ["%s-n%dB%dS%dC%d-%s%s%s%s%s%s%s%s" % (
    DN[d], c[0], c[1], c[2], c[3], c[4], "" if c[5] else "-noupd", "-pre" if c[6] else "", "" if c[7] else "-noaffine",
    "" if c[8] else "-nonb", "-acc" if c[9] else "", "" if c[10] else "-nodpar", "-offset" if c[11] else "")
    for d, c in SEG_ALL]


def seg_mask(kind, nseg, B, rs):
    if kind == "null":
        return None
    R_ = nseg * B
    m = (rs.rand(R_) < 0.6).astype(np.uint8)
    j = rs.randint(B)
    m[j + B * np.arange(nseg)] = 1  # a live row in every segment
    if B > 1:
        m[(j + 1) % B] = 0  # and a row outside the mask in the first
    dead = {"dead_first": 0, "dead_mid": nseg // 2, "dead_last": nseg - 1}.get(kind)
    if dead is not None:
        m[dead * B:(dead + 1) * B] = 0
    elif kind == "only_last":
        m[:(nseg - 1) * B] = 0
    elif kind == "one":  # exactly one live row in segment 0
        m[:B] = 0
        m[B // 2] = 1
    elif kind == "zeros":
        m[:] = 0
    return m


def seg_case(dt, spec):
    """Inputs as stored, the model's forward, the backward on the model's f32 statistics.  Built once and shared,
    unchanged, except the large cases (the forward and the backward test each rebuild theirs)."""
    return (_seg_case_cached if spec[0] * spec[1] * spec[2] * spec[3] <= CACHE_ELEMS else _seg_case)(dt, spec)


def _seg_case(dt, spec):
    nseg, B, S, C, kind, update, pre, affine, nb, acc, dpar, offset = spec
    rs = np.random.RandomState(zlib.crc32(repr((dt,) + spec).encode()))
    Rw = nseg * B
    x = R.round_to(rs.randn(Rw, S, C) * 0.5 + 8.0 if offset else rs.randn(Rw, S, C) * 2 + 0.5, dt)
    dy = (rs.randn(Rw, S, C) + 0.3 * (x - (8.0 if offset else 0.5)) + 0.4).astype(np.float32).astype(np.float64)
    mask = seg_mask(kind, nseg, B, rs)
    gamma = rs.uniform(0.5, 1.5, C).astype(np.float32) if affine else None
    beta = rs.uniform(-0.3, 0.3, C).astype(np.float32) if affine else None
    rm, rv = rs.randn(C).astype(np.float32), rs.uniform(0.5, 2.0, C).astype(np.float32)
    pv = None
    if pre:  # an earlier call's stats: other data, other live-row counts, a dead segment of its own (segment 1 of > 1)
        pm = (np.arange(Rw) % 3 != 0).astype(np.uint8)
        if nseg > 1:
            pm[B:2 * B] = 0
        fp = R.seg_forward(R.round_to(rs.randn(Rw, S, C) + 1.0, dt), pm, nseg, None, None, EPS)
        pv = R.stats_vector(fp).astype(np.float32)
        nc = nseg * C
        pre_d = dict(mean=pv[:nc].reshape(nseg, C).astype(np.float64), unb=pv[2 * nc:3 * nc].reshape(nseg, C).astype(np.float64),
                     rows=pv[3 * nc:].astype(np.float64))
    g64 = None if gamma is None else gamma.astype(np.float64)
    b64 = None if beta is None else beta.astype(np.float64)
    f = R.seg_forward(x, mask, nseg, g64, b64, EPS, MOM, rm.astype(np.float64) if update else None,
                      rv.astype(np.float64) if update else None, NB0 if update else None, pre_d if pre else None)
    if pre:
        assert nseg == 1 or (pre_d["rows"] != f["rows"]).any()
    sv = R.stats_vector(f).astype(np.float32)  # the backward's statistics: the model's, as f32
    nc = nseg * C
    mean32, inv32 = (sv[i * nc:(i + 1) * nc].reshape(nseg, C).astype(np.float64) for i in (0, 1))
    dg0, db0 = rs.randn(C).astype(np.float32), rs.randn(C).astype(np.float32)
    bw = R.seg_backward(x, dy, mask, nseg, g64, mean32, inv32, f["rows"],
                        (dg0.astype(np.float64), db0.astype(np.float64)) if acc else None)
    return dict(spec=spec, dt=dt, x=x, dy=dy, mask=mask, gamma=gamma, beta=beta, rm=rm, rv=rv, pre=pv,
                pre_d=pre_d if pre else None, f=f, sv=sv, mean32=mean32, inv32=inv32, dg0=dg0, db0=db0, bw=bw)


_seg_case_cached = functools.lru_cache(maxsize=None)(_seg_case)


def seg_not_vacuous(k):
    nseg, B, S, C, kind, update, pre, affine, nb, acc, dpar, offset = k["spec"]
    rows = k["f"]["rows"]
    if kind == "ragged":
        assert (rows > 0).all() and (rows < B).any()
    if kind.startswith("dead"):
        assert int((rows == 0).sum()) == 1 and rows[{"dead_first": 0, "dead_mid": nseg // 2, "dead_last": nseg - 1}[kind]] == 0
    if kind == "only_last":
        assert not rows[:-1].any() and rows[-1] > 0 and nseg == 32
    if kind == "one":
        assert rows[0] == 1 and k["f"]["n"][0] == S
    if kind == "zeros":
        assert not rows.any()
    if offset:
        assert (k["f"]["ex2"] / k["f"]["var"] >= 100).all()


@pytest.mark.parametrize("dt,spec", [a for a in SEG_ALL if a[1][0] * a[1][1] * a[1][2] * a[1][3] < 100000],
                         ids=[i for i, a in zip(SEG_IDS, SEG_ALL) if a[1][0] * a[1][1] * a[1][2] * a[1][3] < 100000])
def test_seg_case_is_not_vacuous(dt, spec):
    """CPU: the masks are what their names say (the small cases; the GPU tests check every case)."""
    seg_not_vacuous(seg_case(dt, spec))


def _sc(v, B, S):
    """[nseg][C] -> [nseg*B][S][C] broadcastable."""
    return np.repeat(v, B, axis=0)[:, None, :]


def seg_stat_bounds(k, small):
    f = k["f"]
    nseg, B, S, C = k["spec"][:4]
    r = (B * S + 4) * 2.0 ** -53
    dmean = U * np.abs(f["mean"]) + r * f["eabs"]
    dvar = r * (f["ex2"] + 2 * np.abs(f["mean"]) * f["eabs"] + f["mean"] ** 2) if small else r * f["var"]
    dis = f["invstd"] * (dvar / (2 * (f["var"] + EPS)) + U + 2.0 ** -51)
    n = f["n"].astype(np.float64)[:, None]
    fac = np.where(n > 1, n / np.maximum(n - 1, 1), 1.0)
    dunb = dvar * fac + (U + 2.0 ** -51) * f["unb"]
    return dmean, dis, dunb


def running_bound(k, dmean, dunb):
    """The error bound of the running statistics, replayed over the model's update sequence."""
    f, nseg = k["f"], k["spec"][0]
    rm, rv = k["rm"].astype(np.float64), k["rv"].astype(np.float64)
    em, ev = np.zeros_like(rm), np.zeros_like(rv)
    seq = []
    for sg in range(nseg):
        if k["pre_d"] is not None and k["pre_d"]["rows"][sg] > 0:
            seq.append((k["pre_d"]["mean"][sg], 0.0, k["pre_d"]["unb"][sg], 0.0))
        if f["rows"][sg] > 0:
            seq.append((f["mean"][sg], dmean[sg], f["unb"][sg], dunb[sg]))
    for mean, dm, unb, du in seq:
        em = (1 - MOM) * em + MOM * dm + 4 * U * (np.abs((1 - MOM) * rm) + np.abs(MOM * mean))
        ev = (1 - MOM) * ev + MOM * du + 4 * U * (np.abs((1 - MOM) * rv) + np.abs(MOM * unb))
        rm, rv = (1 - MOM) * rm + MOM * mean, (1 - MOM) * rv + MOM * unb
    return em, ev, len(seq)


def seg_forward_run(k, small):
    L = lib()
    nseg, B, S, C, kind, update, pre, affine, nb, acc, dpar, offset = k["spec"]
    dt = k["dt"]
    x = Buf(k["x"].size, TD[dt], fill=0.0, data=k["x"])
    y, st = Buf(k["x"].size, torch.float32), Buf(3 * nseg * C + nseg, torch.float32)
    rm, rv = (Buf(C, torch.float32, data=k["rm"]), Buf(C, torch.float32, data=k["rv"])) if update else (None, None)
    nbt = Buf(1, torch.int64, fill=0x7F7F, data=np.array([NB0])) if update and nb else None
    mask = None if k["mask"] is None else Buf(nseg * B, torch.uint8, fill=0x7F, data=k["mask"])
    p = lambda b: b.t if b is not None else None
    args = [dt, x.t, p(mask), nseg, B, S, C, f32_in(k["gamma"]), f32_in(k["beta"]), EPS, y.t, st.t, st.n * 4, int(update),
            MOM, p(rm), p(rv), p(nbt), f32_in(k["pre"])]
    ws = None
    if small:
        ws = Workspace(L.query("gmz_seg_bn_small_workspace_bytes", nseg, C))
        assert ws.nbytes == nseg * 64 * 17 * 8 + nseg * 16 * 4
        args += [ws.t, ws.nbytes]
    L.call("gmz_seg_bn_forward_small" if small else "gmz_seg_bn_forward", *args, L.stream_ptr())
    torch.cuda.synchronize()
    assert all(b.intact() for b in (x, y, st, rm, rv, nbt, mask) if b is not None) and (ws is None or ws.intact())
    return dict(y=y, st=st, rm=rm, rv=rv, nbt=nbt)


def seg_backward_run(k, small):
    L = lib()
    nseg, B, S, C, kind, update, pre, affine, nb, acc, dpar, offset = k["spec"]
    dt = k["dt"]
    x = Buf(k["x"].size, TD[dt], fill=0.0, data=k["x"])
    dy = Buf(k["x"].size, torch.float32, fill=0.0, data=k["dy"])
    dx = Buf(k["x"].size, TD[dt])
    st = Buf(3 * nseg * C + nseg, torch.float32, data=k["sv"])
    dg = Buf(C, torch.float32, data=k["dg0"] if acc else None) if dpar else None
    db = Buf(C, torch.float32, data=k["db0"] if acc else None) if dpar else None
    mask = None if k["mask"] is None else Buf(nseg * B, torch.uint8, fill=0x7F, data=k["mask"])
    p = lambda b: b.t if b is not None else None
    args = [dt, x.t, dy.t, p(mask), nseg, B, S, C, f32_in(k["gamma"]), st.t, st.n * 4, dx.t, p(dg), p(db), int(acc)]
    ws = None
    if small:
        ws = Workspace(L.query("gmz_seg_bn_small_workspace_bytes", nseg, C))
        args += [ws.t, ws.nbytes]
    L.call("gmz_seg_bn_backward_small" if small else "gmz_seg_bn_backward", *args, L.stream_ptr())
    torch.cuda.synchronize()
    assert all(b.intact() for b in (x, dy, dx, st, dg, db, mask) if b is not None) and (ws is None or ws.intact())
    return dict(dx=dx, dg=dg, db=db)


def check_seg_forward(k, o, small, tag):
    nseg, B, S, C, kind, update, pre, affine, nb, acc, dpar, offset = k["spec"]
    f, dt = k["f"], k["dt"]
    dmean, dis, dunb = seg_stat_bounds(k, small)
    st = o["st"].f64()
    nc = nseg * C
    mean, inv, unb = (st[i * nc:(i + 1) * nc].reshape(nseg, C) for i in (0, 1, 2))
    assert np.array_equal(st[3 * nc:], f["rows"].astype(np.float64)), "live rows"
    if dt == 1:  # the f64 sum of f16 values is exact in any order
        assert np.array_equal(mean, f["mean"].astype(np.float32).astype(np.float64)), "mean is not float32(sum / n)"
    within(tag + "mean", dt, mean, f["mean"], dmean)
    within(tag + "invstd", dt, inv, f["invstd"], dis)
    within(tag + "unb", dt, unb, f["unb"], dunb + 2.0 ** -149)
    g = np.ones(C) if k["gamma"] is None else np.abs(k["gamma"].astype(np.float64))
    b = np.zeros(C) if k["beta"] is None else np.abs(k["beta"].astype(np.float64))
    d = np.abs(k["x"] - _sc(f["mean"], B, S))
    D = _sc(dmean * f["invstd"] * g, B, S) + d * _sc(dis * g, B, S) + 4 * U * (d * _sc(f["invstd"] * g, B, S) + b)
    within(tag + "y", dt, o["y"].f64().reshape(k["x"].shape), f["y"], D + 2.0 ** -149)
    if update:
        em, ev, updates = running_bound(k, dmean, dunb)
        if updates == 0:  # no live segment anywhere: untouched, exactly
            assert f32_bits_equal(o["rm"], k["rm"]) and f32_bits_equal(o["rv"], k["rv"])
        else:
            within(tag + "running_mean", dt, o["rm"].f64(), f["rm"], em)
            within(tag + "running_var", dt, o["rv"].f64(), f["rv"], ev)
        if o["nbt"] is not None:
            assert int(o["nbt"].t[0]) == f["nb"] == NB0 + updates


def check_seg_backward(k, o, tag):
    nseg, B, S, C, kind, update, pre, affine, nb, acc, dpar, offset = k["spec"]
    bw, dt = k["bw"], k["dt"]
    r = (B * S + 4) * 2.0 ** -53
    n = np.maximum(k["f"]["rows"].astype(np.float64) * S, 1.0)[:, None]
    dG1, dG2 = r * bw["A1"], (2 * U + r) * bw["A2"]
    dc1, dc2 = dG1 / n + U * np.abs(bw["c1"]), dG2 / n + U * np.abs(bw["c2"])
    g = np.ones(C) if k["gamma"] is None else np.abs(k["gamma"].astype(np.float64))
    k1 = _sc(g * k["inv32"], B, S)
    ady, axh = np.abs(k["dy"]), np.abs(bw["xhat"])
    live = bw["live"][:, None, None]
    Dl = k1 * (_sc(dc1, B, S) + axh * _sc(dc2, B, S) + 6 * U * (ady + _sc(np.abs(bw["c1"]), B, S) + axh * _sc(np.abs(bw["c2"]), B, S)))
    D = np.where(live, Dl, 3 * U * k1 * ady)
    within(tag + "dx", dt, o["dx"].f64().reshape(k["x"].shape), bw["dx"], D + UT[dt] * (np.abs(bw["dx"]) + D) + TINY[dt])
    if dpar:
        sg, sb = bw["G2"].sum(axis=0), bw["G1"].sum(axis=0)
        extra = (lambda v: U * np.abs(v)) if acc else (lambda v: 0.0)
        within(tag + "dgamma", dt, o["dg"].f64(), bw["dgamma"], dG2.sum(axis=0) + U * np.abs(sg) + extra(bw["dgamma"]) + 2.0 ** -149)
        within(tag + "dbeta", dt, o["db"].f64(), bw["dbeta"], dG1.sum(axis=0) + U * np.abs(sb) + extra(bw["dbeta"]) + 2.0 ** -149)


@gpu
@pytest.mark.parametrize("dt,spec", SEG_ALL, ids=SEG_IDS)
def test_seg_bn_forward(dt, spec):
    """gmz_seg_bn_forward, and for C <= 8 gmz_seg_bn_forward_small on the same inputs, each against the model."""
    need_gpu()
    k = seg_case(dt, spec)
    seg_not_vacuous(k)
    check_seg_forward(k, seg_forward_run(k, False), False, "seg ")
    if spec[3] <= 8:
        check_seg_forward(k, seg_forward_run(k, True), True, "seg_small ")


@gpu
@pytest.mark.parametrize("dt,spec", SEG_ALL, ids=SEG_IDS)
def test_seg_bn_backward(dt, spec):
    """gmz_seg_bn_backward, and for C <= 8 gmz_seg_bn_backward_small, on the model's statistics."""
    need_gpu()
    k = seg_case(dt, spec)
    check_seg_backward(k, seg_backward_run(k, False), "seg ")
    if spec[3] <= 8:
        check_seg_backward(k, seg_backward_run(k, True), "seg_small ")
