"""gmz_opt_step, gmz_opt_layout and gmz_grad_add_t(_cols) (csrc/gmz_train.hip) against tests/opt_ref.py, the float64
model of what include/gmz.h documents, element by element, through raw ``_lib.call``.

Rules (those of tests/test_bn_kernels_gpu.py)
  * every parameter, target, gradient and moment buffer lies between NaN guards that must survive; the item table
    is built by hand from gmz_opt_layout's item size and chunk; the workspace is exactly gmz_opt_layout's bytes
    between byte sentinels;
  * what can be exact is asserted bit for bit: step, coef[0], the zeroed gradient, everything a skipped step must
    leave alone, and gmz_grad_add_t_cols (one f32 add per element: float32(dst + src) is the only correct answer);
  * the bounds below are per element, first order in u = 2^-24, from the kernel's public arithmetic (f32 throughout,
    f64 for the sum of squares) and the model's magnitudes.  No constant was chosen by looking at the kernel's error.
    The largest error / bound ratios and the mutants these tests catch are in profiles/heads_opt_kernel_tests.txt.

Bounds.  A correctly rounded f32 operation is off by u relative; division, sqrtf: 1 ulp <= 2u; powf: 2 ulp <= 4u
(the device library documents 1 ulp; nothing public holds it to that for every argument, so one more is allowed).
The scales used are powers of two, so 1 / scale and inv * clip are exact; 1 - beta is exact for beta in [0.5, 1]
(Sterbenz), so the model's (1 - beta) from the float32 beta is the kernel's.
  norm      N exact squares summed in f64 (N 2^-53), sqrt, times inv, one rounding to f32: (N 2^-54 + 2^-53 + u) rel.
  coef[1]   norm + 1e-6f (u, and the f32 constant is within u of 1e-6), the division (2u), min with 1 (exact):
            c = 5u + N 2^-53 relative; exactly 1 / scale where neither side of the min is within c of the other
  g'        gs = g coef[1]: (c + u) |gs|; wd p: u |wd p|; the sum: u |g'|       -> dg
  m         b1 m + (1 - b1) g': (1 - b1) dg + 2u (|b1 m| + (1 - b1) |g'|)                       -> dm
  v         b2 v + ((1 - b2) g') g': (1 - b2) 2 |g'| dg + 3u v'                                 -> dv
  bc        1 - powf(b, s): 4u b^s, and u bc for the subtraction: rel(bc) = 4u b^s / (1 - b^s) + u.  This is where
            the powf error is amplified: at s = 1, b2 = 0.999 it is 4u * 999 + u; at s = 10,001 it is 5e-5 * 4u + u
  step size lr / bc1: rel(bc1) + 2u.   sqrtf(bc2): rel(bc2) / 2 + 2u
  denom     sqrtf(v') / sqrtf(bc2) + eps: q = sqrt(v' / bc2), dq = dv / (2 sqrt(v') sqrt(bc2)) + q (2u + rel(bc2) / 2
            + 2u + 2u), d denom = dq + u denom
  p         upd = (step size * m') / denom: |upd| (rel(step size) + d denom / denom + 3u) + (lr / bc1) dm / denom;
            dp = d upd + u |p'|
  t         (1 - tau) in f32 (u), two products, one sum: dt = tau dp + 3u (|(1 - tau) t| + |tau p'|)
  and 2^-149, one subnormal quantum, on each, for a result that small.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import opt_ref as R
from kernel_guards import TD, U, Buf, Workspace, bits, f32_in, lib, need_gpu, same, within as _within

gpu = pytest.mark.gpu
HP = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, tau=0.05)
SUB = 2.0 ** -149
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_report():
    yield
    path = os.environ.get("GMZ_OPT_RATIOS")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(dict(sorted(RATIOS.items())), f, indent=1)


def within(name, got, want, bound):
    _within(RATIOS, name, 0, got, want, bound)


# ------------------------------------------------------------------------------------------------ the layout
SIZES = [1, 3, 4095, 4096, 4097, 10001]  # 22,293 elements: 22,293 % 4 = 1, the sum of squares' scalar tail runs
NO_TARGET = {1, 3}  # parameters (by index) whose t is NULL
ITEM = np.dtype([("p", "<u8"), ("t", "<u8"), ("off", "<i8"), ("n", "<i4"), ("pi", "<i4")])


def _pieces(sizes, chunk):
    """(parameter, first element within it, length): chunks of at most ``chunk``; parameter 2 (4,095 elements) is cut
    at 1,000 as well, so p_index != 0 occurs inside one chunk's worth too."""
    out = []
    for i, n in enumerate(sizes):
        cuts = list(range(0, n, chunk)) + [n]
        if i == 2 and n > 1000:
            cuts = [0, 1000, n]
        out += [(i, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    return out


def layout():
    L = lib()
    ib, ch, wb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
    L.call("gmz_opt_layout", ctypes.byref(ib), ctypes.byref(ch), ctypes.byref(wb))
    return ib.value, ch.value, wb.value


@functools.lru_cache(maxsize=None)
def state(sizes, seed, zero_moments):
    """The f32 values of one optimiser state, as float64 (built once, never changed)."""
    rs = np.random.RandomState(seed)
    N = sum(sizes)
    r = lambda a: np.asarray(a, np.float32).astype(np.float64)
    p, t = r(rs.randn(N) * 0.3), r(rs.randn(N) * 0.3)
    g = r(rs.randn(N) * 0.02)  # norm about 0.02 sqrt(N): 3 at N = 22,293
    m = np.zeros(N) if zero_moments else r(rs.randn(N) * 0.01)
    v = np.zeros(N) if zero_moments else r(rs.uniform(1e-5, 1e-3, N))
    return p, t, g, m, v


class Device:
    """The buffers of one state on the device, every one between NaN guards, and its shuffled item table."""

    def __init__(self, sizes, p, t, g, m, v, step, scale):
        ib, ch, wb = layout()
        assert ib == ITEM.itemsize == 32 and ch == 4096 and wb >= 1024 * 8 + 4
        self.sizes, self.offs = sizes, np.concatenate([[0], np.cumsum(sizes)])
        self.p = [Buf(n, torch.float32, data=p[o:o + n]) for n, o in zip(sizes, self.offs)]
        self.t = [None if i in NO_TARGET else Buf(n, torch.float32, data=t[o:o + n])
                  for i, (n, o) in enumerate(zip(sizes, self.offs))]
        self.has_t = np.concatenate([np.full(n, tt is not None) for n, tt in zip(sizes, self.t)])
        N = int(self.offs[-1])
        self.g, self.m, self.v = (Buf(N, torch.float32, data=a) for a in (g, m, v))
        assert self.g.t.data_ptr() % 16 == 0
        pcs = _pieces(sizes, ch)
        np.random.RandomState(5).shuffle(pcs)
        assert any(a != 0 for _, a, _ in pcs) and all(n <= ch for _, _, n in pcs)
        tab = np.zeros(len(pcs), ITEM)
        for k, (i, a, n) in enumerate(pcs):
            tab[k] = (self.p[i].t.data_ptr(), self.t[i].t.data_ptr() if self.t[i] else 0, int(self.offs[i]) + a, n, a)
        self.items = torch.from_numpy(tab.view(np.uint8)).cuda()
        self.n_items = len(pcs)
        self.step, self.coef = Buf(1, torch.float32, data=np.array([step])), Buf(2, torch.float32)
        self.lr = f32_in(np.array([HP["lr"]]))
        self.scale = None if scale is None else f32_in(np.array([scale]))
        self.ws = Workspace(wb, zero=True)
        self.N = N

    def call(self, skip_on_inf, max_norm, wd):
        L = lib()
        try:
            L.call("gmz_opt_step", self.items, self.n_items, self.g.t, self.m.t, self.v.t, ctypes.c_longlong(self.N),
                   self.scale, int(skip_on_inf), max_norm, self.lr, HP["beta1"], HP["beta2"], HP["eps"], wd, HP["tau"],
                   self.step.t, self.coef.t, self.ws.t, self.ws.nbytes, L.stream_ptr())
        finally:
            torch.cuda.synchronize()
        assert self.ws.intact(), "workspace sentinels"
        for b in self.p + [b for b in self.t if b] + [self.g, self.m, self.v, self.step, self.coef]:
            assert b.intact(), "guards"

    def flat(self, bufs, fallback):
        return np.concatenate([b.f64() if b else fallback[o:o + n] for b, n, o in zip(bufs, self.sizes, self.offs)])


def bounds(o, p, t, m, v, N, wd):
    """(d coef[1] relative, dm, dv, dp, dt) from the model's intermediates o (a step that was taken)."""
    f = R.f32
    b1, b2, lr, eps, wd, tau = f(HP["beta1"]), f(HP["beta2"]), f(HP["lr"]), f(HP["eps"]), f(wd), f(HP["tau"])
    c = 5 * U + N * 2.0 ** -53
    gs, g2, s = np.abs(o["gs"]), np.abs(o["g2"]), o["step"]
    dg = (c + U) * gs + U * np.abs(wd * p) + U * g2
    dm = (1 - b1) * dg + 2 * U * (np.abs(b1 * m) + (1 - b1) * g2) + SUB
    dv = (1 - b2) * 2 * g2 * dg + 3 * U * o["v"] + SUB
    rbc1 = 4 * U * b1 ** s / o["bc1"] + U
    rbc2 = 4 * U * b2 ** s / o["bc2"] + U
    sv = np.sqrt(o["v"])
    q = sv / np.sqrt(o["bc2"])
    dq = np.where(sv > 0, dv / (2 * np.where(sv > 0, sv, 1) * np.sqrt(o["bc2"])), 0) + q * (6 * U + rbc2 / 2)
    dden = dq + U * o["denom"]
    dupd = np.abs(o["upd"]) * (rbc1 + 2 * U + dden / o["denom"] + 3 * U) + (lr / o["bc1"]) * dm / o["denom"]
    dp = dupd + U * np.abs(o["p"]) + SUB
    dt = tau * dp + 3 * U * (np.abs((1 - tau) * t) + np.abs(tau * o["p"])) + SUB
    return c, dm, dv, dp, dt


def target_bound(t, p2, dp):
    tau = R.f32(HP["tau"])
    return tau * dp + 3 * U * (np.abs((1 - tau) * t) + np.abs(tau * p2)) + SUB


def check_taken(tag, d, o, p, t, m, v, wd):
    c, dm, dv, dp, dt = bounds(o, p, t, m, v, d.N, wd)
    coef = d.coef.f64()
    assert coef[0] == 0.0 and float(d.step.f64()[0]) == o["step"]
    within(tag + "coef1", coef[1:], np.array([o["coef"][1]]), c * abs(o["coef"][1]))
    within(tag + "m", d.m.f64(), o["m"], dm)
    within(tag + "v", d.v.f64(), o["v"], dv)
    within(tag + "p", d.flat(d.p, None), o["p"], dp)
    within(tag + "t", d.flat(d.t, t), o["t"], np.where(d.has_t, dt, 0))
    assert not bits(d.g.t).any(), "gradient not exactly +0"


# (name, scale, clip binds, weight decay, starting step, zero moments, gradient multiplier)
CASES = [
    ("bind-s0", None, True, 0.0, 0.0, True, 1.0),
    ("free-s0-wd", None, False, 1e-2, 0.0, True, 1.0),
    ("bind-s1-wd-scale16th", 1 / 16, True, 1e-2, 1.0, False, 1.0),
    ("free-s1-scale64k", 65536.0, False, 0.0, 1.0, False, 1.0),
    ("bind-s10000-wd-scale64k", 65536.0, True, 1e-4, 10000.0, False, 1.0),
    ("free-s10000", None, False, 0.0, 10000.0, True, 1.0),
    # a norm of 7e-4 clipped to 2^-12: the 1e-6 in the clip's denominator is 1.4e-3 of it, 4,000 times the bound
    ("bind-tiny-norm-s1", None, True, 0.0, 1.0, False, 2.0 ** -12),
]


@gpu
@pytest.mark.parametrize("name,scale,binds,wd,step0,zero,gmul", CASES, ids=[c[0] for c in CASES])
def test_opt_step_matches_the_model(name, scale, binds, wd, step0, zero, gmul):
    need_gpu()
    sizes = tuple(SIZES)
    p, t, g, m, v = state(sizes, 1, zero)
    sc = (1.0 if scale is None else scale) * gmul
    g = (g * sc).astype(np.float32).astype(np.float64)  # a power of two: the scaled gradient is exact
    max_norm = (1.0 if binds else 50.0) * gmul
    d = Device(sizes, p, t, g, m, v, step0, scale)
    o = R.opt_step(p, t, d.has_t, g, m, v, step0, scale, 1, max_norm, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], wd,
                   HP["tau"])
    assert (o["clip"] < 0.5) if binds else (o["clip"] == 1.0 and o["norm"] < 0.5 * max_norm), (o["norm"], o["clip"])
    assert not zero or not (m.any() or v.any())
    d.call(1, max_norm, wd)
    check_taken(name + " ", d, o, p, t, m, v, wd)


@gpu
def test_skipped_step_then_a_finite_one_on_the_same_workspace():
    """One inf with skip_on_inf = 1: parameters, moments and step bit-identical, the target still updated, the
    gradient zeroed, coef[0] = 1.  Then a finite step on the same workspace: the non-finite flag was reset."""
    need_gpu()
    sizes = tuple(SIZES)
    p, t, g, m, v = state(sizes, 2, False)
    gi = g.copy()
    gi[12345] = np.inf
    d = Device(sizes, p, t, gi, m, v, 7.0, 65536.0)
    before = [b.t.clone() for b in d.p] + [d.m.t.clone(), d.v.t.clone(), d.step.t.clone()]
    o = R.opt_step(p, t, d.has_t, gi, m, v, 7.0, 65536.0, 1, 1.0, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 1e-2, HP["tau"])
    assert o["skip"]
    d.call(1, 1.0, 1e-2)
    after = [b.t for b in d.p] + [d.m.t, d.v.t, d.step.t]
    assert all(same(a, b) for a, b in zip(before, after))
    assert d.coef.f64()[0] == 1.0
    assert not bits(d.g.t).any()
    within("skip t", d.flat(d.t, t), o["t"], np.where(d.has_t, target_bound(t, p, 0.0), 0))
    assert (np.abs(o["t"] - t)[d.has_t] > 0).mean() > 0.9  # the update is not a no-op
    # the same device state, a finite gradient: the step is taken
    t1 = d.flat(d.t, t)
    d.g.t.copy_(torch.from_numpy(g).float())
    o2 = R.opt_step(p, t1, d.has_t, g, m, v, 7.0, 65536.0, 1, 1.0, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 1e-2, HP["tau"])
    d.call(1, 1.0, 1e-2)
    check_taken("after-skip ", d, o2, p, t1, m, v, 1e-2)


@gpu
def test_non_finite_gradient_without_skip_on_inf():
    """skip_on_inf = 0: the header promises only that the step is taken (coef[0] = 0, step advanced) and the
    gradient zeroed; nothing about the values a non-finite gradient leaves."""
    need_gpu()
    sizes = (3, 4097)
    p, t, g, m, v = state(sizes, 3, False)
    g = g.copy()
    g[100] = np.inf
    d = Device(sizes, p, t, g, m, v, 3.0, None)
    d.call(0, 1.0, 0.0)
    assert d.coef.f64()[0] == 0.0 and float(d.step.f64()[0]) == 4.0
    assert not bits(d.g.t).any()


@gpu
def test_a_bucket_where_every_norm_workgroup_loops_again():
    """1,024 x 256 x 4 + 5 elements: one float4 more than the sum-of-squares grid covers in one pass, and a scalar
    tail; 257 items of one parameter."""
    need_gpu()
    sizes = (1024 * 256 * 4 + 5,)
    p, t, g, m, v = state(sizes, 4, False)
    d = Device(sizes, p, t, g, m, v, 1.0, None)
    assert d.n_items == 257
    o = R.opt_step(p, t, d.has_t, g, m, v, 1.0, None, 1, 1.0, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 1e-4, HP["tau"])
    assert o["clip"] < 0.5
    d.call(1, 1.0, 1e-4)
    check_taken("big ", d, o, p, t, m, v, 1e-4)


# ------------------------------------------------------------------------------------------------ gmz_grad_add_t(_cols)
# (P, C, O, ldo, col0): partial 64 x 64 tiles in both directions, ldo > O, col0 > 0 with col0 + O == ldo, C = 1, P = 1
GCASES = [(70, 3, 65, 65, 0), (130, 2, 70, 100, 30), (64, 1, 64, 64, 0), (1, 5, 3, 8, 2), (225, 1, 17, 20, 3),
          (33, 4, 1, 9, 8)]


@gpu
@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("P,C,O,ldo,col0", GCASES)
def test_grad_add_t_cols_is_bit_identical(dt, P, C, O, ldo, col0):
    need_gpu()
    L = lib()
    rs = np.random.RandomState(P * 7 + O)
    src = torch.from_numpy(rs.randn(P * C * ldo)).to(TD[dt])
    dst0 = rs.randn(O * C * P).astype(np.float32)
    want = R.grad_add_t_cols(dst0, src.double().numpy(), P, C, O, ldo, col0).astype(np.float32)  # one f32 rounding
    s = Buf(P * C * ldo, TD[dt], fill=0.0, data=src.double().numpy())
    d = Buf(O * C * P, torch.float32, data=dst0)
    L.call("gmz_grad_add_t_cols", dt, s.t, P, C, O, ldo, col0, d.t, L.stream_ptr())
    torch.cuda.synchronize()
    assert d.intact() and s.intact()
    assert same(d.t, torch.from_numpy(want.ravel()).cuda())
    if ldo == O and col0 == 0:  # gmz_grad_add_t is the same call
        d2 = Buf(O * C * P, torch.float32, data=dst0)
        L.call("gmz_grad_add_t", dt, s.t, P, C, O, d2.t, L.stream_ptr())
        torch.cuda.synchronize()
        assert d2.intact() and same(d2.t, d.t)
