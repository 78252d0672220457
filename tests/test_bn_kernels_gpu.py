"""Every gmz_bn_* entry point of include/gmz.h (csrc/gmz_train.hip) against tests/bn_ref.py, the float64 model of
its documented arithmetic, element by element, through raw ``_lib.call``.

Rules every test here follows
  * output buffers are pre-filled with NaN (dgamma / dbeta too unless accumulating) between NaN guard elements, and
    must be finite afterwards with the guards still NaN: a skipped tail position or a store past the end shows;
  * every workspace is a slice, exactly gmz_bn_workspace_bytes long, of a larger buffer with a sentinel pattern on
    both sides, that number is what ws_bytes says, and the sentinels must be intact afterwards;
  * the backward is tested on its own: its y and save inputs are the model's (rounded to the storage type / f32),
    never the forward kernel's outputs;
  * the bounds are derived (below), per element, from unit roundoffs and the model's magnitudes; no constant in
    them was chosen by looking at the kernels' error.  The largest observed error / bound ratios and the mutants the
    tests were shown to catch are in profiles/bn_kernel_tests.txt.

Bounds.  u = 2^-24 (f32 arithmetic), uT = 2^-24 / 2^-11 / 2^-8 (the one final store to f32 / f16 / bf16), tT = half
the smallest subnormal of the storage type (an absolute floor: f16 flushes 1e-9 to 0).  First order in u.
  reduction   a channels-last workgroup's thread adds at most L pixels in f32 (L = ceil(P / ns), ns = P / 16 splits
              capped at 1,024, by the public split rule; every f32 partial then goes to f64), so a sum of terms t
              is off by at most r * sum|t| with r = L u + N 2^-53 (N = P: the f64 part).  NCHW and the *_stats
              entry points sum in f64 only: L = 0.
  mean        |dmean| <= u |mean| + r E|x|                              (the f32 rounding of the f64 quotient)
  var (f64)   |dvar|  <= r (E[x^2] + 2 |mean| E|x|)                     (sum x^2 / n - mean^2 before any rounding)
  invstd      var -> f32 (u var), + eps (u (var + eps)), sqrtf and the division (<= 1 ulp = 2u each):
              |dinvstd| / invstd <= (dvar + u var + u (var + eps)) / (2 (var + eps)) + 4u
              — dvar / (var + eps) carries the cancellation factor E[x^2] / (var + eps)
  y           sc = gamma invstd: |dsc| <= |gamma| dinvstd + u |sc|.  ((x - mean) sc + beta) + res: four roundings,
              D = dmean |sc| + |x - mean| dsc + 4u (|x - mean| |sc| + |beta| + |res|); the ReLU is 1-Lipschitz;
              |dy| <= D + uT (|y| + D) + tT
  running     (1 - m) rm + m mean in f32, <= 3 roundings a term: 3u (|(1 - m) rm| + |m mean|) + m dmean;
              variance likewise with unb = var n / (n - 1): 3u (|(1 - m) rv| + |m unb|) + m (dvar n / (n - 1) + u unb)
  dbeta       r sum|dz| + u |dbeta|.   dgamma: xhat = (x - mean) invstd and its product add 3 roundings a term:
              (r + 3u) sum|dz xhat| + u |dgamma|
  dx          mg = dbeta / n: dmg <= r sum|dz| / n + u |mg|; mgx = dgamma / n likewise.  Valid rows:
              k1 ((dz - mg) - ((x - mean) invstd) mgx), k1 = gamma invstd: at most 7 roundings touch any term,
              D = |k1| (dmg + |xhat| dmgx + 7u (|dz| + |mg| + |xhat mgx|)); other rows D = 2u |k1 dz|;
              |ddx| <= D + uT (|dx| + D) + tT.   dres = dz exactly.
  eval        mean = running_mean exactly, |dinvstd| / invstd <= u / 2 + 4u, then as y.
"""
import functools
import json
import os
import re
import zlib

import numpy as np
import pytest
import torch

import bn_ref as R
from conftest import REPO

gpu = pytest.mark.gpu
U = 2.0 ** -24
UT = {0: 2.0 ** -24, 1: 2.0 ** -11, 2: 2.0 ** -8}
TINY = {0: 2.0 ** -150, 1: 2.0 ** -25, 2: 2.0 ** -134}
TD = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
DN = {0: "f32", 1: "f16", 2: "bf16"}
EPS, MOM = float(np.float32(1e-4)), float(np.float32(0.1))  # what the C float arguments hold
GUARD = 16  # NaN elements on both sides of every output
WS_GUARD = 4096  # sentinel bytes on both sides of every workspace
SENT = 0xA5
NB0 = 5
REFUSAL = "relu_mask needs channels-last 16-B aligned operands"

RATIOS = {}  # (output, dtype name) -> largest error / bound seen (written out when GMZ_BN_RATIOS names a file)


@pytest.fixture(scope="module", autouse=True)
def _ratio_report():
    yield
    path = os.environ.get("GMZ_BN_RATIOS")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"%s %s" % k: v for k, v in sorted(RATIOS.items())}, f, indent=1)


# ------------------------------------------------------------------------------------------------ the cases
# (layout, B, C, S, mask kind, res, relu, running statistics, misaligned operand, offset input)
def _c(layout, B, C, S, mask="rand", res=True, relu=True, running=True, mis=None, offset=False):
    return (layout, B, C, S, mask, res, relu, running, mis, offset)


NHWC = [
    # V = 8: C = 8 (256 positions a step), 128 (production), 144 (14 positions, 4 idle threads), 512 (4 positions);
    # B = 37, S = 36 with a ragged mask: split ranges cross row boundaries
    _c(1, 37, 8, 36), _c(1, 37, 128, 36, res=False), _c(1, 37, 144, 36, relu=False), _c(1, 37, 512, 36, running=False),
    _c(1, 5, 128, 25, "ones"),  # P = 125, 16 positions a step, 4 blocks: the pair's second position 61 + 64 is past the end
    _c(1, 5, 144, 25, "null", res=False), _c(1, 5, 512, 25, relu=False), _c(1, 5, 8, 25, "null", relu=False),
    # V = 2: C = 2, C = 6 (85 positions a step, one idle thread)
    _c(1, 37, 2, 36, relu=False), _c(1, 5, 6, 25, "null", res=False, running=False), _c(1, 37, 6, 36),
    # positions: 1, 15 (below one split), 17
    _c(1, 1, 8, 1, "null", res=False), _c(1, 1, 128, 1, "ones", relu=False), _c(1, 3, 128, 5), _c(1, 15, 6, 1),
    _c(1, 17, 8, 1), _c(1, 17, 144, 1, "null", relu=False),
    # B * S = 16,445 at C = 8: 1,027 > 1,024 splits, the cap binds
    _c(1, 65, 8, 253),
    # masks: all zeros, exactly one valid row (S = 1 and 25), first row only, last row only
    _c(1, 5, 8, 25, "zeros"), _c(1, 5, 128, 25, "zeros", res=False), _c(1, 9, 8, 1, "one", res=False),
    _c(1, 5, 128, 25, "one"), _c(1, 5, 128, 25, "first", relu=False), _c(1, 5, 8, 25, "last"),
    _c(1, 5, 2, 25, "last", res=False),
    # a misaligned C = 512: one position a step
    _c(1, 3, 512, 7, mis="x"), _c(1, 3, 512, 7, relu=False, mis="y"),
]
# C = 128 with each operand in turn 2 elements off 16-byte alignment: nhwc_vec falls back to V = 2
MISALIGNED = [_c(1, 5, 128, 25, mis=m) for m in ("x", "res", "y", "dy", "dx", "dres")]
# f16 only: mean 8, std 0.5, E[x^2] - mean^2 cancels ~256-fold
OFFSET = [_c(1, 37, 128, 36, offset=True), _c(0, 33, 16, 36, offset=True)]
_NK1 = ["null", "ones", "zeros"]
_NKB = ["rand", "null", "first", "last", "one", "zeros", "ones"]
NCHW = []
for _i, (_C, _S, _B) in enumerate((c, s, b) for c in (1, 3, 16, 512) for s in (1, 36) for b in (1, 5, 33)):
    # C = 16: 32 splits, so B = 1 and 5 are below the split count and B = 33 gives ragged split_rows
    NCHW.append(_c(0, _B, _C, _S, (_NK1 if _B == 1 else _NKB)[_i % (3 if _B == 1 else 7)], res=_i % 2 == 0,
                   relu=_i % 3 != 0, running=_i % 5 != 0))
NCHW += [_c(0, 9, 16, 1, "one"), _c(0, 5, 3, 25, "one", res=False)]
CASES = NHWC + MISALIGNED + NCHW
ALL = [(d, c) for c in CASES for d in (0, 1, 2)] + [(1, c) for c in OFFSET]
IDS = ["%s-%s-B%dC%dS%d-%s%s%s%s%s%s" % (DN[d], "nhwc" if c[0] else "nchw", c[1], c[2], c[3], c[4],
                                        "-res" if c[5] else "", "-relu" if c[6] else "", "" if c[7] else "-norun",
                                        "-mis_" + c[8] if c[8] else "", "-offset" if c[9] else "") for d, c in ALL]


def _round(a, dt):
    """float64 values -> what the storage type holds, widened back exactly."""
    return torch.from_numpy(a).to(TD[dt]).double().numpy()


def _mask(kind, B, rs):
    if kind == "null":
        return None
    m = np.zeros(B, np.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind == "one":
        m[B // 2] = 1
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[-1] = 1
    elif kind == "rand":
        m[:] = rs.rand(B) < 0.6
        m[rs.randint(B)] = 1
        if m.all():
            m[rs.randint(B)] = 0
    return m


def _split_len(P, nseg=1):
    """L: the most pixels one reduction workgroup (hence one of its threads) sums in f32 — P / 16 splits, at most
    1,024, shared out over the segments with at least one each."""
    ns = max(1, min(P // 16, 1024))
    sps = max(1, ns // nseg)
    return -(-(P // nseg) // sps)


@functools.lru_cache(maxsize=None)
def case(dt, spec):
    """Inputs as stored, the model's forward and backward, the bounds' ingredients.  Built once per (dtype, case)
    and shared, unchanged, by every test that needs it.  A ReLU case of a few dozen elements can miss the 20 % / 20 %
    condition by chance: the first seed whose MODEL output meets it is taken (check_not_vacuous asserts it)."""
    for salt in range(64):
        k = _build(dt, spec, salt)
        if not spec[6] or ((k["f"]["y"] == 0).mean() >= 0.2 and (k["f"]["y"] > 0).mean() >= 0.2):
            break
    return k


def _build(dt, spec, salt):
    layout, B, C, S, kind, use_res, relu, running, mis, offset = spec
    rs = np.random.RandomState(zlib.crc32(repr((dt, salt) + spec).encode()))
    x = _round(rs.randn(B, C, S) * 0.5 + 8.0 if offset else rs.randn(B, C, S) * 2 + 0.5, dt)
    res = _round(rs.randn(B, C, S), dt) if use_res else None
    # dy correlated with x and off centre, so that dbeta / n and dgamma / n are of order 1 like dy itself
    dy = _round(rs.randn(B, C, S) + 0.6 * ((x - 8.0) * 2 if offset else (x - 0.5) / 2) + 0.4, dt)
    mask = _mask(kind, B, rs)
    gamma = rs.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rs.uniform(-0.3, 0.3, C).astype(np.float32)
    if C >= 8:  # stored zeros for the ReLU: y = 0 exactly, and y = 1e-9 > 0 in f32 that f16 stores as 0
        gamma[1], beta[1] = 0, 0
        gamma[3], beta[3] = 0, 1e-9
    rm, rv = rs.randn(C).astype(np.float32), rs.uniform(0.5, 2.0, C).astype(np.float32)
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    f = R.forward(x, mask, g64, b64, EPS, MOM, res, relu, rm.astype(np.float64) if running else None,
                  rv.astype(np.float64) if running else None, NB0 if running else None)
    # the backward's inputs: the model's y rounded to the storage type, its (mean, invstd) rounded to f32
    y_st = _round(f["y"], dt)
    save = np.stack([f["mean"], f["invstd"]]).astype(np.float32)
    bw = R.backward(x, y_st, dy, mask, g64, save[0].astype(np.float64), save[1].astype(np.float64), relu)
    P = B * S
    L = _split_len(P) if layout else 0
    return dict(spec=spec, dt=dt, x=x, res=res, dy=dy, mask=mask, gamma=gamma, beta=beta, rm=rm, rv=rv, f=f,
                y_st=y_st, save=save, bw=bw, L=L, N=P)


def check_not_vacuous(k):
    layout, B, C, S, kind, use_res, relu, running, mis, offset = k["spec"]
    f = k["f"]
    if relu:
        assert (f["y"] == 0).mean() >= 0.2 and (f["y"] > 0).mean() >= 0.2, ((f["y"] == 0).mean(), (f["y"] > 0).mean())
    if kind in ("rand", "one", "first", "last"):
        assert f["n"] > 0 and 0 < int((k["mask"] != 0).sum()) < B
    if kind == "zeros":
        assert f["n"] == 0
    if offset:
        assert (f["ex2"] / f["var"] >= 100).all()
    if k["dt"] == 1 and C >= 8 and not use_res:  # f16: positive before the store, zero after it
        assert (f["y"][:, 3] > 0).all() and not k["y_st"][:, 3].any()


@pytest.mark.parametrize("dt,spec", ALL, ids=IDS)
def test_case_is_not_vacuous(dt, spec):
    """The conditions on the model alone (CPU): ReLU cases have >= 20 % zeros and >= 20 % positives, masked cases a
    valid and an invalid row, the offset case E[x^2] / var >= 100."""
    check_not_vacuous(case(dt, spec))


def test_every_header_entry_point_is_called_here():
    hdr = open(os.path.join(REPO, "include", "gmz.h")).read()
    names = set(re.findall(r"^int\s+(gmz_bn_\w+)\(", hdr, re.M))
    assert len(names) >= 12
    src = open(os.path.abspath(__file__)).read()
    assert not [n for n in names if '"%s"' % n not in src]


# ------------------------------------------------------------------------------------------------ the bounds
def _chan(v):
    return v[None, :, None]


def stat_bounds(f, L, N):
    """(dmean, dvar before rounding, dinvstd) per channel."""
    r = L * U + N * 2.0 ** -53
    dmean = U * np.abs(f["mean"]) + r * f["eabs"]
    dvar = r * (f["ex2"] + 2 * np.abs(f["mean"]) * f["eabs"])
    vpe = f["var"] + EPS
    dis = f["invstd"] * ((dvar + U * f["var"] + U * vpe) / (2 * vpe) + 4 * U)
    return dmean, dvar, dis


def y_bound(k, x, res, mean, invstd, y, dmean, dis, gamma=None, beta=None):
    g = np.abs((k["gamma"] if gamma is None else gamma).astype(np.float64))
    b = np.abs((k["beta"] if beta is None else beta).astype(np.float64))
    sc = g * invstd
    dsc = g * dis + U * sc
    d = np.abs(x - _chan(mean))
    D = _chan(dmean * sc) + d * _chan(dsc) + 4 * U * (d * _chan(sc) + _chan(b) + (0 if res is None else np.abs(res)))
    return D + UT[k["dt"]] * (np.abs(y) + D) + TINY[k["dt"]]


def running_bounds(f, rm, rv, dmean, dvar):
    n = f["n"]
    fac = n / (n - 1.0) if n > 1 else 1.0
    unb = f["var"] * fac
    drm = 3 * U * (np.abs((1 - MOM) * rm) + np.abs(MOM * f["mean"])) + MOM * dmean
    drv = 3 * U * (np.abs((1 - MOM) * rv) + np.abs(MOM * unb)) + MOM * (dvar * fac + U * unb)
    return drm, drv


def grad_bounds(k, L, N):
    """dbeta, dgamma per channel and dx per element."""
    bw, dt = k["bw"], k["dt"]
    r = L * U + N * 2.0 ** -53
    n = max(bw["n"], 1)
    dbeta = r * bw["sabs_dz"] + U * np.abs(bw["dbeta"])
    dgamma = (r + 3 * U) * bw["sabs_dzx"] + U * np.abs(bw["dgamma"])
    dmg = r * bw["sabs_dz"] / n + U * np.abs(bw["mg"])
    dmgx = (r + 3 * U) * bw["sabs_dzx"] / n + U * np.abs(bw["mgx"])
    k1 = np.abs(k["gamma"].astype(np.float64) * k["save"][1].astype(np.float64))
    az, ax = np.abs(bw["dz"]), np.abs(bw["xhat"])
    D = 2 * U * _chan(k1) * az
    v = np.ones(az.shape[0], bool) if k["mask"] is None else k["mask"] != 0
    Dv = _chan(k1) * (_chan(dmg) + ax * _chan(dmgx) + 7 * U * (az + _chan(np.abs(bw["mg"])) + ax * _chan(np.abs(bw["mgx"]))))
    D[v] = Dv[v]
    dx = D + UT[dt] * (np.abs(bw["dx"]) + D) + TINY[dt]
    return dbeta, dgamma, dx


def within(name, dt, got, want, bound):
    """|got - want| <= bound, element by element; records the largest error / bound."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "%s: %d elements not written" % (name, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    bound = np.broadcast_to(bound, err.shape)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    print("%s %s: max error / bound = %.3g (max error %.3g)" % (name, DN[dt], ratio, float(err.max())))
    key = (name, DN[dt])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    i = int(np.argmax(err - bound))
    assert ratio <= 1.0, "%s: error %.3g > bound %.3g at flat index %d (got %r, want %r)" % (
        name, err.flat[i], bound.flat[i], i, got.flat[i], np.asarray(want).flat[i])


# ------------------------------------------------------------------------------------------------ device plumbing
def _lib():
    import datou_gomoku_muzero_amd._lib as L
    return L


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Buf:
    """A device tensor of ``n`` elements inside a larger allocation: GUARD NaN (or 0x7f for bytes / integers)
    elements before and after it, the tensor itself ``off`` elements off the allocation's 16-byte grid."""

    def __init__(self, n, dtype, off=0, fill=float("nan")):
        self.raw = torch.full((n + 2 * GUARD + 8,), fill, dtype=dtype, device="cuda")
        self.lo, self.n = GUARD + off, n
        self.t = self.raw[self.lo:self.lo + n]
        self.fill = fill

    def intact(self):
        g = torch.cat([self.raw[:self.lo], self.raw[self.lo + self.n:]])
        return bool(torch.isnan(g).all()) if self.fill != self.fill else bool((g == self.fill).all())

    def untouched(self):
        return bool(torch.isnan(self.t).all()) if self.fill != self.fill else bool((self.t == self.fill).all())


def act_in(a, dt, layout, off=0):
    """[B][C][S] float64 (already representable) -> the kernel's operand: storage type, NCHW or channels-last."""
    if a is None:
        return None
    b = Buf(a.size, TD[dt], off, fill=0.0)
    src = a.transpose(0, 2, 1) if layout else a
    b.t.copy_(torch.from_numpy(np.ascontiguousarray(src)).reshape(-1).to(TD[dt]))
    return b


def act_out(k, off=0):
    _, B, C, S = k["spec"][:4]
    return Buf(B * C * S, TD[k["dt"]], off)


def widen(buf, k):
    layout, B, C, S = k["spec"][:4]
    a = buf.t.double().cpu().numpy()
    return a.reshape(B, S, C).transpose(0, 2, 1) if layout else a.reshape(B, C, S)


def f32_in(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def mask_in(m):
    return None if m is None else torch.from_numpy(m).cuda()


class Workspace:
    """``nbytes`` of workspace (NaN doubles) between two sentinel regions; ``after`` widens the one behind it."""

    def __init__(self, nbytes, after=WS_GUARD):
        assert nbytes % 8 == 0
        after = -(-max(after, WS_GUARD) // 512) * 512
        self.raw = torch.full((WS_GUARD + nbytes + after,), SENT, dtype=torch.uint8, device="cuda")
        self.t = self.raw[WS_GUARD:WS_GUARD + nbytes]
        self.t.fill_(0xFF)
        self.nbytes = nbytes
        assert self.t.data_ptr() % 8 == 0

    def intact(self):
        return bool((self.raw[:WS_GUARD] == SENT).all()) and bool((self.raw[WS_GUARD + self.nbytes:] == SENT).all())


def workspace(layout, B, C, S, after=WS_GUARD):
    return Workspace(_lib().query("gmz_bn_workspace_bytes", layout, B, C, S), after)


def bits(t):
    """Bit-for-bit comparison key."""
    return t.contiguous().view(torch.uint8).cpu()


def same(a, b):
    return torch.equal(bits(a), bits(b))


def _offs(spec, names):
    return [2 if spec[8] == n else 0 for n in names]


def run_forward(k, entry="gmz_bn_forward", rmask=None):
    """One forward call on fresh NaN-filled outputs; returns the outputs."""
    L = _lib()
    layout, B, C, S, kind, use_res, relu, running, mis, offset = k["spec"]
    dt = k["dt"]
    ox, orr, oy = _offs(k["spec"], ("x", "res", "y"))
    x, res, y = act_in(k["x"], dt, layout, ox), act_in(k["res"], dt, layout, orr), act_out(k, oy)
    save = Buf(2 * C, torch.float32)
    rm, rv = (f32_in(k["rm"]), f32_in(k["rv"])) if running else (None, None)
    nb = torch.tensor([NB0], dtype=torch.int64, device="cuda") if running else None
    ws = workspace(layout, B, C, S)
    args = [dt, layout, x.t, res.t if res else None, mask_in(k["mask"]), B, C, S, f32_in(k["gamma"]), f32_in(k["beta"]),
            EPS, MOM, rm, rv, nb, int(relu), y.t, save.t, ws.t, ws.nbytes]
    if entry == "gmz_bn_forward_m":
        args.append(rmask.t)
    args.append(L.stream_ptr())
    out = dict(y=y, save=save, rm=rm, rv=rv, nb=nb, ws=ws)
    try:
        L.call(entry, *args)
    finally:
        torch.cuda.synchronize()
        out["guards"] = ws.intact() and y.intact() and save.intact()
    return out


def check_forward_outputs(k, o, L, N, tag=""):
    f, dt = k["f"], k["dt"]
    assert o["guards"]
    dmean, dvar, dis = stat_bounds(f, L, N)
    sv = o["save"].t.double().cpu().numpy().reshape(2, -1)
    within(tag + "save.mean", dt, sv[0], f["mean"], dmean)
    within(tag + "save.invstd", dt, sv[1], f["invstd"], dis)
    if o["y"] is not None:
        within(tag + "y", dt, widen(o["y"], k), f["y"], y_bound(k, k["x"], k["res"], f["mean"], f["invstd"], f["y"], dmean, dis))
    if o["rm"] is not None:
        if f["n"] == 0:  # untouched, exactly
            assert same(o["rm"], f32_in(k["rm"])) and same(o["rv"], f32_in(k["rv"])) and int(o["nb"]) == NB0
        else:
            drm, drv = running_bounds(f, k["rm"].astype(np.float64), k["rv"].astype(np.float64), dmean, dvar)
            within(tag + "running_mean", dt, o["rm"].double().cpu().numpy(), f["rm"], drm)
            within(tag + "running_var", dt, o["rv"].double().cpu().numpy(), f["rv"], drv)
            assert int(o["nb"]) == f["nb"] == NB0 + 1


def pack(y_bcs):
    """uint8 [B * S][C / 8]: bit j of byte [pixel][c / 8] = y > 0."""
    B, C, S = y_bcs.shape
    return np.packbits(y_bcs.transpose(0, 2, 1).reshape(B * S, C) > 0, axis=1, bitorder="little")


# ------------------------------------------------------------------------------------------------ forward
@gpu
@pytest.mark.parametrize("dt,spec", ALL, ids=IDS)
def test_forward(dt, spec):
    """gmz_bn_forward against the model; gmz_bn_forward_deferred(stats = NULL) leaves the same save and running
    statistics bit for bit (when both take the same vector width: the deferred form looks at x's alignment only);
    gmz_bn_forward_m equals it in every shared output and writes packbits(stored y > 0), or, with a misaligned
    operand or C % 8 != 0, refuses with the documented message and writes nothing."""
    _need_gpu()
    L = _lib()
    k = case(dt, spec)
    check_not_vacuous(k)
    layout, B, C, S, kind, use_res, relu, running, mis, offset = spec
    o = run_forward(k)
    check_forward_outputs(k, o, k["L"], k["N"])
    if not layout:
        return
    if mis in (None, "x", "dy", "dx", "dres"):
        save = Buf(2 * C, torch.float32)
        rm, rv = (f32_in(k["rm"]), f32_in(k["rv"])) if running else (None, None)
        nb = torch.tensor([NB0], dtype=torch.int64, device="cuda") if running else None
        ws = workspace(1, B, C, S)
        x = act_in(k["x"], dt, 1, 2 if mis == "x" else 0)
        L.call("gmz_bn_forward_deferred", dt, x.t, mask_in(k["mask"]), B, C, S, EPS, MOM, rm, rv, nb, save.t, None, 0, 0,
               ws.t, ws.nbytes, L.stream_ptr())
        torch.cuda.synchronize()
        assert ws.intact() and save.intact() and same(save.t, o["save"].t)
        if running:
            assert same(rm, o["rm"]) and same(rv, o["rv"]) and int(nb) == int(o["nb"])
    if not relu:
        return
    rmask = Buf(B * S * max(C // 8, 1), torch.uint8, fill=0x7F)
    if C % 8 == 0 and mis not in ("x", "res", "y"):
        m = run_forward(k, "gmz_bn_forward_m", rmask)
        assert m["guards"] and rmask.intact()
        assert same(m["y"].t, o["y"].t) and same(m["save"].t, o["save"].t)
        if running:
            assert same(m["rm"], o["rm"]) and same(m["rv"], o["rv"]) and int(m["nb"]) == int(o["nb"])
        want = pack(widen(o["y"], k))
        assert np.array_equal(rmask.t.cpu().numpy().reshape(want.shape), want)
    else:
        with pytest.raises(L.GmzError, match=REFUSAL):
            m = run_forward(k, "gmz_bn_forward_m", rmask)
        assert rmask.untouched() and rmask.intact()


@gpu
@pytest.mark.parametrize("dt", [0, 1, 2])
def test_refusals_write_nothing(dt):
    """One of running_mean / running_var alone is refused by every forward entry point; the *_m entry points refuse
    a misaligned operand; a refused call leaves its outputs as they were."""
    _need_gpu()
    L = _lib()
    B, C, S = 5, 128, 25
    k = case(dt, _c(1, B, C, S))
    x, res = act_in(k["x"], dt, 1), act_in(k["res"], dt, 1)
    g, b, rm = f32_in(k["gamma"]), f32_in(k["beta"]), f32_in(k["rm"])
    parts = torch.zeros(C * 3, dtype=torch.float64, device="cuda")
    st = L.stream_ptr()
    for entry in ("gmz_bn_forward", "gmz_bn_forward_m", "gmz_bn_forward_stats", "gmz_bn_forward_stats_m",
                  "gmz_bn_forward_deferred", "gmz_bn_forward_seg", "gmz_bn_forward_m misaligned",
                  "gmz_bn_forward_stats_m misaligned"):
        for pair in ((rm, None), (None, rm)):
            y, save, ws = act_out(k), Buf(2 * C, torch.float32), workspace(1, B, C, S)
            rmask = Buf(B * S * C // 8, torch.uint8, fill=0x7F)
            head = [dt, x.t, res.t]
            tail = [B, C, S, g, b, EPS, MOM, pair[0], pair[1], None, 1, y.t, save.t]
            msg = "running stats pair"
            if entry.endswith("misaligned"):
                y, msg = act_out(k, 2), REFUSAL
                tail = [B, C, S, g, b, EPS, MOM, None, None, None, 1, y.t, save.t]
            with pytest.raises(L.GmzError, match=msg):
                if entry == "gmz_bn_forward":
                    L.call(entry, dt, 1, x.t, res.t, None, *tail, ws.t, ws.nbytes, st)
                elif entry.startswith("gmz_bn_forward_m"):
                    L.call("gmz_bn_forward_m", dt, 1, x.t, res.t, None, *tail, ws.t, ws.nbytes, rmask.t, st)
                elif entry == "gmz_bn_forward_stats":
                    L.call(entry, *head, *tail, parts, 1, C * 24, st)
                elif entry.startswith("gmz_bn_forward_stats_m"):
                    L.call("gmz_bn_forward_stats_m", *head, *tail, parts, 1, C * 24, rmask.t, st)
                elif entry == "gmz_bn_forward_deferred":
                    L.call(entry, dt, x.t, None, B, C, S, EPS, MOM, pair[0], pair[1], None, save.t, None, 0, 0, ws.t,
                           ws.nbytes, st)
                else:
                    L.call(entry, dt, x.t, res.t, None, B, 1, C, S, g, b, EPS, MOM, pair[0], pair[1], None, 1, y.t, save.t,
                           ws.t, ws.nbytes, None, 0, st)
            torch.cuda.synchronize()
            assert y.untouched() and save.untouched() and rmask.untouched() and ws.intact()
            assert bool((ws.t == 0xFF).all())


# ------------------------------------------------------------------------------------------------ backward
def run_backward(k, entry, accumulate=None, preset=None, rmask=None, stats=None, keep=None):
    L = _lib()
    layout, B, C, S, kind, use_res, relu, running, mis, offset = k["spec"]
    dt = k["dt"]
    ox, oy, ody, odx, odr = _offs(k["spec"], ("x", "y", "dy", "dx", "dres"))
    x, y, dy = act_in(k["x"], dt, layout, ox), act_in(k["y_st"], dt, layout, oy), act_in(k["dy"], dt, layout, ody)
    dx, dres = act_out(k, odx), (act_out(k, odr) if use_res else None)
    dg, db = Buf(C, torch.float32), Buf(C, torch.float32)
    if preset is not None:
        dg.t.copy_(preset[0])
        db.t.copy_(preset[1])
    ws = workspace(layout, B, C, S)
    if keep is not None:  # the outputs of a call that is expected to raise
        keep.update(dx=dx, dres=dres, dgamma=dg, dbeta=db, ws=ws)
    args = [dt] + ([] if stats is not None else [layout]) + [
        x.t, y.t, dy.t, mask_in(k["mask"]), B, C, S, f32_in(k["gamma"]), f32_in(k["save"]), int(relu), dx.t,
        dres.t if dres else None, dg.t, db.t]
    if stats is not None:
        args += [stats, stats.numel() // (3 * C), stats.numel() * 8]
    args += [ws.t, ws.nbytes]
    if rmask is not None:
        args.append(rmask)
    args.append(L.stream_ptr())
    if accumulate is not None:
        args.append(accumulate)
    try:
        L.call(entry, *args)
    finally:
        torch.cuda.synchronize()
        ok = ws.intact() and dx.intact() and dg.intact() and db.intact() and (dres is None or dres.intact())
    return dict(dx=dx, dres=dres, dgamma=dg, dbeta=db, guards=ok)


def check_backward_outputs(k, o, L, N, tag=""):
    bw, dt = k["bw"], k["dt"]
    assert o["guards"]
    dbeta, dgamma, dxb = grad_bounds(k, L, N)
    within(tag + "dbeta", dt, o["dbeta"].t.double().cpu().numpy(), bw["dbeta"], dbeta)
    within(tag + "dgamma", dt, o["dgamma"].t.double().cpu().numpy(), bw["dgamma"], dgamma)
    within(tag + "dx", dt, widen(o["dx"], k), bw["dx"], dxb)
    if o["dres"] is not None:  # dz is dy or 0: nothing to round
        got = widen(o["dres"], k)
        assert np.isfinite(got).all() and np.array_equal(got, bw["dres"])


def same_grads(a, b):
    return (same(a["dx"].t, b["dx"].t) and same(a["dgamma"].t, b["dgamma"].t) and same(a["dbeta"].t, b["dbeta"].t)
            and (a["dres"] is None or same(a["dres"].t, b["dres"].t)))


@gpu
@pytest.mark.parametrize("dt,spec", ALL, ids=IDS)
def test_backward(dt, spec):
    """gmz_bn_backward_acc(accumulate = 0) against the model, from the MODEL's y and save; gmz_bn_backward equals
    it bit for bit; accumulate = 1 onto preset gradients gives float32(preset + that result); gmz_bn_backward_acc_m
    fed packbits(stored y > 0) equals the plain form, or refuses a misaligned operand / C % 8 != 0."""
    _need_gpu()
    L = _lib()
    k = case(dt, spec)
    layout, B, C, S, kind, use_res, relu, running, mis, offset = spec
    o = run_backward(k, "gmz_bn_backward_acc", accumulate=0)
    check_backward_outputs(k, o, k["L"], k["N"])
    assert same_grads(run_backward(k, "gmz_bn_backward"), o)
    preset = (torch.linspace(-3, 5, C, device="cuda"), torch.linspace(0.25, -7, C, device="cuda"))
    a = run_backward(k, "gmz_bn_backward_acc", accumulate=1, preset=preset)
    assert a["guards"] and same(a["dx"].t, o["dx"].t)
    assert same(a["dgamma"].t, preset[0] + o["dgamma"].t) and same(a["dbeta"].t, preset[1] + o["dbeta"].t)
    if not (layout and relu):
        return
    rmask = torch.from_numpy(pack(k["y_st"])).cuda() if C % 8 == 0 else torch.zeros(B * S, dtype=torch.uint8, device="cuda")
    if C % 8 == 0 and mis in (None, "res"):
        for acc, ref in ((0, o), (1, a)):
            m = run_backward(k, "gmz_bn_backward_acc_m", accumulate=acc, preset=preset if acc else None, rmask=rmask)
            assert m["guards"] and same_grads(m, ref)
    else:
        kept = {}
        with pytest.raises(L.GmzError, match=REFUSAL):
            run_backward(k, "gmz_bn_backward_acc_m", accumulate=0, rmask=rmask, keep=kept)
        assert all(kept[n].untouched() and kept[n].intact() for n in ("dx", "dgamma", "dbeta"))
        assert kept["ws"].intact() and bool((kept["ws"].t == 0xFF).all())


# ------------------------------------------------------------------------------------------------ partials
STATS_CASES = [_c(1, 37, 128, 36), _c(1, 5, 8, 25, "null", res=False), _c(1, 17, 6, 1, relu=False),
               _c(1, 5, 128, 25, "zeros")]


@gpu
@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("spec", STATS_CASES, ids=lambda s: "B%dC%dS%d-%s" % (s[1], s[2], s[3], s[4]))
def test_entry_points_fed_partials_do_not_depend_on_the_cut(dt, spec):
    """gmz_bn_forward_stats, _stats_m, _deferred(stats) and gmz_bn_backward_stats fed the model's exact f64
    partials, the pixels cut into ns = 1, 5 and 300 ranges (empty ranges, ranges fully masked out): within the
    bounds with L = 0 whatever the cut, and two cuts agree to the f32 roundings the f64 noise can flip (mean: one,
    <= 2u; invstd: var, var + eps, sqrtf, the division, <= 8u; a gradient sum: one)."""
    _need_gpu()
    L = _lib()
    k = case(dt, spec)
    _, B, C, S, kind, use_res, relu, running, mis, offset = spec
    P = B * S
    bw = k["bw"]
    st = L.stream_ptr()
    prev = None
    for ns, seed in ((1, 0), (5, 1), (300, 2), (5, 3)):
        bounds = R.cuts(P, ns, seed)
        parts = torch.from_numpy(R.partials(k["x"], k["x"] * k["x"], k["mask"], bounds)).cuda()
        assert parts.shape == (C, ns, 3)
        x, res, y = act_in(k["x"], dt, 1), act_in(k["res"], dt, 1), act_out(k)
        save = Buf(2 * C, torch.float32)
        rm, rv, nb = f32_in(k["rm"]), f32_in(k["rv"]), torch.tensor([NB0], dtype=torch.int64, device="cuda")
        g, b = f32_in(k["gamma"]), f32_in(k["beta"])
        L.call("gmz_bn_forward_stats", dt, x.t, res.t if res else None, B, C, S, g, b, EPS, MOM, rm, rv, nb, int(relu),
               y.t, save.t, parts, ns, parts.numel() * 8, st)
        torch.cuda.synchronize()
        o = dict(y=y, save=save, rm=rm, rv=rv, nb=nb, guards=y.intact() and save.intact())
        check_forward_outputs(k, o, 0, P, "stats.")
        # the deferred form: the same finalisation, no elementwise pass
        save2 = Buf(2 * C, torch.float32)
        rm2, rv2, nb2 = f32_in(k["rm"]), f32_in(k["rv"]), torch.tensor([NB0], dtype=torch.int64, device="cuda")
        L.call("gmz_bn_forward_deferred", dt, None, None, B, C, S, EPS, MOM, rm2, rv2, nb2, save2.t, parts, ns,
               parts.numel() * 8, None, 0, st)
        torch.cuda.synchronize()
        assert save2.intact() and same(save2.t, save.t) and same(rm2, rm) and same(rv2, rv) and int(nb2) == int(nb)
        if relu and C % 8 == 0:
            y3, save3, rmask = act_out(k), Buf(2 * C, torch.float32), Buf(P * C // 8, torch.uint8, fill=0x7F)
            rm3, rv3, nb3 = f32_in(k["rm"]), f32_in(k["rv"]), torch.tensor([NB0], dtype=torch.int64, device="cuda")
            L.call("gmz_bn_forward_stats_m", dt, x.t, res.t if res else None, B, C, S, g, b, EPS, MOM, rm3, rv3, nb3, 1,
                   y3.t, save3.t, parts, ns, parts.numel() * 8, rmask.t, st)
            torch.cuda.synchronize()
            assert y3.intact() and rmask.intact() and same(y3.t, y.t) and same(save3.t, save.t)
            assert same(rm3, rm) and same(rv3, rv) and int(nb3) == int(nb)
            want = pack(widen(y, k))
            assert np.array_equal(rmask.t.cpu().numpy().reshape(want.shape), want)
        gparts = torch.from_numpy(R.partials(bw["dz"], bw["dz"] * bw["xhat"], k["mask"], R.cuts(P, ns, seed + 10))).cuda()
        ob = run_backward(k, "gmz_bn_backward_stats", accumulate=0, stats=gparts)
        check_backward_outputs(k, ob, 0, P, "stats.")
        cur = (save.t.double().cpu().numpy().reshape(2, C), ob["dgamma"].t.double().cpu().numpy(),
               ob["dbeta"].t.double().cpu().numpy())
        if prev is not None:
            assert (np.abs(cur[0][0] - prev[0][0]) <= 2 * U * np.abs(k["f"]["mean"]) + 2.0 ** -150).all()
            assert (np.abs(cur[0][1] - prev[0][1]) <= 8 * U * k["f"]["invstd"]).all()
            assert (np.abs(cur[1] - prev[1]) <= 2 * U * np.abs(bw["dgamma"]) + P * 2.0 ** -52 * bw["sabs_dzx"]).all()
            assert (np.abs(cur[2] - prev[2]) <= 2 * U * np.abs(bw["dbeta"]) + P * 2.0 ** -52 * bw["sabs_dz"]).all()
        prev = cur


# ------------------------------------------------------------------------------------------------ segments
# (nseg, B, S, C, mask kind): the last three have segments of fewer than 16 pixels
SEG_CASES = [(1, 5, 25, 144, "rand"), (2, 6, 25, 128, "deadseg"), (6, 12, 9, 8, "rand"), (2, 6, 25, 8, "zeros"),
             (6, 12, 9, 128, "null"), (6, 6, 9, 8, "deadseg"), (32, 32, 4, 128, "rand"), (2, 2, 9, 8, "null")]


@gpu
@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("board_stats", [False, True], ids=["reduce", "board_stats"])
@pytest.mark.parametrize("sc", SEG_CASES, ids=lambda s: "nseg%d-B%dS%dC%d-%s" % s)
def test_forward_seg(dt, board_stats, sc):
    """gmz_bn_forward_seg against the model: per-segment save and y, the running statistics equal to the segments
    applied in order with empty segments skipped.  Segments of fewer than 16 pixels need C * nseg * 24 bytes for
    their partials, more than gmz_bn_workspace_bytes: without board_stats the call on that workspace is refused
    before any launch, naming the size, and succeeds on a workspace of that size (a sentinel region of at least
    C * nseg * 24 bytes follows the workspace either way)."""
    _need_gpu()
    L = _lib()
    nseg, B, S, C, kind = sc
    rs = np.random.RandomState(nseg * 1000 + B * 10 + C + dt)
    x, res = _round(rs.randn(B, C, S) * 2 + 0.5, dt), _round(rs.randn(B, C, S), dt)
    rows = B // nseg
    if kind == "deadseg":  # one segment with no live row
        mask = np.ones(B, np.uint8)
        mask[rows:2 * rows] = 0
        if rows > 1:
            mask[0] = 0
    else:
        mask = _mask(kind, B, rs)
    gamma, beta = rs.uniform(0.5, 1.5, C).astype(np.float32), rs.uniform(-0.3, 0.3, C).astype(np.float32)
    rm, rv = rs.randn(C).astype(np.float32), rs.uniform(0.5, 2.0, C).astype(np.float32)
    segs, erm, erv, enb = R.forward_seg(x, mask, nseg, gamma.astype(np.float64), beta.astype(np.float64), EPS, MOM, res,
                                        True, rm.astype(np.float64), rv.astype(np.float64), NB0)
    if kind == "deadseg":
        assert segs[1]["n"] == 0 and segs[0]["n"] > 0 and enb == NB0 + nseg - 1
    k = dict(spec=_c(1, B, C, S), dt=dt, gamma=gamma, beta=beta)
    need = L.query("gmz_bn_workspace_bytes", 1, B, C, S)
    seg_need = C * nseg * 24
    small = rows * S < 16
    parts = torch.from_numpy(R.board_partials(x, mask)).cuda() if board_stats else None
    st = L.stream_ptr()

    def call(ws):
        xd, rd, y, save = act_in(x, dt, 1), act_in(res, dt, 1), act_out(k), Buf(nseg * 2 * C, torch.float32)
        rmd, rvd, nb = f32_in(rm), f32_in(rv), torch.tensor([NB0], dtype=torch.int64, device="cuda")
        try:
            L.call("gmz_bn_forward_seg", dt, xd.t, rd.t, mask_in(mask), B, nseg, C, S, f32_in(gamma), f32_in(beta), EPS,
                   MOM, rmd, rvd, nb, 1, y.t, save.t, ws.t, ws.nbytes, parts, parts.numel() * 8 if board_stats else 0, st)
        finally:
            torch.cuda.synchronize()
            assert ws.intact() and y.intact() and save.intact()
        return y, save, rmd, rvd, nb

    ws = Workspace(need, after=seg_need)
    if small and not board_stats:
        assert seg_need > need - C * 8
        with pytest.raises(L.GmzError, match="workspace of %d bytes.*need %d" % (need, seg_need)):
            call(ws)
        assert bool((ws.t == 0xFF).all())
        ws = Workspace(max(need, seg_need), after=seg_need)
    y, save, rmd, rvd, nb = call(ws)
    sv = save.t.double().cpu().numpy().reshape(nseg, 2, C)
    yk = widen(y, k)
    Lr = 0 if board_stats else _split_len(B * S, nseg)
    crm, crv = rm.astype(np.float64), rv.astype(np.float64)
    drm_acc, drv_acc = np.zeros(C), np.zeros(C)
    for g, f in enumerate(segs):
        sl = slice(g * rows, (g + 1) * rows)
        dmean, dvar, dis = stat_bounds(f, Lr, rows * S)
        within("seg.save.mean", dt, sv[g, 0], f["mean"], dmean)
        within("seg.save.invstd", dt, sv[g, 1], f["invstd"], dis)
        within("seg.y", dt, yk[sl], f["y"], y_bound(k, x[sl], res[sl], f["mean"], f["invstd"], f["y"], dmean, dis))
        if f["n"]:  # a step's error: its own roundings plus (1 - m) times what the steps before it left
            drm, drv = running_bounds(f, crm, crv, dmean, dvar)
            drm_acc, drv_acc = (1 - MOM) * drm_acc + drm, (1 - MOM) * drv_acc + drv
            crm, crv = f["rm"], f["rv"]
    if enb == NB0:
        assert same(rmd, f32_in(rm)) and same(rvd, f32_in(rv))
    else:
        within("seg.running_mean", dt, rmd.double().cpu().numpy(), erm, drm_acc)
        within("seg.running_var", dt, rvd.double().cpu().numpy(), erv, drv_acc)
    assert int(nb) == enb


# ------------------------------------------------------------------------------------------------ eval
EVAL_CASES = [_c(1, 5, 128, 25), _c(1, 37, 144, 36, res=False), _c(1, 17, 6, 1, relu=False), _c(1, 5, 128, 25, mis="res"),
              _c(0, 33, 16, 36), _c(0, 5, 3, 1, res=False), _c(0, 1, 512, 36, relu=False)]


@gpu
@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("spec", EVAL_CASES, ids=lambda s: "%s-B%dC%dS%d%s" % ("nhwc" if s[0] else "nchw", s[1], s[2], s[3],
                                                                              "-mis" if s[8] else ""))
def test_eval(dt, spec):
    """gmz_bn_eval against the model: the running statistics instead of the batch's."""
    _need_gpu()
    L = _lib()
    k = case(dt, spec)
    layout, B, C, S, kind, use_res, relu, running, mis, offset = spec
    e = R.evaluate(k["x"], k["gamma"].astype(np.float64), k["beta"].astype(np.float64), k["rm"].astype(np.float64),
                   k["rv"].astype(np.float64), EPS, k["res"], relu)
    if relu:
        assert (e["y"] == 0).mean() >= 0.2 and (e["y"] > 0).mean() >= 0.2
    ox, orr, oy = _offs(spec, ("x", "res", "y"))
    x, res, y = act_in(k["x"], dt, layout, ox), act_in(k["res"], dt, layout, orr), act_out(k, oy)
    ws = workspace(layout, B, C, S)
    L.call("gmz_bn_eval", dt, layout, x.t, res.t if res else None, B, C, S, f32_in(k["gamma"]), f32_in(k["beta"]),
           f32_in(k["rm"]), f32_in(k["rv"]), EPS, int(relu), y.t, ws.t, ws.nbytes, L.stream_ptr())
    torch.cuda.synchronize()
    assert ws.intact() and y.intact()
    within("eval.y", dt, widen(y, k), e["y"],
           y_bound(k, k["x"], k["res"], e["mean"], e["invstd"], e["y"], np.zeros(C), e["invstd"] * 4.5 * U))
