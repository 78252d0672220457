"""Float64 model of the row-masked BatchNorm family (the gmz_bn_* contract of include/gmz.h), in plain numpy.

Every function takes activations as float64 arrays of shape [B][C][S] (S = 1 for BatchNorm1d) holding the inputs
AS STORED (16-bit inputs widened exactly), whatever layout the kernel under test reads, and returns float64.  The
model imports nothing from the package under test; tests/test_bn_ref.py pins it to torch.nn.BatchNorm1d/2d in
float64.

  statistics  valid rows = mask[b] != 0 (mask None: every row), n = valid rows * S,
              mean = sum x / n, var = max(sum x^2 / n - mean^2, 0), invstd = 1 / sqrt(var + eps);
              n = 0: mean = 0, var = 0, running statistics and num_batches untouched, every row still normalised
  forward     y = relu?((x - mean) * gamma * invstd + beta (+ res)), save = (mean, invstd),
              running_mean = (1 - m) rm + m mean, running_var = (1 - m) rv + m var n / (n - 1) (m var when n = 1),
              num_batches += 1
  backward    dz = dy * [y > 0] on the y handed in (or dy without ReLU), dbeta = sum_valid dz,
              dgamma = sum_valid dz * xhat, xhat = (x - mean) * invstd with the (mean, invstd) handed in,
              dx = gamma invstd (dz - dbeta / n - xhat dgamma / n) on valid rows, gamma invstd dz on the others,
              dres = dz
"""
import numpy as np


def _rows(mask, B):
    return np.ones(B, bool) if mask is None else (np.asarray(mask) != 0)


def stats(x, mask=None):
    """n, and per channel: mean, biased variance, E|x|, E[x^2] over the valid rows (zeros when n = 0)."""
    B, C, S = x.shape
    v = _rows(mask, B)
    n = int(v.sum()) * S
    if n == 0:
        z = np.zeros(C)
        return 0, z, z.copy(), z.copy(), z.copy()
    xv = x[v]
    mean = xv.sum(axis=(0, 2)) / n
    ex2 = (xv * xv).sum(axis=(0, 2)) / n
    var = np.maximum(ex2 - mean * mean, 0.0)
    return n, mean, var, np.abs(xv).sum(axis=(0, 2)) / n, ex2


def running_update(n, mean, var, rm, rv, nb, momentum):
    """nn.BatchNorm's training-mode update (unbiased variance; the biased one when n = 1); untouched when n = 0."""
    if n == 0 or rm is None:
        return rm, rv, nb
    unb = var * n / (n - 1) if n > 1 else var
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unb, None if nb is None else nb + 1


def apply(x, mean, invstd, gamma, beta, res=None, relu=False):
    """The elementwise pass: the value before the ReLU and the output."""
    c = (None, slice(None), None)
    pre = (x - mean[c]) * (gamma * invstd)[c] + beta[c]
    if res is not None:
        pre = pre + res
    return pre, (np.maximum(pre, 0.0) if relu else pre)


def forward(x, mask, gamma, beta, eps, momentum, res=None, relu=False, rm=None, rv=None, nb=None):
    n, mean, var, eabs, ex2 = stats(x, mask)
    invstd = 1.0 / np.sqrt(var + eps)
    pre, y = apply(x, mean, invstd, gamma, beta, res, relu)
    rm2, rv2, nb2 = running_update(n, mean, var, rm, rv, nb, momentum)
    return dict(n=n, mean=mean, var=var, invstd=invstd, eabs=eabs, ex2=ex2, pre=pre, y=y, rm=rm2, rv=rv2, nb=nb2)


def forward_seg(x, mask, nseg, gamma, beta, eps, momentum, res=None, relu=False, rm=None, rv=None, nb=None):
    """nseg equal row segments, each over its own valid rows; the running statistics updated segment after segment
    (an empty segment is skipped).  Returns the per-segment forward() results and the final running statistics."""
    B = x.shape[0]
    rows = B // nseg
    segs = []
    for g in range(nseg):
        sl = slice(g * rows, (g + 1) * rows)
        f = forward(x[sl], None if mask is None else np.asarray(mask)[sl], gamma, beta, eps, momentum,
                    None if res is None else res[sl], relu, rm, rv, nb)
        rm, rv, nb = f["rm"], f["rv"], f["nb"]
        segs.append(f)
    return segs, rm, rv, nb


def evaluate(x, gamma, beta, rm, rv, eps, res=None, relu=False):
    """gmz_bn_eval: the running statistics instead of the batch's."""
    invstd = 1.0 / np.sqrt(rv + eps)
    pre, y = apply(x, rm, invstd, gamma, beta, res, relu)
    return dict(mean=rm, invstd=invstd, pre=pre, y=y)


def backward(x, y, dy, mask, gamma, mean, invstd, relu=False):
    """The gradients from the (mean, invstd) and the y handed in (the stored values the kernel reads)."""
    B, C, S = x.shape
    v = _rows(mask, B)
    n = int(v.sum()) * S
    c = (None, slice(None), None)
    dz = dy * (y > 0) if relu else dy.copy()
    xhat = (x - mean[c]) * invstd[c]
    dbeta = dz[v].sum(axis=(0, 2))
    dgamma = (dz[v] * xhat[v]).sum(axis=(0, 2))
    mg = dbeta / n if n else np.zeros(C)
    mgx = dgamma / n if n else np.zeros(C)
    k1 = (gamma * invstd)[c]
    dx = k1 * dz
    dx[v] = k1 * (dz[v] - mg[c] - xhat[v] * mgx[c])
    return dict(n=n, dz=dz, xhat=xhat, dx=dx, dres=dz, dgamma=dgamma, dbeta=dbeta, mg=mg, mgx=mgx,
                sabs_dz=np.abs(dz[v]).sum(axis=(0, 2)), sabs_dzx=np.abs(dz[v] * xhat[v]).sum(axis=(0, 2)))


def cuts(P, ns, seed=0, empty=True):
    """ns + 1 sorted boundaries 0 = c[0] <= ... <= c[ns] = P of ns contiguous pixel ranges; with ``empty`` (and
    ns > 1) some ranges are empty."""
    rs = np.random.RandomState(seed)
    inner = np.sort(rs.randint(0, P + 1, size=ns - 1))
    if empty and ns > 2:
        inner[1] = inner[0]
    return np.concatenate([[0], inner, [P]]).astype(np.int64)


def partials(a, b, mask, bounds):
    """Exact-in-f64 partial sums [C][ns][3] = (sum a, sum b, valid pixels) of the pixels (pixel = row * S + s) in
    each range [bounds[t], bounds[t + 1]), over the valid rows only.  A range may be empty or fully masked out.
    Forward statistics: a = x, b = x * x.  Backward: a = dz, b = dz * xhat."""
    B, C, S = a.shape
    v = _rows(mask, B)
    pv = np.repeat(v, S)  # per pixel
    af = a.transpose(0, 2, 1).reshape(B * S, C)
    bf = b.transpose(0, 2, 1).reshape(B * S, C)
    ns = len(bounds) - 1
    out = np.zeros((C, ns, 3))
    for t in range(ns):
        lo, hi = int(bounds[t]), int(bounds[t + 1])
        sel = pv[lo:hi]
        out[:, t, 0] = af[lo:hi][sel].sum(axis=0)
        out[:, t, 1] = bf[lo:hi][sel].sum(axis=0)
        out[:, t, 2] = float(sel.sum())
    return out


def board_partials(x, mask):
    """The per-board form [C][B][3]: one range per row (zeros for a masked-out row)."""
    B, _, S = x.shape
    return partials(x, x * x, mask, np.arange(B + 1, dtype=np.int64) * S)


def stats_from_partials(parts):
    """n, mean, biased variance from partials [C][ns][3] (what the finalisation computes)."""
    a, b, n = parts[:, :, 0].sum(axis=1), parts[:, :, 1].sum(axis=1), parts[:, :, 2].sum(axis=1)
    nn = np.where(n > 0, n, 1.0)
    mean = a / nn
    return n, mean, np.maximum(b / nn - mean * mean, 0.0)
