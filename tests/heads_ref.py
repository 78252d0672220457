"""Float64 models of the heads' kernels (csrc/gmz_heads.hip; the gmz_head_conv1x1_* and gmz_seg_bn_* contracts of
include/gmz.h), in plain numpy.  Nothing here imports the package under test; tests/test_heads_ref.py pins the
models to torch float64 (conv2d, nn.BatchNorm1d/2d, autograd).

Head conv (x [P][128] as stored, widened exactly; dtype 0 = f32, 1 = f16, 2 = bf16)
  W, b      rounded to x's dtype first (the f32 parameters under autocast)
  forward   y[p][o] = round_T(sum_c x[p][c] W[o][c] + b[o]): ONE rounding of the exact value; head 0 owns the first
            O0 rows, head 1 the next O1 (O1 = 0: no second head)
  backward  dx[p][c] = round_T(sum_o dy[p][o] W[o][c]) over the rows of BOTH heads; dW[o][c] = sum_p dy[p][o] x[p][c],
            db[o] = sum_p dy[p][o] (float64 sums), written, or added to what the destination held (accumulate); a
            NULL destination is skipped

Segmented BatchNorm (x [nseg*B][S][C] as stored, row mask uint8 [nseg*B] or None) — ONE model for the general and the
few-channel variant
  segment   n = live rows * S; mean = sum_live x / n, var = max(sum_live x^2 / n - mean^2, 0) (biased),
            invstd = 1 / sqrt(var + eps).  n = 0: mean = 0, var = 0, invstd = 1 / sqrt(eps)
  y         (x - mean) invstd gamma + beta for EVERY row of the segment, live or not
  stats     [mean (nseg, C) | invstd (nseg, C) | unbiased var (nseg, C) | live rows (nseg)]; the unbiased variance is
            var n / (n - 1), and the biased var itself when n <= 1
  running   segment after segment: first pre_stats' segment s (when pre_stats is given and ITS live-row count of s
            is > 0), then this call's segment s (when it has a live row); each update is
            rm = (1 - m) rm + m mean, rv = (1 - m) rv + m unbiased var (the biased one at n = 1);
            num_batches += the updates made
  backward  xhat = (x - mean) invstd with the (mean, invstd, live rows) HANDED IN; per segment G1 = sum dy,
            G2 = sum dy xhat over EVERY row; dx = gamma invstd (dy - w (G1 + xhat G2) / n), w = 1 on live rows, 0 on
            the others (n = 0: dx = gamma invstd dy); dgamma = sum_s G2, dbeta = sum_s G1, written or added
"""
import numpy as np

from bn_ref import running_update, stats as bn_stats
from conv_ref import round_to as _round16

HC = 128


def round_to(a, dtype):
    """float64 -> the storage type (0 = f32, 1 = f16, 2 = bf16), one rounding to nearest even, as float64."""
    a = np.asarray(a, np.float64)
    return a.astype(np.float32).astype(np.float64) if dtype == 0 else _round16(a, dtype)


# ------------------------------------------------------------------------------------------------ head conv
def head_weights(w0, b0, w1, b1, dtype):
    """(W [O][128], b [O]) rounded to dtype; b = 0 where a head has no bias.  w1 None: O1 = 0."""
    ws = [np.asarray(w0, np.float64).reshape(-1, HC)] + ([] if w1 is None else [np.asarray(w1, np.float64).reshape(-1, HC)])
    bs = [np.zeros(len(ws[0])) if b0 is None else np.asarray(b0, np.float64)]
    if w1 is not None:
        bs.append(np.zeros(len(ws[1])) if b1 is None else np.asarray(b1, np.float64))
    return round_to(np.concatenate(ws), dtype), round_to(np.concatenate(bs), dtype)


def head_forward(x, w0, b0, w1, b1, dtype):
    """exact = x W^T + b (float64, before the store), y = round_T(exact), sabs = sum_c |x W| + |b|."""
    W, b = head_weights(w0, b0, w1, b1, dtype)
    exact = x @ W.T + b
    return dict(W=W, b=b, exact=exact, y=round_to(exact, dtype), sabs=np.abs(x) @ np.abs(W).T + np.abs(b))


def head_backward(x, dy, w0, w1, dtype, acc=None):
    """dy [P][O0 + O1] (both heads side by side).  acc: (dW, db) float64 already in the destinations (accumulate)."""
    W, _ = head_weights(w0, None, w1, None, dtype)
    exact = dy @ W
    dW, db = dy.T @ x, dy.sum(axis=0)
    out = dict(W=W, dx_exact=exact, dx=round_to(exact, dtype), sabs_dx=np.abs(dy) @ np.abs(W), dW_sum=dW, db_sum=db,
               sabs_dW=np.abs(dy).T @ np.abs(x), sabs_db=np.abs(dy).sum(axis=0))
    out["dW"], out["db"] = (dW, db) if acc is None else (acc[0] + dW, acc[1] + db)
    return out


# ------------------------------------------------------------------------------------------------ segmented BatchNorm
def _seg(a, sg, B):
    return a[sg * B:(sg + 1) * B]


def seg_forward(x, mask, nseg, gamma, beta, eps, momentum=None, rm=None, rv=None, nb=None, pre=None):
    """x [nseg*B][S][C].  pre: an earlier call's stats dict(mean, unb, rows) whose update goes first per segment.
    Returns per (segment, channel) mean, var, invstd, unb, eabs, ex2; rows [nseg]; y; the running statistics."""
    R, S, C = x.shape
    B = R // nseg
    g = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    bt = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    mean, var, eabs, ex2 = (np.zeros((nseg, C)) for _ in range(4))
    rows, n = np.zeros(nseg, np.int64), np.zeros(nseg, np.int64)
    for sg in range(nseg):
        m = None if mask is None else _seg(np.asarray(mask), sg, B)
        n[sg], mean[sg], var[sg], eabs[sg], ex2[sg] = bn_stats(_seg(x, sg, B).transpose(0, 2, 1), m)
        rows[sg] = n[sg] // S
    invstd = 1.0 / np.sqrt(var + eps)
    fac = np.where(n > 1, n / np.maximum(n - 1.0, 1.0), 1.0)
    unb = var * fac[:, None]
    y = np.empty_like(x)
    for sg in range(nseg):
        _seg(y, sg, B)[:] = (_seg(x, sg, B) - mean[sg]) * invstd[sg] * g + bt
    if rm is not None:
        for sg in range(nseg):
            if pre is not None and pre["rows"][sg] > 0:  # the stored unbiased variance goes in as it is
                rm, rv = (1 - momentum) * rm + momentum * pre["mean"][sg], (1 - momentum) * rv + momentum * pre["unb"][sg]
                nb = None if nb is None else nb + 1
            rm, rv, nb = running_update(int(n[sg]), mean[sg], var[sg], rm, rv, nb, momentum)
    return dict(n=n, rows=rows, mean=mean, var=var, invstd=invstd, unb=unb, eabs=eabs, ex2=ex2, y=y, rm=rm, rv=rv, nb=nb)


def stats_vector(f):
    """The stats buffer [mean | invstd | unbiased var | live rows] as float64."""
    return np.concatenate([f["mean"].ravel(), f["invstd"].ravel(), f["unb"].ravel(), f["rows"].astype(np.float64)])


def seg_backward(x, dy, mask, nseg, gamma, mean, invstd, rows, acc=None):
    """The gradients from the (mean [nseg][C], invstd [nseg][C], rows [nseg]) handed in."""
    R, S, C = x.shape
    B = R // nseg
    g = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    live = np.ones(R, bool) if mask is None else (np.asarray(mask) != 0)
    dx, xhat = np.empty_like(x), np.empty_like(x)
    G1, G2, A1, A2 = (np.zeros((nseg, C)) for _ in range(4))
    c1, c2 = np.zeros((nseg, C)), np.zeros((nseg, C))
    for sg in range(nseg):
        xs, ds = _seg(x, sg, B), _seg(dy, sg, B)
        xh = (xs - mean[sg]) * invstd[sg]
        _seg(xhat, sg, B)[:] = xh
        G1[sg], G2[sg] = ds.sum(axis=(0, 1)), (ds * xh).sum(axis=(0, 1))
        A1[sg], A2[sg] = np.abs(ds).sum(axis=(0, 1)), np.abs(ds * xh).sum(axis=(0, 1))
        n = float(rows[sg]) * S
        if n > 0:
            c1[sg], c2[sg] = G1[sg] / n, G2[sg] / n
        w = _seg(live, sg, B)[:, None, None].astype(np.float64)
        _seg(dx, sg, B)[:] = g * invstd[sg] * (ds - w * (c1[sg] + xh * c2[sg]))
    dgamma, dbeta = G2.sum(axis=0), G1.sum(axis=0)
    if acc is not None:
        dgamma, dbeta = acc[0] + dgamma, acc[1] + dbeta
    return dict(dx=dx, xhat=xhat, G1=G1, G2=G2, A1=A1, A2=A2, c1=c1, c2=c2, dgamma=dgamma, dbeta=dbeta, live=live)
