"""Float64 model of the f16/bf16 3x3 convolution family (the gmz_conv3x3_* contract of include/gmz.h), in plain numpy.

Activations are float64 arrays [N][H*H][128] (channels-last, position p = row * H + column) holding the inputs AS
STORED (16-bit values widened exactly); weights are float64 [O][C][3][3].  Tap t = 3 ky + kx reads the cell at
offset d(t) = (ky - 1, kx - 1); cells off the board are zero.  The model imports nothing from the package under
test; tests/test_conv_ref.py pins it to torch's float64 conv2d and its autograd.

  conv         y[n][p][o] = sum_t sum_c x[n][p + d(t)][c] W[o][c][t]
  w_eff        transpose = 0: W;  transpose = 1: W'[c][o][t] = W[o][c][8 - t], so that dx = conv(dy, W')
  round_to     round to nearest even into f16 (dtype 1) / bf16 (dtype 2), widened back; the packed weights are
               round_to(w_eff(W)), the outputs round_to(sum): ONE rounding of the exact sum
  forward_add  round_to(conv + addend)
  stamp        out[n][q][o] += table[tap][o] for q in the 3x3 window of board n's action cell a,
               tap = (a - q) + (1, 1) as 3 * dy + dx; window cells off the board are dropped; before the rounding
  stats        (sum, sum of squares, counted positions) per channel of the ROUNDED output over the live boards
  bwd_stats    (sum dz, sum dz * xhat, counted positions), dz = y * [bn_y > 0] (relu) or y, y the ROUNDED output,
               xhat = (bn_x - mean) * invstd
  wgrad        dW[o][c][t] = sum_n sum_p dy[n][p][o] x[n][p + d(t)][c]  (+ dW0 when accumulating; over every
               segment's boards in the segment form)
A zero sum is +0.0 (the accumulators start from +0.0 and round to nearest).
"""
import numpy as np

CC = 128
# significand bits, exponent of the smallest subnormal, largest finite value
_FMT = {1: (11, -24, 65504.0), 2: (8, -133, float.fromhex("0x1.fep127"))}


def round_to(a, dtype):
    """Round to nearest even into f16 (1) / bf16 (2), one rounding from float64, as float64."""
    bits, emin, fmax = _FMT[dtype]
    a = np.asarray(a, np.float64)
    _, e = np.frexp(a)  # |a| = m 2^e, 0.5 <= m < 1
    q = np.ldexp(1.0, np.maximum(e - bits, emin))
    r = np.rint(a / q) * q  # the division and the product are exact (powers of two); rint rounds to even
    return np.where(np.abs(r) > fmax, np.copysign(np.inf, a), r)


def ulp_gap(a, dtype):
    """(lower neighbour, quantum) of |a| on dtype's grid, for building ties: |a| in [lo, lo + q)."""
    bits, emin, _ = _FMT[dtype]
    a = np.abs(np.asarray(a, np.float64))
    _, e = np.frexp(a)
    q = np.ldexp(1.0, np.maximum(e - bits, emin))
    return np.floor(a / q) * q, q


def is_tie(a, dtype):
    """The value lies exactly half way between two neighbours of dtype's grid."""
    lo, q = ulp_gap(a, dtype)
    return np.abs(np.asarray(a, np.float64)) - lo == q / 2


def w_eff(W, transpose):
    W = np.asarray(W, np.float64)
    return W.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1].copy() if transpose else W


def _padded(x, H):
    N, A, C = x.shape
    assert A == H * H
    xp = np.zeros((N, H + 2, H + 2, C))
    xp[:, 1:H + 1, 1:H + 1] = x.reshape(N, H, H, C)
    return xp


def conv(x, W, H):
    """[N][H*H][C] x [O][C][3][3] -> [N][H*H][O], padding 1, exact up to float64."""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    N = x.shape[0]
    xp = _padded(x, H)
    y = np.zeros((N, H, H, W.shape[0]))
    for ky in range(3):
        for kx in range(3):
            y += xp[:, ky:ky + H, kx:kx + H] @ W[:, :, ky, kx].T
    return y.reshape(N, H * H, -1) + 0.0


def abs_conv(x, W, H):
    """sum_t sum_c |x W|: what bounds every partial sum of the products, in any order."""
    return conv(np.abs(x), np.abs(W), H)


def stamp_terms(actions, table, H):
    """[N][H*H][O]: the action stamp alone."""
    table = np.asarray(table, np.float64)
    out = np.zeros((len(actions), H, H, table.shape[1]))
    for n, a in enumerate(actions):
        ay, ax = divmod(int(a), H)
        for dy in range(3):
            for dx in range(3):
                qy, qx = ay - dy + 1, ax - dx + 1  # tap = (a - q) + (1, 1)
                if 0 <= qy < H and 0 <= qx < H:
                    out[n, qy, qx] += table[dy * 3 + dx]
    return out.reshape(len(actions), H * H, -1)


def forward(x, Wq, H, dtype, addend=None, actions=None, table=None):
    """The stored output: round_to(conv(x, Wq) (+ stamp) (+ addend)); Wq = the packed (rounded) weights."""
    pre = conv(x, Wq, H)
    if actions is not None:
        pre = pre + stamp_terms(actions, table, H)
    if addend is not None:
        pre = pre + addend
    return round_to(pre + 0.0, dtype)


def live(mask, N):
    return np.ones(N, bool) if mask is None else (np.asarray(mask) != 0)


def stats(y, mask=None):
    """[C][3] = (sum, sum of squares, counted positions) of the stored output over the live boards."""
    v = live(mask, y.shape[0])
    yv = y[v]
    out = np.zeros((y.shape[2], 3))
    out[:, 0] = yv.sum(axis=(0, 1))
    out[:, 1] = (yv * yv).sum(axis=(0, 1))
    out[:, 2] = float(v.sum() * y.shape[1])
    return out


def board_stats(y, mask=None):
    """[C][N][3]: the same per board, (0, 0, 0) for a board outside the mask."""
    N, A, C = y.shape
    v = live(mask, N)
    out = np.zeros((C, N, 3))
    out[:, :, 0] = (y.sum(axis=1) * v[:, None]).T
    out[:, :, 1] = ((y * y).sum(axis=1) * v[:, None]).T
    out[:, :, 2] = (v * float(A))[None, :]
    return out


def bwd_terms(y, bn_x, bn_y, mean, invstd, relu):
    """dz and dz * xhat per element (y: the stored output)."""
    dz = y * (bn_y > 0) if relu else y
    return dz, dz * ((bn_x - mean[None, None, :]) * invstd[None, None, :])


def bwd_stats(y, bn_x, bn_y, mean, invstd, relu, mask=None):
    v = live(mask, y.shape[0])
    dz, dzx = bwd_terms(y, bn_x, bn_y, mean, invstd, relu)
    out = np.zeros((y.shape[2], 3))
    out[:, 0] = dz[v].sum(axis=(0, 1))
    out[:, 1] = dzx[v].sum(axis=(0, 1))
    out[:, 2] = float(v.sum() * y.shape[1])
    return out


def wgrad(x, dy, H, dw0=None):
    """[O][C][3][3] = (dw0 +) sum_n sum_p dy[n][p][o] x[n][p + d(t)][c]."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    N = x.shape[0]
    xp = _padded(x, H)
    d = dy.reshape(N * H * H, -1)
    dw = np.zeros((dy.shape[2], x.shape[2], 3, 3))
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = d.T @ xp[:, ky:ky + H, kx:kx + H].reshape(N * H * H, -1)
    dw = dw + 0.0
    return dw if dw0 is None else dw + np.asarray(dw0, np.float64)


def wgrad_segments(xs, dys, H, dw0=None):
    """The segment form: the boards of every (x, dy) pair, in any order."""
    dw = sum(wgrad(x, dy, H) for x, dy in zip(xs, dys))
    return dw if dw0 is None else dw + np.asarray(dw0, np.float64)
