"""Float64 model of the inference network (the gmz_net_* contract of include/gmz.h: csrc/gmz_net.hip's k_tower3,
k_head_gemm and k_head_finish), in plain numpy.  It imports nothing from the package under test; tests/test_net_ref.py
pins it to oracle/netref.py (itself pinned to the reference forward) and to network.pack_weights.

Activations are float64 [N][H*H][128] (channels-last, position p = row * H + column, the hidden-state pool's order)
holding the values AS STORED (16-bit values widened exactly).  dtype: 1 = f16, 2 = bf16 (tests/conv_ref.py's ids).

  fold         eval-mode BatchNorm, eps 1e-4, in numpy float32 (correctly rounded operations, no fused multiply-add):
               s = gamma / sqrt(var + eps), W' = W * s, b' = beta - mean * s; a head 1x1 conv with its own bias c:
               b' = c * s + (beta - mean * s)
  16-bit W     round_to(W') for the stem, every 3x3 conv (the dynamics conv's 128 hidden-state channels) and
               reward_fc.0, f16 clamped to +-65504 first; everything else stays float32
  action table T[tap][o] = sum_c W'[o][128 + c][tap] * embed[c], a float32 table
  stem, conv   pre = sum_t sum_c x[p + d(t)][c] W16[o][c][t] + b'[o]
                     (+ T[tap][o] on the cells q of the action's 3x3 window that are on the board, tap = (a - q) + (1, 1):
                      layer 0 of the dynamics tower)
                     (+ the block's input as stored: conv2 of a block)
  store        min(max(round_to(pre), +0), 65504 in f16): ONE rounding to nearest even of the exact sum, subnormals
               kept (FLUSH_SUBNORMAL_STORES = False); a zero is +0.0
  head planes  relu(b'[o] + sum_c W'[o][c] h[p][c]), float32, o = policy 0, policy 1, value
  logits       policy_fc (k = o * A + p) + bias
  value        relu(value_fc1 + bias) -> value_fc2 + bias: 3 support logits -> support_to_scalar
  reward       relu(reward_fc.0 (16-bit, k = c * A + p) + bias) -> reward_fc.2 + bias -> support_to_scalar
  support_to_scalar   softmax(l) . (-1, 0, 1), here in float64

Every sum above is returned as a Layer: the exact value `pre`, the sum of its terms' absolute values `mag` (products,
bias, action term, residual) and, per row n, the quantum q[n] every term is a multiple of (rows are independent
sums; a product's quantum is taken input channel by input channel).  Where mag < 2^24 q every partial sum in any
order is exact in float32, fused or not, so the kernels' float32 accumulators hold `pre` and what they store or pass
on is determined bit for bit.
"""
import collections

import numpy as np

import conv_ref as R

C = 128
EPS = np.float32(1e-4)
F16_MAX = 65504.0
# the hardware keeps f16 subnormals in the 16-bit conversion of a store; True would model a flush to +0
FLUSH_SUBNORMAL_STORES = False

Layer = collections.namedtuple("Layer", "name pre mag q")


def _lowbit(a):
    """Per element: the largest power of two that divides it (inf for a zero)."""
    a = np.abs(np.asarray(a, np.float64))
    m, e = np.frexp(a)
    k = (m * 2.0 ** 53).astype(np.int64)
    return np.where(a != 0, np.ldexp((k & -k).astype(np.float64), e - 53), np.inf)


def quantum(a):
    """The largest power of two that divides every element (inf when all are zero)."""
    return float(_lowbit(a).min(initial=np.inf))


def row_quantum(a):
    """quantum() of every row a[n]: rows are independent sums, so each has a quantum of its own."""
    a = np.asarray(a)
    return _lowbit(a).reshape(len(a), -1).min(axis=1)


def product_quantum(x, W):
    """Per row n of x [N][...][C] against W [O][C][...]: a power of two that divides every product
    x[n][..][c] W[o][c][..], the smallest over c of (quantum of the row's channel c) x (quantum of the weights on c)."""
    qx = np.moveaxis(_lowbit(x), -1, 1).reshape(x.shape[0], x.shape[-1], -1).min(axis=2)  # [N][C]
    qw = np.moveaxis(_lowbit(W), 1, 0).reshape(W.shape[1], -1).min(axis=1)                 # [C]
    with np.errstate(invalid="ignore"):
        q = qx * qw[None, :]
    return np.where(np.isnan(q), np.inf, q).min(axis=1)


def span_bits(layer):
    """log2 of the largest mag / q over the rows: below 24 the layer is exact in float32."""
    N = len(layer.mag)
    return float(np.log2((layer.mag.reshape(N, -1).max(axis=1) / layer.q).max()))


def exact(layer):
    """The exactness condition of one Layer."""
    return span_bits(layer) < 24


def _f32(a):
    return np.asarray(a, np.float32)


def fold(sd, prefix):
    g, b, m, v = (_f32(sd[prefix + k]) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    s = g / np.sqrt(v + EPS)
    return s, b - m * s


def to16(w32, dtype):
    """float32 -> the 16-bit weight, as float64."""
    w = _f32(w32).astype(np.float64)
    if dtype == 1:
        w = np.clip(w, -F16_MAX, F16_MAX)
    return R.round_to(w, dtype)


def store(pre, dtype):
    y = np.minimum(np.maximum(R.round_to(pre, dtype), 0.0), F16_MAX if dtype == 1 else np.inf) + 0.0
    if FLUSH_SUBNORMAL_STORES and dtype == 1:
        y = np.where(y < 2.0 ** -14, 0.0, y)
    return y


def _conv_terms(x, W, H):
    """(sum, sum of absolute values) of the 3x3 convolution; a tap multiplies only the input channels it has weights
    for, so sparse weights cost little."""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    N = x.shape[0]
    pre, mag = np.zeros((N, H * H, W.shape[0])), np.zeros((N, H * H, W.shape[0]))
    ax = np.abs(x)
    for t in range(9):
        Wt = W[:, :, t // 3, t % 3]
        cols = np.flatnonzero(Wt.any(axis=0))
        if cols.size:
            pre += _one_tap(x[:, :, cols], Wt[:, cols], H, t)
            mag += _one_tap(ax[:, :, cols], np.abs(Wt[:, cols]), H, t)
    return pre + 0.0, mag


def _one_tap(x, Wt, H, t):
    """[N][A][C] x [O][C] at tap t: y[p] = x[p + d(t)] Wt^T, cells off the board zero."""
    N, _, Cin = x.shape
    xp = np.zeros((N, H + 2, H + 2, Cin))
    xp[:, 1:H + 1, 1:H + 1] = x.reshape(N, H, H, Cin)
    ky, kx = divmod(t, 3)
    return (xp[:, ky:ky + H, kx:kx + H] @ Wt.T).reshape(N, H * H, -1)


def support_to_scalar(l):
    l = np.asarray(l, np.float64)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return p[:, 2] - p[:, 0]


class Model:
    """The folded, rounded weights of one reference-keyed state_dict and the forward passes on them."""

    def __init__(self, sd, dtype, size):
        sd = {k: np.asarray(v) for k, v in sd.items()}
        self.dtype, self.H, self.A = dtype, size, size * size
        self.blocks = len({k.split(".")[2] for k in sd if k.startswith("representation_net.resblocks.")})

        def conv_bn(w, bn):
            s, b = fold(sd, bn)
            return _f32(sd[w]) * s[:, None, None, None], b

        def tower(prefix):
            out = []
            for i in range(self.blocks):
                for k in (1, 2):
                    p = "%s.resblocks.%d." % (prefix, i)
                    w, b = conv_bn(p + "conv%d.weight" % k, p + "bn%d" % k)
                    out.append((to16(w, dtype), b.astype(np.float64)))
            return out

        w, b = conv_bn("representation_net.conv.weight", "representation_net.bn")
        self.stem = (to16(w, dtype), b.astype(np.float64))
        self.repr = tower("representation_net")
        wd, b = conv_bn("dynamics_net.conv.weight", "dynamics_net.bn")
        emb = _f32(sd["dynamics_net.action_embed_conv.weight"]).reshape(16).astype(np.float64)
        table = np.einsum("ncyx,c->yxn", wd[:, C:].astype(np.float64), emb).reshape(9, C)
        self.action = table.astype(np.float32).astype(np.float64)
        self.dyn = [(to16(wd[:, :C], dtype), b.astype(np.float64))] + tower("dynamics_net")
        hw, hb = [], []
        for name in ("policy", "value"):
            s, b = fold(sd, "prediction_net.%s_bn" % name)
            w = _f32(sd["prediction_net.%s_conv.weight" % name])
            hw.append(w.reshape(w.shape[0], C) * s[:, None])
            hb.append(_f32(sd["prediction_net.%s_conv.bias" % name]) * s + b)
        self.head_w, self.head_b = np.concatenate(hw).astype(np.float64), np.concatenate(hb).astype(np.float64)
        f = lambda k: _f32(sd[k]).astype(np.float64)
        self.policy = (f("prediction_net.policy_fc.weight"), f("prediction_net.policy_fc.bias"))
        self.value1 = (f("prediction_net.value_fc1.weight"), f("prediction_net.value_fc1.bias"))
        self.value2 = (f("prediction_net.value_fc2.weight"), f("prediction_net.value_fc2.bias"))
        self.reward1 = (to16(sd["dynamics_net.reward_fc.0.weight"], dtype), f("dynamics_net.reward_fc.0.bias"))
        self.reward2 = (f("dynamics_net.reward_fc.2.weight"), f("dynamics_net.reward_fc.2.bias"))

    # ---- towers
    def _conv(self, name, x, wb, extra=()):
        W, b = wb
        pre, mag = _conv_terms(x, W, self.H)
        pre, mag = pre + b, mag + np.abs(b)
        q = np.minimum(product_quantum(x, W), quantum(b))
        for e in extra:
            pre, mag = pre + e, mag + np.abs(e)
            q = np.minimum(q, row_quantum(e))
        return Layer(name, pre + 0.0, mag, q)

    def _blocks(self, x, convs, layers, first):
        for i in range(self.blocks):
            l1 = self._conv("block %d conv1" % i, x, convs[first + 2 * i])
            l2 = self._conv("block %d conv2" % i, store(l1.pre, self.dtype), convs[first + 2 * i + 1], extra=(x,))
            layers += [l1, l2]
            x = store(l2.pre, self.dtype)
        return x

    def representation(self, obs):
        """obs [N][3][H][H] of 0 / 1 -> (hidden state as stored, [Layer])."""
        N = len(obs)
        x = np.asarray(obs, np.float64).reshape(N, 3, self.A).transpose(0, 2, 1)
        layers = [self._conv("stem", x, self.stem)]
        return self._blocks(store(layers[0].pre, self.dtype), self.repr, layers, 0), layers

    def dynamics(self, h, actions):
        """h [N][A][128] as stored, actions [N] -> (next hidden state as stored, [Layer])."""
        stamp = R.stamp_terms(actions, self.action, self.H)
        layers = [self._conv("dynamics conv", h, self.dyn[0], extra=(stamp,))]
        return self._blocks(store(layers[0].pre, self.dtype), self.dyn, layers, 1), layers

    # ---- heads
    @staticmethod
    def _fc(name, x, wb):
        W, b = wb
        return Layer(name, x @ W.T + b + 0.0, np.abs(x) @ np.abs(W).T + np.abs(b),
                     np.minimum(product_quantum(x, W), quantum(b)))

    def heads(self, h, reward):
        """-> dict: logits [N][A], value_logits [N][3], value [N] (reward_logits, reward), layers."""
        N = len(h)
        pl = Layer("head planes", np.einsum("npc,oc->nop", h, self.head_w) + self.head_b[None, :, None] + 0.0,
                   np.einsum("npc,oc->nop", np.abs(h), np.abs(self.head_w)) + np.abs(self.head_b)[None, :, None],
                   np.minimum(product_quantum(h, self.head_w), quantum(self.head_b)))
        planes = np.maximum(pl.pre, 0.0)
        lg = self._fc("policy_fc", planes[:, :2].reshape(N, 2 * self.A), self.policy)
        v1 = self._fc("value_fc1", planes[:, 2], self.value1)
        v2 = self._fc("value_fc2", np.maximum(v1.pre, 0.0), self.value2)
        out = dict(planes=planes, logits=lg.pre, value_hidden=np.maximum(v1.pre, 0.0), value_logits=v2.pre,
                   value=support_to_scalar(v2.pre), layers=[pl, lg, v1, v2])
        if reward:
            r1 = self._fc("reward_fc.0", h.transpose(0, 2, 1).reshape(N, C * self.A), self.reward1)
            r2 = self._fc("reward_fc.2", np.maximum(r1.pre, 0.0), self.reward2)
            out.update(reward_hidden=np.maximum(r1.pre, 0.0), reward_logits=r2.pre, reward=support_to_scalar(r2.pre))
            out["layers"] += [r1, r2]
        return out

    def initial(self, obs):
        h, layers = self.representation(obs)
        out = self.heads(h, False)
        out.update(hidden=h, layers=layers + out["layers"], tower=layers)
        return out

    def recurrent(self, h, actions):
        h2, layers = self.dynamics(h, actions)
        out = self.heads(h2, True)
        out.update(hidden=h2, layers=layers + out["layers"], tower=layers)
        return out


def bits16(a, dtype):
    """Stored values (float64, representable) -> their uint16 patterns."""
    a32 = np.asarray(a, np.float32)
    if dtype == 1:
        return a32.astype(np.float16).view(np.uint16)
    return (a32.view(np.uint32) >> 16).astype(np.uint16)


def from_bits16(u, dtype):
    u = np.asarray(u, np.uint16)
    if dtype == 1:
        return u.view(np.float16).astype(np.float64)
    return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
