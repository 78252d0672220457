"""Test data for the inference network's exact tiers (tests/test_net_ref.py on the CPU, tests/test_net_kernels_gpu.py
on the GPU): reference-keyed state_dicts whose forward pass tests/net_ref.py determines bit for bit, with the model's
outputs, built once per case and shared.

A case is drawn as TARGETS, the folded weights and biases the network is meant to compute with, and then unfolded into
a state_dict whose BatchNorms fold back to them exactly: gamma a power of two, running_var one of the three float32
values with var + 1e-4 == 1, 4 or 0.25, an integer running_mean, beta = bias + mean * scale.

Rows: 13 (odd, no multiple of 2 or 5); rows SKIP are skipped (out slot -1): row 4's partner in a packed workgroup of
a full grid is a live row (11, or 7 and 10 at five boards), row 9 is the partner of row 2.
"""
import functools

import numpy as np

import conv_ref as R
import net_ref as M

C, HD = 128, 64
ROWS = 13
SKIP = (4, 9)
SIZES = list(range(5, 20))
ONE_BLOCK_SIZES = [5, 8, 13, 17]
CASES = [(s, 2) for s in SIZES] + [(s, 1) for s in ONE_BLOCK_SIZES]
PREC = {1: "fp16", 2: "bf16"}
# float32 running_var with var + 1e-4 == v exactly, by sqrt(v)
VAR = {1.0: float.fromhex("0x1.fff2e4p-1"), 2.0: float.fromhex("0x1.fffcbap+1"), 0.5: float.fromhex("0x1.ffcb92p-3")}


# ---------------------------------------------------------------- targets -> state_dict
def _bn(sd, prefix, bias, rs):
    """BatchNorm tensors that fold to (scale, bias) exactly; returns the scale (a power of two per channel)."""
    n = len(bias)
    g = 2.0 ** rs.randint(-1, 2, n)
    root = rs.choice([0.5, 1.0, 2.0], n)
    s = g / root
    mean = rs.randint(-2, 3, n).astype(np.float64)
    sd[prefix + ".weight"] = g.astype(np.float32)
    sd[prefix + ".running_var"] = np.array([VAR[r] for r in root], np.float32)
    sd[prefix + ".running_mean"] = mean.astype(np.float32)
    sd[prefix + ".bias"] = (np.asarray(bias, np.float64) + mean * s).astype(np.float32)
    return s


def unfold(t, seed):
    """Targets -> a reference-keyed state_dict (float32 numpy) that folds back to them."""
    rs = np.random.RandomState(seed)
    sd = {}

    def conv(w, bn, wb):
        W, b = wb
        s = _bn(sd, bn, b, rs)
        sd[w] = (W / s.reshape((-1,) + (1,) * (W.ndim - 1))).astype(np.float32)

    conv("representation_net.conv.weight", "representation_net.bn", t["stem"])
    for prefix, convs in (("representation_net", t["repr"]), ("dynamics_net", t["dyn"][1:])):
        for i, wb in enumerate(convs):
            p = "%s.resblocks.%d." % (prefix, i // 2)
            conv(p + "conv%d.weight" % (i % 2 + 1), p + "bn%d" % (i % 2 + 1), wb)
    conv("dynamics_net.conv.weight", "dynamics_net.bn", t["dyn"][0])
    sd["dynamics_net.action_embed_conv.weight"] = t["embed"].reshape(16, 1, 1, 1).astype(np.float32)
    for name in ("policy", "value"):
        W, c, b = t[name + "_conv"]  # b' = c * s + bn bias: the BatchNorm's share is b - c (with s folded out)
        o = len(c)
        s = _bn(sd, "prediction_net.%s_bn" % name, b - c, rs)
        sd["prediction_net.%s_conv.weight" % name] = (W / s[:, None]).reshape(o, C, 1, 1).astype(np.float32)
        sd["prediction_net.%s_conv.bias" % name] = (c / s).astype(np.float32)
    for key, name in (("policy_fc", "prediction_net.policy_fc"), ("value_fc1", "prediction_net.value_fc1"),
                      ("value_fc2", "prediction_net.value_fc2"), ("reward_fc1", "dynamics_net.reward_fc.0"),
                      ("reward_fc2", "dynamics_net.reward_fc.2")):
        sd[name + ".weight"], sd[name + ".bias"] = (a.astype(np.float32) for a in t[key])
    return sd


# ---------------------------------------------------------------- Tier B: exact dense data
def _sparse(rs, shape, nnz, values, p=None):
    """[O][...] with nnz nonzeros per output row, drawn from `values`."""
    O, K = shape[0], int(np.prod(shape[1:]))
    W = np.zeros((O, K))
    for o in range(O):
        W[o, rs.choice(K, nnz, replace=False)] = rs.choice(values, nnz, p=p)
    return W.reshape(shape)


W5 = [1.0, -1.0, 2.0, -2.0, 0.5]
W4 = W5[:4]
WNEG = [1.0, -1.0, 2.0, -2.0, -2.0]
HALVING = 2
DYN_SPEC = {2: [(12, W5, 2.0 ** -6, 4096.0), (12, W4, 2.0 ** -3, 0.0), (12, W4, 0.25, 16384.0), (12, W4, 2.0 ** -3, 0.0),
                (8, WNEG, 0.5, 0.0)],
            1: [(8, W4, 0.25, 8192.0), (12, W4, 2.0 ** -4, 0.0), (12, W4, 0.25, 0.0)]}


@functools.lru_cache(maxsize=None)
def dense_targets(size, blocks):
    """The folded network of the exact dense tier.  Representation tower: 24 nonzero weights per output channel of
    every 128 -> 128 conv, 9 per stem channel, from {+-1, +-2, 0.5}, integer biases in [-8, 8]; magnitudes grow about
    fivefold a layer and the sums' span by 2 to 3.5 bits.  Dynamics tower: DYN_SPEC.  Heads: 3 or 4 weights a row
    (8 for reward_fc.0) of +-1 and 2, biases that keep most of every ReLU's inputs positive, and support layers scaled
    by a power of two so the support logits differ by a few units, not thousands.  Every knob here was set against
    the CONDITIONS of tests/test_net_ref.py, which only the model decides; none was set against a kernel."""
    rs = np.random.RandomState(100 * size + blocks)
    A = size * size
    ib = lambda n, lo=-8, hi=8: rs.randint(lo, hi + 1, n).astype(np.float64)
    # one block: wider stem weights (odd multiples of 1/64), so that the only block's sums already outgrow 11 bits
    stem_vals = W5 if blocks == 2 else list(np.arange(-127, 128, 2) / 64.0)
    t = {"stem": (_sparse(rs, (C, 3, 3, 3), 9, stem_vals), ib(C))}
    # the quantum halves in the stem and the first HALVING convs only
    vals = lambda i: W5 if i < HALVING else W4
    t["repr"] = [(_sparse(rs, (C, C, 3, 3), 24, vals(i)), ib(C)) for i in range(2 * blocks)]
    # The dynamics tower follows the representation tower, whose states already span 18 bits, so its sums could not
    # stay below 24 bits at that tower's growth.  A layer whose bias LIFTs every sum into [lift / 2, 2 lift) stores
    # outputs that span 12 (bf16: 9) bits whatever its inputs spanned: the dynamics conv and conv2 of block 0 are
    # lifted (no ReLU clips there; the other layers' do).  Two blocks: biases after a lift are multiples of 16 x the
    # layer's scale, about the lifted values' last place, so that the last block's sums carry only a few bits too
    # many and exact ties stay frequent in bf16.  (nonzeros per channel, values, scale, lift) per layer:
    spec = DYN_SPEC[blocks]
    for k, (nnz, values, scale, lift) in enumerate(spec):
        W = _sparse(rs, (C, C, 3, 3), nnz, values) * scale
        if k == 0:
            W = np.concatenate([W, _sparse(rs, (C, 16, 3, 3), 6, [1.0, -1.0, 2.0])], axis=1)
        bias = ib(C) if k == 0 or blocks == 1 else ib(C) * 16 * scale
        t.setdefault("dyn", []).append((W, bias + lift))
    t["embed"] = rs.randint(-8, 9, 16).astype(np.float64) * 16
    hv = [1.0, -1.0, 2.0]
    t["policy_conv"] = (np.abs(_sparse(rs, (2, C), 4, hv)), ib(2, 0, 4), ib(2, 0, 64) * 16)
    t["value_conv"] = (np.abs(_sparse(rs, (1, C), 4, hv)), ib(1, 0, 4), ib(1, 0, 64) * 16)
    t["policy_fc"] = (_sparse(rs, (A, 2 * A), 3, hv), ib(A, -64, 64))
    t["value_fc1"] = (_sparse(rs, (HD, A), 3, hv), ib(HD, 0, 64) * 16)
    t["value_fc2"] = (_sparse(rs, (3, HD), 4, [1.0, -1.0]) / 2.0 ** (16 if blocks == 2 else 13), ib(3, -2, 2))
    t["reward_fc1"] = (_sparse(rs, (HD, C * A), 8, hv), ib(HD, 0, 64) * 16)
    t["reward_fc2"] = (_sparse(rs, (3, HD), 4, [1.0, -1.0]) / 2.0 ** (16 if blocks == 2 else 13), ib(3, -2, 2))
    return t


# ---------------------------------------------------------------- inputs
def observations(size, seed=0):
    """[ROWS][3][H][H] of 0 / 1, about a third of the cells set."""
    return (np.random.RandomState(7 * size + seed).rand(ROWS, 3, size, size) < 0.3).astype(np.float32)


def actions(size):
    """One action per row: the four corners, a non-corner cell on each edge, a cell next to a corner and four interior
    cells, all different, so packed workgroups hold different actions."""
    H, m = size, size // 2
    cells = [(0, 0), (0, H - 1), (H - 1, 0), (H - 1, H - 1), (0, m), (m, 0), (m, H - 1), (H - 1, m), (0, 1),
             (1, 1), (m, m), (H - 2, H - 2), (1, H - 2)]
    assert len(set(cells)) == ROWS
    return np.array([y * H + x for y, x in cells], np.int32)


def hand_states(size, n, dtype, seed=0):
    """[n][A][128] integer-valued states j 2^s (j < 128: 16-bit patterns of either type), about half zero like a
    ReLU's output, a few entries per board near the top of the f16 range (f16) / at 2^11 and above (bf16)."""
    rs = np.random.RandomState(31 * size + seed)
    A = size * size
    x = rs.randint(0, 128, (n, A, C)) * 2.0 ** rs.randint(0, 3, (n, A, C)) * (rs.rand(n, A, C) < 0.5)
    top = [65504.0, 65024.0, 32768.0] if dtype == 1 else [2048.0, 127 * 32.0, 4096.0]
    for i in range(n):
        k = 6
        x[i, rs.randint(0, A, k), rs.randint(0, C, k)] = rs.choice(top, k)
    return x


@functools.lru_cache(maxsize=2)
def dense_case(size, blocks, dtype):
    """Tier B at one (size, blocks, dtype): state_dict, inputs and the model's two passes.  The last two cases are kept
    (a 19x19 case holds about 160 MiB): the GPU tests run a case's two grids one after the other; every other case
    builder here is used by one test at a time and is not cached."""
    sd = unfold(dense_targets(size, blocks), 1000 + size)
    m = M.Model(sd, dtype, size)
    obs = observations(size)
    init = m.initial(obs)
    states = np.concatenate([init["hidden"][:7], hand_states(size, ROWS - 7, dtype)])
    acts = actions(size)
    return dict(sd=sd, model=m, obs=obs, init=init, states=states, actions=acts, rec=m.recurrent(states, acts))


def shares(layers, dtype):
    """(inexact, tie, negative) shares over the pre-activations of the given layers."""
    pre = np.concatenate([l.pre.ravel() for l in layers])
    return float((R.round_to(pre, dtype) != pre).mean()), float(R.is_tie(pre, dtype).mean()), float((pre < 0).mean())


def scaled_targets(t, variant, factor=8.0):
    """Tier B variants (f16).  "saturate": the last block's conv2 of the representation tower times `factor`, so sums pass 65504
    in the convs' store (the dynamics tower's pass it in the base case already at most sizes).  "saturate_stem": the
    stem's channels STEM_SAT times 2^13, so their sums of 8 and more pass 65504 in the STEM's store, which has a clamp
    of its own; conv1 of every block has no weight on those channels (their coarse values would cost the later
    sums their 24 bits), and the residual adds carry the clamped values to the hidden state and the heads.
    "subnormal24" / "subnormal31": the stem's weights and every bias times 2^-24 / 2^-31; the network is positively
    homogeneous, so every sum is the base case's times that until a store rounds on the subnormal grid.  2^-24 puts
    the one-block representation tower's hidden state into [2^-24, 2^-14), 2^-31 the dynamics tower's."""
    t = {k: (list(v) if isinstance(v, list) else v) for k, v in t.items()}
    if variant == "saturate":
        W, b = t["repr"][-1]
        t["repr"][-1] = (W * factor, b * factor)
    elif variant == "saturate_stem":
        W, b = (a.copy() for a in t["stem"])
        W[STEM_SAT], b[STEM_SAT] = W[STEM_SAT] * 2.0 ** 13, b[STEM_SAT] * 2.0 ** 13
        t["stem"] = (W, b)
        for i in range(0, len(t["repr"]), 2):
            W = t["repr"][i][0].copy()
            W[:, STEM_SAT] = 0.0
            t["repr"][i] = (W, t["repr"][i][1])
    elif variant.startswith("subnormal"):
        k = 2.0 ** -int(variant[9:])
        t["stem"] = (t["stem"][0] * k, t["stem"][1] * k)
        for key in ("repr", "dyn"):
            t[key] = [(W, b * k) for W, b in t[key]]
        for key in ("policy_conv", "value_conv"):
            W, c, b = t[key]
            t[key] = (W, c * k, b * k)
        for key in ("policy_fc", "value_fc1", "value_fc2", "reward_fc1", "reward_fc2"):
            t[key] = (t[key][0], t[key][1] * k)
        t["embed"] = t["embed"] * k
    else:
        raise ValueError(variant)
    return t


def variant_case(size, blocks, variant):
    """dense_case's f16 variant.  The saturating ones have an initial pass only: the dynamics tower of the base case
    already stores sums past 65504 (asserted at SATURATE_REC_SIZES).  The subnormal ones start their recurrent rows
    from states scaled alike."""
    factor = 1.0
    if variant == "saturate":  # the power of two that takes about 1 % of the base case's last sums past 65504
        pre = dense_case(size, blocks, 1)["init"]["tower"][-1].pre
        factor = 2.0 ** np.ceil(np.log2(65504.0 / np.quantile(pre, 0.99)))
    sd = unfold(scaled_targets(dense_targets(size, blocks), variant, factor), 1000 + size)
    m = M.Model(sd, 1, size)
    obs = observations(size)
    out = dict(sd=sd, model=m, obs=obs, init=m.initial(obs), actions=actions(size))
    if variant.startswith("subnormal"):
        hand = M.store(hand_states(size, ROWS - 7, 1) * 2.0 ** -int(variant[9:]), 1)  # onto the subnormal grid
        out["states"] = np.concatenate([out["init"]["hidden"][:7], hand])
        out["rec"] = m.recurrent(out["states"], out["actions"])
    return out


STEM_SAT = [3, 40, 77, 114]
SATURATE_REC_SIZES = [7, 15, 19]  # where at least 0.5 % of the dense recurrent pass's last sums pass 65504


# ---------------------------------------------------------------- Tier A: single taps
def tap_targets(size, t0, blocks=2):
    """Every output channel o of every 3x3 conv has ONE weight: W[o][(o + 17) % 128][tap] = 1, a channel rotation, at
    tap (o + k + t0) % 9 in layer k of its tower (the stem, layer 0 of the representation tower, reads plane o % 3;
    the dynamics conv also has one weight on action plane o % 16).  Every layer so uses every tap, on different
    channels, and each output is a shifted, clipped copy of one input channel plus a small integer bias (a ReLU
    clips): nothing rounds, and a wrong cell or channel names its tap."""
    t = dict(dense_targets(size, blocks))  # the heads of the dense tier
    o, n = np.arange(C), 1 + 2 * blocks
    bias = lambda k: ((o + k) % 5 - 2).astype(np.float64)
    taps = dict(repr=[(o + k + t0) % 9 for k in range(n)], dyn=[(o + k + 4 + t0) % 9 for k in range(n)])

    def one(cin, tap, src, val):
        W = np.zeros((C, cin, 3, 3))
        W[o, src, tap // 3, tap % 3] = val
        return W

    t["taps"] = taps
    t["stem"] = (one(3, taps["repr"][0], o % 3, 1.0 + o % 4), bias(0))
    t["repr"] = [(one(C, tap, (o + 17) % C, 1.0), bias(k + 1)) for k, tap in enumerate(taps["repr"][1:])]
    Wd = np.concatenate([one(C, taps["dyn"][0], (o + 17) % C, 1.0), one(16, (o + 2 + t0) % 9, o % 16, 1.0)], axis=1)
    t["dyn"] = [(Wd, bias(5))] + [(one(C, tap, (o + 17) % C, 1.0), bias(k + 6))
                                  for k, tap in enumerate(taps["dyn"][1:])]
    t["embed"] = np.arange(1, 17).astype(np.float64) * 4
    return t


TAP_OFFSETS = (0, 5)


def tap_observations(size):
    """Sparse planes: the corners, an edge cell and the centre in turn, plus a few random cells per row."""
    H = size
    obs = (np.random.RandomState(size).rand(ROWS, 3, H, H) < 0.04).astype(np.float32)
    marks = [(0, 0), (0, H - 1), (H - 1, 0), (H - 1, H - 1), (0, H // 2), (H // 2, 0), (H - 1, H // 2), (H // 2, H - 1),
             (H // 2, H // 2)]
    for r in range(ROWS):
        y, x = marks[r % len(marks)]
        obs[r, r % 3, y, x] = 1
    return obs


def tap_case(size, dtype, t0, blocks=2):
    t = tap_targets(size, t0, blocks)
    sd = unfold(t, 2000 + size)
    m = M.Model(sd, dtype, size)
    obs = tap_observations(size)
    init = m.initial(obs)
    states = np.concatenate([init["hidden"][:7], hand_states(size, ROWS - 7, 2) % 8])
    acts = actions(size)
    return dict(sd=sd, model=m, obs=obs, init=init, states=states, actions=acts, rec=m.recurrent(states, acts),
                taps=t["taps"])


# ---------------------------------------------------------------- small magnitudes: nothing rounds
def small_case(size, blocks, dtype):
    """Dense but small: 3 weights of +-1 per channel, biases in [-1, 1]; every stored value is a small integer, so
    float32 arithmetic (oracle/netref.py) computes exactly what the model does."""
    rs = np.random.RandomState(5000 + size)
    t = dict(dense_targets(size, blocks))
    ib = lambda n: rs.randint(-1, 2, n).astype(np.float64)
    pm = [1.0, -1.0]
    t["stem"] = (_sparse(rs, (C, 3, 3, 3), 3, pm), ib(C))
    t["repr"] = [(_sparse(rs, (C, C, 3, 3), 3, pm), ib(C)) for _ in range(2 * blocks)]
    Wd = np.concatenate([_sparse(rs, (C, C, 3, 3), 3, pm), _sparse(rs, (C, 16, 3, 3), 2, pm)], axis=1)
    t["dyn"] = [(Wd, ib(C))] + [(_sparse(rs, (C, C, 3, 3), 3, pm), ib(C)) for _ in range(2 * blocks)]
    t["embed"] = rs.randint(-2, 3, 16).astype(np.float64)
    sd = unfold(t, 3000 + size)
    m = M.Model(sd, dtype, size)
    obs = observations(size, seed=1)
    init = m.initial(obs)
    acts = actions(size)
    return dict(sd=sd, model=m, obs=obs, init=init, states=init["hidden"], actions=acts,
                rec=m.recurrent(init["hidden"], acts))
