"""tests/net_ref.py, the float64 model of the inference network, and the data of tests/net_cases.py (CPU only).

  * the model's convolution is tests/conv_ref.py's (pinned there to torch's float64 conv2d);
  * where no stored value needs rounding the model equals oracle/netref.py exactly, both towers and every head, at
    two sizes, so it inherits netref's pin to the reference forward;
  * network.pack_weights of the test state_dicts gives exactly the model's folded, rounded weights, biases and
    action table, read back through the documented index maps of pack_conv3x3 / pack_stem / pack_reward_fc1;
  * the conditions under which tests/test_net_kernels_gpu.py may demand bit equality hold for every case, decided
    by the model alone:
      exactness   every layer's and head's terms are multiples of its quantum q and sum |terms| < 2^24 q
      the rounding bites   over the last block's two convolutions at least 40 % (f16) / 80 % (bf16) of the exact sums
                  are not representable, at least 3 % are exact ties and at least 20 % are negative
      heads       at least a quarter of each head plane and each 64-wide hidden layer is nonzero after its ReLU, and no
                  row's three support logits are all equal
"""
import numpy as np
import pytest

import conv_ref as R
import net_cases as K
import net_ref as M
import netref

DN = {1: "f16", 2: "bf16"}


def test_magic_running_variances_fold_to_exact_powers_of_two():
    for root, var in K.VAR.items():
        assert np.float32(var) + np.float32(1e-4) == np.float32(root * root)
        assert np.sqrt(np.float32(var) + np.float32(1e-4)) == np.float32(root)


def test_quantum():
    assert M.quantum([0.0, 6.0, -20.0, 0.75]) == 0.25
    assert M.quantum([0.0]) == np.inf
    assert M.quantum([3 * 2.0 ** -30, 2.0 ** 40]) == 2.0 ** -30
    assert list(M.row_quantum(np.array([[4.0, 8.0], [1.5, 0.0]]))) == [4.0, 0.5]
    # channel by channel: row 0's fine channel meets coarse weights, row 1's zero channel meets none
    x = np.array([[[4.0, 0.25]], [[0.0, 8.0]]])  # [N][A][C]
    W = np.array([[0.5, 16.0], [1.0, 0.0]])      # [O][C]
    assert list(M.product_quantum(x, W)) == [2.0, 128.0]


def test_model_convolution_is_conv_ref():
    rs = np.random.RandomState(0)
    for H in (5, 8):
        x = rs.randint(-4, 5, (3, H * H, 128)).astype(np.float64)
        W = rs.randint(-3, 4, (128, 128, 3, 3)) / 4.0
        W[:, :, 1, 2] = 0  # a tap the model skips
        pre, mag = M._conv_terms(x, W, H)
        assert np.array_equal(pre, R.conv(x, W, H)) and np.array_equal(mag, R.abs_conv(x, W, H))


def test_store():
    pre = np.array([-3.0, -0.0, 0.0, 2049.0, 2051.0, 65519.0, 65520.0, 1e9, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26])
    want = np.array([0.0, 0.0, 0.0, 2048.0, 2052.0, 65504.0, 65504.0, 65504.0, 0.0, 2.0 ** -23, 0.0])
    got = M.store(pre, 1)
    assert np.array_equal(got, want) and not np.signbit(got).any()
    assert np.array_equal(M.store(np.array([257.0, 259.0, -1.0, 1e9]), 2), [256.0, 260.0, 0.0, 238 * 2.0 ** 22])
    for dt in (1, 2):
        y = M.store(got, dt)
        assert np.array_equal(M.from_bits16(M.bits16(y, dt), dt), y)


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("size,blocks", [(6, 1), (11, 2)])
def test_model_equals_netref_where_nothing_rounds(size, blocks, dtype):
    c = K.small_case(size, blocks, dtype)
    for o in (c["init"], c["rec"]):
        for l in o["tower"]:
            assert np.array_equal(R.round_to(l.pre, dtype), l.pre), l.name
        assert all(M.exact(l) for l in o["layers"])
    sd, H = c["sd"], size
    nchw = lambda h: h.transpose(0, 2, 1).reshape(len(h), 128, H, H)
    h = netref.representation(sd, c["obs"])
    assert h.max() > 4 and np.array_equal(h, nchw(c["init"]["hidden"]))
    lg, vl = netref.prediction(sd, h)
    assert np.array_equal(lg, c["init"]["logits"]) and np.array_equal(vl, c["init"]["value_logits"])
    nxt, rl = netref.dynamics(sd, h, c["actions"])
    assert np.array_equal(nxt, nchw(c["rec"]["hidden"])) and np.array_equal(rl, c["rec"]["reward_logits"])
    lg2, vl2 = netref.prediction(sd, nxt)
    assert np.array_equal(lg2, c["rec"]["logits"]) and np.array_equal(vl2, c["rec"]["value_logits"])
    for got, logits in ((c["init"]["value"], vl), (c["rec"]["value"], vl2), (c["rec"]["reward"], rl)):
        assert np.abs(got - netref.support_to_scalar(logits)[:, 0]).max() < 1e-6


def _unpack(N, packed, dtype):
    """pack_conv3x3's [9][4][8][64][8] back to float64 [o][c][3][3] through its documented index maps."""
    ks, nt, l, j = np.meshgrid(np.arange(4), np.arange(8), np.arange(64), np.arange(8), indexing="ij")
    o, c = N.output_channel(nt, l & 15), N.conv_input_channel(ks, l, j)
    W = np.full((128, 128, 9), np.nan)
    W[o, c] = np.moveaxis(M.from_bits16(packed, dtype), 0, -1)
    assert not np.isnan(W).any()
    return W.reshape(128, 128, 3, 3)


@pytest.mark.parametrize("case,dtype", [("dense", 1), ("dense", 2), ("taps", 1), ("taps", 2), ("saturate", 1),
                                        ("saturate_stem", 1), ("subnormal24", 1)])
def test_pack_weights_gives_the_models_weights(case, dtype):
    from datou_gomoku_muzero_amd import network as N
    from datou_gomoku_muzero_amd.config import GmzConfig
    size, blocks = (7, 2) if case != "subnormal24" else (5, 1)
    c = {"dense": lambda: K.dense_case(size, blocks, dtype), "taps": lambda: K.tap_case(size, dtype, 4)}.get(
        case, lambda: K.variant_case(size, blocks, case))()
    m, A = c["model"], size * size
    p = N.pack_weights(c["sd"], GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=blocks), K.PREC[dtype])
    nt, l, j = np.meshgrid(np.arange(8), np.arange(64), np.arange(8), indexing="ij")
    stem = np.zeros((128, 32))
    stem[N.output_channel(nt, l & 15), 8 * (l >> 4) + j] = M.from_bits16(p["repr_stem_w"], dtype)
    want = np.zeros((128, 32))
    want[:, :27] = m.stem[0].transpose(0, 2, 3, 1).reshape(128, 27)  # k = tap * 3 + c
    assert np.array_equal(stem, want) and np.array_equal(p["repr_stem_b"], m.stem[1])
    for name, convs in (("repr", m.repr), ("dyn", m.dyn)):
        assert len(p[name + "_convs"]) == len(convs)
        for k, (W, b) in enumerate(convs):
            assert np.array_equal(_unpack(N, p[name + "_convs"][k], dtype), W), (name, k)
            assert np.array_equal(p[name + "_bias"][k], b), (name, k)
    assert np.array_equal(p["dyn_action"], m.action)
    assert np.array_equal(p["head_conv_w"], m.head_w) and np.array_equal(p["head_conv_b"], m.head_b)
    assert np.array_equal(p["policy_fc_w"][:A, :2 * A], m.policy[0]) and np.array_equal(p["policy_fc_b"], m.policy[1])
    assert not p["policy_fc_w"][A:].any() and not p["policy_fc_w"][:, 2 * A:].any()
    assert np.array_equal(p["value_fc1_w"][:, :A], m.value1[0]) and not p["value_fc1_w"][:, A:].any()
    assert np.array_equal(p["value_fc2_w"].T, m.value2[0]) and np.array_equal(p["reward_fc2_w"].T, m.reward2[0])
    for key, wb in (("value_fc1_b", m.value1), ("value_fc2_b", m.value2), ("reward_fc1_b", m.reward1),
                    ("reward_fc2_b", m.reward2)):
        assert np.array_equal(p[key], wb[1]), key
    kk, nt, l, j = np.meshgrid(np.arange(A * 4), np.arange(4), np.arange(64), np.arange(8), indexing="ij")
    Wn = np.full((A * 128, 64), np.nan)  # [k = p * 128 + c][n]
    Wn[kk * 32 + 8 * (l >> 4) + j, nt * 16 + (l & 15)] = M.from_bits16(p["reward_fc1_w"], dtype)
    assert np.array_equal(Wn.reshape(A, 128, 64).transpose(2, 1, 0).reshape(64, 128 * A), m.reward1[0])


def check_exact(name, out):
    for l in out["layers"]:
        assert M.exact(l), "%s %s: sum |terms| spans %.2f bits of its quantum" % (name, l.name, M.span_bits(l))


def check_heads(name, out):
    assert ((out["planes"] > 0).mean(axis=(0, 2)) >= 0.25).all(), name
    for k in ("value", "reward"):
        if k + "_hidden" in out:
            assert (out[k + "_hidden"] > 0).mean() >= 0.25, (name, k)
            assert (np.ptp(out[k + "_logits"], axis=1) > 0).all(), (name, k)


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("size,blocks", K.CASES)
def test_dense_cases_meet_the_conditions(size, blocks, dtype):
    c = K.dense_case(size, blocks, dtype)
    for name in ("init", "rec"):
        out, what = c[name], "%dx%d %d blocks %s %s" % (size, size, blocks, DN[dtype], name)
        check_exact(what, out)
        check_heads(what, out)
        inexact, ties, neg = K.shares(out["tower"][-2:], dtype)
        print("%s: inexact %.3f ties %.3f negative %.3f, widest layer %.2f bits" % (
            what, inexact, ties, neg, max(M.span_bits(l) for l in out["layers"])))
        assert inexact >= (0.4 if dtype == 1 else 0.8) and ties >= 0.03 and neg >= 0.2, (what, inexact, ties, neg)
    assert np.array_equal(R.round_to(c["states"], dtype), c["states"])
    assert (c["states"][7:] == np.rint(c["states"][7:])).all() and c["states"][7:].max() >= (32768 if dtype == 1 else 2048)
    H = size
    ys, xs = np.divmod(c["actions"], H)
    edge = (ys == 0) | (ys == H - 1) | (xs == 0) | (xs == H - 1)
    corner = ((ys == 0) | (ys == H - 1)) & ((xs == 0) | (xs == H - 1))
    assert corner.sum() == 4 and (edge & ~corner).sum() >= 5 and (~edge).sum() >= 4 and len(set(c["actions"])) == K.ROWS


@pytest.mark.parametrize("size", K.SIZES)
def test_saturation_cases(size):
    """Sums past 65504 in the convs' store (at least 0.5 % of the last layer's) and in the stem's (at least two)."""
    c = K.variant_case(size, 2, "saturate")
    check_exact("saturate %d" % size, c["init"])
    check_heads("saturate %d" % size, c["init"])
    outs = [c["init"]] + ([K.dense_case(size, 2, 1)["rec"]] if size in K.SATURATE_REC_SIZES else [])
    for out in outs:
        pre = out["tower"][-1].pre
        assert (pre > 65504).mean() >= 0.005 and out["hidden"].max() == 65504.0 and np.isfinite(out["logits"]).all()
    c = K.variant_case(size, 2, "saturate_stem")
    check_exact("saturate_stem %d" % size, c["init"])
    check_heads("saturate_stem %d" % size, c["init"])
    stem = c["init"]["tower"][0].pre
    assert (stem > 65504).sum() >= 2
    assert (c["init"]["hidden"][:, :, K.STEM_SAT] >= 32768).any()  # the residual adds carried them to the hidden state


@pytest.mark.parametrize("size", K.SIZES)
def test_subnormal_cases(size):
    """One block: with two the magnitudes grow 1,400-fold from the stem to the hidden state, and a scale that puts the
    hidden state below 2^-14 rounds the stem's outputs away."""
    for variant, name in (("subnormal24", "init"), ("subnormal31", "rec")):
        c = K.variant_case(size, 1, variant)
        check_exact("%s %d" % (variant, size), c[name])
        h = c[name]["hidden"]
        nz = h[h > 0]
        assert (h > 0).mean() >= 0.25 and nz.min() >= 2.0 ** -24 and len(np.unique(nz)) >= 100
        assert (nz < 2.0 ** -14).mean() >= (1.0 if name == "init" else 0.95), (variant, (nz < 2.0 ** -14).mean())
        assert (np.ptp(c[name]["value_logits"], axis=1) > 0).all()


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("size,blocks", K.CASES)
def test_single_tap_cases_are_exact_and_cover_every_tap(size, blocks, dtype):
    for t0 in K.TAP_OFFSETS:
        c = K.tap_case(size, dtype, t0, blocks)
        assert c["model"].blocks == blocks
        for name in ("init", "rec"):
            check_exact("taps %d %d %s" % (size, t0, name), c[name])
            for l in c[name]["tower"]:
                assert np.array_equal(R.round_to(l.pre, dtype), l.pre) and (l.pre < 0).any()
            assert (c[name]["hidden"] > 0).mean() > 0.2
        for key, convs in (("repr", [c["model"].stem] + c["model"].repr), ("dyn", c["model"].dyn)):
            assert len(convs) == 1 + 2 * blocks == len(c["taps"][key])
            for k, (W, _) in enumerate(convs):
                nz = W[:, :128 if k or key == "dyn" else 3].reshape(128, -1, 9) != 0
                assert (nz.sum(axis=(1, 2)) == 1).all()  # one weight per output channel
                assert np.array_equal(nz.any(axis=1).argmax(axis=1), c["taps"][key][k])
                assert set(c["taps"][key][k]) == set(range(9))
