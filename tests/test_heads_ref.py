"""tests/heads_ref.py pinned to independent arithmetic (CPU only): torch float64 conv2d(1x1) and
nn.BatchNorm1d/2d applied segment by segment to the live rows, with autograd for every gradient."""
import numpy as np
import pytest
import torch

import heads_ref as H

EPS, MOM = 1e-4, 0.1


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("O0,O1,bias", [(1, 0, True), (2, 1, True), (1, 3, False), (2, 2, True), (2, 0, False)])
def test_head_conv_model_is_conv2d(dt, O0, O1, bias):
    rs = np.random.RandomState(7 * O0 + O1 + dt)
    P = 45
    x = H.round_to(rs.randn(P, 128), dt)
    w0, w1 = rs.randn(O0, 128) * 0.1, (rs.randn(O1, 128) * 0.1 if O1 else None)
    b0, b1 = (rs.randn(O0), rs.randn(O1) if O1 else None) if bias else (None, None)
    f = H.head_forward(x, w0, b0, w1, b1, dt)
    # the parameters as the kernel sees them: rounded to the activation dtype
    W = _t(H.round_to(np.concatenate([w0] + ([w1] if O1 else [])), dt), True)
    b = _t(H.round_to(np.concatenate([b0] + ([b1] if O1 else [])), dt) if bias else np.zeros(O0 + O1))
    assert np.array_equal(W.detach().numpy(), f["W"]) and np.array_equal(b.numpy(), f["b"])
    xt = _t(x.reshape(5, 9, 128).transpose(0, 2, 1).reshape(5, 128, 3, 3), True)  # NCHW view of the channels-last rows
    bt = b.clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(xt, W.reshape(O0 + O1, 128, 1, 1), bt)
    want = y.detach().numpy().transpose(0, 2, 3, 1).reshape(P, O0 + O1)
    np.testing.assert_allclose(f["exact"], want, rtol=1e-13, atol=1e-13)
    assert np.array_equal(f["y"], H.round_to(f["exact"], dt))
    dy = H.round_to(rs.randn(P, O0 + O1), dt)
    y.backward(_t(dy.reshape(5, 3, 3, O0 + O1).transpose(0, 3, 1, 2)))
    acc = (rs.randn(O0 + O1, 128), rs.randn(O0 + O1))
    for a in (None, acc):
        bw = H.head_backward(x, dy, w0, w1, dt, a)
        np.testing.assert_allclose(bw["dx_exact"], xt.grad.numpy().transpose(0, 2, 3, 1).reshape(P, 128), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(bw["dW"], W.grad.numpy() + (0 if a is None else a[0]), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(bw["db"], bt.grad.numpy() + (0 if a is None else a[1]), rtol=1e-13, atol=1e-13)
        assert np.array_equal(bw["dx"], H.round_to(bw["dx_exact"], dt))


def test_round_to_is_one_rounding_to_nearest_even():
    a = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -30, 2049.0, 65520.0])
    assert np.array_equal(H.round_to(a, 1), [1.0, 1 + 2.0 ** -9, 1 + 2.0 ** -10, 2048.0, np.inf])
    # torch rounds float64 to a 16-bit type through float32 (element 2 shows it: two roundings), so compare from f32
    b = a[[0, 1, 3, 4]]
    assert np.array_equal(H.round_to(b, 1), torch.tensor(b).float().to(torch.float16).double().numpy())
    assert np.array_equal(H.round_to(b[:3], 2), torch.tensor(b[:3]).float().to(torch.bfloat16).double().numpy())


def _torch_segments(x, mask, nseg, gamma, beta, S, bn, order_pre=None):
    """nn.BatchNorm over each segment's live rows (in segment order, a pre-call's segment first), y for every row,
    and autograd's gradients of sum(dy * y)."""
    R, _, C = x.shape
    B = R // nseg
    live = np.ones(R, bool) if mask is None else mask != 0
    xt = _t(x, True)
    ys = []
    for sg in range(nseg):
        if order_pre is not None and len(order_pre[sg]):
            bn(_t(order_pre[sg]))
        xs = xt[sg * B:(sg + 1) * B]
        lv = torch.from_numpy(live[sg * B:(sg + 1) * B])
        if not lv.any():  # a dead segment: no statistics step; mean 0, var 0
            ys.append(xs / np.sqrt(EPS) * bn.weight + bn.bias)
            continue
        xl = xs[lv]  # [rows][S][C]
        flat = xl.reshape(-1, C)
        yl = bn(flat).reshape(xl.shape)
        mean, var = flat.mean(0), flat.var(0, unbiased=False)
        yo = (xs - mean) / torch.sqrt(var + EPS) * bn.weight + bn.bias  # the rows outside the mask: same statistics
        full = yo.clone()
        full[lv] = yl
        ys.append(full)
    return xt, torch.cat(ys)


@pytest.mark.parametrize("nseg,B,S,C,kind", [(1, 7, 1, 3, "null"), (4, 6, 5, 2, "ragged"), (3, 5, 4, 9, "dead_mid"),
                                             (3, 5, 1, 1, "dead_first"), (3, 4, 3, 2, "dead_last")])
def test_seg_bn_model_is_batchnorm_per_segment(nseg, B, S, C, kind):
    rs = np.random.RandomState(nseg * 100 + B)
    R = nseg * B
    x, x_pre = rs.randn(R, S, C) * 2 + 0.5, rs.randn(R, S, C) + 1
    dy = rs.randn(R, S, C)
    mask = None
    if kind != "null":
        mask = (rs.rand(R) < 0.6).astype(np.uint8)
        mask[::B] = 1
        mask[1::B] = 1  # two live rows at least: nn.BatchNorm refuses one value per channel
        dead = {"dead_first": 0, "dead_mid": 1, "dead_last": nseg - 1}.get(kind)
        if dead is not None:
            mask[dead * B:(dead + 1) * B] = 0
    mask_pre = (np.arange(R) % 3 != 0).astype(np.uint8)  # other live-row counts than this call's
    mask_pre[:B] = 0  # and a dead segment of its own: skipped in the interleaved order too
    gamma, beta = rs.uniform(0.5, 1.5, C), rs.uniform(-0.3, 0.3, C)
    rm0, rv0 = rs.randn(C), rs.uniform(0.5, 2, C)
    fp = H.seg_forward(x_pre, mask_pre, nseg, None, None, EPS)
    assert (fp["rows"] != H.seg_forward(x, mask, nseg, None, None, EPS)["rows"]).any()
    for pre in (None, fp):
        f = H.seg_forward(x, mask, nseg, gamma, beta, EPS, MOM, rm0, rv0, 5, pre)
        bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM).double()
        with torch.no_grad():
            bn.weight.copy_(_t(gamma)), bn.bias.copy_(_t(beta))
            bn.running_mean.copy_(_t(rm0)), bn.running_var.copy_(_t(rv0))
            bn.num_batches_tracked.fill_(5)
        order = None if pre is None else [x_pre[sg * B:(sg + 1) * B][mask_pre[sg * B:(sg + 1) * B] != 0].reshape(-1, C)
                                          for sg in range(nseg)]
        xt, y = _torch_segments(x, mask, nseg, gamma, beta, S, bn, order)
        np.testing.assert_allclose(f["y"], y.detach().numpy(), rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(f["rm"], bn.running_mean.numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(f["rv"], bn.running_var.numpy(), rtol=1e-12, atol=1e-12)
        assert f["nb"] == int(bn.num_batches_tracked)
        live_segs = int((f["rows"] > 0).sum()) + (0 if pre is None else int((fp["rows"] > 0).sum()))
        assert f["nb"] == 5 + live_segs
    if kind == "null":
        assert (f["rows"] == B).all()
    y.backward(_t(dy))
    bw = H.seg_backward(x, dy, mask, nseg, gamma, f["mean"], f["invstd"], f["rows"])
    np.testing.assert_allclose(bw["dx"], xt.grad.numpy(), rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(bw["dgamma"], bn.weight.grad.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(bw["dbeta"], bn.bias.grad.numpy(), rtol=1e-10, atol=1e-10)
    acc = (rs.randn(C), rs.randn(C))
    bwa = H.seg_backward(x, dy, mask, nseg, gamma, f["mean"], f["invstd"], f["rows"], acc)
    assert np.array_equal(bwa["dgamma"], acc[0] + bw["dgamma"]) and np.array_equal(bwa["dbeta"], acc[1] + bw["dbeta"])
    # the layout of the stats vector
    sv = H.stats_vector(f)
    assert sv.shape == (3 * nseg * C + nseg,) and np.array_equal(sv[-nseg:], f["rows"])
    assert np.array_equal(sv[nseg * C:2 * nseg * C].reshape(nseg, C), f["invstd"])


def test_seg_bn_model_2d_is_batchnorm2d():
    """S > 1 against nn.BatchNorm2d on an NCHW view of the live rows."""
    rs = np.random.RandomState(3)
    nseg, B, S, C = 2, 4, 9, 3
    x = rs.randn(nseg * B, S, C)
    mask = np.array([1, 0, 1, 1, 0, 1, 1, 0], np.uint8)
    f = H.seg_forward(x, mask, nseg, None, None, EPS, MOM, np.zeros(C), np.ones(C), 0)
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM).double()
    for sg in range(nseg):
        xs = x[sg * B:(sg + 1) * B][mask[sg * B:(sg + 1) * B] != 0]
        y = bn(_t(xs.transpose(0, 2, 1).reshape(-1, C, 3, 3))).detach().numpy().reshape(-1, C, S).transpose(0, 2, 1)
        np.testing.assert_allclose(f["y"][sg * B:(sg + 1) * B][mask[sg * B:(sg + 1) * B] != 0], y, rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(f["rm"], bn.running_mean.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f["rv"], bn.running_var.numpy(), rtol=1e-12, atol=1e-12)
    assert f["nb"] == 2 and np.array_equal(f["rows"], [3, 2])


def test_seg_bn_model_single_live_row_and_dead_segment():
    """What nn.BatchNorm refuses (one value per channel) and never sees (no live row), by the documented rule."""
    x = np.array([[[3.0, -1.0]], [[5.0, 2.0]], [[7.0, 4.0]], [[9.0, 8.0]]])  # nseg = 2, B = 2, S = 1, C = 2
    mask = np.array([0, 1, 0, 0], np.uint8)
    rm0, rv0 = np.array([1.0, 2.0]), np.array([3.0, 4.0])
    f = H.seg_forward(x, mask, 2, None, None, EPS, MOM, rm0, rv0, 0)
    assert np.array_equal(f["rows"], [1, 0]) and np.array_equal(f["mean"], [[5.0, 2.0], [0.0, 0.0]])
    assert not f["var"].any() and not f["unb"].any()  # n = 1: the biased variance (0), no division by n - 1
    assert np.allclose(f["invstd"], 1 / np.sqrt(EPS), rtol=1e-15)
    np.testing.assert_allclose(f["rm"], 0.9 * rm0 + 0.1 * np.array([5.0, 2.0]), rtol=1e-15)
    np.testing.assert_allclose(f["rv"], 0.9 * rv0, rtol=1e-15)
    assert f["nb"] == 1
    np.testing.assert_allclose(f["y"][2:], x[2:] / np.sqrt(EPS), rtol=1e-15)  # the dead segment is still normalised
    dy = np.ones_like(x)
    bw = H.seg_backward(x, dy, mask, 2, None, f["mean"], f["invstd"], f["rows"])
    np.testing.assert_allclose(bw["dx"][2:], dy[2:] / np.sqrt(EPS), rtol=1e-15)  # n = 0: dx = gamma invstd dy
    # segment 0: G1 = 2, G2 = sum xhat over BOTH rows; only the live row takes the mean / variance terms
    xh = (x[:2] - f["mean"][0]) * f["invstd"][0]
    G2 = xh.sum(axis=(0, 1))
    np.testing.assert_allclose(bw["dx"][1], f["invstd"][0] * (1 - (2 + xh[1] * G2)), rtol=1e-12)
    np.testing.assert_allclose(bw["dx"][0], f["invstd"][0] * np.ones((1, 2)), rtol=1e-15)
