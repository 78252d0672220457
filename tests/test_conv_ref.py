"""tests/conv_ref.py (the float64 model the conv kernel tests compare with) against torch on the CPU: float64
F.conv2d and its autograd for the forward, the input gradient through the transposed weights and the weight
gradient; torch's own f32 -> f16 / bf16 conversion for the rounding; brute-force loops for the stamp and the sums."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref
import conv_ref as R

TD = {1: torch.float16, 2: torch.bfloat16}
SHAPES = [(6, 1), (6, 3), (9, 2), (9, 3)]


def _nchw(a, H):
    N, A, C = a.shape
    return torch.from_numpy(np.ascontiguousarray(a.reshape(N, H, H, C).transpose(0, 3, 1, 2)))


def _nhwc(t):
    N, C, H, _ = t.shape
    return t.detach().numpy().transpose(0, 2, 3, 1).reshape(N, H * H, C)


def _data(H, N, seed, C=R.CC, O=R.CC):
    rs = np.random.RandomState(seed)
    return rs.randn(N, H * H, C), rs.randn(O, C, 3, 3) / 34, rs.randn(N, H * H, O)


@pytest.mark.parametrize("H,N", SHAPES)
def test_conv_and_both_gradients_are_torch_float64(H, N):
    x, W, dy = _data(H, N, 10 * H + N)
    xt, wt = _nchw(x, H).requires_grad_(), torch.from_numpy(W).requires_grad_()
    yt = F.conv2d(xt, wt, padding=1)
    yt.backward(_nchw(dy, H))
    y = R.conv(x, W, H)
    scale = np.abs(_nhwc(yt)).max()
    assert np.abs(y - _nhwc(yt)).max() <= 1e-13 * scale
    # dx = conv(dy, W'), W'[c][o][t] = W[o][c][8 - t]
    dx = R.conv(dy, R.w_eff(W, 1), H)
    assert np.abs(dx - _nhwc(xt.grad)).max() <= 1e-13 * np.abs(_nhwc(xt.grad)).max()
    dw = R.wgrad(x, dy, H)
    assert dw.shape == (128, 128, 3, 3)
    assert np.abs(dw - wt.grad.numpy()).max() <= 1e-13 * np.abs(wt.grad.numpy()).max()
    # the accumulate form and the segment form (any order, unequal to the address order)
    dw0 = np.random.RandomState(1).randn(128, 128, 3, 3)
    assert np.array_equal(R.wgrad(x, dy, H, dw0), dw + dw0)
    if N == 3:
        segs = [(x[i:i + 1], dy[i:i + 1]) for i in (2, 0, 1)]
        got = R.wgrad_segments([s[0] for s in segs], [s[1] for s in segs], H, dw0)
        assert np.abs(got - (dw + dw0)).max() <= 1e-13 * np.abs(dw).max()


def test_conv_taps_by_hand():
    """One 1.0 at (row 1, column 2), channel 5, of a 6x6 board: y[q][o] = W[o][5][t] with d(t) = cell - q."""
    H = 6
    x = np.zeros((1, 36, 128))
    x[0, 1 * H + 2, 5] = 1.0
    W = np.random.RandomState(0).randn(128, 128, 3, 3)
    y = R.conv(x, W, H).reshape(H, H, 128)
    want = np.zeros((H, H, 128))
    for ky in range(3):
        for kx in range(3):
            want[1 - (ky - 1), 2 - (kx - 1)] = W[:, 5, ky, kx]  # q + d(t) = cell
    assert np.array_equal(y, want)
    assert not np.signbit(y).any() or (y[np.signbit(y)] != 0).all()  # zeros are +0.0
    # the weight gradient of that x with dy one-hot at cell (2, 2), channel 9: d(t) = (1, 2) - (2, 2) = (-1, 0): t = 1
    dy = np.zeros((1, 36, 128))
    dy[0, 2 * H + 2, 9] = 1.0
    dw = R.wgrad(x, dy, H)
    assert dw[9, 5, 0, 1] == 1.0 and np.count_nonzero(dw) == 1
    # cells that are neighbours only by wrapping across a row end contribute nothing
    x2, dy2 = np.zeros((1, 36, 128)), np.zeros((1, 36, 128))
    x2[0, 1 * H + 0, 0], dy2[0, 0 * H + 5, 0] = 1.0, 1.0
    assert not R.wgrad(x2, dy2, H).any()


def test_transposed_weights_round_trip():
    W = np.random.RandomState(3).randn(128, 128, 3, 3)
    assert R.w_eff(W, 0) is W or np.array_equal(R.w_eff(W, 0), W)
    Wt = R.w_eff(W, 1)
    assert Wt[7, 100, 0, 2] == W[100, 7, 2, 0] and Wt[3, 4, 1, 1] == W[4, 3, 1, 1]
    for t in range(9):
        assert np.array_equal(Wt[:, :, t // 3, t % 3], W[:, :, (8 - t) // 3, (8 - t) % 3].T)
    assert np.array_equal(R.w_eff(Wt, 1), W)
    # <conv(x, W), dy> = <x, conv(dy, W')>: the adjoint identity, with no autograd in it
    x, _, dy = _data(6, 2, 4)
    a, b = (R.conv(x, W, 6) * dy).sum(), (x * R.conv(dy, Wt, 6)).sum()
    assert abs(a - b) <= 1e-12 * abs(a)


@pytest.mark.parametrize("dt", [1, 2])
def test_round_to_is_the_types_own_rounding(dt):
    rs = np.random.RandomState(dt)
    v = np.concatenate([rs.randn(20000) * 10.0 ** rs.uniform(-9, 4.5, 20000), [0.0, -0.0, 65504.0, 65519.9, 65520.0,
                        1e-8, 2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -25, 70000.0, 3.3e38, 3.4e38]])
    v = v.astype(np.float32).astype(np.float64)  # f32 values: torch's conversion from f32 is ONE rounding
    want = torch.from_numpy(v.astype(np.float32)).to(TD[dt]).double().numpy()
    got = R.round_to(v, dt)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    # exact ties go to the even neighbour, both parities, and one rounding from float64 is not two through f32
    lo, q = R.ulp_gap(np.minimum(np.abs(v[:20000]), 6e4) + 2.0 ** -20, dt)  # below the f16 overflow
    ties = lo + q / 2
    assert R.is_tie(ties, dt).all() and not R.is_tie(lo, dt).any()
    r = R.round_to(ties, dt)
    odd = np.rint(lo / q) % 2 == 1
    assert odd.any() and (~odd).any()
    assert np.array_equal(r, np.where(odd, lo + q, lo))
    assert np.array_equal(R.round_to(-ties, dt), -r)
    above = ties * (1 + 2.0 ** -40)  # through f32 this would collapse onto the tie and could round down
    assert np.array_equal(R.round_to(above, dt), lo + q)
    assert np.array_equal(R.round_to(r, dt), r)  # idempotent


def test_forward_add_rounds_once():
    H, dt = 6, 1
    x = np.zeros((1, 36, 128))
    x[0, 14, 0] = 1.0
    W = np.zeros((128, 128, 3, 3))
    W[:, 0, 1, 1] = 1.0 + 2.0 ** -11  # a tie of f16 were it stored alone: 1.0 (even)
    add = np.full((1, 36, 128), 2.0 ** -11)
    y = R.forward(x, W, H, dt, addend=add)
    assert (y[0, 14] == 1.0 + 2.0 ** -10).all()  # the exact sum 1 + 2^-10 is representable
    assert (R.round_to(R.round_to(R.conv(x, W, H), dt) + add, dt)[0, 14] == 1.0).all()  # two roundings differ
    assert (y[0, 13] == 2.0 ** -11).all()


@pytest.mark.parametrize("H", [6, 9])
def test_stamp_is_the_144_channel_conv_of_a_one_hot_action_plane(H):
    """The model's stamp against (a) a brute-force loop over output cells and taps and (b) torch's float64 conv of
    the full 144-plane input of network.py:79-96: 128 hidden planes + the 16-plane embedding at the action cell."""
    N = 3
    rs = np.random.RandomState(H)
    x = rs.randn(N, H * H, 128)
    W = rs.randn(128, 144, 3, 3) / 34
    embed = rs.randn(16)
    actions = np.array([0, H * H - 1, 2 * H + H - 1])  # two corners and a right-edge cell
    table = np.stack([(W[:, 128:, t // 3, t % 3] * embed[None, :]).sum(axis=1) for t in range(9)])
    st = R.stamp_terms(actions, table, H)
    brute = np.zeros((N, H * H, 128))
    for n in range(N):
        ay, ax = divmod(int(actions[n]), H)
        for qy in range(H):
            for qx in range(H):
                dy, dx = ay - qy + 1, ax - qx + 1
                if 0 <= dy <= 2 and 0 <= dx <= 2:
                    brute[n, qy * H + qx] += table[dy * 3 + dx]
    assert np.array_equal(st, brute)
    assert [int((np.abs(st[n]).sum(axis=1) > 0).sum()) for n in range(N)] == [4, 4, 6]  # off-board cells dropped
    full = np.zeros((N, H * H, 144))
    full[:, :, :128] = x
    for n in range(N):
        full[n, actions[n], 128:] = embed
    want = _nhwc(F.conv2d(_nchw(full, H), torch.from_numpy(W), padding=1))
    got = R.conv(x, W[:, :128], H) + st
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # forward() adds it before the one rounding
    y = R.forward(x, W[:, :128], H, 2, actions=actions, table=table)
    assert np.array_equal(y, R.round_to(got, 2))


@pytest.mark.parametrize("mask", [None, [1, 1, 1], [0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]])
def test_statistics_forms(mask):
    H, N = 6, 3
    rs = np.random.RandomState(5)
    y = R.round_to(rs.randn(N, H * H, 128), 1)
    v = [n for n in range(N) if mask is None or mask[n]]
    s = R.stats(y, mask)
    want = np.zeros((128, 3))
    for n in v:
        for p in range(H * H):
            want[:, 0] += y[n, p]
            want[:, 1] += y[n, p] ** 2
            want[:, 2] += 1
    assert np.allclose(s, want, rtol=1e-13, atol=1e-13) and np.array_equal(s[:, 2], want[:, 2])
    b = R.board_stats(y, mask)
    assert b.shape == (128, N, 3)
    assert np.allclose(b.sum(axis=1), s, rtol=1e-13, atol=1e-13)
    for n in range(N):
        if n not in v:
            assert not b[:, n].any()
        else:
            assert (b[:, n, 2] == H * H).all()
    # the per-board form is bn_ref's (the layout gmz_bn_forward_seg consumes)
    assert np.allclose(b, bn_ref.board_partials(y.transpose(0, 2, 1), mask), rtol=1e-13, atol=1e-13)
    # backward sums = bn_ref's dbeta / dgamma with the conv output as the BatchNorm's dy
    bn_x, bn_y = rs.randn(N, H * H, 128), np.maximum(rs.randn(N, H * H, 128), 0)
    mean, invstd = rs.randn(128), rs.uniform(0.5, 2, 128)
    for relu in (False, True):
        got = R.bwd_stats(y, bn_x, bn_y, mean, invstd, relu, mask)
        bw = bn_ref.backward(bn_x.transpose(0, 2, 1), bn_y.transpose(0, 2, 1), y.transpose(0, 2, 1), mask,
                             np.ones(128), mean, invstd, relu)
        assert np.allclose(got[:, 0], bw["dbeta"], rtol=1e-12, atol=1e-12)
        assert np.allclose(got[:, 1], bw["dgamma"], rtol=1e-12, atol=1e-12)
        assert (got[:, 2] == bw["n"]).all()
