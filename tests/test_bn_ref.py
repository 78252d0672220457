"""tests/bn_ref.py (the float64 model the BatchNorm kernel tests compare against) pinned to torch.nn.BatchNorm1d/2d in
float64 on the rows the mask selects, and to closed forms where nn.BatchNorm has no say (rows outside the mask,
n = 0, n = 1).  CPU only."""
import numpy as np
import pytest
import torch

import bn_ref as R

EPS, MOM = 1e-4, 0.1
TOL = 1e-11  # float64 against float64: a few hundred roundings of 2^-53 on values of order 1 to 10


def _case(B, C, S, nvalid, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(B, C, S) * 2 + 0.5
    res = rs.randn(B, C, S)
    dy = rs.randn(B, C, S)
    mask = np.zeros(B, np.uint8)
    mask[rs.permutation(B)[:nvalid]] = 1
    gamma, beta = rs.uniform(0.5, 1.5, C), rs.uniform(-0.3, 0.3, C)
    rm, rv = rs.randn(C), rs.uniform(0.5, 2.0, C)
    return x, res, dy, mask, gamma, beta, rm, rv


def _torch_bn(C, S, gamma, beta, rm, rv):
    m = (torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM) if S == 1 else torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM))
    m = m.double()
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(gamma))
        m.bias.copy_(torch.from_numpy(beta))
        m.running_mean.copy_(torch.from_numpy(rm))
        m.running_var.copy_(torch.from_numpy(rv))
    return m


def _shape(a, S):  # [b][C][S] -> what BatchNorm1d ([b][C]) or BatchNorm2d ([b][C][S][1]) takes
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t[:, :, 0] if S == 1 else t[:, :, :, None]


def _back(t, S):
    a = t.detach().numpy()
    return a[:, :, None] if S == 1 else a[:, :, :, 0]


@pytest.mark.parametrize("B,C,S,nvalid", [(9, 5, 1, 6), (7, 3, 12, 4), (6, 4, 25, 6), (5, 2, 9, 2)])
@pytest.mark.parametrize("use_res,relu", [(False, False), (True, True), (False, True)])
def test_training_forward_and_backward_match_torch_on_the_masked_rows(B, C, S, nvalid, use_res, relu):
    x, res, dy, mask, gamma, beta, rm, rv = _case(B, C, S, nvalid, B * 100 + S)
    v = mask != 0
    m = _torch_bn(C, S, gamma, beta, rm, rv).train()
    xt = _shape(x[v], S).clone().requires_grad_(True)
    rt = _shape(res[v], S).clone().requires_grad_(True)
    yt = m(xt) + (rt if use_res else 0)
    if relu:
        yt = torch.relu(yt)
    yt.backward(_shape(dy[v], S))
    f = R.forward(x, mask, gamma, beta, EPS, MOM, res if use_res else None, relu, rm, rv, 3)
    assert f["n"] == nvalid * S
    np.testing.assert_allclose(f["y"][v], _back(yt, S), rtol=0, atol=TOL)
    np.testing.assert_allclose(f["rm"], m.running_mean.numpy(), rtol=0, atol=TOL)
    np.testing.assert_allclose(f["rv"], m.running_var.numpy(), rtol=0, atol=TOL)
    assert f["nb"] == 3 + int(m.num_batches_tracked) == 4
    b = R.backward(x, f["y"], dy, mask, gamma, f["mean"], f["invstd"], relu)
    np.testing.assert_allclose(b["dx"][v], _back(xt.grad, S), rtol=0, atol=TOL)
    np.testing.assert_allclose(b["dgamma"], m.weight.grad.numpy(), rtol=0, atol=TOL)
    np.testing.assert_allclose(b["dbeta"], m.bias.grad.numpy(), rtol=0, atol=TOL)
    if use_res:
        np.testing.assert_allclose(b["dres"][v], _back(rt.grad, S), rtol=0, atol=TOL)
    # rows outside the mask: normalised with the masked rows' statistics, no mean terms in dx (closed forms)
    c = (None, slice(None), None)
    sc = (gamma / np.sqrt(f["var"] + EPS))[c]
    pre = (x[~v] - f["mean"][c]) * sc + beta[c] + (res[~v] if use_res else 0)
    np.testing.assert_allclose(f["y"][~v], np.maximum(pre, 0) if relu else pre, rtol=0, atol=TOL)
    dz = dy[~v] * (pre > 0) if relu else dy[~v]
    np.testing.assert_allclose(b["dx"][~v], sc * dz, rtol=0, atol=TOL)
    np.testing.assert_array_equal(b["dres"][~v], dz)


@pytest.mark.parametrize("S", [1, 12])
def test_eval_matches_torch(S):
    B, C = 6, 5
    x, res, _, _, gamma, beta, rm, rv = _case(B, C, S, B, 77 + S)
    m = _torch_bn(C, S, gamma, beta, rm, rv).eval()
    want = torch.relu(m(_shape(x, S)) + _shape(res, S))
    got = R.evaluate(x, gamma, beta, rm, rv, EPS, res, True)
    np.testing.assert_allclose(got["y"], _back(want, S), rtol=0, atol=TOL)


def test_empty_mask_and_single_element_closed_forms():
    B, C, S = 4, 3, 1
    x, res, dy, _, gamma, beta, rm, rv = _case(B, C, S, 0, 5)
    c = (None, slice(None), None)
    # n = 0: mean 0, var 0, running statistics and the counter untouched, every row normalised all the same
    f = R.forward(x, np.zeros(B, np.uint8), gamma, beta, EPS, MOM, None, False, rm, rv, 7)
    assert f["n"] == 0 and not f["mean"].any() and not f["var"].any()
    np.testing.assert_allclose(f["invstd"], EPS ** -0.5, rtol=1e-15)
    assert f["rm"] is rm and f["rv"] is rv and f["nb"] == 7
    np.testing.assert_allclose(f["y"], x * (gamma * EPS ** -0.5)[c] + beta[c], rtol=0, atol=1e-9)
    b = R.backward(x, f["y"], dy, np.zeros(B, np.uint8), gamma, f["mean"], f["invstd"], False)
    assert not b["dgamma"].any() and not b["dbeta"].any()
    np.testing.assert_allclose(b["dx"], dy * (gamma * EPS ** -0.5)[c], rtol=1e-14)
    # n = 1: var 0, and the running variance takes m * var (no n / (n - 1))
    mask = np.array([0, 0, 1, 0], np.uint8)
    f = R.forward(x, mask, gamma, beta, EPS, MOM, None, False, rm, rv, 7)
    assert f["n"] == 1 and not f["var"].any()
    np.testing.assert_array_equal(f["mean"], x[2, :, 0])
    np.testing.assert_allclose(f["rm"], 0.9 * rm + 0.1 * x[2, :, 0], rtol=0, atol=TOL)
    np.testing.assert_allclose(f["rv"], 0.9 * rv, rtol=0, atol=TOL)
    assert f["nb"] == 8
    np.testing.assert_allclose(f["y"][2, :, 0], beta, rtol=0, atol=TOL)
    b = R.backward(x, f["y"], dy, mask, gamma, f["mean"], f["invstd"], False)
    np.testing.assert_allclose(b["dx"][2], 0, atol=1e-9)  # dz - dz / 1 - 0 * dgamma


def test_segments_are_forward_calls_in_order():
    B, C, S, nseg = 6, 3, 4, 3
    x, res, _, mask, gamma, beta, rm, rv = _case(B, C, S, 4, 11)
    mask[:] = [1, 0, 0, 0, 1, 1]  # the middle segment has no live row
    segs, rm2, rv2, nb2 = R.forward_seg(x, mask, nseg, gamma, beta, EPS, MOM, res, True, rm, rv, 0)
    erm, erv, enb = rm, rv, 0
    for g in range(nseg):
        sl = slice(2 * g, 2 * g + 2)
        f = R.forward(x[sl], mask[sl], gamma, beta, EPS, MOM, res[sl], True, erm, erv, enb)
        erm, erv, enb = f["rm"], f["rv"], f["nb"]
        np.testing.assert_array_equal(segs[g]["y"], f["y"])
    assert nb2 == enb == 2
    np.testing.assert_array_equal(rm2, erm)
    np.testing.assert_array_equal(rv2, erv)
    assert segs[1]["n"] == 0 and not segs[1]["mean"].any()


@pytest.mark.parametrize("ns", [1, 5, 300])
def test_partials_do_not_depend_on_the_cut(ns):
    B, C, S = 7, 4, 9
    x, _, dy, mask, *_ = _case(B, C, S, 4, 3)
    n, mean, var, _, _ = R.stats(x, mask)
    for seed in (0, 1):
        bounds = R.cuts(B * S, ns, seed)
        assert bounds[0] == 0 and bounds[-1] == B * S and (np.diff(bounds) >= 0).all()
        p = R.partials(x, x * x, mask, bounds)
        assert p.shape == (C, ns, 3)
        pn, pm, pv = R.stats_from_partials(p)
        assert (pn == n).all()
        np.testing.assert_allclose(pm, mean, rtol=0, atol=TOL)
        np.testing.assert_allclose(pv, var, rtol=0, atol=TOL)
    if ns > 2:
        assert (np.diff(R.cuts(B * S, ns, 0)) == 0).any()  # an empty range
    pb = R.board_partials(x, mask)
    assert pb.shape == (C, B, 3) and not pb[:, mask == 0].any() and (pb[:, mask != 0, 2] == S).all()
    np.testing.assert_allclose(R.stats_from_partials(pb)[1], mean, rtol=0, atol=TOL)
    b = R.backward(x, x, dy, mask, np.ones(C), mean, 1 / np.sqrt(var + EPS), True)
    p = R.partials(b["dz"], b["dz"] * b["xhat"], mask, R.cuts(B * S, ns, 2))
    np.testing.assert_allclose(p[:, :, 0].sum(axis=1), b["dbeta"], rtol=0, atol=TOL)
    np.testing.assert_allclose(p[:, :, 1].sum(axis=1), b["dgamma"], rtol=0, atol=TOL)


def test_model_does_not_import_the_package():
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "bn_ref.py")).read()
    assert "datou" not in src and "import torch" not in src
