"""tests/opt_ref.py pinned to independent arithmetic (CPU only): torch.optim.Adam(weight_decay) in float64 over
several steps, torch.nn.utils.clip_grad_norm_, the GradScaler's skip rule and the soft target update as plain code,
and a brute-force loop for gmz_grad_add_t_cols."""
import numpy as np
import pytest
import torch

import opt_ref as O

HP = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def _f(v):
    return O.f32(v)


@pytest.mark.parametrize("scale", [None, 1 / 16, 65536.0])
@pytest.mark.parametrize("wd,max_norm", [(0.0, 5.0), (1e-2, 5.0), (1e-4, 1e9)])
def test_opt_model_is_clip_adam_and_soft_update(scale, wd, max_norm):
    rs = np.random.RandomState(11)
    sizes = [5, 1, 17]
    ps = [torch.tensor(rs.randn(n), dtype=torch.float64, requires_grad=True) for n in sizes]
    ts = [torch.tensor(rs.randn(n), dtype=torch.float64) for n in sizes]
    has = [True, False, True]
    tau = 0.05
    opt = torch.optim.Adam(ps, lr=_f(HP["lr"]), betas=(_f(HP["beta1"]), _f(HP["beta2"])), eps=_f(HP["eps"]),
                           weight_decay=_f(wd))
    N = sum(sizes)
    p, t = np.concatenate([q.detach().numpy() for q in ps]), np.concatenate([q.numpy() for q in ts])
    has_t = np.concatenate([np.full(n, h) for n, h in zip(sizes, has)])
    m, v, step = np.zeros(N), np.zeros(N), 0.0
    sc = 1.0 if scale is None else scale
    clipped = []
    for it in range(6):
        g_unscaled = rs.randn(N) * (0.1 if it % 2 else 3.0)
        g = g_unscaled * sc  # the bucket holds the scaled gradient
        if it == 3:
            g[7] = np.inf
        # --- the reference sequence: unscale, found_inf, clip, step unless found_inf, soft update
        grads = np.split(g / sc, np.cumsum(sizes)[:-1])
        found_inf = not np.isfinite(g).all()
        for q, gr in zip(ps, grads):
            q.grad = torch.tensor(gr)
        if not found_inf:
            total = torch.nn.utils.clip_grad_norm_(ps, _f(max_norm))
            clipped.append(float(total) > _f(max_norm))
            opt.step()
        with torch.no_grad():
            for q, tt, h in zip(ps, ts, has):
                if h:
                    tt.mul_(1 - _f(tau)).add_(_f(tau) * q)
        # --- the model
        o = O.opt_step(p, t, has_t, g, m, v, step, scale, 1, max_norm, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], wd, tau)
        assert o["skip"] == found_inf and o["coef"][0] == float(found_inf)
        assert o["step"] == step + (0 if found_inf else 1)
        if found_inf:
            assert np.array_equal(o["p"], p) and np.array_equal(o["m"], m) and np.array_equal(o["v"], v)
        else:
            np.testing.assert_allclose(o["norm"], float(total), rtol=1e-13)
        p, t, m, v, step = o["p"], o["t"], o["m"], o["v"], o["step"]
        assert not o["g"].any()
        np.testing.assert_allclose(p, np.concatenate([q.detach().numpy() for q in ps]), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(t, np.concatenate([q.numpy() for q in ts]), rtol=1e-10, atol=1e-13)
        st = opt.state[ps[0]]
        if st:
            np.testing.assert_allclose(m[:5], st["exp_avg"].numpy(), rtol=1e-10, atol=1e-15)
            np.testing.assert_allclose(v[:5], st["exp_avg_sq"].numpy(), rtol=1e-10, atol=1e-18)
    assert step == 5.0
    assert (any(clipped) and not all(clipped)) if max_norm == 5.0 else not any(clipped)  # both sides of the clip ran


def test_opt_model_without_skip_takes_the_step():
    g = np.array([1.0, np.inf])
    z = np.zeros(2)
    o = O.opt_step(z, z, np.array([True, True]), g, z, z, 4.0, None, 0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.5)
    assert not o["skip"] and o["coef"][0] == 0.0 and o["step"] == 5.0 and not o["g"].any()


def test_opt_model_uses_the_float32_arguments():
    one = np.ones(1)
    o = O.opt_step(one, one, np.array([False]), one, 0 * one, 0 * one, 0.0, None, 1, 1e9, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0)
    b1 = float(np.float32(0.9))
    assert o["bc1"] == 1 - b1 and o["m"][0] == (1 - b1) * 1.0 and o["bc1"] != 1 - 0.9


@pytest.mark.parametrize("P,C,O_,ldo,col0", [(3, 2, 4, 7, 3), (1, 1, 1, 1, 0), (5, 1, 2, 2, 0), (2, 3, 1, 4, 2)])
def test_grad_add_t_cols_model_is_the_indexed_add(P, C, O_, ldo, col0):
    rs = np.random.RandomState(P + C)
    src, dst = rs.randn(P * C * ldo), rs.randn(O_ * C * P)
    want = dst.copy()
    for o in range(O_):
        for c in range(C):
            for p in range(P):
                want[(o * C + c) * P + p] += src[(p * C + c) * ldo + col0 + o]
    assert np.array_equal(O.grad_add_t_cols(dst, src, P, C, O_, ldo, col0).ravel(), want)
