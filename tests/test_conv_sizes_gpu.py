"""The trainer's 128 -> 128 3x3 convolutions (csrc/gmz_conv.hip) at the board sizes beyond 9 and 15: 19x19 (config
C5; one workgroup per CU in the forward, the weight gradient in two row bands of LDS) and 6x6 (the reference's default
BOARD_SIZE).  Forward, input and weight gradients, the multi-segment weight gradient, the epilogue's masked
BatchNorm statistics, the BatchNorm-apply prologue, one residual block, the reference-pinned training step and the
graph-captured trainer.  Tolerances are the ones the 9x9 / 15x15 tests of tests/test_trainer.py and
tests/test_bn_apply_gpu.py state, cited per test."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import test_bn_apply_gpu as bnapply
import test_trainer as tt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from datou_gomoku_muzero_amd import trainer
    return trainer


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _count_hip_calls(T, monkeypatch):
    """Counting wrappers around the HIP conv and weight-gradient entries of the trainer -> the counter dict."""
    calls = {"conv": 0, "wgrad": 0}
    conv, wgrad = T._conv3x3_hip, T._conv3x3_wgrad_hip

    def conv_counted(*a, **k):
        calls["conv"] += 1
        return conv(*a, **k)

    def wgrad_counted(*a, **k):
        calls["wgrad"] += 1
        return wgrad(*a, **k)
    monkeypatch.setattr(T, "_conv3x3_hip", conv_counted)
    monkeypatch.setattr(T, "_conv3x3_wgrad_hip", wgrad_counted)
    return calls


# N = 1: 7 of the 8 weight-gradient chunks and most workgroups have no board.  N = 13: not a multiple of 8 or 16 (the
# XCD pairing of the forward's workgroups, workgroups past the boards).  N = 520: more boards than the forward's grid
# cap (512 at 256 CUs) and than the 80 weight-gradient chunks, so both stride loops run more than once.
@pytest.mark.parametrize("H,dtype,N", [(19, torch.float16, 1), (19, torch.float16, 13), (19, torch.bfloat16, 13),
                                       (19, torch.float16, 520), (6, torch.float16, 1), (6, torch.bfloat16, 13),
                                       (6, torch.float16, 520)])
def test_forward_input_grad_and_weight_grad(T, H, dtype, N, monkeypatch):
    """_Conv3x3NHWC (gmz_conv3x3_forward, its transposed-weight input gradient, gmz_conv3x3_wgrad) vs torch's float32
    conv2d on the same rounded operands, as test_trainer.test_hip_conv3x3_forward_and_input_grad: output and dx
    within 4e-3 (f16) / 1.6e-2 (bf16) of the reference's max magnitude, dW within twice that."""
    monkeypatch.setattr(T, "HIP_WGRAD", True)
    calls = _count_hip_calls(T, monkeypatch)
    g = torch.Generator().manual_seed(H * 1000 + N)
    x = _cl(torch.randn(N, 128, H, H, generator=g).cuda().to(dtype))
    w = (torch.randn(128, 128, 3, 3, generator=g) / 34.0).cuda()
    w_cl = _cl(w).requires_grad_(True)
    dy = _cl(torch.randn(N, 128, H, H, generator=g).cuda().to(dtype))
    xi = x.clone().requires_grad_(True)
    y = T._Conv3x3NHWC.apply(xi, w_cl)
    assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
    y.backward(dy)
    assert calls == {"conv": 2, "wgrad": 1}
    wr = w.to(dtype).float().requires_grad_(True)
    xr = x.float().requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr, wr, padding=1)
    yr.backward(dy.float())
    tol = 4e-3 if dtype == torch.float16 else 1.6e-2
    for name, a, b, t in (("y", y, yr, tol), ("dx", xi.grad, xr.grad, tol), ("dW", w_cl.grad, wr.grad, 2 * tol)):
        a, b = a.detach(), b.detach()
        sc, err = float(b.abs().max()), float((a.float() - b).abs().max())
        print("%s: max error %.3g of scale %.3g (bound %.3g)" % (name, err, sc, t * sc))
        assert err <= t * sc, (name, err, sc)


@pytest.mark.parametrize("H,dtype", [(19, torch.float16), (6, torch.bfloat16)])
def test_multi_segment_weight_gradient(T, H, dtype):
    """gmz_conv3x3_wgrad_segments over 3 segments of 5 boards, accumulating into a non-zero f32 gradient = that
    gradient + three single-use gmz_conv3x3_wgrad launches, within 1e-3 of its norm (the bound of
    test_trainer.test_deferred_multi_segment_wgrad_equals_per_use_wgrad for kernels on the same inputs)."""
    from datou_gomoku_muzero_amd import _lib
    L = _lib.load()
    g = torch.Generator().manual_seed(H)
    xs = [_cl(torch.randn(5, 128, H, H, generator=g).cuda().to(dtype)) for _ in range(3)]
    gs = [_cl(torch.randn(5, 128, H, H, generator=g).cuda().to(dtype)) for _ in range(3)]
    init = torch.randn(128, 128, 3, 3, generator=g).cuda()
    code = T._CONV_DTYPES[dtype]

    def workspace(n):
        nb = ctypes.c_size_t()
        _lib.check(L.gmz_conv3x3_wgrad_workspace_bytes(n, ctypes.byref(nb)))
        return torch.empty(nb.value // 4, dtype=torch.float32, device="cuda")
    want = init.double()
    for x, gy in zip(xs, gs):
        one, ws = torch.empty_like(init), workspace(5)
        s = one.stride()
        _lib.check(L.gmz_conv3x3_wgrad(code, H, _lib.ptr(x), _lib.ptr(gy), 5, _lib.ptr(one), s[0], s[1], s[2], s[3], 0,
                                       _lib.ptr(ws), _lib.nbytes(ws), _lib.stream_ptr()))
        want += one.double()
    got, ws = init.clone(), workspace(15)
    s = got.stride()
    xp = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in xs])
    gp = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in gs])
    _lib.check(L.gmz_conv3x3_wgrad_segments(code, H, ctypes.cast(xp, ctypes.c_void_p), ctypes.cast(gp, ctypes.c_void_p), 3,
                                            5, _lib.ptr(got), s[0], s[1], s[2], s[3], 1, _lib.ptr(ws), _lib.nbytes(ws),
                                            _lib.stream_ptr()))
    torch.cuda.synchronize()
    err, norm = float((got.double() - want).norm()), float(want.norm())
    print("segments vs single launches: %.3g of norm %.3g" % (err, norm))
    assert float((want - init.double()).norm()) > 0.5 * norm  # the launches, not the initial value, carry the norm
    assert err <= 1e-3 * norm


@pytest.mark.parametrize("H,N", [(19, 13), (6, 13)])
@pytest.mark.parametrize("per_board", [False, True])
def test_masked_statistics(T, H, N, per_board):
    """gmz_conv3x3_forward_stats / _forward_board_stats with ~30 % of the boards masked out: per-channel count, mean
    and variance from the partials (summed over the slots, resp. over the live boards' slots) vs float64 statistics
    of the kernel's own rounded output over the live boards — count exact, mean and variance within rtol 1e-4 /
    atol 1e-5 (the bound of test_trainer.test_batched_consistency_kernels_match_per_step_representations); a dead
    board's own slot carries count 0."""
    from datou_gomoku_muzero_amd import _lib
    L = _lib.load()
    g = torch.Generator().manual_seed(H * 100 + N)
    x = _cl(torch.randn(N, 128, H, H, generator=g).cuda().half())
    packed = T._packed_conv_weight((torch.randn(128, 128, 3, 3, generator=g) / 34.0).cuda(), torch.float16, 0)
    live = torch.ones(N, dtype=torch.bool)
    live[torch.randperm(N, generator=g)[:(3 * N + 5) // 10]] = False  # ~30 % of the boards dead
    mask = live.cuda().view(torch.uint8)
    y = torch.empty_like(x)
    if per_board:
        st, ns = torch.full((128 * N * 3,), float("nan"), dtype=torch.float64, device="cuda"), N
        fn = L.gmz_conv3x3_forward_board_stats
    else:
        ns = T._conv_stats_buffer(N, x.device)[1]
        st = torch.full((128 * ns * 3,), float("nan"), dtype=torch.float64, device="cuda")
        fn = L.gmz_conv3x3_forward_stats
    _lib.check(fn(1, H, _lib.ptr(x), _lib.ptr(packed), _lib.ptr(y), N, _lib.ptr(mask), _lib.ptr(st), ns,
                  _lib.stream_ptr()))
    torch.cuda.synchronize()
    part = st.view(128, ns, 3).cpu()
    if per_board:
        assert torch.equal(part[:, ~live, 2], torch.zeros(128, int((~live).sum()), dtype=torch.float64))
        part = part[:, live]
    tot = part.sum(1)
    nlive = int(live.sum()) * H * H
    assert torch.equal(tot[:, 2], torch.full((128,), float(nlive), dtype=torch.float64))
    mean, var = tot[:, 0] / nlive, tot[:, 1] / nlive - (tot[:, 0] / nlive) ** 2
    yl = y.cpu()[live].double().permute(1, 0, 2, 3).reshape(128, -1)
    rmean, rvar = yl.mean(1), yl.var(1, unbiased=False)
    print("mean: max |d| %.3g; variance: max |d| %.3g" % (float((mean - rmean).abs().max()), float((var - rvar).abs().max())))
    assert torch.allclose(mean, rmean, rtol=1e-4, atol=1e-5) and torch.allclose(var, rvar, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("H,N,dt,res,relu", [(19, 13, torch.float16, True, True), (19, 3, torch.bfloat16, False, True),
                                             (6, 24, torch.float16, True, True), (6, 5, torch.bfloat16, True, False)])
def test_bnapply_prologue_is_bit_identical(T, H, N, dt, res, relu):
    """tests/test_bn_apply_gpu.py's harness at the new sizes: the BatchNorm output, the conv output, its statistics
    partials, the running statistics and the saved statistics bit-identical to gmz_bn_forward_stats +
    gmz_conv3x3_forward_stats."""
    bnapply.test_bnapply_conv_equals_bn_then_conv(T, H, N, dt, res, relu)


@pytest.mark.parametrize("H", [19, 6])
def test_residual_block_three_ways(T, H, monkeypatch):
    """One residual block, channels-last, row mask with 4 dead rows, N = 24: fp16 autocast on the HIP convs, fp16
    autocast on MIOpen (FUSED_CONV off) and float32.  The two fp16 outputs within 3e-3 relative norm on the live rows;
    every gradient (input, conv weights, BatchNorm parameters) no further from float32 than 1.25x the MIOpen path's
    distance + 1e-3 (the rule of test_trainer.test_dynamics_stem_on_hip_matches_the_144_channel_conv).  The HIP path
    must really be the HIP kernels: the counting wrappers see its convs and weight gradients, and none in the others.

    MIOpen runs its deterministic algorithms (as in test_trainer's reference-pinned steps): with Find, the comparator's
    own distance from float32 changes from process to process — at 6x6, bn2.weight's gradient (720 live positions per
    channel) measured 0.00080 in one and 0.00152 in the next on the same inputs, against the HIP path's reproducible
    0.00244, i.e. on either side of the bound 1.25 x MIOpen + 1e-3.  With the deterministic algorithms (MI355X) the
    two fp16 paths' outputs agree to 6e-5 and their distances from float32 coincide to three digits: at 6x6 x 0.0157,
    conv1.weight 0.0124, bn1.weight 0.0115, bn1.bias 0.0195, conv2.weight 0.0081, bn2.weight 0.0024, bn2.bias 0.0039;
    at 19x19 x 0.0176, conv1.weight 0.0050, bn1.weight 0.0126, bn1.bias 0.0312, conv2.weight 0.0028, bn2.weight
    0.0018, bn2.bias 0.0015."""
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(T, "HIP_WGRAD", True)
    calls = _count_hip_calls(T, monkeypatch)
    torch.manual_seed(3)
    N = 24
    blk0 = T._Block(128).cuda().to(memory_format=torch.channels_last)
    for mod in blk0.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.1)
    x0 = _cl(torch.randn(N, 128, H, H, device="cuda").relu().half())
    mask = torch.ones(N, dtype=torch.bool, device="cuda")
    mask[5:9] = False
    outs, seen = {}, {}
    for mode in ("fp32", "miopen", "hip"):
        monkeypatch.setattr(T, "FUSED_CONV", mode == "hip")
        calls["conv"] = calls["wgrad"] = 0
        blk = copy.deepcopy(blk0).train()
        x = (x0.float() if mode == "fp32" else x0).clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=mode != "fp32"):
            y = blk(x, mask)
        (y.float() * torch.linspace(-1, 1, y.numel(), device="cuda").view_as(y)).sum().backward()
        seen[mode] = dict(calls)
        outs[mode] = [y.detach().float(), x.grad.float()] + [p.grad.float() for p in blk.parameters()]
    names = ["y", "x"] + [n for n, _ in blk0.named_parameters()]
    assert seen["hip"]["conv"] >= 4 and seen["hip"]["wgrad"] >= 2, seen  # 2 forward + 2 input-gradient convs, 2 wgrads
    assert seen["fp32"] == seen["miopen"] == {"conv": 0, "wgrad": 0}, seen
    rel = lambda a, b: float((a - b).norm() / (b.norm() + 1e-12))  # noqa: E731
    f, m, hp = outs["fp32"], outs["miopen"], outs["hip"]
    print("y: HIP vs MIOpen fp16, live rows: %.3g" % rel(hp[0][mask], m[0][mask]))
    assert rel(hp[0][mask], m[0][mask]) < 3e-3
    for k in range(1, len(names)):
        em, eh = rel(m[k], f[k]), rel(hp[k], f[k])
        print("grad %-14s vs float32: HIP %.3g, MIOpen %.3g" % (names[k], eh, em))
        assert eh <= 1.25 * em + 1e-3, (names[k], eh, em)


@pytest.mark.parametrize("fixture", ["train_loss_c19full.npz", "train_loss_c6w128full.npz"])
def test_production_step_matches_reference(T, fixture, monkeypatch):
    """test_trainer.test_production_training_step_matches_reference_at_128_filters on the reference's float32
    calculate_loss at 19x19 and 6x6 (128 filters, 2 blocks, 16 games live for all 5 steps; fixtures of
    tests/golden/make_golden_trainer_sizes.py), its bounds unchanged: both shapes get the per-tensor
    max(0.10, 1.5 x reference-AMP error) bound.  It prints every tensor's error.  The residual convs must be the HIP
    ones."""
    calls = _count_hip_calls(T, monkeypatch)
    tt.test_production_training_step_matches_reference_at_128_filters(T, fixture)
    assert calls["conv"] > 0 and calls["wgrad"] > 0, calls


def test_trainer_end_to_end_at_19(T, monkeypatch):
    """Trainer at 19x19 (2 blocks, batch 8) in its default graph mode through warm-up, capture and replays, on a
    seeded synthetic batch, against an eager trainer on the same batches: losses finite and equal within 2e-3
    relative (the fp16-autocast bound of test_trainer.test_graph_replayed_step_matches_eager_step); the eager run goes
    through the HIP convs."""
    from datou_gomoku_muzero_amd import weights as W
    cfg = T.TrainConfig(BOARD_SIZE=19, NUM_RES_BLOCKS=2, PHYSICAL_BATCH_SIZE=8, LEARNING_RATE=1e-3)
    batches = []
    for i in range(2):
        obs, act, rew, pol, val = W.synthetic_slices(8, 19, cfg.NUM_UNROLL_STEPS, np.random.RandomState(5 + i))
        bt = [torch.as_tensor(v).cuda() for v in (obs, act, rew, pol, val)]
        bt[0] = bt[0].float()
        batches.append(bt)
    w = torch.rand(8, generator=torch.Generator().manual_seed(1)).cuda() + 0.5
    calls = _count_hip_calls(T, monkeypatch)
    runs = []
    for graph in (False, None):
        torch.manual_seed(0)
        tr = T.Trainer(cfg, device="cuda", **({} if graph is None else {"graph": graph}))
        logs = np.array([tr.step(batches[i % 2], w, k=i % 4, flip=bool(i % 2))[0] for i in range(7)])
        assert (tr._graphs is not None) == (graph is None)
        if graph is False:
            assert calls["conv"] > 0, calls
        runs.append(logs)
    eager, graphed = runs
    print("eager", eager[:, 0], "graph", graphed[:, 0])
    assert np.isfinite(eager).all() and np.isfinite(graphed).all()
    assert np.allclose(eager, graphed, rtol=2e-3, atol=1e-6), (eager, graphed)
