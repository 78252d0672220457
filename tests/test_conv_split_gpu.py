"""The split-f16 3x3 convolution on the GPU (gmz_conv3x3_forward_split: float32 in and out, each operand as two f16
halves, three of the four partial products on the f16 MFMA pipe) and the trainer's path through it
(TrainNet.initial_value(split=True), trainer.TARGET_SPLIT).  The truth in every case is a float64 CPU convolution or
forward of the same inputs; the yardstick for "float32-grade" is the error of torch's float32 CPU computation of the
same thing."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from test_conv_split import bits22

pytestmark = pytest.mark.gpu

SIZES = [6, 9, 15, 19]
PACK_INT16 = 294912  # 2 x 294,912 bytes


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from datou_gomoku_muzero_amd import trainer
    return trainer


def _pack(w, transpose=0):
    from datou_gomoku_muzero_amd import _lib
    out = torch.empty(PACK_INT16, dtype=torch.int16, device="cuda")
    s = w.stride()
    _lib.check(_lib.load().gmz_conv3x3_pack_split(_lib.ptr(w), s[0], s[1], s[2], s[3], int(transpose), _lib.ptr(out),
                                                  _lib.stream_ptr()))
    return out


def _conv(x, packed, bn=None, res=None, relu=0):
    """gmz_conv3x3_forward_split of the float32 channels-last x [N, 128, H, H] -> y like x.  bn = (gamma, beta, mean,
    var, eps)."""
    from datou_gomoku_muzero_amd import _lib
    assert x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    y = torch.full_like(x, float("nan"), memory_format=torch.channels_last)
    g, b, m, v, eps = bn if bn is not None else (None, None, None, None, 0.0)
    _lib.check(_lib.load().gmz_conv3x3_forward_split(x.shape[2], _lib.ptr(x), _lib.ptr(packed), _lib.ptr(y), x.shape[0],
                                                     _lib.ptr(g), _lib.ptr(b), _lib.ptr(m), _lib.ptr(v), float(eps),
                                                     _lib.ptr(res), int(relu), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return y


def _nhwc(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _w_eff(w, transpose):
    """the weight the kernel convolves with: W, or W'[c][o][t] = W[o][c][8 - t]"""
    return w.transpose(0, 1).flip(2, 3).contiguous() if transpose else w


def _errors(y, y64):
    """(relative rms error, max abs error) of y against the float64 truth"""
    e = y.double() - y64
    return float(e.norm() / y64.norm()), float(e.abs().max())


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("H", SIZES)
def test_exact_geometry(T, H, transpose):
    """One cell per board holding 1.0 (corner / centre / last cell; channels 0 / 77 / 127) and 22-bit weights: the
    output is the weight taps stamped around the cell and zero elsewhere, every product and sum exact, so it must
    equal the float64 result BITWISE — any wrong tap, channel chunk, transpose, hi/lo fragment offset or 2^-11
    factor is a wrong bit."""
    w = torch.from_numpy(bits22(np.random.RandomState(10 + H), (128, 128, 3, 3)))
    x = torch.zeros(3, 128, H, H)
    x[0, 0, 0, 0] = 1.0
    x[1, 77, H // 2, H // 2] = 1.0
    x[2, 127, H - 1, H - 1] = 1.0
    y64 = F.conv2d(x.double(), _w_eff(w, transpose).double(), padding=1)
    want = y64.float()
    assert torch.equal(want.double(), y64)  # the truth is float32-representable
    assert int((want != 0).sum()) == 128 * (4 + 9 + 4)
    y = _conv(_nhwc(x), _pack(w.cuda(), transpose)).cpu().contiguous()
    assert torch.equal(y.view(torch.int32), want.contiguous().view(torch.int32))


def _accuracy_case(H, N, seed):
    g = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(128, generator=g) * 4.0 - 3.0)
    x = torch.relu(torch.randn(N, 128, H, H, generator=g)) * scale[None, :, None, None]
    w = torch.randn(128, 128, 3, 3, generator=g) / 34.0
    return x, w


@pytest.mark.parametrize("H", SIZES)
def test_accuracy_is_float32_grade(T, H):
    """x = relu(randn) x a per-channel scale 10^U(-3, 1) (half the values zero, magnitudes over four decades), w =
    randn / 34: rel-rms error <= 2 x and max-abs error <= 4 x those of torch's float32 CPU convolution of the same
    inputs (the margins cover another accumulation order; the CPU emulation of the arithmetic gives 1.0-1.1 and
    <= 1.25; a missing cross term lands 1000x above)."""
    torch.set_num_threads(4)
    x, w = _accuracy_case(H, 5, 100 + H)
    y64 = F.conv2d(x.double(), w.double(), padding=1)
    r32, m32 = _errors(F.conv2d(x, w, padding=1), y64)
    y = _conv(_nhwc(x), _pack(w.cuda())).cpu()
    r, m = _errors(y, y64)
    print("H=%d split conv: rel-rms %.3g (f32 CPU %.3g, ratio %.2f), max-abs %.3g (f32 CPU %.3g, ratio %.2f)"
          % (H, r, r32, r / r32, m, m32, m / m32))
    assert r <= 2 * r32 and m <= 4 * m32


def test_board_stride_past_the_grid_cap(T):
    """6x6 with 3 boards more than the capped grid takes one each (gmz_conv3x3_stats_slots' cap = the board stride:
    512 boards on 256 CUs), so workgroups stride over boards: boards 0, bstride and N - 1 each bitwise equal to the
    same board launched alone."""
    from datou_gomoku_muzero_amd import _lib
    L = _lib.load()

    def slots(n):
        s = ctypes.c_int()
        _lib.check(L.gmz_conv3x3_stats_slots(n, ctypes.byref(s)))
        return s.value

    bstride = slots(1 << 20)  # the cap: one workgroup pair per slot, each starting at its own board
    assert slots(bstride) == bstride and slots(bstride - 16) < bstride  # bstride boards is the first capped launch
    N = bstride + 3
    g = torch.Generator().manual_seed(7)
    x = _nhwc(torch.randn(N, 128, 6, 6, generator=g))
    pk = _pack((torch.randn(128, 128, 3, 3, generator=g) / 34.0).cuda())
    y = _conv(x, pk)
    assert torch.isfinite(y).all()
    for b in (0, bstride, N - 1):
        alone = _conv(x[b:b + 1].contiguous(memory_format=torch.channels_last), pk)
        assert torch.equal(y[b:b + 1].view(torch.int32), alone.view(torch.int32)), b


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("H", [9, 19])
def test_fused_batchnorm_epilogue(T, H, with_res, relu):
    """The fused eval-BatchNorm (+ residual, ReLU) epilogue: the accuracy bounds against float64, with the float32 CPU
    computation of the same composition as the yardstick, and the same bounds with the unfused composition — the
    plain split conv followed by gmz_bn_eval in float32 — as the comparator."""
    torch.set_num_threads(4)
    x, w = _accuracy_case(H, 3, 200 + H)
    g = torch.Generator().manual_seed(300 + H)
    gamma, beta = torch.randn(128, generator=g), torch.randn(128, generator=g)
    mean = torch.rand(128, generator=g) - 0.5
    var = 0.5 + 1.5 * torch.rand(128, generator=g)
    res = torch.randn(3, 128, H, H, generator=g) if with_res else None
    eps = 1e-4

    def compose(x, w, dt):
        z = F.conv2d(x.to(dt), w.to(dt), padding=1)
        inv = 1.0 / torch.sqrt(var.to(dt) + eps)
        z = (z - mean.to(dt)[None, :, None, None]) * (gamma.to(dt) * inv)[None, :, None, None] + beta.to(dt)[None, :, None, None]
        if res is not None:
            z = z + res.to(dt)
        return torch.relu(z) if relu else z

    y64 = compose(x, w, torch.float64)
    r32, m32 = _errors(compose(x, w, torch.float32), y64)
    xs, pk = _nhwc(x), _pack(w.cuda())
    bn = tuple(t.cuda() for t in (gamma, beta, mean, var)) + (eps,)
    rs = _nhwc(res) if with_res else None
    r, m = _errors(_conv(xs, pk, bn, rs, relu).cpu(), y64)
    mod = torch.nn.BatchNorm2d(128, eps=eps).cuda().eval()
    with torch.no_grad():
        for dst, src in ((mod.weight, gamma), (mod.bias, beta), (mod.running_mean, mean), (mod.running_var, var)):
            dst.copy_(src)
        unfused = T._bn_eval(mod, _conv(xs, pk), rs, bool(relu))
    torch.cuda.synchronize()
    ru, mu = _errors(unfused.cpu(), y64)
    print("H=%d res=%s relu=%d fused: rel-rms %.3g max-abs %.3g; f32 CPU %.3g %.3g; unfused %.3g %.3g"
          % (H, with_res, relu, r, m, r32, m32, ru, mu))
    assert r <= 2 * r32 and m <= 4 * m32
    assert r <= 2 * ru and m <= 4 * mu


def _value64(target, obs):
    """the value head's scalar of a float64 CPU copy of ``target`` (eval mode)"""
    t = copy.deepcopy(target).cpu().double().eval()
    t.channels_last = False
    c = t.cfg
    with torch.no_grad():
        _, vl = t.prediction(t.representation(obs.cpu().double()))
        grid = torch.linspace(c.VALUE_SUPPORT_MIN, c.VALUE_SUPPORT_MAX, c.VALUE_SUPPORT_BINS, dtype=torch.float64)
        return (torch.softmax(vl, dim=1) * grid).sum(1)


def _value_bound(target_cpu, obs, v64):
    """bound E: 1e-4 (VERDICT's), and 4 x the float32 CPU forward's own error on the same inputs"""
    e32 = float((target_cpu.initial_value(obs)[:, 0].double() - v64).abs().max())
    return min(1e-4, 4 * e32), e32


@pytest.mark.parametrize("fixture", ["train_loss_c128full.npz", "train_loss_c6w128full.npz", "train_loss_c15full.npz"])
def test_value_with_split_trunk_is_float32_grade(T, fixture, monkeypatch):
    """initial_value(obs, split=True) on a fixture's target weights and final observations: max |dv| against the float64
    CPU forward <= 1e-4 and <= 4 x the float32 CPU forward's own error; the f16 trunk's error printed beside it."""
    import test_trainer as tt
    torch.set_num_threads(4)
    d = np.load(os.path.join(GOLDEN, fixture))
    cfg, _, target = tt._nets(T, *tt._shape(d))
    obs = torch.from_numpy(d["obs"])[:, -1]
    v64 = _value64(target, obs)
    bound, e32 = _value_bound(target, obs, v64)
    tg = copy.deepcopy(target).cuda().to(memory_format=torch.channels_last)
    tg.channels_last = True
    calls = []
    real = T._conv3x3_split_hip
    monkeypatch.setattr(T, "_conv3x3_split_hip", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    vs = tg.initial_value(obs.cuda(), split=True)[:, 0].double().cpu()
    assert len(calls) == 2 * cfg.NUM_RES_BLOCKS  # the split kernel ran: one launch per residual conv
    v16 = tg.initial_value(obs.cuda(), f16=True)[:, 0].double().cpu()
    es, e16 = float((vs - v64).abs().max()), float((v16 - v64).abs().max())
    print("%s: max|dv| vs float64: split %.3g, float32 CPU %.3g, f16 trunk %.3g (bound %.3g)" % (fixture, es, e32, e16, bound))
    assert es <= bound


def test_production_step_with_target_split_matches_reference(T, monkeypatch):
    """trainer.TARGET_SPLIT: the production step on train_loss_c128full.npz (fp16 autocast model, channels-last, the
    target's value through the split trunk) meets the reference's loss, components and td errors as the f16-trunk
    step does (test_trainer.test_target_value_f16_trunk_matches_float32)."""
    import test_trainer as tt
    d = np.load(os.path.join(GOLDEN, "train_loss_c128full.npz"))
    p = "c0/"
    monkeypatch.setattr(T, "TARGET_SPLIT", True)
    calls = []
    real = T._conv3x3_split_hip
    monkeypatch.setattr(T, "_conv3x3_split_hip", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    cfg, model, target = tt._nets(T, *tt._shape(d))
    model, target = (m.cuda().to(memory_format=torch.channels_last) for m in (model, target))
    model.channels_last = target.channels_last = True
    batch = [torch.from_numpy(d[k]).cuda() for k in ("obs", "act", "rew", "pol", "val")]
    loss, logs, td = T.muzero_loss(model, target, batch, torch.from_numpy(d["isw"]).cuda(), cfg, k=int(d[p + "k"]),
                                   flip=bool(d[p + "flip"]), amp=True)
    torch.cuda.synchronize()
    assert len(calls) == 2 * cfg.NUM_RES_BLOCKS
    monkeypatch.setattr(T, "TARGET_SPLIT", False)
    logs_amp, td_amp, _ = tt._gpu_grads(T, d, p, "native")
    print("loss: split target %.6g, reference AMP path %.6g, reference f32 %.6g" % (logs[0], logs_amp[0], float(d[p + "loss"])))
    tt._assert_logs_near_reference(logs, td.float().cpu().numpy(), d, p, logs_amp, td_amp)


def test_graph_replays_keep_the_split_packs_current(T, monkeypatch):
    """Trainer(graph=True, graph_warmup=1) at 9x9 / 2 blocks / B = 8 with TARGET_SPLIT: one eager and three replayed
    steps give the losses of a graph=False trainer from the same seed (compared as
    test_trainer.test_graph_replayed_step_matches_eager_step compares the two modes under autocast: 2e-3), which a
    replay on stale split packs would not; and the target's split value on its CURRENT weights afterwards meets the
    value bound against a float64 forward of those weights."""
    from datou_gomoku_muzero_amd import weights as W
    torch.set_num_threads(4)
    monkeypatch.setattr(T, "TARGET_SPLIT", True)
    cfg = T.TrainConfig(BOARD_SIZE=9, NUM_RES_BLOCKS=2, PHYSICAL_BATCH_SIZE=8, LEARNING_RATE=1e-3)
    arrs = W.synthetic_slices(8, 9, cfg.NUM_UNROLL_STEPS, np.random.RandomState(11))
    batch = [torch.as_tensor(a).cuda() for a in arrs]
    batch[0] = batch[0].float()
    w = torch.ones(8, device="cuda")
    runs = []
    for graph in (False, True):
        torch.manual_seed(0)
        tr = T.Trainer(cfg, device="cuda", graph=graph, graph_warmup=1)
        assert tr.target.channels_last
        logs = [tr.step(batch, w, k=i % 4, flip=bool(i % 2))[0] for i in range(4)]
        torch.cuda.synchronize()
        assert (tr._graphs is not None) == graph
        runs.append(np.array(logs))
    assert any(isinstance(k, tuple) and k and k[0] == "split" for k in tr._pack_tables), "no batched split re-pack"
    assert np.allclose(runs[0], runs[1], rtol=2e-3, atol=1e-6), runs
    obs = batch[0][:, -1]
    tcpu = copy.deepcopy(tr.target).cpu().to(memory_format=torch.contiguous_format)
    tcpu.channels_last = False
    v64 = _value64(tcpu, obs.cpu())
    bound, e32 = _value_bound(tcpu, obs.cpu(), v64)
    vs = tr.target.initial_value(obs, split=True)[:, 0].double().cpu()
    es = float((vs - v64).abs().max())
    print("after 1 eager + 3 replayed steps: max|dv| vs float64 %.3g (float32 CPU %.3g, bound %.3g)" % (es, e32, bound))
    assert es <= bound
