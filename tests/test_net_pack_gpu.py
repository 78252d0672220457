"""The device weight push (gmz_net_pack, GomokuNetHip.load_device_state_dict, C4Loop(device_weights=True)) on the GPU.
The yardstick throughout is the host path: network.pack_weights on a CPU copy of the same tensors, compared on the raw
bytes of all 19 packed arrays."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _cfg(board, blocks, sims=8):
    from datou_gomoku_muzero_amd.config import GmzConfig
    return GmzConfig(BOARD_SIZE=board, NUM_RES_BLOCKS=blocks, NUM_SIMULATIONS=sims)


@functools.lru_cache(maxsize=None)
def _planted_state_dict(board, blocks):
    """A random reference-shaped state dict (float32 numpy): running_var log-uniform in 1e-6..1e3, and in every family
    of 16-bit outputs (a tower conv of each net, the dynamics conv, the stem, reward_fc.0) entries whose folded value
    is above the fp16 clamp (both signs), in the f16 subnormal range, and exactly +0 and -0."""
    from datou_gomoku_muzero_amd import network as N, weights as W
    cfg = _cfg(board, blocks)
    rs = np.random.RandomState(1000 * board + blocks)
    sd = W.synthetic_state_dict(cfg, seed=board * 7 + blocks, with_projection=False)
    for k in sd:
        if k.endswith("running_var"):
            sd[k] = (10.0 ** rs.uniform(-6, 3, sd[k].shape)).astype(np.float32)
    convs = [("representation_net.conv", "representation_net.bn"), ("dynamics_net.conv", "dynamics_net.bn"),
             ("representation_net.resblocks.0.conv2", "representation_net.resblocks.0.bn2"),
             ("dynamics_net.resblocks.%d.conv1" % (blocks - 1), "dynamics_net.resblocks.%d.bn1" % (blocks - 1))]
    for conv, bn in convs:
        w = sd[conv + ".weight"]
        s, _ = N.fold_bn(sd, bn)
        flat = w.reshape(w.shape[0], -1)
        cols = rs.permutation(min(flat.shape[1], 128 * 9))[:6]  # (the dynamics conv: inside its 128 hidden channels)
        if w.shape[1] > 128:
            cols = np.array([np.ravel_multi_index((c // 9, c % 9 // 3, c % 3), w.shape[1:]) for c in cols])
        for o in rs.permutation(w.shape[0])[:5]:
            for col, folded in zip(cols, (1e5, -3e6, 1e-6, -3.1e-7, 0.0, -0.0)):
                flat[o, col] = np.float32(folded) / s[o] if folded else np.float32(folded)
    r = sd["dynamics_net.reward_fc.0.weight"]
    r[3, :6] = [1e5, -3e6, 1e-6, -3.1e-7, 0.0, -0.0]
    r[60, -6:] = [-0.0, 0.0, 7e4, -65520.0, 5.9e-8, -2.9e-8]
    return sd


@functools.lru_cache(maxsize=None)
def _reference(board, blocks, precision, channels_last=False):
    """pack_weights on the CPU copy of the sources, strides included (numpy's einsum sums dyn_action in another order
    when the channels are contiguous, tests/test_net_pack.py)."""
    from datou_gomoku_muzero_amd import network as N
    cpu = _device_sources(_planted_state_dict(board, blocks), channels_last, device="cpu")
    want = N.pack_weights(cpu, _cfg(board, blocks), precision)
    assert len(want) == 19
    return want


def _device_sources(sd, channels_last, device="cuda"):
    out = {}
    for k, v in sd.items():
        t = torch.from_numpy(np.array(v)).to(device)
        if channels_last and t.dim() == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        out[k] = t
    return out


def _raw(x):
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.ascontiguousarray(x)
    return a.reshape(-1).view(np.uint8)


def _assert_packed(net, want):
    torch.cuda.synchronize()
    assert sorted(net._tensors) == sorted(want)
    for k, v in want.items():
        got = net._tensors[k]
        assert tuple(got.shape) == v.shape and got.element_size() == v.itemsize, k
        a, b = _raw(got), _raw(v)
        assert np.array_equal(a, b), "%s: %d of %d bytes differ, first at %d" % (
            k, int((a != b).sum()), a.size, int(np.flatnonzero(a != b)[0]))


def _poison(net):
    """0xFF in every byte of the packed tensors: what the pack does not write shows."""
    for t in net._tensors.values():
        t.view(torch.uint8).fill_(0xFF)


def _other_net(board, blocks, precision, **kw):
    """A network on OTHER weights (what a push must replace)."""
    from datou_gomoku_muzero_amd import network as N, weights as W
    cfg = _cfg(board, blocks)
    return N.GomokuNetHip(W.synthetic_state_dict(cfg, seed=99, with_projection=False), cfg, precision=precision, **kw)


def _pointers(net):
    from test_net_pack import FIELDS
    return {k: t.data_ptr() for k, t in net._tensors.items()}, [getattr(net.w, f) for f in FIELDS]


# ---------------------------------------------------------------------------------------------------- 1. bitwise pack
def test_the_planted_values_reach_the_edge_cases():
    """The fixture does what it says: the host reference itself holds clamped, subnormal and signed-zero entries."""
    want = _reference(6, 2, "fp16")
    for k in ("repr_stem_w", "repr_convs", "dyn_convs", "reward_fc1_w"):
        bits = want[k].reshape(-1)
        mag = bits & 0x7fff
        assert (bits == 0x7bff).any() and (bits == 0xfbff).any(), k          # +-65504: clamped, not inf
        assert ((mag > 0) & (mag < 0x400)).any(), k                          # f16 subnormals
        assert (bits == 0x8000).any() and (bits == 0).any(), k               # -0 and +0
        assert not (mag == 0x7c00).any(), k
    assert (_reference(6, 2, "bf16")["dyn_convs"].reshape(-1) & 0x7fff).max() > 0x4780  # bf16: above 65504, no clamp
    var = _planted_state_dict(6, 2)["dynamics_net.bn.running_var"]
    assert var.min() < 1e-4 and var.max() > 10


@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("board", [5, 6, 15, 19])
def test_device_pack_equals_pack_weights_bitwise(board, blocks, precision, layout):
    from datou_gomoku_muzero_amd.network import r16
    A = board * board
    assert (r16(A), r16(2 * A)) == {5: (32, 64), 6: (48, 80), 15: (240, 464), 19: (368, 736)}[board]
    sd = _planted_state_dict(board, blocks)
    src = _device_sources(sd, layout == "channels_last")
    if layout == "channels_last":
        w = src["representation_net.resblocks.0.conv1.weight"]
        assert w.stride() == (9 * 128, 1, 3 * 128, 128)
    before = {k: v.clone() for k, v in src.items()}
    net = _other_net(board, blocks, precision)
    _poison(net)
    net.load_device_state_dict(src)
    _assert_packed(net, _reference(board, blocks, precision, layout == "channels_last"))
    for k, v in src.items():
        assert v.stride() == before[k].stride() and np.array_equal(_raw(v), _raw(before[k])), k


# ---------------------------------------------------------------------------------------------------- 2. in place
def test_push_is_in_place_and_split_halves_follow_it():
    from datou_gomoku_muzero_amd import network as N, weights as W
    board, blocks = 6, 2
    # (weights of ordinary magnitudes: the planted extremes would drive the activations to inf and NaN)
    sd = W.synthetic_state_dict(_cfg(board, blocks), seed=5, with_projection=False)
    net = _other_net(board, blocks, "fp16", num_slots=32, max_rows=8)
    halves = net.split(2)
    ptrs = [_pointers(q) for q in [net] + halves]
    net.load_device_state_dict(_device_sources(sd, True))
    assert [_pointers(q) for q in [net] + halves] == ptrs
    assert all(q._tensors is net._tensors for q in halves)
    cpu = _device_sources(sd, True, device="cpu")  # the same tensors, strides included, on the host
    _assert_packed(net, N.pack_weights(cpu, _cfg(board, blocks), "fp16"))
    fresh = N.GomokuNetHip(cpu, _cfg(board, blocks), num_slots=16, max_rows=8)
    rs = np.random.RandomState(4)
    obs = (rs.rand(8, 3, board, board) < 0.3).astype(np.float32)
    actions = rs.randint(0, board * board, 8)

    def run(q):
        lg, v, _ = q.initial_inference(obs)
        lg2, v2, _ = q.recurrent_inference(np.arange(8), actions, np.arange(8, 16))
        torch.cuda.synchronize()
        return lg, v, lg2, v2

    want = run(fresh)
    for q in halves:
        for got, w in zip(run(q), want):
            assert torch.equal(got, w)


# ---------------------------------------------------------------------------------------------------- 3. capturable
def test_push_replays_from_a_captured_graph():
    from datou_gomoku_muzero_amd import network as N
    board, blocks = 6, 2
    cfg = _cfg(board, blocks)
    src = _device_sources(_planted_state_dict(board, blocks), True)
    net = _other_net(board, blocks, "fp16")
    net.load_device_state_dict(src)  # eager: builds and uploads the job table
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one stream, three kernel nodes in a line
        net.load_device_state_dict(src)
    _assert_packed(net, _reference(board, blocks, "fp16", True))
    for k, t in src.items():  # new values in the same memory (variances stay positive)
        if t.dtype == torch.float32:
            t.mul_(1.25).add_(0.001 if k.endswith("running_var") else 0.0)
    _poison(net)
    g.replay()
    _assert_packed(net, N.pack_weights({k: v.cpu() for k, v in src.items()}, cfg, "fp16"))


# ---------------------------------------------------------------------------------------------------- 4. trainer
def _initial_weights(tcfg, seed):
    from datou_gomoku_muzero_amd import trainer as T
    torch.manual_seed(seed)
    return {k: v.detach().cpu().numpy() for k, v in T.TrainNet(tcfg).state_dict().items()}


def test_trainer_parameters_pack_where_they_live():
    from datou_gomoku_muzero_amd import network as N, replay as RP, trainer as T, weights as W
    tcfg = T.TrainConfig(BOARD_SIZE=6, NUM_RES_BLOCKS=2, PHYSICAL_BATCH_SIZE=8, TRAIN_BUFFER_SIZE=64, ENABLE_PER=True)
    tr = T.Trainer(tcfg, device="cuda", graph=False)
    rb = RP.ReplayBuffer(tcfg, device="cuda")
    rs = np.random.RandomState(2)
    rb.add_arrays(*W.synthetic_slices(32, 6, tcfg.NUM_UNROLL_STEPS, rs))
    for _ in range(2):
        batch, idx, w = rb.sample(8, rs)
        tr.step(batch, w)
    dsd = tr.device_state_dict()
    live = dict(tr.model.state_dict())
    assert all(v.data_ptr() == live[k].data_ptr() for k, v in dsd.items())  # no copy
    conv = dsd["dynamics_net.resblocks.0.conv1.weight"]
    assert conv.is_cuda and not conv.is_contiguous()  # the GPU trainer is channels-last
    cfg = _cfg(6, 2)
    net = _other_net(6, 2, "fp16")
    _poison(net)
    net.load_device_state_dict(dsd)
    _assert_packed(net, N.pack_weights(tr.state_dict_cpu(), cfg, "fp16"))


# ---------------------------------------------------------------------------------------------------- 5, 6. the loop
def _run_loop(device_weights, concurrent, monkeypatch=None):
    from datou_gomoku_muzero_amd import loop as LP, replay as RP, trainer as T, weights as W
    cfg = _cfg(6, 2, sims=8)
    tcfg = T.TrainConfig(BOARD_SIZE=6, NUM_RES_BLOCKS=2, PHYSICAL_BATCH_SIZE=16, TRAIN_BUFFER_SIZE=1024, ENABLE_PER=True)
    sd = _initial_weights(tcfg, 3)
    torch.manual_seed(0)
    np.random.seed(5)
    tr = T.Trainer(tcfg, device="cuda", state_dict=sd, graph=False)
    sp = LP.SelfPlay(cfg, 16, tr.state_dict_cpu(), seed=3)
    rb = RP.ReplayBuffer(tcfg, device="cuda")
    rb.add_arrays(*W.synthetic_slices(48, 6, tcfg.NUM_UNROLL_STEPS, np.random.RandomState(11)))  # training starts at once
    if device_weights and monkeypatch is not None:
        def no_host_copy():
            raise AssertionError("the device push went through Trainer.state_dict_cpu")
        monkeypatch.setattr(tr, "state_dict_cpu", no_host_copy)
    lp = LP.C4Loop(sp, tr, rb, tcfg, 16, moves_per_iter=3, train_steps_per_iter=1, model_update_interval=1, seed=7,
                   concurrent=concurrent, device_weights=device_weights)
    assert lp.device_weights is device_weights and lp.concurrent is concurrent
    st = lp.run(6)
    torch.cuda.synchronize()
    assert st["train_steps"] == 6 and st["weight_pushes"] == 6
    for eng in getattr(sp.eng, "engines", [sp.eng]):
        assert eng.errors() == 0
    return lp, sp, tr, rb, st


def test_sliced_loop_with_device_weights_equals_the_host_push(monkeypatch):
    from test_replay_ingest_gpu import _assert_rings_equal
    from datou_gomoku_muzero_amd import network as N
    lp0, sp0, tr0, rb0, st0 = _run_loop(False, False)
    lp1, sp1, tr1, rb1, st1 = _run_loop(True, False, monkeypatch)
    assert st0 == st1
    _assert_rings_equal(rb0, rb1)
    for (k, a), b in zip(tr0.model.state_dict().items(), tr1.model.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(lp0.last_logs, lp1.last_logs)
    for k, t in sp0.net._tensors.items():
        assert np.array_equal(_raw(t), _raw(sp1.net._tensors[k])), k
    _assert_packed(sp1.net, N.pack_weights({k: v.cpu() for k, v in tr1.device_state_dict().items()}, _cfg(6, 2), "fp16"))
    sp0.close()
    sp1.close()


def test_concurrent_loop_with_device_weights_ends_on_the_trainers_weights():
    from datou_gomoku_muzero_amd import network as N
    lp, sp, tr, rb, st = _run_loop(True, True)
    assert lp.train_stream is not None
    assert torch.isfinite(lp.last_logs).all()
    _assert_packed(sp.net, N.pack_weights(tr.state_dict_cpu(), _cfg(6, 2), "fp16"))
    sp.close()


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_load_device_state_dict_refuses_what_it_cannot_pack():
    board, blocks = 5, 1
    net = _other_net(board, blocks, "fp16")
    good = _device_sources(_planted_state_dict(board, blocks), False)
    key = "dynamics_net.resblocks.0.conv1.weight"

    def refused(match, **change):
        sd = dict(good)
        for k, v in change.items():
            sd[k.replace("__", ".")] = v
        with pytest.raises(ValueError, match=match):
            net.load_device_state_dict(sd)

    refused("CUDA tensor", **{key: good[key].cpu()})
    refused("CUDA tensor", **{key: good[key].cpu().numpy()})
    refused("float32", **{key: good[key].half()})
    refused("float32", **{"prediction_net.value_bn.running_var": good["prediction_net.value_bn.running_var"].double()})
    refused("shape", **{key: good[key][:, :64]})
    refused("shape", **{"prediction_net.policy_fc.bias": good["prediction_net.policy_fc.bias"][:-1]})
    missing = dict(good)
    del missing["dynamics_net.action_embed_conv.weight"]
    with pytest.raises(ValueError, match="missing key 'dynamics_net.action_embed_conv.weight'"):
        net.load_device_state_dict(missing)
    if torch.cuda.device_count() > 1:
        refused("is on cuda:1", **{key: good[key].to("cuda:1")})
    # ignored: num_batches_tracked (an int64) and keys pack_weights does not read
    extra = dict(good, **{"projection_net.fc1.bias": torch.zeros(3), "x.num_batches_tracked": torch.tensor(7)})
    net.load_device_state_dict(extra)
    _assert_packed(net, _reference(board, blocks, "fp16"))


def test_loop_refuses_device_weights_off_the_gpu_and_across_ranks():
    from test_loop import _ScriptedSelfPlay
    from datou_gomoku_muzero_amd import loop as LP, replay as RP, trainer as T

    class _World2:
        def get_rank(self):
            return 0

        def get_world_size(self):
            return 2

    tcfg = T.TrainConfig(BOARD_SIZE=6, NUM_RES_BLOCKS=1, PHYSICAL_BATCH_SIZE=8, TRAIN_BUFFER_SIZE=64)
    rb = RP.ReplayBuffer(tcfg, device="cuda")
    with pytest.raises(ValueError, match="on a GPU"):
        LP.C4Loop(_ScriptedSelfPlay(1), None, rb, tcfg, 8, device="cpu", device_weights=True)
    with pytest.raises(ValueError, match="multi-rank"):
        LP.C4Loop(_ScriptedSelfPlay(1), None, rb, tcfg, 8, dist=_World2(), device_weights=True)
    with pytest.raises(ValueError, match="load_device_weights"):  # a self-play source without the device entry
        LP.C4Loop(_ScriptedSelfPlay(1), T.Trainer(tcfg, device="cuda", graph=False), rb, tcfg, 8, device_weights=True)
