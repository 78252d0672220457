"""gmz_net_pack at the C boundary (no GPU: fake pointers, every call must stop at a check before any launch) and the
numpy behaviour its kernels restate.  tests/test_net_pack_gpu.py holds the kernels themselves to network.pack_weights."""
import ctypes

import numpy as np
import pytest
import torch

from test_abi_messages import ODD, got_past_validation, p

FIELDS = ("repr_stem_w", "repr_stem_b", "repr_convs", "repr_bias", "dyn_convs", "dyn_bias", "dyn_action", "head_conv_w",
          "head_conv_b", "policy_fc_w", "policy_fc_b", "value_fc1_w", "value_fc1_b", "value_fc2_w", "value_fc2_b",
          "reward_fc1_w", "reward_fc1_b", "reward_fc2_w", "reward_fc2_b")

no_gpu = pytest.mark.skipif(torch.cuda.is_available(),
                            reason="fake pointers: for machines without a GPU, where no case can launch")


def _lib():
    import datou_gomoku_muzero_amd._lib as L
    import datou_gomoku_muzero_amd.network  # noqa: F401  (registers the gmz_net_* signatures)
    return L.load()


def _job_bytes(lib, blocks):
    out = ctypes.c_size_t()
    assert lib.gmz_net_pack_job_bytes(blocks, ctypes.byref(out)) == 0
    return out.value


def _weights(blocks=2, **wrong):
    from datou_gomoku_muzero_amd.network import NetWeights
    w = NetWeights(15, 128, blocks, 64)
    for i, f in enumerate(FIELDS):
        setattr(w, f, p(i + 1))
    w.dtype = 0
    for k, v in wrong.items():
        setattr(w, k, v)
    return w


def test_job_table_size_grows_with_blocks():
    lib = _lib()
    sizes = [_job_bytes(lib, b) for b in (1, 2, 8, 16)]
    assert sizes == sorted(set(sizes)) and sizes[0] > 0
    # one 40-byte entry per source tensor: 33 + 20 per block (include/gmz.h), the sources network.py lists
    from datou_gomoku_muzero_amd.config import GmzConfig
    from datou_gomoku_muzero_amd.network import device_pack_sources
    for b, s in zip((1, 2, 8, 16), sizes):
        assert s == 40 * (33 + 20 * b) == 40 * len(device_pack_sources(GmzConfig(BOARD_SIZE=15, NUM_RES_BLOCKS=b)))
    out = ctypes.c_size_t()
    assert lib.gmz_net_pack_job_bytes(0, ctypes.byref(out)) != 0 and "blocks" in lib.gmz_last_error().decode()
    assert lib.gmz_net_pack_job_bytes(2, None) != 0 and "null" in lib.gmz_last_error().decode()


REFUSALS = [
    ("null_weights", None, "null weights"),
    ("channels", dict(channels=64), "channels must be 128"),
    ("head_hidden", dict(head_hidden=32), "head_hidden must be 64"),
    ("blocks", dict(blocks=0), "blocks must be"),
    ("board_4", dict(board_size=4), "board_size must be 5 to 19"),
    ("board_20", dict(board_size=20), "board_size must be 5 to 19"),
    ("dtype", dict(dtype=2), "dtype must be GMZ_NET_F16 or GMZ_NET_BF16"),
    ("null_destination", dict(dyn_action=None), "null destination dyn_action"),
    ("null_first_destination", dict(repr_stem_w=None), "null destination repr_stem_w"),
    ("null_last_destination", dict(reward_fc2_b=None), "null destination reward_fc2_b"),
    ("unaligned_destination", dict(policy_fc_w=ODD), "policy_fc_w must be 16-byte aligned"),
    ("unaligned_small_destination", dict(value_fc2_b=ODD), "value_fc2_b must be 16-byte aligned"),
]


@no_gpu
@pytest.mark.parametrize("name,wrong,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_pack_refuses_what_the_host_can_see(name, wrong, text):
    lib = _lib()
    need = _job_bytes(lib, 2)
    w = None if wrong is None else ctypes.byref(_weights(**wrong))
    assert lib.gmz_net_pack(w, p(40), need, None) != 0
    msg = lib.gmz_last_error().decode()
    assert text in msg and msg.startswith("gmz_net_pack: ") and not got_past_validation(msg), msg


@no_gpu
def test_pack_refuses_a_job_table_of_another_size():
    lib = _lib()
    need = _job_bytes(lib, 2)
    for have in (need - 40, need + 40, 0, _job_bytes(lib, 1)):
        assert lib.gmz_net_pack(ctypes.byref(_weights()), p(40), have, None) != 0
        msg = lib.gmz_last_error().decode()
        assert "job table of %d bytes" % have in msg and str(need) in msg and "gmz_net_pack_job_bytes" in msg
        assert not got_past_validation(msg)
    assert lib.gmz_net_pack(ctypes.byref(_weights()), None, need, None) != 0
    assert "null job table" in lib.gmz_last_error().decode()


@no_gpu
def test_board_size_refusal_reads_like_the_other_net_calls():
    lib = _lib()
    w = _weights(board_size=20)
    out = ctypes.c_size_t()
    assert lib.gmz_net_workspace_bytes(ctypes.byref(w), 8, ctypes.byref(out)) != 0
    theirs = lib.gmz_last_error().decode().split(": ", 1)[1]
    assert lib.gmz_net_pack(ctypes.byref(w), p(40), _job_bytes(lib, 2), None) != 0
    assert lib.gmz_last_error().decode().split(": ", 1)[1] == theirs


def test_cpu_loop_refuses_device_weights():
    from test_loop import _ScriptedSelfPlay
    from datou_gomoku_muzero_amd import loop as LP, replay as RP, trainer as T
    cfg = T.TrainConfig(BOARD_SIZE=6, NUM_RES_BLOCKS=1, PHYSICAL_BATCH_SIZE=8, TRAIN_BUFFER_SIZE=64)
    rb = RP.ReplayBuffer(cfg, device="cpu")
    with pytest.raises(ValueError, match="device_weights needs the loop on a GPU"):
        LP.C4Loop(_ScriptedSelfPlay(1), None, rb, cfg, 8, device="cpu", device_weights=True)
    assert LP.C4Loop(_ScriptedSelfPlay(1), None, rb, cfg, 8, device="cpu").device_weights is False  # the default stays


def _dyn_action_case(seed, channels_last):
    from datou_gomoku_muzero_amd import network as N, weights as W
    from datou_gomoku_muzero_amd.config import GmzConfig
    cfg = GmzConfig(BOARD_SIZE=5, NUM_RES_BLOCKS=1)
    f32 = np.float32
    rs = np.random.RandomState(seed)
    sd = W.synthetic_state_dict(cfg, seed=seed, with_projection=False)
    w = sd["dynamics_net.conv.weight"]
    w *= (10.0 ** rs.uniform(-4, 4, w.shape)).astype(f32)  # mixed magnitudes: another order of additions would show
    emb = sd["dynamics_net.action_embed_conv.weight"]
    emb *= (10.0 ** rs.uniform(-3, 3, emb.shape)).astype(f32)
    if channels_last:  # what Trainer.state_dict_cpu() hands pack_weights on the GPU: [o][ky][kx][c] in memory
        for k, v in sd.items():
            if v.ndim == 4:
                sd[k] = torch.from_numpy(v).contiguous(memory_format=torch.channels_last).numpy()
        assert sd["dynamics_net.conv.weight"].strides == (4 * 9 * 144, 4, 4 * 3 * 144, 4 * 144)
    got = N.pack_weights(sd, cfg)["dyn_action"]
    s, _ = N.fold_bn(sd, "dynamics_net.bn")
    wd = np.ascontiguousarray((sd["dynamics_net.conv.weight"] * s[:, None, None, None])[:, 128:]).reshape(128, 16, 9)
    assert wd.dtype == f32 and got.dtype == f32
    prod = (wd.transpose(2, 0, 1) * emb.reshape(16)).astype(f32)  # [t][n][c], each product rounded to float32
    return got, prod


def test_dyn_action_is_the_sequential_float32_sum():
    """The guard under the kernel's dyn_action for a plain ([o][c][ky][kx]) state dict: pack_weights'
    einsum("ncyx,c->yxn") over the 16 action-embedding input channels equals, bit for bit, the sum over c = 0..15 in
    that order, in float32, from 0, of the ROUNDED products (wd[n][128 + c][t] * emb[c]) with wd the dynamics conv
    weight already multiplied by its folded scale."""
    for seed in range(6):
        got, prod = _dyn_action_case(seed, False)
        acc = np.zeros((9, 128), np.float32)
        for c in range(16):
            acc = acc + prod[:, :, c]
        assert np.array_equal(got.view(np.uint32), acc.view(np.uint32)), seed


def test_dyn_action_of_channel_contiguous_weights_is_four_partial_sums():
    """The same guard for the host copy of a channels-last weight (the trainer's on the GPU): numpy's einsum then runs
    its contiguous sum-of-products loop, four float32 partial sums (lane i over c = i mod 4) that take the rounded
    products in the order c = 12.., 8.., 4.., 0.., combined as (l0 + l1) + (l2 + l3).  k_pack_towers restates this
    order when the source's channel stride is 1."""
    for seed in range(6):
        got, prod = _dyn_action_case(seed, True)
        lane = np.zeros((9, 128, 4), np.float32)
        for k in (3, 2, 1, 0):
            lane = prod[:, :, 4 * k:4 * k + 4] + lane
        acc = (lane[..., 0] + lane[..., 1]) + (lane[..., 2] + lane[..., 3])
        assert np.array_equal(got.view(np.uint32), acc.view(np.uint32)), seed
