"""Board sizes 5..19 of the inference network, on the CPU: the two size gates (network.BOARD_SIZES in Python,
TowerSizes in csrc/gmz_net.hip) accept the same sizes, the weight packing is size-generic (the float32 emulation
of test_network_pack on packed weights against the oracle forward), and oracle/netref.py reproduces the
reference forward at the four new fixture sizes (tests/golden/make_golden_net_sizes.py: 5, 8, 13, 17)."""
import ctypes

import numpy as np
import pytest

import netref
import test_network_pack as tp
from datou_gomoku_muzero_amd import engine as E
from datou_gomoku_muzero_amd import network as N
from datou_gomoku_muzero_amd import weights as W
from datou_gomoku_muzero_amd.config import GmzConfig

NEW_FIXTURES = ["net_c5.npz", "net_c8.npz", "net_c13.npz", "net_c17.npz"]


def test_board_sizes_is_5_to_19():
    assert tuple(N.BOARD_SIZES) == tuple(range(5, 20))


@pytest.mark.parametrize("size", range(3, 24))
def test_python_and_c_gates_accept_exactly_board_sizes(size):
    """GomokuNetHip's gate (built on the CPU device here: packing and the workspace query need no GPU) and
    gmz_net_workspace_bytes accept a size exactly when it is in network.BOARD_SIZES; a refusal names the range."""
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    w = N.NetWeights()
    w.board_size, w.channels, w.blocks, w.head_hidden, w.dtype = size, 128, 1, 64, 0
    need = ctypes.c_size_t()
    rc = lib.gmz_net_workspace_bytes(ctypes.byref(w), 13, ctypes.byref(need))
    cfg = GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=1)
    if size in N.BOARD_SIZES:
        assert rc == 0 and need.value > 0
        sd = W.synthetic_state_dict(cfg, seed=size, with_projection=False)
        net = N.GomokuNetHip(sd, cfg, num_slots=1, max_rows=13, device="cpu")
        assert net.workspace.numel() == need.value and net.pool.numel() == size * size * 128
    else:
        assert rc < 0
        assert "5 to 19" in lib.gmz_last_error().decode()
        with pytest.raises(ValueError, match="5 to 19"):
            N.GomokuNetHip({}, cfg, device="cpu")


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("size", [5, 8, 13, 17])
def test_packed_emulation_matches_oracle_at_new_sizes(size, prec, monkeypatch):
    """test_network_pack.test_packed_emulation_matches_oracle (its emulation and its bounds) at 5, 8, 13, 17."""
    monkeypatch.setattr(tp, "PREC", prec)
    cfg = GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=2)
    sd = W.synthetic_state_dict(cfg, seed=9 + size, with_projection=False)
    pk = N.pack_weights(sd, cfg, prec)
    A = size * size
    assert pk["policy_fc_w"].shape == (N.r16(A), N.r16(2 * A)) and pk["value_fc1_w"].shape == (64, N.r16(A))
    assert pk["reward_fc1_w"].shape == (A * 4, 4, 64, 8)
    rs = np.random.RandomState(size)
    obs = (rs.rand(3, 3, size, size) < 0.3).astype(np.float32)
    p, v, h = netref.initial_inference(sd, obs)
    ep, ev, eh, _ = tp.emulate(pk, cfg, obs=obs)
    tol = 0.003 if prec == "fp16" else 0.02  # weight rounding only: 2^-11 vs 2^-8 relative
    assert np.abs(ep - p).max() <= tol * np.abs(p).max() + 1e-3
    assert np.abs(ev - v).max() <= tol
    acts = np.array([0, A // 2 - 1, A - 1])  # both corners: the action term's border clipping
    p2, v2, h2, r2 = netref.recurrent_inference(sd, h, acts)
    ep2, ev2, eh2, er2 = tp.emulate(pk, cfg, h=h, action=acts)
    assert np.abs(ep2 - p2).max() <= tol * np.abs(p2).max() + 1e-3
    assert np.abs(ev2 - v2).max() <= tol and np.abs(er2 - r2).max() <= tol
    assert np.abs(eh2 - h2).max() <= tol * np.abs(h2).max()


@pytest.mark.parametrize("name", NEW_FIXTURES)
def test_netref_matches_reference_forward_at_new_sizes(golden, name):
    """test_netref.test_netref_matches_reference_forward's checks and bound on the new fixtures."""
    d = golden(name)
    assert (int(d["C"]), int(d["blocks"]), int(d["hd"])) == (128, 2, 64) and d["obs"].shape[0] == 2
    cfg = GmzConfig(BOARD_SIZE=int(d["size"]), NUM_RES_BLOCKS=2)
    sd = W.synthetic_state_dict(cfg, seed=int(d["seed"]))
    ws = np.array([float(np.sum(np.abs(x.astype(np.float64)))) for x in sd.values()])
    assert np.allclose(ws, d["wsum"], rtol=1e-12, atol=0)
    p, v, h = netref.initial_inference(sd, d["obs"])
    p2, v2, h2, r2 = netref.recurrent_inference(sd, h, d["actions"])
    tol = dict(rtol=1e-4, atol=1e-5)
    assert np.allclose(p, d["p"], **tol) and np.allclose(v, d["v"], **tol)
    assert np.allclose(p2, d["p2"], **tol) and np.allclose(v2, d["v2"], **tol) and np.allclose(r2, d["r2"], **tol)
    assert np.allclose(h.astype(np.float64).sum(axis=(1, 2, 3)), d["h_sum"], rtol=1e-4)
    assert np.allclose(h2.astype(np.float64).sum(axis=(1, 2, 3)), d["h2_sum"], rtol=1e-4)
    assert np.allclose(h[:, :8, :4, :4], d["h_corner"], **tol)
    assert np.allclose(h2[:, :8, :4, :4], d["h2_corner"], **tol)


@pytest.mark.parametrize("size", [5, 8, 13, 17])
def test_engine_sizing_helpers_are_size_generic(size):
    """engine.hidden_slots is the search schedule's slot count at any size; the two-stream rule stays 15x15's."""
    for mode, sims in (("MuZero", 50), ("AlphaZero", 50)):
        cfg = GmzConfig(BOARD_SIZE=size, NUM_SIMULATIONS=sims, MCTS_IMPLEMENTATION=mode)
        n = E.hidden_slots(cfg, 4)
        assert n % 4 == 0 and 4 * 3 <= n <= 4 * (sims + 2)
        assert E.default_streams(cfg, 1024) == 1
