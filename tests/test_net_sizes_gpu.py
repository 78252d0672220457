"""The HIP GomokuNetEZ (csrc/gmz_net.hip) at the 11 board sizes between 5 and 19 that are not 6, 9, 15 or 19, on the
GPU: the checks of tests/test_net_gpu.py (its tolerances TOL and _check, imported, not restated), of
tests/test_split_gpu.py and of the pipeline tests, at small shapes.  Every tower path is covered: five boards packed
into a workgroup (5), two boards (7, 10; 8: A % 16 == 0, no tile saved), one board with two LDS images (11..14) and
one board with a single image and the residual scratch (16..18)."""
import queue

import numpy as np
import pytest

import netref
import test_net_gpu as tg
import test_split_gpu as ts
from test_net_gpu import TOL, _check, _positions

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NEW_SIZES = [5, 7, 8, 10, 11, 12, 13, 14, 16, 17, 18]
FIXTURES = ["net_c5.npz", "net_c8.npz", "net_c13.npz", "net_c17.npz"]


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from datou_gomoku_muzero_amd import network as N, weights as W
    from datou_gomoku_muzero_amd.config import GmzConfig
    return N, W, GmzConfig


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("size,blocks", [(s, 2) for s in NEW_SIZES] + [(s, 1) for s in (5, 8, 13, 17)])
def test_hip_net_matches_oracle(mods, size, blocks, prec):
    """test_net_gpu.test_hip_net_matches_oracle's body on 13 rows: odd, and no multiple of any boards-per-workgroup
    count, so the last workgroup repeats its partner row."""
    N, W, GmzConfig = mods
    _, _, SCALAR_ABS, HID_REL = TOL[prec]
    cfg = GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=blocks)
    sd = W.synthetic_state_dict(cfg, seed=size + blocks, with_projection=False)
    rs = np.random.RandomState(size)
    n = 13
    obs = _positions(size, n, rs)
    net = N.GomokuNetHip(sd, cfg, num_slots=2 * n, max_rows=n, precision=prec)
    lg, v, slots = net.initial_inference(obs)
    torch.cuda.synchronize()
    pr, vr, hr = netref.initial_inference(sd, obs)
    _check(lg.cpu().numpy(), v.cpu().numpy(), pr, vr[:, 0], "initial %dx%d" % (size, size), prec)
    h = net.hidden(np.arange(n)).cpu().numpy()
    rel = np.linalg.norm((h - hr).reshape(n, -1), axis=1) / np.linalg.norm(hr.reshape(n, -1), axis=1)
    print("hidden rel L2 %.3g" % rel.max())
    assert rel.max() <= HID_REL, rel.max()
    # recurrent from the HIP hidden states; the oracle starts from the same (16-bit-rounded) states
    acts = rs.randint(0, size * size, n)
    lg2, v2, r2 = net.recurrent_inference(np.arange(n), acts, np.arange(n, 2 * n))
    torch.cuda.synchronize()
    p2r, v2r, h2r, r2r = netref.recurrent_inference(sd, h, acts)
    _check(lg2.cpu().numpy(), v2.cpu().numpy(), p2r, v2r[:, 0], "recurrent %dx%d" % (size, size), prec)
    assert np.abs(r2.cpu().numpy() - r2r[:, 0]).max() <= SCALAR_ABS
    h2 = net.hidden(np.arange(n, 2 * n)).cpu().numpy()
    rel2 = np.linalg.norm((h2 - h2r).reshape(n, -1), axis=1) / np.linalg.norm(h2r.reshape(n, -1), axis=1)
    print("recurrent hidden rel L2 %.3g" % rel2.max())
    assert rel2.max() <= HID_REL, rel2.max()


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_hip_net_matches_reference_fixture(mods, golden, name, prec):
    """test_net_gpu.test_hip_net_matches_reference_fixture's body on the reference network.py forwards at 5, 8, 13
    and 17 (tests/golden/make_golden_net_sizes.py)."""
    N, W, GmzConfig = mods
    _, _, SCALAR_ABS, HID_REL = TOL[prec]
    d = golden(name)
    cfg = GmzConfig(BOARD_SIZE=int(d["size"]), NUM_RES_BLOCKS=int(d["blocks"]))
    sd = W.synthetic_state_dict(cfg, seed=int(d["seed"]))
    net = N.GomokuNetHip(sd, cfg, num_slots=8, max_rows=4, precision=prec)
    lg, v, _ = net.initial_inference(d["obs"])
    lg2, v2, r2 = net.recurrent_inference([0, 1], d["actions"], [2, 3])
    torch.cuda.synchronize()
    _check(lg.cpu().numpy(), v.cpu().numpy(), d["p"], d["v"][:, 0], "fixture initial", prec)
    _check(lg2.cpu().numpy(), v2.cpu().numpy(), d["p2"], d["v2"][:, 0], "fixture recurrent", prec)
    assert np.abs(r2.cpu().numpy() - d["r2"][:, 0]).max() <= SCALAR_ABS
    h2 = net.hidden([2, 3]).cpu().numpy().astype(np.float64)
    assert np.allclose(h2.sum(axis=(1, 2, 3)), d["h2_sum"], rtol=HID_REL)


@pytest.mark.parametrize("size", NEW_SIZES)
def test_rows_are_batch_invariant(mods, size):
    """7 rows with one skipped slot, then the same rows on a grid capped at 2 workgroups (each takes several boards or
    board groups: static strides for packed boards, tickets for one board per workgroup, on one workspace across
    launches of different row counts): every row, initial and recurrent outputs and hidden state, is bit-for-bit
    what it is in a launch of its own."""
    N, W, GmzConfig = mods
    cfg = GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=2)
    sd = W.synthetic_state_dict(cfg, seed=7 + size, with_projection=False)
    n = 7
    obs = _positions(size, n, np.random.RandomState(size + 1))
    acts = np.random.RandomState(size + 2).randint(0, size * size, n)
    net = N.GomokuNetHip(sd, cfg, num_slots=4 * n, max_rows=n)
    slots = np.arange(n)
    slots[3] = -1
    runs = []
    for cap in (0, 2):
        net.w.max_grid = cap
        lg, v, _ = net.initial_inference(obs, slots=slots)
        lg2, v2, r2 = net.recurrent_inference(np.where(slots < 0, 0, slots), acts, np.where(slots < 0, -1, slots + n))
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy().copy() for t in (lg, v, lg2, v2, r2)] +
                    [net.hidden(np.arange(n)).cpu().numpy(), net.hidden(np.arange(n, 2 * n)).cpu().numpy()])
    net.w.max_grid = 0
    for i in range(n):
        if slots[i] < 0:
            continue
        o = 2 * n + i
        a, b, _ = net.initial_inference(obs[i:i + 1], slots=[o])
        c, d, e = net.recurrent_inference([o], acts[i:i + 1], [3 * n + i])
        torch.cuda.synchronize()
        alone = [t.cpu().numpy()[0] for t in (a, b, c, d, e)] + [net.hidden([o]).cpu().numpy()[0],
                                                                net.hidden([3 * n + i]).cpu().numpy()[0]]
        for batch in runs:
            for got, want in zip(alone, batch):
                assert np.array_equal(got, want[i]), (size, i)


@pytest.mark.parametrize("size,sims,mode,blocks,G", [(8, 50, "AlphaZero", 1, 4), (13, 50, "MuZero", 1, 4),
                                                   (17, 50, "MuZero", 1, 2)])
def test_engine_with_hip_net_matches_oracle_driving_same_net(mods, size, sims, mode, blocks, G):
    """test_net_gpu's engine-against-oracle test (actions, values and visit counts exact, policy within 1e-12)."""
    tg.test_engine_with_hip_net_matches_oracle_driving_same_net(mods, size, sims, mode, blocks, G)


def test_split_equals_single_hip_net_at_13(mods):
    """test_split_gpu.test_split_equals_single_hip_net at 13x13 with 8 games: two half-size engines on two streams
    (tower grid capped) play bit-for-bit the games of one engine."""
    import datou_gomoku_muzero_amd.engine as E
    N, W, GmzConfig = mods
    cfg = GmzConfig(BOARD_SIZE=13, NUM_SIMULATIONS=24, MCTS_IMPLEMENTATION="MuZero", NUM_RES_BLOCKS=1)
    G = 8
    sd = W.synthetic_state_dict(cfg, seed=3, with_projection=False)
    slots = G * (cfg.NUM_SIMULATIONS + 2)
    net1 = N.GomokuNetHip(sd, cfg, num_slots=slots, max_rows=G)
    net2 = N.GomokuNetHip(sd, cfg, num_slots=slots, max_rows=G)
    one = E.BatchedSelfPlayEngine(cfg, num_games=G, net=net1, seed=11)
    two = E.SplitSelfPlayEngine(cfg, num_games=G, net=net2, seed=11, parts=2, max_grid=3)
    one.reset_games()
    two.reset_games()
    rs1, rs2 = np.random.RandomState(4), np.random.RandomState(4)
    ts._same(ts._moves(one, 4, rs1), ts._moves(two, 4, rs2))


def test_trained_weights_hot_swap_at_8(mods):
    """The loop closes at 8x8 (1 block, batch 8): one Trainer.step on synthetic slices, its weights hot-swapped into
    a running GomokuNetHip, and the swapped net against the oracle forward on the new weights."""
    from datou_gomoku_muzero_amd import trainer as T
    N, W, GmzConfig = mods
    cfg = GmzConfig(BOARD_SIZE=8, NUM_RES_BLOCKS=1)
    tc = T.TrainConfig(BOARD_SIZE=8, NUM_RES_BLOCKS=1, PHYSICAL_BATCH_SIZE=8)
    sd0 = W.synthetic_state_dict(cfg, seed=5)
    net = N.GomokuNetHip(sd0, cfg, num_slots=16, max_rows=8)
    tr = T.Trainer(tc, device="cuda", state_dict=sd0)
    obs, act, rew, pol, val = W.synthetic_slices(8, 8, tc.NUM_UNROLL_STEPS, np.random.RandomState(3))
    batch = [torch.as_tensor(x).cuda() for x in (obs, act, rew, pol, val)]
    batch[0] = batch[0].float()
    logs, _ = tr.step(batch, torch.ones(8, device="cuda"))
    assert np.isfinite(logs[0])
    sd1 = {k: v.numpy() for k, v in tr.state_dict_cpu().items()}
    assert any(not np.allclose(np.asarray(sd0[k]), sd1[k]) for k in sd0 if k in sd1)
    net.load_state_dict(sd1)
    n = 8
    rs = np.random.RandomState(8)
    o = _positions(8, n, rs)
    lg, v, _ = net.initial_inference(o)
    torch.cuda.synchronize()
    pr, vr, hr = netref.initial_inference(sd1, o)
    _check(lg.cpu().numpy(), v.cpu().numpy(), pr, vr[:, 0], "hot-swapped initial 8x8")
    h = net.hidden(np.arange(n)).cpu().numpy()
    acts = rs.randint(0, 64, n)
    lg2, v2, r2 = net.recurrent_inference(np.arange(n), acts, np.arange(n, 2 * n))
    torch.cuda.synchronize()
    p2r, v2r, _, r2r = netref.recurrent_inference(sd1, h, acts)
    _check(lg2.cpu().numpy(), v2.cpu().numpy(), p2r, v2r[:, 0], "hot-swapped recurrent 8x8")
    assert np.abs(r2.cpu().numpy() - r2r[:, 0]).max() <= TOL["fp16"][2]


def test_worker_emits_well_formed_records_at_8(mods):
    """gpu_selfplay_worker at 8x8 (test_adapter_gpu.test_worker_emits_reference_messages' shape checks): 64 moves
    fill the board, so every one of the 8 games finishes at least once."""
    from datou_gomoku_muzero_amd.worker import gpu_selfplay_worker
    N, W, GmzConfig = mods
    cfg = GmzConfig(BOARD_SIZE=8, NUM_SIMULATIONS=16, NUM_RES_BLOCKS=1)

    class Ev:
        def is_set(self):
            return False

    dq, lq, uq, tq = queue.Queue(), queue.Queue(), queue.Queue(), queue.Queue()
    gpu_selfplay_worker(0, None, dq, lq, uq, Ev(), trainer_event_queue=tq, num_games=8, cfg=cfg, max_moves=64,
                        emit_move_notices=False)
    items = []
    while not dq.empty():
        items.append(dq.get())
    assert len(items) >= 8
    for record, slices, version in items:
        n = len(record.actions)
        assert 9 <= n <= 64 and len(slices) == n and len(record.rewards) == n and len(record.values) == n
        assert record.observations[0].shape == (3, 8, 8) and record.policies[0].shape == (64,)
        assert all(abs(float(np.sum(p)) - 1.0) < 1e-5 for p in record.policies)
        assert len(set(int(a) for a in record.actions)) == n and all(0 <= int(a) < 64 for a in record.actions)
        assert slices[0].observation.shape == (6, 3, 8, 8) and slices[0].action_history.dtype == np.int32
        assert abs(record.rewards[-1]) in (0.0, 1.0)
    assert tq.qsize() == len(items) and lq.qsize() == len(items)
