"""GPU numerics of the HIP GomokuNetEZ (csrc/gmz_net.hip) against the float32 oracle
(oracle/netref.py, itself pinned to the reference forward) and the reference fixture net_c15.npz.

The HIP path computes with 16-bit operands (weights and activations; f16 by default, bf16 as an
option) and float32 accumulation; the residual stream is the layer outputs as stored (16-bit).
Tolerances (stated here), f16 / bf16:
  policy logits : |Δ| <= 0.005 * max|logit| + 0.002  /  0.03 * max|logit| + 0.01   (per row)
  value, reward : |Δ| <= 0.005  /  0.03                                            (scalars in [-1, 1])
  hidden state  : relative L2 error <= 5e-3  /  3e-2
  top-1 policy: identical wherever the reference's top-1 margin exceeds twice the row's logit error
"""
import numpy as np
import pytest

import netref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# (logit rel, logit abs, scalar abs, hidden rel L2) per precision
TOL = {"fp16": (0.005, 0.002, 0.005, 5e-3), "bf16": (0.03, 0.01, 0.03, 3e-2)}


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from datou_gomoku_muzero_amd import network as N, weights as W
    from datou_gomoku_muzero_amd.config import GmzConfig
    return N, W, GmzConfig


def _positions(size, n, rs):
    A = size * size
    obs = np.zeros((n, 3, size, size), np.float32)
    for i in range(n):
        k = rs.randint(0, min(A - 1, 60))
        cells = rs.permutation(A)[:k]
        b = np.zeros(A, np.int8)
        p = 1
        for c in cells:
            b[c] = p
            p = -p
        obs[i, 0] = (b == p).reshape(size, size)
        obs[i, 1] = (b == -p).reshape(size, size)
        if k:
            obs[i, 2].reshape(-1)[cells[-1]] = 1
    return obs


def _check(p, v, pr, vr, what, prec="fp16"):
    LOGIT_REL, LOGIT_ABS, SCALAR_ABS, _ = TOL[prec]
    err = np.abs(p - pr).max(axis=1)
    bound = LOGIT_REL * np.abs(pr).max(axis=1) + LOGIT_ABS
    top1 = (p.argmax(1) == pr.argmax(1)).mean()
    print("%s [%s]: max|dlogit| %.4g (bound %.4g), max|dv| %.4g, top1 %.3f" % (what, prec, err.max(), bound.min(),
                                                                               np.abs(v - vr).max(), top1))
    assert (err <= bound).all()
    assert np.abs(v - vr).max() <= SCALAR_ABS
    # top-1 must agree wherever the reference's top-1 margin exceeds twice the logit error seen on
    # that row: a flip there cannot come from 16-bit rounding (near-ties may flip; the rate is printed)
    srt = np.sort(pr, axis=1)
    decisive = (srt[:, -1] - srt[:, -2]) > 2 * err
    assert (p.argmax(1) == pr.argmax(1))[decisive].all()
    assert decisive.mean() >= 0.5  # the criterion must actually bite


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("size,blocks", [(15, 8), (9, 2), (6, 1), (19, 16), (19, 2)])
def test_hip_net_matches_oracle(mods, size, blocks, prec):
    """(19, 16) is config C5's network: single-LDS-image tower path with the residual scratch."""
    N, W, GmzConfig = mods
    _, _, SCALAR_ABS, HID_REL = TOL[prec]
    cfg = GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=blocks)
    sd = W.synthetic_state_dict(cfg, seed=size + blocks, with_projection=False)
    rs = np.random.RandomState(size)
    n = 48 if size < 19 else 12
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
def test_hip_net_matches_reference_fixture(mods, golden, prec):
    """Reference network.py forward (tests/golden/net_c15.npz) on the same numpy-seeded weights."""
    N, W, GmzConfig = mods
    _, _, SCALAR_ABS, HID_REL = TOL[prec]
    d = golden("net_c15.npz")
    cfg = GmzConfig(BOARD_SIZE=15, NUM_RES_BLOCKS=8)
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


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("size", [6, 9])
def test_two_board_workgroups_are_batch_invariant(mods, size, prec):
    """Small boards run two rows per tower workgroup (gmz_net.hip TowerCfg NB = 2): an odd row count
    (the last row has no partner), a skipped partner (slot -1) and every pairing must give each row
    bit-for-bit the output it gets alone."""
    N, W, GmzConfig = mods
    cfg = GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=2)
    sd = W.synthetic_state_dict(cfg, seed=7 + size, with_projection=False)
    n = 7
    obs = _positions(size, n, np.random.RandomState(size + 1))
    acts = np.random.RandomState(size + 2).randint(0, size * size, n)
    net = N.GomokuNetHip(sd, cfg, num_slots=4 * n, max_rows=n, precision=prec)
    slots = np.arange(n)
    slots[3] = -1  # rows 2 and 3 share a workgroup; row 3 is skipped
    lg, v, _ = net.initial_inference(obs, slots=slots)
    lg2, v2, r2 = net.recurrent_inference(np.where(slots < 0, 0, slots), acts, np.where(slots < 0, -1, slots + n))
    torch.cuda.synchronize()
    batch = [t.cpu().numpy().copy() for t in (lg, v, lg2, v2, r2)]
    hb = net.hidden(np.arange(n, 2 * n)).cpu().numpy()
    for i in range(n):
        if slots[i] < 0:
            continue
        o = 2 * n + i
        a, b, _ = net.initial_inference(obs[i:i + 1], slots=[o])
        c, d, e = net.recurrent_inference([o], acts[i:i + 1], [3 * n + i])
        torch.cuda.synchronize()
        for got, want in zip((a, b, c, d, e), batch):
            assert np.array_equal(got.cpu().numpy()[0], want[i]), i
        assert np.array_equal(net.hidden([3 * n + i]).cpu().numpy()[0], hb[i])



@pytest.mark.parametrize("size", [15, 19])
def test_ticket_scheduled_towers_are_batch_invariant(mods, size):
    """One-board tower workgroups (15x15, 19x19) take rows in ticket order from counters in the net's
    workspace that every launch must leave at zero: launches of different row counts on the same
    workspace — more rows than CUs (workgroups take several boards, in any order), skipped rows
    (slot -1), a capped grid — give every row bit-for-bit its output from a launch of its own."""
    N, W, GmzConfig = mods
    cfg = GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=1)
    sd = W.synthetic_state_dict(cfg, seed=11 + size, with_projection=False)
    n = 300 if size == 15 else 160
    rs = np.random.RandomState(size + 3)
    obs = _positions(size, n, rs)
    acts = rs.randint(0, size * size, n)
    net = N.GomokuNetHip(sd, cfg, num_slots=4 * n, max_rows=n)
    slots = np.arange(n)
    slots[rs.choice(n, n // 7, replace=False)] = -1
    outs = []
    for rows, cap in ((n, 0), (37, 0), (n, 64)):
        net.w.max_grid = cap
        sl = slots[:rows]
        lg, v, _ = net.initial_inference(obs[:rows], slots=sl)
        lg2, v2, r2 = net.recurrent_inference(np.where(sl < 0, 0, sl), acts[:rows], np.where(sl < 0, -1, sl + n))
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy().copy() for t in (lg, v, lg2, v2, r2)])
    net.w.max_grid = 0
    for i in rs.choice(np.flatnonzero(slots[:37] >= 0), 6, replace=False):
        o = 2 * n + i
        a, b, _ = net.initial_inference(obs[i:i + 1], slots=[o])
        c, d, e = net.recurrent_inference([o], acts[i:i + 1], [3 * n + i])
        torch.cuda.synchronize()
        for batch in outs:
            for got, want in zip((a, b, c, d, e), batch):
                assert np.array_equal(got.cpu().numpy()[0], want[i]), i
    for got, want in zip(outs[0], outs[2]):  # the full batch on a capped grid: identical
        live = slots >= 0
        assert np.array_equal(got[live], want[live])


def test_skipped_rows_untouched(mods):
    N, W, GmzConfig = mods
    cfg = GmzConfig(BOARD_SIZE=9, NUM_RES_BLOCKS=1)
    sd = W.synthetic_state_dict(cfg, seed=1, with_projection=False)
    net = N.GomokuNetHip(sd, cfg, num_slots=4, max_rows=4)
    obs = _positions(9, 2, np.random.RandomState(0))
    lg, v, _ = net.initial_inference(obs, slots=[0, -1])
    torch.cuda.synchronize()
    assert torch.isfinite(lg[0]).all()
    # the same through the backend interface, on buffers whose contents are known: slot 1 live, slots 0, 2, 3 not
    # named; logits, value and reward start as NaN.  The live row ends finite; the skipped row's outputs and every
    # slot not named are untouched, in the initial and in the recurrent pass.
    from datou_gomoku_muzero_amd import _lib
    dev = net.device
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    net.pool.fill_(-91)  # 0xFFA5: a NaN in f16
    lg, v = nan(2, 81), nan(2)
    net.initial(torch.from_numpy(obs).to(dev), i32([1, -1]), lg, v, _lib.stream_ptr())
    torch.cuda.synchronize()
    pool = net.pool.view(4, -1).cpu().numpy()
    assert (pool[[0, 2, 3]] == -91).all() and np.isfinite(net.hidden([1]).cpu().numpy()).all()
    assert torch.isfinite(lg[0]).all() and torch.isfinite(v[0]) and torch.isnan(lg[1]).all() and torch.isnan(v[1])
    lg, v, r = nan(2, 81), nan(2), nan(2)
    net.recurrent(i32([1, 1]), i32([40, 7]), i32([-1, 3]), lg, v, r, _lib.stream_ptr())
    torch.cuda.synchronize()
    after = net.pool.view(4, -1).cpu().numpy()
    assert (after[[0, 2]] == -91).all() and np.array_equal(after[1], pool[1])
    assert np.isfinite(net.hidden([3]).cpu().numpy()).all()
    assert torch.isfinite(lg[1]).all() and torch.isfinite(v[1]) and torch.isfinite(r[1])
    assert torch.isnan(lg[0]).all() and torch.isnan(v[0]) and torch.isnan(r[0])


@pytest.mark.parametrize("size,sims,mode,blocks,G", [(15, 400, "MuZero", 2, 6), (9, 50, "AlphaZero", 1, 6),
                                                   (19, 800, "MuZero", 2, 2)])
def test_engine_with_hip_net_matches_oracle_driving_same_net(mods, size, sims, mode, blocks, G):
    """Engine + GomokuNetHip (batched, slot-indexed) vs the C oracle's search driving the SAME HIP
    network row-by-row through callbacks.  Every network row is computed by its own workgroup with a
    fixed instruction order, so outputs are batch-invariant and the two searches must agree exactly."""
    import oracle
    import datou_gomoku_muzero_amd.engine as E
    N, W, GmzConfig = mods
    cfg = GmzConfig(BOARD_SIZE=size, NUM_SIMULATIONS=sims, MCTS_IMPLEMENTATION=mode, NUM_RES_BLOCKS=blocks)
    sd = W.synthetic_state_dict(cfg, seed=3, with_projection=False)
    A = size * size
    net = N.GomokuNetHip(sd, cfg, num_slots=G * (sims + 2), max_rows=G)
    eng = E.BatchedSelfPlayEngine(cfg, num_games=G, net=net)
    rs = np.random.RandomState(11)
    boards = np.zeros((G, A), np.int8)
    players = np.ones(G, np.int8)
    lastm = np.full(G, -1, np.int32)
    for g in range(G):
        cells = rs.permutation(A)[: rs.randint(0, 30)]
        p = 1
        for c in cells:
            boards[g, c] = p
            p = -p
        players[g], lastm[g] = p, (cells[-1] if len(cells) else -1)
    gumbel = rs.gumbel(0, 1, (G, A))
    eng.set_positions(boards, players, lastm)
    pol, val, act = eng.search(gumbel=gumbel)
    visits = eng.root_stats()[0]
    torch.cuda.synchronize()
    pol, val, act, visits = pol.cpu().numpy(), val.cpu().numpy(), act.cpu().numpy(), visits.cpu().numpy()

    onet = N.GomokuNetHip(sd, cfg, num_slots=4096, max_rows=16)
    nxt = [0]

    def alloc(n):
        s = list(range(nxt[0], nxt[0] + n))
        nxt[0] += n
        assert nxt[0] <= 4096
        return s

    def init(obs):
        slots = alloc(obs.shape[0])
        lg, v, _ = onet.initial_inference(obs, slots=slots)
        torch.cuda.synchronize()
        return lg.cpu().numpy(), v.cpu().numpy(), slots

    def rec(hs, acts):
        out = alloc(len(hs))
        lg, v, r = onet.recurrent_inference(hs, acts, out)
        torch.cuda.synchronize()
        return lg.cpu().numpy(), v.cpu().numpy(), r.cpu().numpy(), out

    cb = oracle.CallbackNet(A, size, init, rec)
    ocfg = oracle.make_cfg(size, sims, mode, hashnet=False)
    for g in range(G):
        nxt[0] = 0
        cb.reset()
        opol, oval, oact, orv, _ = oracle.search(ocfg, boards[g], players[g], None if lastm[g] < 0 else lastm[g],
                                                 int(np.count_nonzero(boards[g])), gumbel[g], net=cb)
        assert act[g] == oact and val[g] == oval and (visits[g] == orv).all(), g
        assert np.abs(pol[g] - opol).max() <= 1e-12
