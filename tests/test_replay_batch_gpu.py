"""Training batches from the device replay ring to the trainer in HIP (gmz_replay_gather, gmz_replay_per_sample,
ReplayBuffer.sample_indices / gather_into, Trainer.step_from, C4Loop(device_batches=True)) on the GPU.  No kernel is
compared with itself: every expected value comes from trainer.augment with torch indexing, from ReplayBuffer.sample,
or from the numpy restatement of the draw's stated summation order (tests/replay_batch_ref.py)."""
import numpy as np
import pytest

import replay_batch_ref as REF

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _ring(H, U, N=37, count=23, per=True, seed=0, scramble=True):
    """A device ring of ``count`` synthetic slices; ``scramble``: random 0/1 planes, random f32 policies and some
    actions of -1, so that no board symmetry maps the data onto itself."""
    from datou_gomoku_muzero_amd import replay as RP, trainer as T, weights as W
    cfg = T.TrainConfig(BOARD_SIZE=H, NUM_UNROLL_STEPS=U, PHYSICAL_BATCH_SIZE=7, TRAIN_BUFFER_SIZE=N, ENABLE_PER=per)
    rb = RP.ReplayBuffer(cfg, device="cuda")
    rs = np.random.RandomState(seed)
    rb.add_arrays(*W.synthetic_slices(count, H, U, rs))
    if scramble:
        g = torch.Generator(device="cpu").manual_seed(seed)
        rb.obs[:count] = torch.randint(0, 2, tuple(rb.obs[:count].shape), generator=g, dtype=torch.uint8).cuda()
        rb.pol[:count] = torch.randn(tuple(rb.pol[:count].shape), generator=g).cuda()
        act = rb.act[:count].cpu()
        act[torch.rand(tuple(act.shape), generator=g) < 0.3] = -1
        rb.act[:count] = act.cuda()
        assert int((rb.act[:count] == -1).sum()) > 0 and int((rb.act[:count] >= 0).sum()) > 0
    return rb


def _expected(rb, idx, w, k, flip):
    """The seven tensors Trainer._augment_into_static leaves in _static for sample's batch, from trainer.augment."""
    from datou_gomoku_muzero_amd import trainer as T
    obs, act, rew, pi, mval = rb.obs[idx].float(), rb.act[idx], rb.rew[idx], rb.pol[idx], rb.val[idx]
    o, p, a = T.augment(obs, pi, act.long(), k, flip)
    return tuple(t.contiguous() for t in (o, act.long(), rew.float(), p, mval.float(), a, w.float()))


def _dst(rb, B, fill=None):
    c = rb.cfg
    U, H = c.NUM_UNROLL_STEPS, c.BOARD_SIZE
    f32, i64 = torch.float32, torch.int64
    spec = ((f32, (B, U + 1, 3, H, H)), (i64, (B, U)), (f32, (B, U)), (f32, (B, U + 1, H * H)), (f32, (B, U + 1)),
            (i64, (B, U)), (f32, (B,)))
    return tuple(torch.full(s, -77 if fill is None else fill, dtype=dt, device="cuda") for dt, s in spec)


@pytest.mark.parametrize("H,U", [(5, 2), (5, 5), (6, 2), (6, 5), (15, 5)])
def test_gather_equals_augment_bit_for_bit(H, U):
    rb = _ring(H, U, seed=10 * H + U)
    rs = np.random.RandomState(1)
    cases = 0
    for B in (7, 1):
        idx = torch.from_numpy(rs.randint(0, rb.count, B)).cuda()
        if B == 7:
            idx[5] = idx[2]  # PER draws repeats
        w = torch.from_numpy(rs.uniform(0.1, 1.0, B).astype(np.float32)).cuda()
        for k in range(4):
            for flip in (False, True):
                for given in (True, False):
                    dst = _dst(rb, B)
                    rb.gather_into(dst, idx, w if given else None, k, flip)
                    want = _expected(rb, idx, w if given else torch.ones(B, device="cuda"), k, flip)
                    for name, g, x in zip("obs act rew pol val act_aug w".split(), dst, want):
                        assert g.dtype == x.dtype and torch.equal(g, x), (name, H, U, B, k, flip, given)
                    cases += 1
    assert cases == 32


def test_gather_row_out_of_range_writes_nothing():
    rb = _ring(6, 5, seed=4)
    idx = torch.tensor([3, rb.count, 0, -1, 22, 3], dtype=torch.int64, device="cuda")
    w = torch.linspace(0.2, 1.0, 6, device="cuda")
    dst = _dst(rb, 6, fill=-77)
    rb.gather_into(dst, idx, w, 3, True)
    ok = torch.tensor([0, 2, 4, 5], device="cuda")
    want = _expected(rb, idx[ok], w[ok], 3, True)
    for g, x in zip(dst, want):
        assert torch.equal(g[ok], x)
        assert bool((g[[1, 3]] == -77).all())  # the sentinel, untouched


def test_gather_into_refuses_mismatches():
    from datou_gomoku_muzero_amd import _lib as L
    rb = _ring(6, 5, seed=4, scramble=False)
    idx = torch.zeros(7, dtype=torch.int64, device="cuda")
    good = _dst(rb, 7)
    rb.gather_into(good, idx, None, 0, False)
    with pytest.raises(ValueError, match="idx"):
        rb.gather_into(good, idx.int(), None, 0, False)
    with pytest.raises(ValueError, match="idx"):
        rb.gather_into(good, idx.cpu(), None, 0, False)
    with pytest.raises(ValueError, match="w must"):
        rb.gather_into(good, idx, torch.ones(7, dtype=torch.float64, device="cuda"), 0, False)
    with pytest.raises(ValueError, match="static inputs"):
        rb.gather_into(good[:6], idx, None, 0, False)
    for i, bad in ((0, good[0].half()), (1, good[1].int()), (3, good[3][:, :, :-1]), (6, torch.ones(8, device="cuda")),
                   (0, good[0].cpu()), (0, _dst(_ring(5, 5, scramble=False), 7)[0])):
        with pytest.raises(ValueError, match="dst"):
            rb.gather_into(good[:i] + (bad,) + good[i + 1:], idx, None, 0, False)
    with pytest.raises(ValueError, match="quarter turns"):
        rb.gather_into(good, idx, None, 4, False)
    from datou_gomoku_muzero_amd import replay as RP, trainer as T
    empty = RP.ReplayBuffer(rb.cfg, device="cuda")
    with pytest.raises(L.GmzError, match="count"):  # the library's own refusal: nothing to read yet
        empty.gather_into(good, idx, None, 0, False)


def _hip_draw(prio, r, B):
    from datou_gomoku_muzero_amd import _lib as L
    count = int(prio.numel())
    need = L.query("gmz_replay_per_sample_workspace_bytes", count, B)
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")
    idx = torch.full((B,), -5, dtype=torch.int64, device="cuda")
    prob = torch.full((B,), -5.0, dtype=torch.float64, device="cuda")
    L.call("gmz_replay_per_sample", prio, r, count, B, idx, L.nbytes(idx), prob, L.nbytes(prob), ws, L.nbytes(ws),
           L.stream_ptr())
    return idx, prob


@pytest.mark.parametrize("count", [1, 23, 5000, 70001])
def test_per_draw_equals_the_stated_order_and_is_deterministic(count):
    rs = np.random.RandomState(count)
    prio = (np.abs(rs.standard_normal(count)) + 1e-6).astype(np.float32)
    pd = torch.from_numpy(prio).cuda()
    for B in (1, 7, 360):
        r = rs.random_sample(B)
        r[0] = 0.0
        r[-1] = 1.0 - 2.0 ** -53  # in the last segment: u rounds up to the total or past it (the clamp)
        if B > 2:
            r[B // 2] = 0.0
        rd = torch.from_numpy(r).cuda()
        want_idx, want_prob = REF.per_sample(prio, r, B)
        idx, prob = _hip_draw(pd, rd, B)
        idx2, prob2 = _hip_draw(pd, rd, B)
        assert np.array_equal(idx.cpu().numpy(), want_idx), (count, B)
        assert np.array_equal(prob.cpu().numpy().view(np.uint64), want_prob.view(np.uint64)), (count, B)
        assert torch.equal(idx, idx2) and torch.equal(prob.view(torch.int64), prob2.view(torch.int64))
        assert int(idx[-1]) == count - 1 and (B == 1 or int(idx[0]) == 0)


@pytest.mark.parametrize("count", [1, 23, 70001])
def test_per_draw_equals_sample_where_every_sum_is_exact(count):
    """The dyadic priorities of tests/test_replay_batch.py on a device ring: sample_indices(hip=True) and sample with
    the same seed give the same idx and the same weights, bit for bit."""
    from datou_gomoku_muzero_amd import replay as RP, trainer as T
    cfg = T.TrainConfig(BOARD_SIZE=5, NUM_UNROLL_STEPS=1, TRAIN_BUFFER_SIZE=count + 11, ENABLE_PER=True)
    rb = RP.ReplayBuffer(cfg, device="cuda")
    rb.count = count
    rb.prio[:count] = torch.from_numpy(REF.dyadic_priorities(count, np.random.RandomState(count))).cuda()
    for B in (1, 7, 360):
        if B > count:
            assert rb.sample_indices(B, np.random.RandomState(0), hip=True) is None
            continue
        r1, r2 = np.random.RandomState(B), np.random.RandomState(B)
        _, idx, w = rb.sample(B, r1)
        hidx, hw = rb.sample_indices(B, r2, hip=True)
        assert hidx.dtype == torch.int64 and torch.equal(hidx, idx)
        assert hw.dtype == torch.float32 and torch.equal(hw, w)
        assert r1.random_sample() == r2.random_sample()  # the same RNG stream afterwards
        tidx, tw = rb.sample_indices(B, np.random.RandomState(B))  # the torch half, on the device
        assert torch.equal(tidx, idx) and torch.equal(tw, w)


def _state_dict(cfg, seed):
    """One set of initial weights for every trainer of a comparison (numpy, as Trainer(state_dict=...) takes them)."""
    from datou_gomoku_muzero_amd import trainer as T
    torch.manual_seed(seed)
    return {k: v.detach().cpu().numpy() for k, v in T.TrainNet(cfg).state_dict().items()}


def _trainer_and_ring(per, seed=0, H=9, B=16, blocks=2, warmup=2):
    from datou_gomoku_muzero_amd import replay as RP, trainer as T, weights as W
    cfg = T.TrainConfig(BOARD_SIZE=H, NUM_RES_BLOCKS=blocks, PHYSICAL_BATCH_SIZE=B, TRAIN_BUFFER_SIZE=200,
                        ENABLE_PER=per, LEARNING_RATE=1e-3)
    sd = _state_dict(cfg, 5)
    torch.manual_seed(seed)
    tr = T.Trainer(cfg, device="cuda", state_dict=sd, graph_warmup=warmup)
    rb = RP.ReplayBuffer(cfg, device="cuda")
    rb.add_arrays(*W.synthetic_slices(150, H, cfg.NUM_UNROLL_STEPS, np.random.RandomState(9)))
    if per:  # unequal priorities from the start
        rb.prio[:150] = torch.from_numpy(np.random.RandomState(2).uniform(0.05, 2.0, 150).astype(np.float32)).cuda()
    return tr, rb


def _state(tr):
    ps = [p.detach().clone() for p in tr.model.parameters()] + [p.detach().clone() for p in tr.target.parameters()]
    ps += [b.detach().clone() for b in tr.model.buffers()]
    for p in tr.params:
        st = tr.opt.state[p]
        ps += [st["exp_avg"].detach().clone(), st["exp_avg_sq"].detach().clone()]
    return ps


def _run(per, modes):
    """``modes``: per step, "torch" = sample_indices(hip=True) + torch indexing + Trainer.step, "hip" = step_from."""
    tr, rb = _trainer_and_ring(per)
    rng = np.random.RandomState(21)
    np.random.seed(33)
    out = []
    for mode in modes:
        if mode == "torch":
            idx, w = rb.sample_indices(tr.cfg.PHYSICAL_BATCH_SIZE, rng, hip=True)
            batch = (rb.obs[idx].float(), rb.act[idx], rb.rew[idx], rb.pol[idx], rb.val[idx])
            logs, td = tr.step(batch, w)
        else:
            logs, td, idx = tr.step_from(rb, rng)
        rb.update_priorities(idx, td)
        out.append((idx.clone(), td.clone(), logs))
    torch.cuda.synchronize()
    assert tr._graphs is not None, "the steps did not cross the capture"
    return out, _state(tr), rb.prio.clone(), np.random.get_state()[1].copy()


def _assert_same_runs(a, b):
    (sa, pa, ra, na), (sb, pb, rb_, nb) = a, b
    for i, ((ia, ta, la), (ib, tb, lb)) in enumerate(zip(sa, sb)):
        assert torch.equal(ia, ib), "idx of step %d" % i
        assert torch.equal(ta, tb), "td of step %d" % i
        assert len(la) == len(lb) == 5 and la == lb, ("logs of step %d" % i, la, lb)
    assert len(pa) == len(pb) and all(torch.equal(x, y) for x, y in zip(pa, pb)), "parameters or Adam moments"
    assert torch.equal(ra, rb_), "ring priorities"
    assert np.array_equal(na, nb), "numpy's global stream"


@pytest.fixture(scope="module")
def torch_runs():
    return {per: _run(per, ["torch"] * 4) for per in (True, False)}


@pytest.mark.parametrize("per", [True, False])
def test_step_from_equals_sample_and_step(per, torch_runs):
    """Two eager steps, the capture and two replays: the same idx, td, logs, parameters, Adam moments and ring
    priorities as torch indexing + Trainer.step from the same seeds."""
    _assert_same_runs(torch_runs[per], _run(per, ["hip"] * 4))


def test_step_and_step_from_mix_on_one_trainer(torch_runs):
    _assert_same_runs(torch_runs[True], _run(True, ["hip", "torch", "hip", "torch"]))
    _assert_same_runs(torch_runs[True], _run(True, ["torch", "hip", "torch", "hip"]))


def test_step_from_returns_none_without_a_batch():
    tr, rb = _trainer_and_ring(True)
    rb.count = 15
    rng = np.random.RandomState(0)
    before = rng.get_state()[1].copy()
    assert tr.step_from(rb, rng) is None and tr.step_count == 0
    assert np.array_equal(rng.get_state()[1], before)


def test_c4_loop_with_device_batches_equals_the_default():
    """C4Loop(device_batches=True) beside the default on test_loop.py's scripted self-play source, PER off (both
    paths draw the same host permutation): identical stats and trainer parameters; and the construction errors."""
    from test_loop import _ScriptedSelfPlay
    from datou_gomoku_muzero_amd import loop as LP, replay as RP, trainer as T
    cfg = T.TrainConfig(BOARD_SIZE=6, NUM_RES_BLOCKS=1, PHYSICAL_BATCH_SIZE=8, TRAIN_BUFFER_SIZE=512, ENABLE_PER=False)
    sd = _state_dict(cfg, 3)
    runs = []
    for dev_batches in (False, True):
        torch.manual_seed(0)
        np.random.seed(5)
        tr = T.Trainer(cfg, device="cuda", state_dict=sd, graph_warmup=2)
        rb = RP.ReplayBuffer(cfg, device="cuda")
        lp = LP.C4Loop(_ScriptedSelfPlay(100), tr, rb, cfg, 8, moves_per_iter=2, train_steps_per_iter=1,
                       model_update_interval=3, seed=7, device_batches=dev_batches)
        assert lp.device_batches is dev_batches
        st = lp.run(8)
        torch.cuda.synchronize()
        runs.append((st, [p.detach().clone() for p in tr.model.parameters()], lp.last_logs.clone()))
    (s0, p0, l0), (s1, p1, l1) = runs
    assert s0 == s1 and s0["train_steps"] >= 4 and s0["weight_pushes"] >= 1
    assert all(torch.equal(x, y) for x, y in zip(p0, p1)) and torch.equal(l0, l1)
    cpu_rb = RP.ReplayBuffer(cfg, device="cpu")
    with pytest.raises(ValueError, match="device-resident"):
        LP.C4Loop(_ScriptedSelfPlay(1), tr, cpu_rb, cfg, 8, device_batches=True)
    with pytest.raises(ValueError, match="PHYSICAL_BATCH_SIZE"):
        LP.C4Loop(_ScriptedSelfPlay(1), tr, rb, cfg, 4, device_batches=True)
