"""ReplayBuffer.add on a CPU ring: the slices' fields land in the ring as numpy's stacked astype of them, bit for bit, at
(ptr + i) mod N, with the admission priority beside them; the second append wraps."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

N, U, H = 16, 5, 6
A = H * H


def _slices(rs, n):
    """TrainingSlice-like objects whose float64 policies and values are not representable in float32."""
    out = []
    for _ in range(n):
        pol = rs.dirichlet(np.full(A, 0.3), U + 1)
        val = rs.uniform(-1, 1, U + 1)
        assert pol.dtype == val.dtype == np.float64
        assert (pol.astype(np.float32).astype(np.float64) != pol).any()
        assert (val.astype(np.float32).astype(np.float64) != val).all()
        out.append(SimpleNamespace(observation=rs.randint(0, 2, (U + 1, 3, H, H)).astype(np.float32),
                                   action_history=[int(a) for a in rs.randint(-1, A, U)],
                                   reward_history=list(rs.choice([-1.0, 0.0, 1.0], U)),
                                   policy_history=pol, value_history=val))
    return out


@pytest.mark.parametrize("per,max_priority", [(True, 0.1), (False, 1.0)])
def test_add_writes_the_stacked_astype_of_every_field(per, max_priority):
    from datou_gomoku_muzero_amd import trainer as T
    cfg = T.TrainConfig(BOARD_SIZE=H, NUM_UNROLL_STEPS=U, TRAIN_BUFFER_SIZE=N, ENABLE_PER=per)
    rb = T.ReplayBuffer(cfg, device="cpu")
    rb.max_priority = max_priority
    rs = np.random.RandomState(11)
    fields = (("obs", "observation", np.uint8), ("act", "action_history", np.int32), ("rew", "reward_history", np.float32),
              ("pol", "policy_history", np.float32), ("val", "value_history", np.float32))
    want = {name: np.zeros(tuple(getattr(rb, name).shape), dt) for name, _, dt in fields}
    want["prio"] = np.zeros(N, np.float32)
    ptr = count = 0
    rb.add([])
    assert (rb.ptr, rb.count) == (0, 0)
    for n in (10, 9):  # the second append wraps: slots 10..15, then 0..2
        slices = _slices(rs, n)
        rb.add(slices)
        idx = (ptr + np.arange(n)) % N
        for name, attr, dt in fields:
            want[name][idx] = np.stack([np.asarray(getattr(s, attr)) for s in slices]).astype(dt)
        want["prio"][idx] = np.float32(max_priority if per else 1.0)
        ptr, count = (ptr + n) % N, min(N, count + n)
        assert (rb.ptr, rb.count, len(rb)) == (ptr, count, count)
        for name in want:
            got = getattr(rb, name)
            assert got.dtype == torch.from_numpy(want[name]).dtype, name
            assert got.numpy().tobytes() == want[name].tobytes(), name
    assert (ptr, count) == (3, 16) and rb.games == []  # slices appended by add have no directory entry
