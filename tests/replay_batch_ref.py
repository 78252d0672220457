"""numpy restatement of gmz_replay_per_sample (csrc/gmz_replay.hip) in the summation order its header states.  Not a
test: tests/test_replay_batch.py and tests/test_replay_batch_gpu.py import it.

Every sum runs left to right in f64: np.add.accumulate along an axis is out[i] = out[i-1] + in[i], one rounded
addition per element, not numpy's pairwise np.sum.
  groups of 16 elements   w[g][e] = p[16g] + ... + p[16g+e],  l[g] = w[g][15]
  chunks of 64 groups     S[c] = l[64c] + ... + l[64c+63]
  chunk prefix            T[c] = S[0] + ... + S[c],  total = T[last]
  bases                   b[c][0] = T[c-1] (0.0 for c = 0),  b[c][t+1] = b[c][t] + l[64c+t]
  cum[1024c + 16t + e]    = min(b[c][t] + w[64c+t][e], T[c]);  = T[c] at the chunk's last element below count
Elements past count are 0.0 (x + 0.0 == x, so padding changes no sum)."""
import numpy as np

GROUP, GROUPS = 16, 64
CHUNK = GROUP * GROUPS


def per_cum(prio):
    """(cum f64 [count], total) of f32 priorities ``prio`` in the kernel's order."""
    prio = np.asarray(prio)
    assert prio.dtype == np.float32 and prio.ndim == 1 and prio.size >= 1
    count = prio.size
    nchunks = -(-count // CHUNK)
    p = np.zeros(nchunks * CHUNK, np.float64)
    p[:count] = prio.astype(np.float64)
    w = np.add.accumulate(p.reshape(nchunks, GROUPS, GROUP), axis=2)
    l = w[:, :, GROUP - 1]                                     # [nchunks, 64]
    S = np.add.accumulate(l, axis=1)[:, GROUPS - 1]
    T = np.add.accumulate(S)
    Tprev = np.concatenate([np.zeros(1), T[:-1]])
    b = np.add.accumulate(np.concatenate([Tprev[:, None], l], axis=1), axis=1)[:, :GROUPS]   # b[c][t]
    cum = np.minimum(b[:, :, None] + w, T[:, None, None]).reshape(-1)[:count].copy()
    last = np.minimum((np.arange(nchunks) + 1) * CHUNK, count) - 1
    cum[last] = T
    assert (np.diff(cum) >= 0).all(), "cum must be non-decreasing for priorities >= 0"
    return cum, T[-1]


def per_sample(prio, r, B):
    """(idx int64 [B], prob f64 [B]) for the host uniforms ``r`` (f64 [B])."""
    prio = np.asarray(prio)
    r = np.asarray(r, np.float64)
    assert r.shape == (B,)
    cum, total = per_cum(prio)
    u = (np.arange(B, dtype=np.float64) + r) * (total / np.float64(B))
    idx = np.minimum(np.searchsorted(cum, u, side="left"), prio.size - 1).astype(np.int64)  # first j: cum[j] >= u
    prob = prio[idx].astype(np.float64) / total
    return idx, prob


def dyadic_priorities(count, rs):
    """f32 priorities that are multiples of 2^-8 in (0, 64): every f64 partial sum of up to 2^20 of them is exact
    (below 2^26 with 8 fraction bits), whatever the order."""
    return (rs.randint(1, 64 * 256, size=count).astype(np.float64) / 256.0).astype(np.float32)
