"""The replay entry points' refusals, word for word, without a GPU: every refusal branch of gmz_replay_ingest,
gmz_replay_positions, gmz_replay_rewrite, gmz_replay_gather and gmz_replay_per_sample (with its _workspace_bytes) is
hit once with fake pointers (every call stops at a check, nothing is launched) and gmz_last_error() is compared to the
text recorded from the library.  Callers and tools match on these texts; a change to the host validation keeps them."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

FAKE = ctypes.c_void_p(1 << 20)
PW = (ctypes.c_double * 34)(*[0.997 ** i for i in range(34)])
GOOD_INGEST = [0, 0, 0, 9, 1, 0, 0, 0]  # game, bank, row0, n, winner, drop, slot, first
GOOD_REWRITE = [5, 9, 9, 0, 1, 0]       # slot, kept, n, drop, winner, first
GOOD_ROWS = [[3, 0], [99, 35]]          # slot, move count


def _table(rows, cols):
    tab = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, cols))
    return tab, ctypes.c_void_p(tab.ctypes.data)


def _ingest(lib, jobs=(GOOD_INGEST,), H=6, U=5, n_steps=10, G=4, L=36, N=100, n_jobs=None, host=True, dev=FAKE, pw=PW,
            hist=(FAKE,) * 6, ring=(FAKE,) * 6, short=0):
    tab, p = _table(jobs, 8)
    return lib.gmz_replay_ingest(H, U, n_steps, G, L, *hist, *ring, N, p if host else None,
                                 len(tab) if n_jobs is None else n_jobs, dev, tab.nbytes - short, pw, None, None)


def _positions(lib, rows=GOOD_ROWS, H=6, U=5, N=100, G=16, P=None, ring=FAKE, host=True, dev=FAKE, outs=(FAKE,) * 4,
               short=None):
    tab, p = _table(rows, 2)
    A = H * H
    caps = dict(ring=N * (U + 1) * 3 * A, rows=tab.nbytes, board=G * A, player=G, last=4 * G, count=4 * G)
    if short:
        caps[short] -= 1
    return lib.gmz_replay_positions(H, U, N, ring, caps["ring"], p if host else None, len(tab) if P is None else P, dev,
                                    caps["rows"], G, outs[0], caps["board"], outs[1], caps["player"], outs[2],
                                    caps["last"], outs[3], caps["count"], None)


def _rewrite(lib, jobs=(GOOD_REWRITE,), H=6, U=5, n_steps=10, N=100, P=50, n_jobs=None, host=True, dev=FAKE, pw=PW,
             ptrs=(FAKE,) * 4, short=None):
    tab, p = _table(jobs, 6)
    A = H * H
    caps = dict(ring_pol=N * (U + 1) * A * 4, ring_val=N * (U + 1) * 4, pol_new=max(P, 0) * A * 8, val_new=max(P, 0) * 4,
                jobs=tab.nbytes)
    if short:
        caps[short] -= 1
    return lib.gmz_replay_rewrite(H, U, n_steps, N, ptrs[0], caps["ring_pol"], ptrs[1], caps["ring_val"], ptrs[2],
                                  caps["pol_new"], ptrs[3], caps["val_new"], P, p if host else None,
                                  len(tab) if n_jobs is None else n_jobs, dev, caps["jobs"], pw, None)


def _gather(lib, H=6, U=5, N=100, count=50, B=7, k=1, flip=1, ring=(FAKE,) * 5, idx=FAKE, outs=(FAKE,) * 7, short=None):
    A = H * H
    need = [B * (U + 1) * 3 * A * 4, B * U * 8, B * U * 4, B * (U + 1) * A * 4, B * (U + 1) * 4, B * U * 8, B * 4]
    sized = []
    for i, (p, n) in enumerate(zip(outs, need)):
        sized += [p, max(n, 0) - (1 if i == short else 0)]
    return lib.gmz_replay_gather(H, U, N, count, B, *ring, idx, None, k, flip, *sized, None)


def _ws_bytes(lib, count=1000, B=7, out=True):
    need = ctypes.c_size_t()
    return lib.gmz_replay_per_sample_workspace_bytes(count, B, ctypes.byref(need) if out else None)


def _draw(lib, count=1000, B=7, prio=FAKE, r=FAKE, idx=FAKE, prob=FAKE, ws=FAKE, ws_short=0, idx_short=0, prob_short=0):
    need = ctypes.c_size_t()
    assert lib.gmz_replay_per_sample_workspace_bytes(max(count, 1), max(B, 1), ctypes.byref(need)) == 0
    return lib.gmz_replay_per_sample(prio, r, count, B, idx, max(B, 0) * 8 - idx_short, prob, max(B, 0) * 8 - prob_short,
                                     ws, need.value - ws_short, None)


def _none_at(i, n):
    return tuple(None if j == i else FAKE for j in range(n))


CASES = [
    # ---- gmz_replay_ingest
    (_ingest, dict(H=4), "gmz_replay_ingest: board_size 4 outside 5..22"),
    (_ingest, dict(H=23), "gmz_replay_ingest: board_size 23 outside 5..22"),
    (_ingest, dict(U=0), "gmz_replay_ingest: unroll 0 < 1"),
    (_ingest, dict(n_steps=0), "gmz_replay_ingest: n_steps 0 outside 1..32"),
    (_ingest, dict(n_steps=33), "gmz_replay_ingest: n_steps 33 outside 1..32"),
    (_ingest, dict(G=0), "gmz_replay_ingest: G, L and N must be positive"),
    (_ingest, dict(L=0), "gmz_replay_ingest: G, L and N must be positive"),
    (_ingest, dict(N=0), "gmz_replay_ingest: G, L and N must be positive"),
    (_ingest, dict(n_jobs=-1), "gmz_replay_ingest: n_jobs < 0"),
    (_ingest, dict(host=False), "gmz_replay_ingest: jobs_host, jobs_dev or discount_pow is NULL"),
    (_ingest, dict(dev=None), "gmz_replay_ingest: jobs_host, jobs_dev or discount_pow is NULL"),
    (_ingest, dict(pw=None), "gmz_replay_ingest: jobs_host, jobs_dev or discount_pow is NULL"),
    (_ingest, dict(hist=_none_at(3, 6)), "gmz_replay_ingest: a history or ring pointer is NULL"),
    (_ingest, dict(ring=_none_at(5, 6)), "gmz_replay_ingest: a history or ring pointer is NULL"),
    (_ingest, dict(jobs=[GOOD_INGEST, [1, 0, 0, 9, 1, 0, 9, 9]], short=32),
     "gmz_replay_ingest: device job table of 32 bytes is short of 2 jobs x 32"),
    (_ingest, dict(jobs=[[4, 0, 0, 9, 1, 0, 0, 0]]), "gmz_replay_ingest: job 0: game 4 outside 0..3"),
    (_ingest, dict(jobs=[[0, 2, 0, 9, 1, 0, 0, 0]]), "gmz_replay_ingest: job 0: bank 2 is neither 0 nor 1"),
    (_ingest, dict(jobs=[[0, 0, 30, 7, 1, 0, 0, 0]]), "gmz_replay_ingest: job 0: rows 30+7 pass the history's L = 36"),
    (_ingest, dict(jobs=[[0, 0, 0, 9, 2, 0, 0, 0]]), "gmz_replay_ingest: job 0: winner 2 outside -1..1"),
    (_ingest, dict(jobs=[[0, 0, 0, 9, 1, 9, 0, 0]]), "gmz_replay_ingest: job 0: drop 9 outside 0..n-1"),
    (_ingest, dict(jobs=[[0, 0, 0, 9, 1, 0, 100, 0]]), "gmz_replay_ingest: job 0: ring slot 100 outside 0..99"),
    (_ingest, dict(jobs=[GOOD_INGEST, [1, 0, 0, 9, 1, 0, 9, 8]]),
     "gmz_replay_ingest: job 1: first 8 is not the kept slices before it"),
    (_ingest, dict(jobs=[[0, 0, 0, 30, 1, 0, 0, 0], [1, 0, 0, 30, 1, 0, 30, 30]], N=50),
     "gmz_replay_ingest: the launch keeps more than the ring's N = 50 slices"),
    (_ingest, dict(jobs=[[0, 0, 0, 9, 1, 0, 5, 0], [1, 0, 0, 14, 1, 0, 95, 9]]),
     "gmz_replay_ingest: kept slices of two jobs overlap at ring slot 5"),
    # ---- gmz_replay_positions
    (_positions, dict(H=4), "gmz_replay_positions: board_size 4 outside 5..22"),
    (_positions, dict(H=23), "gmz_replay_positions: board_size 23 outside 5..22"),
    (_positions, dict(U=0), "gmz_replay_positions: unroll 0 < 1"),
    (_positions, dict(N=0), "gmz_replay_positions: N 0 < 1"),
    (_positions, dict(G=0), "gmz_replay_positions: G 0 < 1"),
    (_positions, dict(P=0), "gmz_replay_positions: P 0 outside 1..G = 16"),
    (_positions, dict(rows=[[0, 0]] * 17), "gmz_replay_positions: P 17 outside 1..G = 16"),
    (_positions, dict(ring=None), "gmz_replay_positions: ring_obs_dev, rows_host or rows_dev is NULL"),
    (_positions, dict(host=False), "gmz_replay_positions: ring_obs_dev, rows_host or rows_dev is NULL"),
    (_positions, dict(dev=None), "gmz_replay_positions: ring_obs_dev, rows_host or rows_dev is NULL"),
    (_positions, dict(outs=_none_at(2, 4)), "gmz_replay_positions: an output pointer is NULL"),
    (_positions, dict(short="ring"), "gmz_replay_positions: ring_obs of 64799 bytes is short of 64800"),
    (_positions, dict(short="rows"), "gmz_replay_positions: device row table of 15 bytes is short of 16"),
    (_positions, dict(short="board"), "gmz_replay_positions: board_out of 575 bytes is short of 576"),
    (_positions, dict(short="player"), "gmz_replay_positions: player_out of 15 bytes is short of 16"),
    (_positions, dict(short="last"), "gmz_replay_positions: last_out of 63 bytes is short of 64"),
    (_positions, dict(short="count"), "gmz_replay_positions: count_out of 63 bytes is short of 64"),
    (_positions, dict(rows=[[3, 0], [100, 0]]), "gmz_replay_positions: row 1: ring slot 100 outside 0..99"),
    (_positions, dict(rows=[[0, 36]]), "gmz_replay_positions: row 0: move count 36 outside 0..35"),
    # ---- gmz_replay_rewrite
    (_rewrite, dict(H=4), "gmz_replay_rewrite: board_size 4 outside 5..22"),
    (_rewrite, dict(H=23), "gmz_replay_rewrite: board_size 23 outside 5..22"),
    (_rewrite, dict(U=0), "gmz_replay_rewrite: unroll 0 < 1"),
    (_rewrite, dict(n_steps=0), "gmz_replay_rewrite: n_steps 0 outside 1..32"),
    (_rewrite, dict(n_steps=33), "gmz_replay_rewrite: n_steps 33 outside 1..32"),
    (_rewrite, dict(N=0), "gmz_replay_rewrite: N 0 < 1"),
    (_rewrite, dict(P=-1), "gmz_replay_rewrite: P -1 < 0"),
    (_rewrite, dict(n_jobs=-1), "gmz_replay_rewrite: n_jobs < 0"),
    (_rewrite, dict(host=False), "gmz_replay_rewrite: jobs_host, jobs_dev or discount_pow is NULL"),
    (_rewrite, dict(dev=None), "gmz_replay_rewrite: jobs_host, jobs_dev or discount_pow is NULL"),
    (_rewrite, dict(pw=None), "gmz_replay_rewrite: jobs_host, jobs_dev or discount_pow is NULL"),
    (_rewrite, dict(ptrs=_none_at(1, 4)), "gmz_replay_rewrite: a ring or staging pointer is NULL"),
    (_rewrite, dict(short="ring_pol"), "gmz_replay_rewrite: ring_pol of 86399 bytes is short of 86400"),
    (_rewrite, dict(short="ring_val"), "gmz_replay_rewrite: ring_val of 2399 bytes is short of 2400"),
    (_rewrite, dict(short="pol_new"), "gmz_replay_rewrite: pol_new of 14399 bytes is short of 14400"),
    (_rewrite, dict(short="val_new"), "gmz_replay_rewrite: val_new of 199 bytes is short of 200"),
    (_rewrite, dict(short="jobs"), "gmz_replay_rewrite: device job table of 23 bytes is short of 24"),
    (_rewrite, dict(jobs=[[100, 9, 9, 0, 1, 0]]), "gmz_replay_rewrite: job 0: ring slot 100 outside 0..99"),
    (_rewrite, dict(jobs=[[5, 0, 9, 9, 1, 0]]), "gmz_replay_rewrite: job 0: kept 0 < 1"),
    (_rewrite, dict(jobs=[[5, 21, 30, 9, 1, 0]], N=20), "gmz_replay_rewrite: job 0: kept 21 passes the ring's N = 20"),
    (_rewrite, dict(jobs=[[5, 9, 12, 2, 1, 0]]), "gmz_replay_rewrite: job 0: n 12, drop 2, kept 9: drop is not n - kept"),
    (_rewrite, dict(jobs=[[5, 9, 9, 0, 2, 0]]), "gmz_replay_rewrite: job 0: winner 2 outside -1..1"),
    (_rewrite, dict(jobs=[GOOD_REWRITE, [20, 4, 4, 0, 0, 8]]),
     "gmz_replay_rewrite: job 1: first 8 is not the staged rows before it"),
    (_rewrite, dict(jobs=[GOOD_REWRITE, [20, 4, 4, 0, 0, 9]], P=12),
     "gmz_replay_rewrite: job 1: staged row 12 outside 0..11"),
    (_rewrite, dict(jobs=[[95, 9, 11, 2, -1, 0], [3, 4, 4, 0, 0, 9]]),
     "gmz_replay_rewrite: the slices of two jobs overlap at ring slot 3"),
    # ---- gmz_replay_gather
    (_gather, dict(H=4), "gmz_replay_gather: board_size 4 outside 5..22"),
    (_gather, dict(H=23), "gmz_replay_gather: board_size 23 outside 5..22"),
    (_gather, dict(U=0), "gmz_replay_gather: unroll 0 < 1"),
    (_gather, dict(B=0), "gmz_replay_gather: B 0 < 1"),
    (_gather, dict(N=0, count=0), "gmz_replay_gather: N 0 < 1"),
    (_gather, dict(count=0), "gmz_replay_gather: count 0 outside 1..N = 100"),
    (_gather, dict(count=101), "gmz_replay_gather: count 101 outside 1..N = 100"),
    (_gather, dict(k=4), "gmz_replay_gather: k 4 outside 0..3"),
    (_gather, dict(flip=2), "gmz_replay_gather: flip 2 is neither 0 nor 1"),
    (_gather, dict(ring=_none_at(4, 5)), "gmz_replay_gather: a ring pointer is NULL"),
    (_gather, dict(idx=None), "gmz_replay_gather: idx_dev is NULL"),
    (_gather, dict(outs=_none_at(6, 7)), "gmz_replay_gather: an output pointer is NULL"),
    (_gather, dict(B=2 ** 31 - 1, U=1), "gmz_replay_gather: B * (unroll + 1) = 4294967294 passes one launch's grid"),
    (_gather, dict(short=0), "gmz_replay_gather: obs_out of 18143 bytes is short of 18144"),
    (_gather, dict(short=1), "gmz_replay_gather: act_out of 279 bytes is short of 280"),
    (_gather, dict(short=2), "gmz_replay_gather: rew_out of 139 bytes is short of 140"),
    (_gather, dict(short=3), "gmz_replay_gather: pol_out of 6047 bytes is short of 6048"),
    (_gather, dict(short=4), "gmz_replay_gather: val_out of 167 bytes is short of 168"),
    (_gather, dict(short=5), "gmz_replay_gather: act_aug_out of 279 bytes is short of 280"),
    (_gather, dict(short=6), "gmz_replay_gather: w_out of 27 bytes is short of 28"),
    # ---- gmz_replay_per_sample_workspace_bytes, gmz_replay_per_sample
    (_ws_bytes, dict(count=0), "gmz_replay_per_sample_workspace_bytes: count 0 < 1"),
    (_ws_bytes, dict(B=0), "gmz_replay_per_sample_workspace_bytes: B 0 < 1"),
    (_ws_bytes, dict(out=False), "gmz_replay_per_sample_workspace_bytes: out is NULL"),
    (_draw, dict(count=0), "gmz_replay_per_sample: count 0 < 1"),
    (_draw, dict(B=0), "gmz_replay_per_sample: B 0 < 1"),
    (_draw, dict(prio=None), "gmz_replay_per_sample: prio_dev is NULL"),
    (_draw, dict(r=None), "gmz_replay_per_sample: r_dev is NULL"),
    (_draw, dict(idx=None), "gmz_replay_per_sample: idx_dev is NULL"),
    (_draw, dict(prob=None), "gmz_replay_per_sample: prob_dev is NULL"),
    (_draw, dict(ws=None), "gmz_replay_per_sample: workspace_dev is NULL"),
    (_draw, dict(ws=ctypes.c_void_p((1 << 20) + 4)), "gmz_replay_per_sample: workspace_dev is not 8-byte aligned"),
    (_draw, dict(ws_short=8),
     "gmz_replay_per_sample: workspace of 504 bytes is short of 512 (gmz_replay_per_sample_workspace_bytes)"),
    (_draw, dict(idx_short=1), "gmz_replay_per_sample: idx of 55 bytes is short of 56"),
    (_draw, dict(prob_short=1), "gmz_replay_per_sample: prob of 55 bytes is short of 56"),
]


def test_every_replay_refusal_keeps_its_text():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    wrong = []
    for fn, kw, want in CASES:
        rc = fn(lib, **kw)
        text = lib.gmz_last_error().decode()
        if rc >= 0 or text != want:
            wrong.append((fn.__name__, sorted(kw), rc, text, want))
    assert not wrong, wrong
    assert {c[0] for c in CASES} == {_ingest, _positions, _rewrite, _gather, _ws_bytes, _draw}
