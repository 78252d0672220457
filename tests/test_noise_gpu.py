"""The device Gumbel noise against its model (tests/noise_ref.py, whose properties tests/test_noise.py states).

  1. gmz_gumbel_keyed (k_gumbel_keyed) equals noise_ref.noise_ld to |d| <= 2^-51 (1 + |ref|) at every (seed, ply, key,
     action) tried, writes G * A doubles and nothing else, and is deterministic.  The bound is derived, not measured:
     1 - u is exact; a log good to 1 ulp leaves a relative 2^-52 on v = -log(1 - u), which the outer log turns into an
     absolute 2^-52, and adds a relative 2^-52 of its own: 2^-52 (1 + |ref|), and a factor 2 of margin.  One flipped
     bit of the hash above its lowest moves a sample by at least e 2^-52, so the bound pins the hash itself.
  2. search(gumbel=None) (k_begin_move's own noise) is that function of key = game + game_offset and counter = the
     engine's begin_move calls so far, whether or not a call brought noise of its own."""
import numpy as np
import pytest

import noise_ref as NR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEEDS = (0, 5, 1 << 32, (1 << 64) - 1, 0xDEADBEEF12345678)
U32 = (1 << 32) - 1
# (key, ply) rows: the corners of both ranges, and rows apart in one argument only
ROWS7 = ((0, 0), (1, 1), (1 << 31, 511), (U32, U32), (0, U32), (U32, 0), (12345, 1))


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import datou_gomoku_muzero_amd._lib as L
    import datou_gomoku_muzero_amd.engine as E
    return dict(L=L, E=E, lib=L.load())


def _u32(values):
    """uint32 values as the int32 tensor of the same bits."""
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def _keyed(m, keys, plies, seed, A, out=None):
    L = m["L"]
    G = len(keys)
    if out is None:
        out = torch.empty(G, A, dtype=torch.float64, device="cuda")
    k, p = _u32(keys), _u32(plies)
    L.check(m["lib"].gmz_gumbel_keyed(L.ptr(k), L.ptr(p), seed, G, A, L.ptr(out), G * A * 8, L.stream_ptr()))
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------ 1. gmz_gumbel_keyed
@pytest.mark.parametrize("A", [1, 25, 225, 361, 484, 512])
@pytest.mark.parametrize("G", [1, 7])
def test_gumbel_keyed_matches_the_model(mods, A, G):
    """Observed on an MI355X: the largest |device - noise_ld| over the twelve shapes is 0.249 of the bound, i.e.
    0.50 * 2^-52 (1 + |ref|) (0.167 at A = 1, G = 1; 0.244-0.249 from A = 225 on)."""
    GUARD = 64
    sentinel = -1234.5
    worst = 0.0
    row_sets = [ROWS7] if G == 7 else [(r,) for r in ROWS7[:4]]
    for seed in SEEDS:
        for rows in row_sets:
            keys, plies = [r[0] for r in rows], [r[1] for r in rows]
            buf = torch.full((G * A + GUARD,), sentinel, dtype=torch.float64, device="cuda")
            out = _keyed(mods, keys, plies, seed, A, buf[:G * A].view(G, A))
            got = buf.cpu().numpy()
            assert (got[G * A:] == sentinel).all()  # G * A doubles and nothing after them
            got = got[:G * A].reshape(G, A)
            assert np.isfinite(got).all() and not (got == sentinel).any()
            ref = NR.rows(seed, plies, keys, A, NR.noise_ld)
            ratio = float(np.max(np.abs(got.astype(np.longdouble) - ref) / (1 + np.abs(ref)))) / 2.0 ** -51
            worst = max(worst, ratio)
            assert ratio <= 1.0, (seed, rows, ratio)
            again = _keyed(mods, keys, plies, seed, A)
            assert torch.equal(again.view(torch.int64), out.view(torch.int64))  # bit-identical
    print("A %d G %d: largest |device - model| = %.3f * 2^-51 (1 + |ref|)" % (A, G, worst))


# ------------------------------------------------------------------------------------------ 2. k_begin_move
SIMS, G6, SEED, MOVES = 16, 6, 5, 3


def _engine(m, size, seed=SEED, offset=0):
    e = m["E"].BatchedSelfPlayEngine(None, num_games=G6, BOARD_SIZE=size, NUM_SIMULATIONS=SIMS,
                                     MCTS_IMPLEMENTATION="MuZero", seed=seed, game_offset=offset)
    e.reset_games()
    return e


def _search(eng, gumbel=None):
    pol, val, act = eng.search(gumbel=gumbel)
    out = [pol, val, act] + list(eng.root_stats())
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in out]


@pytest.mark.parametrize("size", [5, 15, 22])  # A < 64, the flagship, NJ = 8
@pytest.mark.parametrize("offset", [0, 3])
def test_begin_move_draws_the_keyed_noise(mods, size, offset):
    """Three moves of four engines on the same games: device noise; the keyed kernel's rows for (key = offset + g,
    ply = move) fed as gumbel= (everything bit for bit); the numpy model fed as gumbel= (actions and visit counts);
    and device noise with the middle move fed explicitly, which must still count as a move."""
    m = mods
    A = size * size
    dev, twin, model, mixed = (_engine(m, size, offset=offset) for _ in range(4))
    keys = offset + np.arange(G6)
    first = None
    for move in range(MOVES):
        K = _keyed(m, keys, [move] * G6, SEED, A)
        want = _search(dev)
        got = _search(twin, K)
        for a, b in zip(want, got):  # policy, value, action, visits, root N, root W, min-max bounds
            assert np.array_equal(a, b), (move,)
        ref = _search(model, NR.rows(SEED, [move] * G6, keys, A))
        assert np.array_equal(ref[2], want[2]) and np.array_equal(ref[3], want[3]), (move,)
        got = _search(mixed, K if move == 1 else None)
        for a, b in zip(want, got):
            assert np.array_equal(a, b), (move,)
        assert (want[2] >= 0).all() and want[3].sum(axis=1).min() > 0
        first = want[2] if first is None else first
        for e in (dev, twin, model, mixed):
            st = e.play().cpu().numpy()
            assert (st == 2).all()  # nobody finishes in three moves
    # the same (seed, key, ply) on the same position is the same search, whichever engine holds the game
    other = _engine(m, size, offset=3 - offset)
    act = _search(other)[2]
    if offset == 0:
        assert np.array_equal(first[3:], act[:3])
    else:
        assert np.array_equal(first[:3], act[3:])
    # another offset or another seed plays something else somewhere
    assert not np.array_equal(first, act)
    reseeded = _engine(m, size, seed=SEED + 1, offset=offset)
    assert not np.array_equal(first, _search(reseeded)[2])
    for e in (dev, twin, model, mixed, other, reseeded):
        assert e.errors() == 0
        e.close()
