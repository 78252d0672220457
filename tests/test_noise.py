"""What the device Gumbel noise is (CPU only): tests/noise_ref.py restates gumbel_noise() of csrc/gmz_tree.hip, and
this file states the properties every self-play, reanalysis and arena game relies on.  The kernels are held to the
model in tests/test_noise_gpu.py.

The bounds are conditions on the generator, fixed before the model was run: a KS distance at the 0.1 % level, |z| < 4
for every mean and correlation, 1 % on the variance, and a chi-square (224 degrees of freedom, mean 224, sd 21.2)
below 300.  A value outside them is a finding about the generator."""
import numpy as np
import pytest

import noise_ref as NR

SEEDS = (0, 1, 5, 7919, 0xDEADBEEF12345678)
PLIES, KEYS, A = 32, 256, 225
N = PLIES * KEYS * A  # 1,843,200 samples per seed
EULER_GAMMA = 0.5772156649015329
VAR = np.pi ** 2 / 6
# the most games one seed ever keys: 16,384 in one process (tools/tree_microbench.py's largest engine; the bench and
# the tests stop at 8,192; SplitSelfPlayEngine's parts share one key range through game_offset), and every rank has
# a seed of its own
LARGEST_GAME_COUNT = 16384

_blocks = {}


def _block(seed):
    if seed not in _blocks:
        x = NR.block(seed, np.arange(PLIES), np.arange(KEYS), A)
        x.setflags(write=False)
        _blocks[seed] = x
    return _blocks[seed]


def _z(x, y):
    """Pearson correlation of two equally shaped sample sets times sqrt(pairs): ~N(0, 1) when they are unrelated."""
    x, y = np.ravel(x), np.ravel(y)
    return float(np.corrcoef(x, y)[0, 1] * np.sqrt(x.size))


# ------------------------------------------------------------------------------------------ the restatement itself
def test_mix32_and_bit_layout():
    """mix32 is a bijection fixing 0 (xorshift and odd multiplies only), the 53-bit word is (h2 << 21) ^ h3, and the
    float64 and long double samples are the same number to float64 rounding."""
    assert int(NR.mix32(0)) == 0
    x = np.arange(1 << 16, dtype=np.uint64) * np.uint64(65521) + np.uint64(12345)
    assert np.unique(NR.mix32(x)).size == x.size and int(NR.mix32(x).max()) < 1 << 32
    w = NR.h2(5, 3, 7, np.arange(A))
    b = NR.bits(5, 3, 7, np.arange(A))
    h3 = NR.mix32((w + np.uint64(0x1B873593)) & NR.M32)
    assert np.array_equal(b, (w << np.uint64(21)) ^ h3) and int(b.max()) < 1 << 53
    assert np.array_equal(b >> np.uint64(32), w >> np.uint64(11))  # h2's top 21 bits lead the mantissa untouched
    # the seed's halves enter separately, the counter and the key through row_word only
    assert not np.array_equal(NR.bits(5, 3, 7, np.arange(A)), NR.bits(5 << 32, 3, 7, np.arange(A)))
    assert not np.array_equal(NR.bits(5, 3, 7, np.arange(A)), NR.bits(5, 7, 3, np.arange(A)))
    assert int(NR.row_word(1, 0)) == 0x9E3779B1 and int(NR.row_word(0, 1)) == 0x85EBCA77
    assert int(NR.row_word(2 ** 32 - 1, 2 ** 32 - 1)) == (-(0x9E3779B1 + 0x85EBCA77)) % 2 ** 32
    f, ld = NR.noise(5, 3, 7, np.arange(A)), NR.noise_ld(5, 3, 7, np.arange(A))
    assert f.dtype == np.float64 and ld.dtype == np.longdouble
    assert float(np.max(np.abs(f - ld) / (1 + np.abs(ld)))) <= 2.0 ** -51


def test_zero_draw_is_guarded():
    """u = 0 would give -log(-log(1)) = +inf: the guard draws 2^-53 instead, the largest sample there is; u's
    largest value 1 - 2^-53 gives the smallest, -log(53 log 2)."""
    for ft in (np.float64, np.longdouble):
        x = NR.from_bits([0, 1, 2, (1 << 53) - 1], ft)
        assert np.isfinite(x).all() and x[0] == x[1] > x[2] > x[3]
        assert abs(float(x[0]) - 53 * np.log(2)) < 1e-9 and abs(float(x[3]) + np.log(53 * np.log(2))) < 1e-9


# ------------------------------------------------------------------------------------------ statistics of the model
@pytest.mark.parametrize("seed", SEEDS)
def test_marginal_distribution(seed):
    x = np.sort(_block(seed).ravel())
    assert np.isfinite(x).all()
    F = np.exp(-np.exp(-x))
    i = np.arange(1, N + 1, dtype=np.float64)
    ks = max(float(np.max(i / N - F)), float(np.max(F - (i - 1) / N)))
    print("seed %#x: KS*sqrt(n) %.3f" % (seed, ks * np.sqrt(N)))
    assert ks * np.sqrt(N) < 1.95
    z = (x.mean() - EULER_GAMMA) / np.sqrt(VAR / N)
    print("seed %#x: mean z %.3f, variance %.5f" % (seed, z, x.var()))
    assert abs(z) < 4
    assert abs(x.var() / VAR - 1) < 0.01


@pytest.mark.parametrize("seed", SEEDS)
def test_neighbours_are_uncorrelated(seed):
    """Adjacent actions, adjacent game keys, adjacent plies, and the same (ply, key, action) under seed + 1 (low
    word) and seed + 2^32 (high word)."""
    x = _block(seed)
    z = dict(actions=_z(x[:, :, :-1], x[:, :, 1:]), keys=_z(x[:, :-1], x[:, 1:]), plies=_z(x[:-1], x[1:]),
             seed_lo=_z(x, NR.block(seed + 1, np.arange(PLIES), np.arange(KEYS), A)),
             seed_hi=_z(x, NR.block(seed + (1 << 32), np.arange(PLIES), np.arange(KEYS), A)))
    print("seed %#x: %s" % (seed, {k: round(v, 3) for k, v in z.items()}))
    for k, v in z.items():
        assert abs(v) < 4, (k, v)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_loop_s_streams_are_uncorrelated(seed):
    """The seeds loop.py and worker.py derive from one --seed: self-play seed + 7919 * rank, reanalysis
    seed + 104729 * (rank + 1); ranks 0..3.  Every pair of self-play streams, and every reanalysis stream against
    the base seed."""
    sp = [_block(seed)] + [NR.block(seed + 7919 * r, np.arange(PLIES), np.arange(KEYS), A) for r in (1, 2, 3)]
    z = {}
    for i in range(4):
        for j in range(i + 1, 4):
            z["selfplay %d/%d" % (i, j)] = _z(sp[i], sp[j])
    for r in range(4):
        z["reanalysis %d" % r] = _z(sp[0], NR.block(seed + 104729 * (r + 1), np.arange(PLIES), np.arange(KEYS), A))
    print("seed %#x: %s" % (seed, {k: round(v, 3) for k, v in z.items()}))
    for k, v in z.items():
        assert abs(v) < 4, (k, v)


@pytest.mark.parametrize("seed", SEEDS)
def test_row_argmax_is_uniform(seed):
    """Gumbel-top-k with flat logits picks each action equally often: chi-square of the per-row argmax over the
    8,192 rows."""
    am = _block(seed).reshape(-1, A).argmax(axis=1)
    cnt = np.bincount(am, minlength=A)
    e = PLIES * KEYS / A
    chi2 = float(((cnt - e) ** 2 / e).sum())
    print("seed %#x: chi2 %.1f" % (seed, chi2))
    assert chi2 < 300


# ------------------------------------------------------------------------------------------ row collisions
def _smallest_colliding_dkey(dc):
    """The dkey != 0 of smallest magnitude with row_word(c + dc, k + dkey) == row_word(c, k): 0x85EBCA77 is odd, so
    dkey = -dc * 0x9E3779B1 / 0x85EBCA77 mod 2^32 is the one solution; keys are uint32, so the difference of two
    keys is that residue or that residue - 2^32."""
    d = (-dc * 0x9E3779B1 * pow(0x85EBCA77, -1, 1 << 32)) % (1 << 32)
    return min(d, (1 << 32) - d), d


def test_rows_of_one_seed_collide_only_far_apart():
    """Two (ply, game) pairs with equal row words draw identical rows.  Within one ply no two keys collide; across
    plies up to 1,023 apart the nearest colliding game is 2,886,698 keys away (at 154 plies), far beyond the games
    of one seed."""
    assert pow(0x85EBCA77, -1, 1 << 32) * 0x85EBCA77 % (1 << 32) == 1  # dcounter = 0: dkey = 0 only
    best = min((_smallest_colliding_dkey(dc)[0], dc) for dc in range(1, 1024))
    print("smallest colliding |dkey| %d at dcounter %d" % best)
    assert best == (2886698, 154)
    assert best[0] > LARGEST_GAME_COUNT
    # the collision is real: the model's rows are equal there, and differ one key to either side
    _, d = _smallest_colliding_dkey(154)
    k1 = (1000 + d) % (1 << 32)
    a = NR.rows(5, [10], [1000], A)
    assert np.array_equal(a, NR.rows(5, [164], [k1], A))
    assert abs((k1 - 1000 + (1 << 31)) % (1 << 32) - (1 << 31)) == 2886698
    assert not np.array_equal(a, NR.rows(5, [164], [k1 + 1], A))
    assert not np.array_equal(a, NR.rows(5, [164], [k1 - 1], A))


# ------------------------------------------------------------------------------------------ entropy
def test_a_sample_has_32_bits_of_entropy():
    """h3 = mix32(h2 + const) is a function of h2, so the 53-bit word takes at most 2^32 values: the block of seed 5
    repeats 53-bit patterns as often as 32-bit draws do (n^2 / 2^33 = 395.5 expected; 0.0002 at 53 bits).  If the
    generator is ever widened this test is to be rewritten on purpose, with the comment in gumbel_noise()."""
    p, k, a = np.meshgrid(np.arange(PLIES), np.arange(KEYS), np.arange(A), indexing="ij")
    w = NR.h2(5, p, k, a).ravel()
    b = NR.bits(5, p, k, a).ravel()
    assert np.array_equal(b, NR.bits_of_h2(w))  # nothing but h2 enters
    assert int(w.max()) < 1 << 32
    repeats = N - np.unique(b).size
    print("repeated 53-bit patterns: %d (distinct h2 words: %d)" % (repeats, np.unique(w).size))
    assert np.unique(b).size <= np.unique(w).size
    assert 300 <= repeats <= 500
