"""The device Gumbel noise restated in numpy: gumbel_noise() of csrc/gmz_tree.hip, the generator behind
k_begin_move (search(gumbel=None)) and k_gumbel_keyed (gmz_gumbel_keyed).  tests/test_noise.py states what this
generator is; tests/test_noise_gpu.py holds the kernels to it.

Every function broadcasts over its arguments.  The 32-bit words are carried in uint64 and masked, so no product
overflows: (2^32 - 1)^2 < 2^64."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
M53 = np.uint64((1 << 53) - 1)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix32(x):
    """mix32 of csrc/gmz_common.h on the low 32 bits of ``x``."""
    x = _u64(x) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def row_word(counter, key):
    """The only thing the generator sees of (move counter, game key): counter * 0x9E3779B1 + key * 0x85EBCA77
    mod 2^32."""
    c = (_u64(counter) & M32) * np.uint64(0x9E3779B1) & M32
    k = (_u64(key) & M32) * np.uint64(0x85EBCA77) & M32
    return (c + k) & M32


def h2(seed, counter, key, a):
    """The second hash word: the whole sample is a function of it (bits_of_h2)."""
    seed = _u64(seed)
    lo, hi = seed & M32, seed >> np.uint64(32)
    h1 = mix32(lo ^ mix32(row_word(counter, key)))
    return mix32(h1 ^ mix32((_u64(a) + np.uint64(0x68E31DA4)) & M32) ^ hi)


def bits_of_h2(w):
    """The 53-bit integer of a sample from its h2 word, (h2 << 21) ^ h3 with h3 = mix32(h2 + const): 32 bits of
    entropy spread over the mantissa (bits 21..31 hold h2's low bits xor h3's high bits)."""
    w = _u64(w)
    h3 = mix32((w + np.uint64(0x1B873593)) & M32)
    return ((w << np.uint64(21)) ^ h3) & M53


def bits(seed, counter, key, a):
    """The sample's 53-bit integer (uint64), u = bits * 2^-53."""
    return bits_of_h2(h2(seed, counter, key, a))


def from_bits(b, ft=np.float64):
    """-log(-log(1 - u)) of u = b * 2^-53 in the float type ``ft``; a zero draw counts as 2^-53."""
    u = _u64(b).astype(ft) * ft(2.0 ** -53)  # exact: b < 2^53
    u = np.where(u <= 0, ft(2.0 ** -53), u)
    return -np.log(-np.log(ft(1) - u))  # 1 - u is exact too


def _noise(seed, counter, key, a, ft):
    return from_bits(bits(seed, counter, key, a), ft)


def noise(seed, counter, key, a):
    """Gumbel(0, 1) sample of (seed, move counter, game key, action) in float64, as the device computes it."""
    return _noise(seed, counter, key, a, np.float64)


def noise_ld(seed, counter, key, a):
    """The same sample in long double (64-bit mantissa on x86-64): the reference the device is measured against."""
    return _noise(seed, counter, key, a, np.longdouble)


def rows(seed, counters, keys, A, fn=noise):
    """[len(keys), A] rows: row i from (counters[i], keys[i]), as gmz_gumbel_keyed lays them out."""
    c = _u64(counters).reshape(-1, 1)
    k = _u64(keys).reshape(-1, 1)
    return fn(seed, c, k, np.arange(A, dtype=np.uint64).reshape(1, -1))


def block(seed, plies, keys, A, fn=noise):
    """[len(plies), len(keys), A]: every (ply, key) row."""
    c = _u64(plies).reshape(-1, 1, 1)
    k = _u64(keys).reshape(1, -1, 1)
    return fn(seed, c, k, np.arange(A, dtype=np.uint64).reshape(1, 1, -1))
