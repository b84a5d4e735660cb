"""Inputs of the Borda radix-sort tests (test_gpu_borda_sort.py), and a numpy twin of the sort key
(``desc_key`` in csrc/rank.hip) that test_borda_inputs.py uses to check, without a GPU, that each
generator builds what its GPU case claims to exercise.

The sort works on 64-bit keys in eight 8-bit digits (byte 0 = bits 0..7, the first LSD pass),
tiles of 4096 keys per workgroup, and 2048-entry chunks of the [256][ntiles] histogram scan."""
import numpy as np

TILE = 4096
SIGN = np.uint64(1) << np.uint64(63)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint64).view(np.float64)


def desc_key(x):
    """uint64 keys whose ascending order is the descending order of ``x``: NaN (any sign or
    payload) -> all ones, -0 -> +0, then the usual order-preserving map of the bit pattern,
    complemented."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    nan = np.isnan(x)
    b = bits(np.where(x == 0.0, 0.0, x))
    ordered = np.where((b >> np.uint64(63)) != 0, ~b, b | SIGN)
    return np.where(nan, ALL_ONES, ~ordered)


def varying_bytes(col):
    """The digits a sort of this column alone has to run: byte positions in which its keys
    differ (what run_borda derives from the OR and the AND of the keys)."""
    k = desc_key(col)
    v = int(np.bitwise_or.reduce(k) ^ np.bitwise_and.reduce(k))
    return [p for p in range(8) if (v >> (8 * p)) & 0xFF]


# ---------------------------------------------------------------------------- (a) key classes
NAN_PLAIN = 0x7FF8000000000000
NAN_SIGNED = 0xFFF8000000000000
NAN_PAYLOAD = 0x7FF8000000000123
DBL_MIN = np.finfo(np.float64).tiny
DBL_MAX = np.finfo(np.float64).max


def key_class_values():
    """Every class of fp64 the key map treats differently, NaNs as bit patterns."""
    v = [np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, DBL_MIN, -DBL_MIN, DBL_MAX, -DBL_MAX,
         1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0),
         -1.0, np.nextafter(-1.0, -2.0), np.nextafter(-1.0, 0.0)]
    b = bits(np.array(v, dtype=np.float64))
    return np.concatenate([b, np.array([NAN_PLAIN, NAN_SIGNED, NAN_PAYLOAD], dtype=np.uint64)])


def key_class_column(n=5000, seed=101):
    """Seeded normals with every value of ``key_class_values`` twice: once among the first 2400
    rows (tile 0) and once among the last 2400 (tile 1 when n = 5000), so equal keys meet across
    waves and workgroups."""
    rng = np.random.default_rng(seed)
    col = rng.standard_normal(n)
    sp = from_bits(key_class_values())
    lo = rng.choice(2400, size=sp.size, replace=False)
    hi = n - 2400 + rng.choice(2400, size=sp.size, replace=False)
    col[lo] = sp
    col[hi] = sp[rng.permutation(sp.size)]
    return col


# ---------------------------------------------------------------------------- (b) one byte
def one_byte_column(p, negative, n=5000, seed=202):
    """A column whose bit patterns, and so whose keys, differ in byte ``p`` only (at most 256
    values: heavy ties).  Finite, non-zero, not NaN for every digit."""
    rng = np.random.default_rng(seed + 16 * p + int(negative))
    if p == 7:
        base, dig = 0, rng.integers(1, 0x7F, size=n)          # 1 .. 0x7E: exponent below 0x7FF
    else:
        base = 0x3F00000000000000 if p == 6 else 0x3FF0000000000000
        dig = rng.integers(0, 256, size=n)
    b = np.uint64(base) | (dig.astype(np.uint64) << np.uint64(8 * p))
    if negative:
        b = b | SIGN
    return from_bits(b)


ONE_BYTE_CASES = [(p, neg) for p in range(8) for neg in (False, True)]


# ---------------------------------------------------------------------------- (c) sizes
SIZES = [1, 2, 63, 64, 65, 256, 257, 4095, 4096, 4097, 32768, 32769]


def mixed_table(n, c, seed=303):
    """n x c mixed-sign normals, 10 % of the entries one constant, 1 % NaN."""
    rng = np.random.default_rng(seed + 131 * n + c)
    D = rng.standard_normal((n, c))
    D[rng.random((n, c)) < 0.10] = -0.75
    D[rng.random((n, c)) < 0.01] = np.nan
    return D


def rounded_table(n, c, seed=304):
    rng = np.random.default_rng(seed)
    return np.round(rng.standard_normal((n, c)), 2)


# ---------------------------------------------------------------------------- (d) distributions
def distribution_columns(n=2 * TILE + 1, seed=404):
    """name -> column; n = 8193 is two full tiles and one key."""
    rng = np.random.default_rng(seed)
    v = np.sort(rng.standard_normal(n))
    assert np.unique(v).size == n
    two = np.where(np.arange(n) % 2 == 0, 3.5, -2.25)
    tiles = np.full(n, 0.125)
    tiles[:TILE] = -7.0          # tile 0: one value, one digit value in every pass
    tiles[TILE:2 * TILE] = 9.0   # tile 1: another
    return {"ascending": v, "descending": v[::-1].copy(), "all_equal": np.full(n, 2.5),
            "all_nan": np.full(n, np.nan), "alternating": two, "tile_constant": tiles}


# ---------------------------------------------------------------------------- (e) tie flags
TIE_CASES = [(2, 0), (300, 63), (300, 255), (4097, 4095), (8193, 4095), (8193, 8191)]


def distinct_column(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n)
    assert np.unique(v).size == n and not (v == 0.0).any()
    return v


def tie_column(n, p, seed=505):
    """Distinct values but for one equal pair, at positions (p, p + 1) of the descending order;
    rows shuffled."""
    rng = np.random.default_rng(seed + 7 * n + p)
    v = np.sort(distinct_column(n, seed + 7 * n + p + 1))[::-1].copy()
    v[p + 1] = v[p]
    return v[rng.permutation(n)]


def equal_adjacent_pairs(col):
    """Sorted positions j with key[j] == key[j + 1], NaN keys excluded (tie_flag_kernel)."""
    k = np.sort(desc_key(col))
    return np.flatnonzero((k[:-1] == k[1:]) & (k[:-1] != ALL_ONES)).tolist()


# ---------------------------------------------------------------------------- (i) > 1024 chunks
N_CHUNKS_CASE = 8216 * TILE + 7   # 8217 tiles, 256 * 8217 / 2048 -> 1028 scan chunks


def chunk_case_values(n=N_CHUNKS_CASE):
    """Non-negative integers below 1024: the keys differ in their three highest bytes only."""
    i = np.arange(n, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(0x3FF)).astype(np.float64)


def chunk_case_reference(v):
    """Stable descending Borda of one column of integers in [0, 1024), by a 16-bit sort."""
    n = v.shape[0]
    order = np.argsort((1023 - v).astype(np.uint16), kind="stable")
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n, dtype=np.int64)
    return n - pos
