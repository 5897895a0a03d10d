"""Plain numpy references of the small result and construction kernels, written from their
documented rules and from nothing else (no oracle, no torch):

  * sort_rows_kernel   -- stable ascending radix order per row, -0.0 and +0.0 one key, bits kept;
  * merge_results_kernel -- k smallest of the parts' rows, ties: lower part first, then position;
  * uniform_kernel     -- counter-based splitmix64, 24 bits -> (0, 1];
  * nn1_*_kernel       -- float32 of the exact mean, and the maximum.

The input generators below are shared by tests/test_results_reference.py (CPU: the references
against the oracle and the torch stand-in) and tests/test_gpu_results.py (the kernels against the
references), so that both see the same rows."""
import math

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
DENORMAL = np.array([1], np.uint32).view(np.float32)[0]          # 2**-149, the smallest one
# the values a sorted row is drawn from: both zeros, +-inf (an unfilled filtered slot is +inf),
# negatives, denormals of both signs and FLT_MAX -- few values, so most entries tie
SORT_VALUES = np.array([0.0, -0.0, 1.0, 2.0, -1.0, np.inf, -np.inf, DENORMAL, -DENORMAL, FLT_MAX,
                        -2.5], np.float32)
UNIFORM_STREAMS = ((1234, 0), (1234, 3), (0, 0), (2 ** 64 - 1, 2 ** 32 + 5))
# first three values of each stream above as float32 bit patterns
UNIFORM_KNOWN = {
    (1234, 0): (0x3f3b0cf7, 0x3f17c7a2, 0x3e4efbec),
    (1234, 3): (0x3e18b6f8, 0x3f4f36e3, 0x3ef792dc),
    (0, 0): (0x3f6220a9, 0x3edcf13e, 0x3cd88bc0),
    (2 ** 64 - 1, 2 ** 32 + 5): (0x3e801a1a, 0x3f6e69dc, 0x3ebc075c),
}
NN1_SIZES = (1, 255, 256, 257, 262143, 262144, 262145, 300001)


def bits(a):
    """float32 array as its bit patterns"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _key(d):
    """the value a radix sort orders by: -0.0 folded onto +0.0"""
    d = np.asarray(d, np.float32)
    return np.where(d == 0, np.float32(0.0), d)


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def sort_rows_ref(ids, dists):
    """per row: stable ascending order of the distances; outputs gathered from the original
    arrays, so that every entry keeps its bit pattern"""
    ids, dists = np.asarray(ids, np.int32), np.asarray(dists, np.float32)
    order = np.argsort(_key(dists), axis=1, kind="stable")
    return np.take_along_axis(ids, order, 1), np.take_along_axis(dists, order, 1)


def merge_ref(parts_ids, parts_dists, k, id_offset_per_part):
    """parts_*: [P, Nq, stride] sorted rows -> the k best per query; among equal distances the
    lower part first, then the position within the part"""
    parts_ids, parts_dists = np.asarray(parts_ids, np.int32), np.asarray(parts_dists, np.float32)
    P, Nq, stride = parts_ids.shape
    assert P * stride >= k
    offs = (np.arange(P, dtype=np.int32) * np.int32(id_offset_per_part)).reshape(P, 1, 1)
    ids = (parts_ids + offs).astype(np.int32).transpose(1, 0, 2).reshape(Nq, P * stride)
    dists = parts_dists.transpose(1, 0, 2).reshape(Nq, P * stride)
    order = np.argsort(_key(dists), axis=1, kind="stable")[:, :k]
    return (np.ascontiguousarray(np.take_along_axis(ids, order, 1)),
            np.ascontiguousarray(np.take_along_axis(dists, order, 1)))


_M64 = (1 << 64) - 1


def uniform_ref(n, seed, stream_id):
    """splitmix64 of the counter (stream_id * 2**32 + i + 1), top 24 bits -> (0, 1]"""
    start = np.uint64(((stream_id << 32) + 1) & _M64)
    ctr = np.arange(n, dtype=np.uint64) + start                      # wraps like the kernel's
    z = np.uint64(seed & _M64) + np.uint64(0x9E3779B97F4A7C15) * ctr
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    # a 24-bit integer, that integer + 1 <= 2**24 and a power-of-two scale: all exact in float32
    return ((z >> np.uint64(40)).astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -24)


def uniform_python(n, seed, stream_id):
    """uniform_ref once more, in Python integers"""
    out = np.empty(n, np.float32)
    for i in range(n):
        z = (seed + 0x9E3779B97F4A7C15 * ((stream_id * 2 ** 32 + i + 1) & _M64)) & _M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        z ^= z >> 31
        out[i] = np.float32(((z >> 40) + 1) / 2.0 ** 24)              # exact: <= 25 bits / 2**24
    return out


def nn1_ref(v):
    """(float32 of the correctly rounded float64 mean, maximum)"""
    v = np.asarray(v, np.float32)
    return np.float32(math.fsum(v.tolist()) / v.size), v.max()


def same_up_to_tie_order(ids_a, d_a, ids_b, d_b):
    """Two [Nq, K] results that may differ only in how a tie was ordered: the distances are
    bitwise equal; per row every distance value below the row's last one carries the same
    multiset of ids on both sides; of the last value (a tie group that K may have cut, keeping
    other members) only the counts agree -- which the equal distances already say."""
    ids_a, ids_b = np.asarray(ids_a), np.asarray(ids_b)
    if ids_a.shape != ids_b.shape or not np.array_equal(bits(d_a), bits(d_b)):
        return False
    key = _key(d_a)
    for n in range(key.shape[0]):
        row = key[n]
        for v in np.unique(row[row < row[-1]]):
            m = row == v
            if not np.array_equal(np.sort(ids_a[n][m]), np.sort(ids_b[n][m])):
                return False
    return True


# ---------------------------------------------------------------------------------------------
# shared inputs
# ---------------------------------------------------------------------------------------------
def sort_rows_input(rows, row_len, seed):
    """[rows, row_len] heavily tied distances over SORT_VALUES; the ids of a row are a
    permutation of arange(row_len), so that a lost or doubled entry shows"""
    r = np.random.default_rng(seed)
    d = SORT_VALUES[r.integers(0, len(SORT_VALUES), (rows, row_len))]
    ids = np.argsort(r.random((rows, row_len)), axis=1).astype(np.int32)
    return ids, d


def merge_input(P, Nq, stride, seed, signed_zeros=False):
    """[P, Nq, stride] sorted part rows of small integer distances (heavily tied within and
    across parts), ids below 1000; every row ends in a +inf tail of random length -- none, some,
    the whole row -- whose ids are -1 as filtered searches leave them.  signed_zeros: the zeros
    of a random half of the part rows are -0.0, a tie with the +0.0 of the others."""
    r = np.random.default_rng(seed)
    d = np.sort(r.integers(0, 6, (P, Nq, stride)), axis=2).astype(np.float32)
    ids = r.integers(0, 1000, (P, Nq, stride)).astype(np.int32)
    tail = r.integers(0, stride + 1, (P, Nq))
    pick = r.random((P, Nq))
    tail = np.where(pick < 0.3, 0, np.where(pick > 0.85, stride, tail))
    in_tail = np.arange(stride)[None, None, :] >= (stride - tail)[:, :, None]
    d[in_tail] = np.inf
    ids[in_tail] = -1
    if signed_zeros:
        neg = (r.random((P, Nq)) < 0.5)[:, :, None] & (d == 0)
        d[neg] = np.float32(-0.0)
    return ids, d


def nn1_exact_input(N, seed, shift=0.0):
    """multiples of 1/8 below 2**17: every partial sum of up to 2**31 of them is an integer
    multiple of 1/8 below 2**48, exact in float64 -- any summation order gives the same double"""
    v = np.random.default_rng(seed).integers(0, 2 ** 20, N) / 8.0 - shift
    return v.astype(np.float32)


def nn1_generic_input(seed=5, N=100003):
    """unconstrained floats, with the proof that the order of summation cannot show: for the
    exact mean m, every double within m * (1 +- N * 2**-52) -- a bound on what N float64 adds of
    positive terms and one division can be off by -- rounds to the same float32"""
    v = (np.random.default_rng(seed).random(N) * 500).astype(np.float32)
    m = math.fsum(v.tolist()) / N
    slack = N * 2.0 ** -52
    assert np.float32(m * (1 - slack)) == np.float32(m) == np.float32(m * (1 + slack)), \
        "pick another seed: the mean lies too close to a float32 rounding boundary"
    return v
