"""CPU check of the arithmetic behind "Distances from lossless codes" (ggnn_amd/csrc/traversal.hpp,
prescreen.hip): a float32 restatement of the certificate and of the float phase of the query
kernels, in the kernels' own order, on adversarial grids.

Claim: a base whose pre-screen copy carries the lossless-grid flag (every row is o + s*c exactly,
s a power of two, every offset k*s with an integer |k| <= 2^23) and a query that passes
`o_d + s*cq_d == q_d` in every dimension give a float32 distance -- chunked, diff = o - q,
fmaf(diff, diff, a), pairwise group sums -- equal to s^2 * S bit for bit, S = sum (cq_d - c_d)^2.
The GPU tests check the kernels (tests/test_gpu_lossless_prescreen.py); this one checks that the
derivation holds in float32 arithmetic at all, and that the certificate refuses what it must."""
from fractions import Fraction

import numpy as np
import pytest

F = np.float32


def fma(a, b, c):
    """float32 fmaf.  The product of two float32 is exact in float64; where the float64 sum with c
    is exact as well (asserted: every use here), the conversion is the instruction's one rounding"""
    p = np.float64(a) * np.float64(b)
    t = p + np.float64(c)
    assert Fraction(float(t)) == Fraction(float(p)) + Fraction(float(c))
    return F(t)


def group_sum(v, lpr):
    """traversal.hpp group_sum<LPR> over one group of lpr = 8 or 16 lanes: quad_perm [1,0,3,2],
    quad_perm [2,3,0,1], row_half_mirror, row_mirror (LPR = 16); every lane keeps its own total"""
    v = np.asarray(v, F).copy()
    lanes = np.arange(lpr)
    steps = [lanes ^ 1, lanes ^ 2, (lanes & ~7) | (7 - (lanes & 7))]
    if lpr == 16:
        steps.append(15 - lanes)
    for partner in steps:
        v = (v + v[partner]).astype(F)
    return v


def kernel_distance(x, q, lpr, nch):
    """DistEngine<float, lpr, nch>::partial<kL2> + group_sum: lane g owns the 16-byte chunks
    c * lpr + g (four floats each), c = 0 .. nch-1, of rows padded with nothing (chunks beyond D
    are skipped).  Returns the totals of all lanes of the group."""
    D = x.size
    acc = np.zeros(lpr, F)
    for g in range(lpr):
        a = F(0)
        for c in range(nch):
            d0 = (c * lpr + g) * 4
            if d0 >= D:
                continue
            for e in range(4):
                diff = F(x[d0 + e] - q[d0 + e])
                a = fma(diff, diff, a)
        acc[g] = a
    return group_sum(acc, lpr)


def base_flag(o, s, e_max):
    """ps_retry_kernel: the lossless-grid flag of a squared-L2 copy"""
    s = F(s)
    inv_s = F(1) / s
    ok = e_max == 0 and F(2.0 ** -40) <= s <= F(2.0 ** 40)
    for od in np.asarray(o, F):
        k = F(od * inv_s)
        ok = ok and abs(k) <= F(2.0 ** 23) and k == np.rint(k) and F(k * s) == od
    return bool(ok)


def e_max_of(base, o, s):
    """ps_encode_kernel with the power-of-two scale: 0 iff every value is coded without loss"""
    inv_s = F(1) / F(s)
    c = np.clip(np.rint(((base - o).astype(F) * inv_s).astype(F)), 0, 255).astype(F)
    res = base.astype(np.float64) - (o.astype(np.float64) + np.float64(s) * c)
    return float(np.sqrt((res ** 2).sum(1)).max()), c.astype(np.int64)


def query_codes(q, o, s):
    """Prescreen::load: the query's codes, and the certificate o_d + s*cq_d == q_d"""
    s = F(s)
    inv_s = F(1) / s
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((q - o).astype(F) * inv_s).astype(F)
        r = np.rint(t)
        code = np.where(np.isnan(r), F(0), np.clip(r, 0, 255)).astype(F)   # fmaxf(NaN, 0) = 0
        on_grid = (o + (s * code).astype(F)).astype(F) == q
    return code.astype(np.int64), bool(on_grid.all())


def naive_query_test(q, o, s):
    """what the certificate must NOT be: t == rint(t) in float32"""
    t = ((q - o).astype(F) * (F(1) / F(s))).astype(F)
    return bool(((t == np.rint(t)) & (t >= 0) & (t <= 255)).all())


LAYOUTS = {128: (16, 2), 96: (8, 3), 64: (8, 2)}   # pick_dist_config for float32 rows


def offsets(kind, D, s, rng):
    k = {"zero": np.zeros(D), "negative": -rng.integers(1, 1000, D).astype(np.float64),
         "+2^23": np.full(D, 2.0 ** 23), "-2^23": np.full(D, -2.0 ** 23),
         "mixed": rng.choice([-2.0 ** 23, -77.0, 0.0, 12345.0, 2.0 ** 23], D)}[kind]
    return (k * s).astype(F)


@pytest.mark.parametrize("s", [0.25, 1.0, 4.0])
@pytest.mark.parametrize("kind", ["zero", "negative", "+2^23", "-2^23", "mixed"])
@pytest.mark.parametrize("D", [128, 96, 64])
def test_float_phase_equals_scaled_code_sum(s, kind, D):
    rng = np.random.default_rng(int(s * 4) + D)
    lpr, nch = LAYOUTS[D]
    o = offsets(kind, D, s, rng)
    c_rows = rng.integers(0, 256, (12, D))
    c_rows[0] = 0           # the offsets themselves are rows: min over rows
    c_rows[1] = 255
    c_rows[2, ::2] = 0
    c_rows[2, 1::2] = 255
    base = (o.astype(np.float64) + s * c_rows).astype(F)
    assert np.array_equal(base.astype(np.float64), o.astype(np.float64) + s * c_rows)
    e_max, codes = e_max_of(base, o, s)
    assert e_max == 0 and np.array_equal(codes, c_rows)
    assert base_flag(o, s, e_max)
    c_q = rng.integers(0, 256, (6, D))
    c_q[0] = 255
    c_q[1] = 0
    c_q[2] = c_rows[5]      # a query equal to a base row
    queries = (o.astype(np.float64) + s * c_q).astype(F)
    for q, cq in zip(queries, c_q):
        code, ok = query_codes(q, o, s)
        assert ok and np.array_equal(code, cq)
        for x, cx in zip(base, c_rows):
            S = int(((cq - cx) ** 2).sum())
            assert S < 2 ** 24
            want = F(F(s) * F(s)) * F(S)
            assert float(want) == s * s * S          # the product itself is exact
            got = kernel_distance(x, q, lpr, nch)
            assert np.all(got == want), (kind, s, D, got, want)


def test_the_maximum_sum():
    """all-0 row against an all-255 query at D = 128: 128 * 255^2 = 8 323 200 < 2^24"""
    for s in (0.25, 1.0, 4.0):
        o = np.zeros(128, F)
        x = np.zeros(128, F)
        q = np.full(128, 255 * s, F)
        code, ok = query_codes(q, o, s)
        assert ok and np.all(code == 255)
        got = kernel_distance(x, q, 16, 2)
        assert np.all(got == F(s * s * 8323200.0)) and float(got[0]) == s * s * 8323200.0
        assert 128 * 255 * 255 < 2 ** 24


def test_the_certificate_rejects_what_is_off_the_grid():
    D, s = 128, 1.0
    rng = np.random.default_rng(5)
    o = (-rng.integers(100, 200, D)).astype(F)
    c = rng.integers(1, 255, D)
    good = (o + c).astype(F)
    assert query_codes(good, o, s)[1]
    # a fractional coordinate
    q = good.copy()
    q[17] += F(0.5)
    assert not query_codes(q, o, s)[1]
    # one step outside the coded range, on either side (the code is clamped)
    for step in (-1.0, 256.0):
        q = good.copy()
        q[3] = o[3] + F(step)
        assert not query_codes(q, o, s)[1]
    # non-finite coordinates
    for bad in (np.nan, np.inf, -np.inf):
        q = good.copy()
        q[9] = F(bad)
        assert not query_codes(q, o, s)[1]
    # a tiny off-grid component next to a large offset: q - o rounds to an integer in float32,
    # so `t == rint(t)` lets it through; the certificate compares o + s*cq with q itself
    q = good.copy()
    q[40] = F(2.0 ** -20)
    o40 = o.copy()
    o40[40] = F(-200.0)
    assert naive_query_test(q, o40, s)
    assert not query_codes(q, o40, s)[1]
    # the same at a scale of 1/4 and with the component below the grid point
    q = (o * F(0.25) + F(0.25) * c).astype(F)
    q[0] = F(-(2.0 ** -22))
    ob = (o * F(0.25)).astype(F)
    ob[0] = F(-60.0)
    assert naive_query_test(q, ob, 0.25)
    assert not query_codes(q, ob, 0.25)[1]


def test_the_base_flag_rejects_what_is_off_the_grid():
    D = 64
    o = np.zeros(D, F)
    assert base_flag(o, 1.0, 0.0)
    # a lossy first pass
    assert not base_flag(o, 1.0, 1e-3)
    # an offset off the grid of s
    for s, off in ((1.0, 0.5), (4.0, 2.0), (0.25, 0.125), (1.0, 2.0 ** -30)):
        ob = o.copy()
        ob[5] = F(off)
        assert not base_flag(ob, s, 0.0)
    # an offset on the grid but past 2^23 steps: o + 255 s would need more than 24 bits
    for k in (2.0 ** 23 + 1, -(2.0 ** 23) - 1, 2.0 ** 24, 2.0 ** 30):
        ob = o.copy()
        ob[7] = F(k)
        assert not base_flag(ob, 1.0, 0.0)
    ob = o.copy()
    ob[7] = F(2.0 ** 23)
    assert base_flag(ob, 1.0, 0.0)
    # an offset whose quotient underflows: k = o / s flushes towards 0 but k * s != o
    ob = o.copy()
    ob[1] = F(2.0 ** -140)
    assert not base_flag(ob, 2.0 ** 30, 0.0)
    # scales outside 2^-40 .. 2^40 (s^2 * 2^24 must stay finite and normal)
    assert not base_flag(o, 2.0 ** 41, 0.0) and not base_flag(o, 2.0 ** -41, 0.0)
    # non-finite offsets
    ob = o.copy()
    ob[2] = F(np.nan)
    assert not base_flag(ob, 1.0, 0.0)


def test_a_row_that_is_not_lossless_raises_e_max():
    """the base side of the certificate: a single fractional or out-of-range value shows in e_max"""
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, (50, 64)).astype(F)
    base[0] = 0
    o = base.min(0)
    assert e_max_of(base, o, 1.0)[0] == 0
    b = base.copy()
    b[7, 3] += F(0.25)
    assert e_max_of(b, o, 1.0)[0] > 0
    b = base.copy()
    b[9, 11] = F(300)            # past 255 steps: clamped
    assert e_max_of(b, o, 1.0)[0] > 0
