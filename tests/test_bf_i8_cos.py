"""The integer cosine kernel of bf_query (bf_i8_cos.hip) without a GPU: the routing predicate at and one
past each edge, and the fast-path bound of the file's header re-derived in float32 -- no pair with
value <= T may fail dot * rinv >= c."""
import numpy as np
import pytest

# (dtype, measure, D, Nq, N, k, filtered), {hooks} -> cosine kernel?
ROUTES = [
    (("U8", 1, 16, 256, 4096, 16, 0), {"BF_I8_COS": 2}, 1),
    (("I8", 1, 4096, 256, 4096, 1, 0), {"BF_I8_COS": 2}, 1),
    (("U8", 0, 256, 256, 4096, 10, 0), {"BF_I8_COS": 2}, 0),       # squared L2
    (("U8", 1, 256, 256, 4096, 10, 1), {"BF_I8_COS": 2}, 0),       # filtered
    (("U8", 1, 8, 256, 4096, 10, 0), {"BF_I8_COS": 2}, 0),
    (("U8", 1, 24, 256, 4096, 10, 0), {"BF_I8_COS": 2}, 0),        # D % 16 != 0
    (("U8", 1, 4112, 256, 4096, 10, 0), {"BF_I8_COS": 2}, 0),
    (("U8", 1, 256, 256, 4096, 17, 0), {"BF_I8_COS": 2}, 0),
    (("U8", 1, 256, 255, 4096, 10, 0), {"BF_I8_COS": 2}, 0),
    (("U8", 1, 256, 256, 4095, 10, 0), {"BF_I8_COS": 2}, 0),
    (("F32", 1, 256, 256, 4096, 10, 0), {"BF_I8_COS": 2}, 0),
    (("U8", 1, 256, 256, 4096, 10, 0), {"BF_I8_COS": 2, "BF_NO_I8": 1}, 0),
    (("U8", 1, 256, 256, 4096, 10, 0), {"BF_I8_COS": 2, "BF_SCAN": 1}, 0),
    (("U8", 1, 256, 10000, 1000000, 10, 0), {"BF_I8_COS": 1}, 0),
    # auto: from 10k queries x 1M rows on
    (("U8", 1, 128, 10000, 1000000, 10, 0), {}, 1),
    (("I8", 1, 768, 10000, 1000000, 16, 0), {}, 1),
    (("U8", 1, 960, 9999, 1000000, 10, 0), {}, 0),
    (("U8", 1, 960, 10000, 999999, 10, 0), {}, 0),
    (("U8", 1, 256, 1024, 65536, 10, 0), {}, 0),
]


@pytest.mark.parametrize("shape,hooks,routed", ROUTES, ids=[f"{r[0]}-{r[1]}" for r in ROUTES])
def test_routing_predicate(shape, hooks, routed):
    from ggnn_amd import _lib
    with _lib.hooks(**hooks):
        assert _lib.lib().ggnn_debug_bf_i8_cos_route(getattr(_lib, shape[0]), *shape[1:]) == routed


F = np.float32


def value(dot, bn, qn):
    """finish_cos, each operation rounded to float32"""
    ns = F(qn) * F(bn)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.abs(F(1) - F(dot) / np.sqrt(ns))
    return np.where(ns > 0, v, F(1)).astype(F)


def passes(dot, bn, qn, T):
    """the kernel's fused test: the sign of the real dot * rinv - c (24 x 24 bits: exact in float64)"""
    with np.errstate(divide="ignore"):
        rinv = np.where(bn > 0, F(1) / np.sqrt(F(bn)), F(0)).astype(F)
    c = ((F(1) - F(T)) - F(2.0 ** -20)) * np.sqrt(F(qn))
    return F(dot).astype(np.float64) * rinv.astype(np.float64) >= c.astype(np.float64)


@pytest.mark.parametrize("lo,hi,D", [(0, 256, 16), (0, 256, 256), (-128, 128, 64), (-128, 128, 1024), (0, 4, 48)])
def test_no_pair_within_T_fails_the_fast_test(lo, hi, D):
    rng = np.random.default_rng(D + hi)
    o = rng.integers(lo, hi, (300, D)).astype(np.int64)
    o[:40] = rng.integers(lo // 2, hi // 2, (40, D)) // 2 * 2
    o[290:] = 0                                                   # zero rows, zero queries
    q = np.concatenate([o[:100], 2 * o[:40], o[:40] // 2, -o[:40] if lo < 0 else o[40:80] // 2])
    dot, bn, qn = q @ o.T, (o * o).sum(1)[None, :], (q * q).sum(1)[:, None]
    assert max(np.abs(dot).max(), bn.max(), qn.max()) < 1 << 24
    v = value(dot, bn, qn)
    assert (v == 0).any() and (v == 1).any()
    up = np.nextafter(v, F(4))
    for T in (v, up, np.nextafter(up, F(4)), F(0), F(2.0 ** -24), F(2.0 ** -23), F(1), F(1.5), F(2)):
        T = np.broadcast_to(F(T), v.shape)
        assert passes(dot, bn, qn, T)[v <= T].all()
