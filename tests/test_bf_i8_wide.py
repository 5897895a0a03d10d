"""Routing of bf_query's wide-row integer kernel (bf_i8_wide.hip) without a GPU: the shape list at and
one past each edge, hooks BF_I8_WIDE / BF_NO_I8 / BF_SCAN, and the auto thresholds of DESIGN.md 4.6."""
import pytest

BIG = (10000, 1000000)
# (dtype, measure, D, Nq, N, k, filtered), {hooks} -> wide kernel?
ROUTES = [
    (("U8", 0, 144, 256, 4096, 16, 0), {"BF_I8_WIDE": 2}, 1),
    (("I8", 0, 4096, 256, 4096, 1, 0), {"BF_I8_WIDE": 2}, 1),
    (("U8", 0, 128, 256, 4096, 10, 0), {"BF_I8_WIDE": 2}, 0),      # bf_i8v2_kernel's rows
    (("U8", 0, 4112, 256, 4096, 10, 0), {"BF_I8_WIDE": 2}, 0),
    (("U8", 0, 264, 256, 4096, 10, 0), {"BF_I8_WIDE": 2}, 0),      # D % 16 != 0
    (("U8", 0, 256, 256, 4096, 17, 0), {"BF_I8_WIDE": 2}, 0),
    (("I8", 1, 256, 256, 4096, 10, 0), {"BF_I8_WIDE": 2}, 0),      # cosine
    (("U8", 0, 256, 256, 4096, 10, 1), {"BF_I8_WIDE": 2}, 0),      # filtered
    (("U8", 0, 256, 255, 4096, 10, 0), {"BF_I8_WIDE": 2}, 0),
    (("U8", 0, 256, 256, 4095, 10, 0), {"BF_I8_WIDE": 2}, 0),
    (("F32", 0, 256, 256, 4096, 10, 0), {"BF_I8_WIDE": 2}, 0),
    (("U8", 0, 256, 256, 4096, 10, 0), {"BF_I8_WIDE": 2, "BF_NO_I8": 1}, 0),
    (("U8", 0, 256, 256, 4096, 10, 0), {"BF_I8_WIDE": 2, "BF_SCAN": 1}, 0),
    (("U8", 0, 256, *BIG, 10, 0), {"BF_I8_WIDE": 1}, 0),
    # auto: from 10k queries x 1M rows on
    (("U8", 0, 960, *BIG, 10, 0), {}, 1),
    (("I8", 0, 768, *BIG, 16, 0), {}, 1),
    (("U8", 0, 960, 9999, 1000000, 10, 0), {}, 0),
    (("U8", 0, 960, 10000, 999999, 10, 0), {}, 0),
    (("U8", 0, 256, 1024, 65536, 10, 0), {}, 0),
    (("U8", 0, 128, *BIG, 10, 0), {}, 0),
]


@pytest.mark.parametrize("shape,hooks,wide", ROUTES, ids=[f"{r[0]}-{r[1]}" for r in ROUTES])
def test_routing_predicate(shape, hooks, wide):
    from ggnn_amd import _lib
    with _lib.hooks(**hooks):
        assert _lib.lib().ggnn_debug_bf_i8_wide_route(getattr(_lib, shape[0]), *shape[1:]) == wide
