"""GPU tests of "Distances from lossless codes" (ggnn_amd/csrc/traversal.hpp, prescreen.hip): on a
float32 base whose pre-screen copy is lossless on a power-of-two grid, the early-rows query kernels
take a candidate's squared-L2 distance from its codes when the query lies on the grid too, and read
no float row.  Everything here is an equality: ids, distances and work counters of the default
kernels against the same library with the hook PS_EXACT = 0 (always the float rows) and against
set_prescreen(False), on grids, off them, and at the edges of the certificate.  The arithmetic
itself is derived on the CPU in tests/test_lossless_math.py."""
import numpy as np
import pytest

from lossless_helpers import (F, N, NQ, Case, _cases, assert_same, assert_true_distances,
                              bitset_filter, case, label_filter, mixed_queries, table_filter,
                              three_way, true_l2)

pytestmark = pytest.mark.gpu

# 175 iterations: 192-key ring, one bucket register, ring-less (the headline kernel);
# 400: 448 keys, two bucket registers
ITERS = (175, 400)


@pytest.mark.parametrize("iters", ITERS)
def test_integer_base_mixed_batch(case, iters):
    c, grid_q = case("int")
    assert c.flag() == 1.0
    q = mixed_queries(c.base, grid_q, F(1))
    on, off = three_way(c, q, iters=iters)
    assert_true_distances(c, q, on)
    # the on-grid part of the batch read fewer float rows, the rest as many
    assert on[3]["float_rows"] < off[3]["float_rows"]


@pytest.mark.parametrize("iters", ITERS)
def test_integer_base_grid_batch_reads_fewer_float_rows(case, iters):
    c, q = case("int")
    on, off = three_way(c, q, iters=iters)
    assert on[3]["float_rows"] < off[3]["float_rows"]
    assert on[3]["code_rows"] == off[3]["code_rows"] > 0
    assert np.array_equal(on[1], true_l2(c.base, q, on[0]))


def test_integer_base_fractional_batch_is_untouched(case):
    c, grid_q = case("int")
    rng = np.random.default_rng(3)
    q = (grid_q + rng.random(grid_q.shape, dtype=F)).astype(F)
    q[7] = grid_q[7] + F(2.0 ** -12)        # a tiny off-grid component in every dimension
    q[8] = grid_q[8]
    q[8, 100] = F(2.0 ** -20)               # ... and in one dimension only
    on, off = three_way(c, q)
    assert on[3] == off[3]


@pytest.mark.parametrize("name,step,must_flag", [("quarter", 0.25, True), ("four", 4.0, True),
                                                 ("signed", 1.0, True), ("big", 1.0, False)])
def test_dyadic_scales_and_offsets(case, name, step, must_flag):
    c, grid_q = case(name)
    flag = c.flag()
    assert flag in (0.0, 1.0) and (flag == 1.0 or not must_flag)
    on, off = three_way(c, grid_q)
    assert np.array_equal(on[1], true_l2(c.base, grid_q, on[0]))
    if flag:
        assert on[3]["float_rows"] < off[3]["float_rows"]
    else:
        assert on[3] == off[3]
    q = mixed_queries(c.base, grid_q, F(step))
    on, off = three_way(c, q)
    assert_true_distances(c, q, on)


def test_fractional_base_keeps_the_float_phase(case):
    c, q = case("frac")
    assert c.flag() == 0.0
    on, off = three_way(c, q)
    assert on[3] == off[3] and on[3]["float_rows"] > 0


def test_the_maximum_sum(case):
    """rows of all 0 (and five of all 255), queries of all 255 or all 0, D = 128: a distance is 0
    or 128 * 255^2 = 8 323 200, the largest sum the code path forms.  K = 20 exceeds the start
    points' number, so the list fills during the traversal: those distances come from the pops."""
    if ("max", 128) not in _cases:
        base = np.zeros((N, 128), F)
        base[[17, 5000, 9999, 12345, 19999]] = 255
        q = np.zeros((NQ, 128), F)
        q[::2] = 255
        _cases[("max", 128)] = (Case(base), q)
    c, q = _cases[("max", 128)]
    assert c.flag() == 1.0
    on, off = three_way(c, q, k=20)
    found = on[0] >= 0
    want = np.where(c.base[np.maximum(on[0], 0), 0] == q[:, None, 0], F(0), F(8323200))
    assert np.array_equal(on[1][found], want[found])
    assert (on[1][::2] == F(8323200)).any() and (on[1][1::2] == 0).any()


@pytest.mark.parametrize("d", [96, 64])
def test_other_row_lengths(case, d):
    """D = 96: float layout {8, 3}, 128 code dimensions of which 32 are padding; D = 64: half-filled
    code rows of 64 dimensions"""
    c, grid_q = case("int", d)
    assert c.flag() == 1.0
    on, off = three_way(c, grid_q)
    assert on[3]["float_rows"] < off[3]["float_rows"]
    assert np.array_equal(on[1], true_l2(c.base, grid_q, on[0]))
    three_way(c, mixed_queries(c.base, grid_q, F(1)))


@pytest.mark.parametrize("nq", [1, 63, 64, 65])
def test_batch_sizes(case, nq):
    c, grid_q = case("int")
    q = mixed_queries(c.base, grid_q, F(1))[:nq]
    on, off = three_way(c, q)
    assert_true_distances(c, q, on)


def test_under_a_bitset_filter(case):
    c, q = case("int")
    mask = bitset_filter(N)
    on = c.search(q, how="bitset", arg=mask)
    off = c.search(q, exact=0, how="bitset", arg=mask)
    assert_same(on, off)
    assert on[3]["float_rows"] < off[3]["float_rows"] and on[3]["code_rows"] == off[3]["code_rows"]
    assert mask[on[0][on[0] >= 0]].all()


def test_under_a_filter_table(case):
    c, q = case("int")
    masks, fid = table_filter(N)
    c.eng.set_filters(masks)
    try:
        on = c.search(q, how="table", arg=fid)
        off = c.search(q, exact=0, how="table", arg=fid)
    finally:
        c.eng.set_filters(None)
    assert_same(on, off)
    assert on[3]["float_rows"] < off[3]["float_rows"] and on[3]["code_rows"] == off[3]["code_rows"]


@pytest.mark.parametrize("d", [128, 96])
def test_under_labels(case, d):
    c, q = case("int", d)
    labels, ql = label_filter(N)
    c.eng.set_labels(labels)
    try:
        on = c.search(q, how="labels", arg=ql)
        off = c.search(q, exact=0, how="labels", arg=ql)
    finally:
        c.eng.set_labels(None)
    assert_same(on, off)
    assert on[3]["float_rows"] < off[3]["float_rows"] and on[3]["code_rows"] == off[3]["code_rows"]
    hit = on[0] >= 0
    assert (labels[np.maximum(on[0], 0)] == ql[:, None])[hit & (ql[:, None] >= 0)].all()


def test_a_tiny_component_next_to_a_large_offset_keeps_the_float_phase(case):
    """offsets of -128: q - o rounds a coordinate of 2^-20 to the grid point 128, so a certificate of
    the form t == rint(t) would pass these queries; the kernel's (o + s*cq == q) must not -- every
    query of the batch reads its float rows as with PS_EXACT = 0"""
    c, grid_q = case("signed")
    assert c.flag() == 1.0 and (c.base.min(0) == -128).all()
    q = grid_q.copy()
    q[np.arange(NQ), np.arange(NQ) % 128] = F(2.0 ** -20)
    q[1::2, 64] = F(-(2.0 ** -22))
    t = (q - F(-128)).astype(F)
    assert np.array_equal(t, np.rint(t)) and t.min() >= 0 and t.max() <= 255   # the naive test passes
    on, off = three_way(c, q)
    assert on[3] == off[3] and on[3]["float_rows"] > 0
    # ... and the same rows without the component do skip them
    on, off = three_way(c, grid_q)
    assert on[3]["float_rows"] < off[3]["float_rows"]


def test_cosine_on_integer_data_and_back(case):
    """unit-normalised rows are never lossless: the cosine copy carries no flag and both settings
    run the same float phase; coding again for squared L2 brings the flag back"""
    import ggnn_amd as ggnn
    c, q = case("int")
    cos = ggnn.DistanceMeasure.Cosine
    assert c.flag(1) == 0.0
    on = c.search(q, measure=cos)
    off = c.search(q, exact=0, measure=cos)
    assert_same(on, off)
    assert on[3] == off[3]
    on, off = three_way(c, q)
    assert on[3]["float_rows"] < off[3]["float_rows"]
