"""GPU tests of "Distances from lossless codes" (ggnn_amd/csrc/traversal.hpp, prescreen.hip): on a
float32 base whose pre-screen copy is lossless on a power-of-two grid, the early-rows query kernels
take a candidate's squared-L2 distance from its codes when the query lies on the grid too, and read
no float row.  Everything here is an equality: ids, distances and work counters of the default
kernels against the same library with the hook PS_EXACT = 0 (always the float rows) and against
set_prescreen(False), on grids, off them, and at the edges of the certificate.  The arithmetic
itself is derived on the CPU in tests/test_lossless_math.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NQ, K, KBUILD = 20000, 256, 10, 24      # EARLY needs KBuild <= 24
TAU = 0.7
# 175 iterations: 192-key ring, one bucket register, ring-less (the headline kernel);
# 400: 448 keys, two bucket registers
ITERS = (175, 400)
F = np.float32


def _ints(rng, n, d, lo=0, hi=256):
    return rng.integers(lo, hi, (n, d)).astype(F)


# name -> (base, on-grid queries): float32 rows on a dyadic grid of at most 256 levels
SEEDS = {"int": 11, "quarter": 12, "four": 13, "signed": 14, "big": 15, "frac": 16}


def _dataset(name, d=128):
    rng = np.random.default_rng(SEEDS[name] * 1000 + d)
    if name == "int":
        return _ints(rng, N, d), _ints(rng, NQ, d)
    if name == "quarter":                      # values k / 4: scale 2^-2
        return _ints(rng, N, d) * F(0.25), _ints(rng, NQ, d) * F(0.25)
    if name == "four":                         # values 4 k: scale 4
        return _ints(rng, N, d) * F(4), _ints(rng, NQ, d) * F(4)
    if name == "signed":                       # values in [-128, 127]: negative offsets
        return _ints(rng, N, d, -128, 128), _ints(rng, NQ, d, -128, 128)
    if name == "big":                          # values 2^23 + k: offsets at the certificate's edge
        return _ints(rng, N, d) + F(2.0 ** 23), _ints(rng, NQ, d) + F(2.0 ** 23)
    if name == "frac":                         # genuinely fractional rows: no lossless copy
        centres = rng.normal(size=(16, d)) * 30 + 128
        mk = lambda n: (centres[rng.integers(0, 16, n)] + rng.normal(size=(n, d)) * 12).astype(F)
        return mk(N), mk(NQ)
    raise KeyError(name)


class Case:
    """an engine with its graph, kept for the module: one build per data set"""

    def __init__(self, base):
        import ggnn_amd as ggnn
        self.base = base
        self.eng = ggnn.GGNN()
        self.eng.set_collect_counters(True)
        self.eng.set_base(base)
        self.eng.build(KBUILD, 0.5, 1)

    def flag(self, measure=0):
        """params[5] of a pre-screen copy of this base (the engine's own copy is coded alike)"""
        import torch
        from ggnn_amd import ops
        _, params = ops.prescreen_encode(torch.from_numpy(self.base).cuda(), measure)
        return float(params[5].item())

    def search(self, q, *, exact=1, prescreen=True, iters=175, k=K, how="plain", arg=None,
               measure=None):
        """(ids, dists, counters, rows read) of one blocking search"""
        import ggnn_amd as ggnn
        from ggnn_amd import _lib
        m = ggnn.DistanceMeasure.Euclidean if measure is None else measure
        self.eng.set_prescreen(prescreen)
        try:
            with _lib.hooks(PS_EXACT=exact):
                if how == "plain":
                    ids, d = self.eng.query(q, k, TAU, iters, m)
                elif how == "bitset":
                    ids, d = self.eng.query_filtered(q, k, TAU, iters, m, filter=arg)
                elif how == "table":
                    ids, d = self.eng.query_filtered_by(q, k, TAU, iters, m, filter_ids=arg)
                else:
                    ids, d = self.eng.query_labeled(q, k, TAU, iters, m, labels=arg)
        finally:
            self.eng.set_prescreen(True)
        return (np.asarray(ids).copy(), np.asarray(d).copy(), self.eng.last_query_counters(),
                self.eng.last_query_rows_read())


_cases = {}


@pytest.fixture(scope="module")
def case():
    def get(name, d=128):
        if (name, d) not in _cases:
            base, queries = _dataset(name, d)
            _cases[(name, d)] = (Case(base), queries)
        return _cases[(name, d)]
    yield get
    _cases.clear()


def true_l2(base, q, ids):
    """float32 squared distances of the returned ids; exact in float64 for data on these grids"""
    rows = base[np.maximum(ids, 0)].astype(np.float64)
    d = ((rows - q[:, None, :].astype(np.float64)) ** 2).sum(-1)
    return np.where(ids >= 0, d, np.inf).astype(F)


def assert_same(a, b):
    assert np.array_equal(a[0], b[0]), "ids differ"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "distances differ"
    assert a[2] == b[2], (a[2], b[2])


def three_way(c, q, **kw):
    """default kernels against PS_EXACT = 0 and against no pre-screen: ids, distances, n_dist and
    n_pop bit-equal.  Returns the (default, PS_EXACT = 0) results."""
    on = c.search(q, exact=1, **kw)
    off = c.search(q, exact=0, **kw)
    plain = c.search(q, prescreen=False, **kw)
    assert_same(on, off)
    assert_same(on, plain)
    assert off[3]["code_rows"] == on[3]["code_rows"]
    assert plain[3]["code_rows"] == 0
    return on, off


def mixed_queries(base, grid_q, step):
    """on-grid rows, a copy of a base row, one coordinate one step outside the coded range on
    either side (clamped), and fractional rows (rows 4 and 5 of every eight: their float32 sums
    round, INTEGRAL_ROWS are the others)"""
    q = grid_q.copy()
    q[1] = base[4321]
    q[2::8, 5] = base[:, 5].min() - step
    q[3::8, 77 % q.shape[1]] = base[:, 77 % q.shape[1]].max() + step
    q[4::8] += F(0.5) * step
    q[5::8, 11] += F(0.25) * step
    return q


INTEGRAL_ROWS = (np.arange(NQ) % 8 < 4) | (np.arange(NQ) % 8 > 5)


def assert_true_distances(c, q, res):
    rows = INTEGRAL_ROWS[:len(q)]
    assert np.array_equal(res[1][rows], true_l2(c.base, q[rows], res[0][rows]))


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
    mask = np.random.default_rng(1).random(N) < 0.3
    on = c.search(q, how="bitset", arg=mask)
    off = c.search(q, exact=0, how="bitset", arg=mask)
    assert_same(on, off)
    assert on[3]["float_rows"] < off[3]["float_rows"] and on[3]["code_rows"] == off[3]["code_rows"]
    assert mask[on[0][on[0] >= 0]].all()


def test_under_a_filter_table(case):
    c, q = case("int")
    rng = np.random.default_rng(2)
    c.eng.set_filters(np.stack([rng.random(N) < 0.5, rng.random(N) < 0.05]))
    try:
        fid = rng.integers(-1, 2, NQ).astype(np.int32)
        on = c.search(q, how="table", arg=fid)
        off = c.search(q, exact=0, how="table", arg=fid)
    finally:
        c.eng.set_filters(None)
    assert_same(on, off)
    assert on[3]["float_rows"] < off[3]["float_rows"] and on[3]["code_rows"] == off[3]["code_rows"]


@pytest.mark.parametrize("d", [128, 96])
def test_under_labels(case, d):
    c, q = case("int", d)
    rng = np.random.default_rng(4)
    labels = rng.integers(0, 4, N).astype(np.int32)
    c.eng.set_labels(labels)
    ql = rng.integers(-1, 4, NQ).astype(np.int32)
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
