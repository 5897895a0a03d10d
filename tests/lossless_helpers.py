"""What the GPU tests of "Distances from lossless codes" share (tests/test_gpu_lossless_prescreen.py,
tests/test_gpu_lossless_matrix.py): data on dyadic grids, an engine per data set kept for the module,
the comparison of the default kernels with hook PS_EXACT = 0 and with set_prescreen(False), and the
filters of the filtered cells.  Importing it needs no GPU."""
import numpy as np
import pytest

N, NQ, K, KBUILD = 20000, 256, 10, 24      # EARLY needs KBuild <= 24
TAU = 0.7
F = np.float32


def _ints(rng, n, d, lo=0, hi=256):
    return rng.integers(lo, hi, (n, d)).astype(F)


# name -> (base, on-grid queries): float32 rows on a dyadic grid of at most 256 levels
SEEDS = {"int": 11, "quarter": 12, "four": 13, "signed": 14, "big": 15, "frac": 16}


def dataset(name, d=128, n=N):
    rng = np.random.default_rng(SEEDS[name] * 1000 + d)
    if name == "int":
        return _ints(rng, n, d), _ints(rng, NQ, d)
    if name == "quarter":                      # values k / 4: scale 2^-2
        return _ints(rng, n, d) * F(0.25), _ints(rng, NQ, d) * F(0.25)
    if name == "four":                         # values 4 k: scale 4
        return _ints(rng, n, d) * F(4), _ints(rng, NQ, d) * F(4)
    if name == "signed":                       # values in [-128, 127]: negative offsets
        return _ints(rng, n, d, -128, 128), _ints(rng, NQ, d, -128, 128)
    if name == "big":                          # values 2^23 + k: offsets at the certificate's edge
        return _ints(rng, n, d) + F(2.0 ** 23), _ints(rng, NQ, d) + F(2.0 ** 23)
    if name == "frac":                         # genuinely fractional rows: no lossless copy
        centres = rng.normal(size=(16, d)) * 30 + 128
        mk = lambda m: (centres[rng.integers(0, 16, m)] + rng.normal(size=(m, d)) * 12).astype(F)
        return mk(n), mk(NQ)
    raise KeyError(name)


class Case:
    """an engine with its graph, kept for the module: one build per data set"""

    def __init__(self, base, kbuild=KBUILD):
        import ggnn_amd as ggnn
        self.base = base
        self.eng = ggnn.GGNN()
        self.eng.set_collect_counters(True)
        self.eng.set_base(base)
        self.eng.build(kbuild, 0.5, 1)

    def flag(self, measure=0):
        """params[5] of a pre-screen copy of this base (the engine's own copy is coded alike: rows
        padded with zeros to whole 16-byte chunks)"""
        import torch
        from ggnn_amd import ops
        base = np.pad(self.base, ((0, 0), (0, -self.base.shape[1] % 4)))
        _, params = ops.prescreen_encode(torch.from_numpy(base).cuda(), measure)
        return float(params[5].item())

    def search(self, q, *, exact=1, prescreen=True, iters=175, k=K, tau=TAU, how="plain", arg=None,
               measure=None, hooks=None):
        """(ids, dists, counters, rows read) of one blocking search"""
        import ggnn_amd as ggnn
        from ggnn_amd import _lib
        m = ggnn.DistanceMeasure.Euclidean if measure is None else measure
        self.eng.set_prescreen(prescreen)
        try:
            with _lib.hooks(PS_EXACT=exact, **(hooks or {})):
                if how == "plain":
                    ids, d = self.eng.query(q, k, tau, iters, m)
                elif how == "bitset":
                    ids, d = self.eng.query_filtered(q, k, tau, iters, m, filter=arg)
                elif how == "table":
                    ids, d = self.eng.query_filtered_by(q, k, tau, iters, m, filter_ids=arg)
                else:
                    ids, d = self.eng.query_labeled(q, k, tau, iters, m, labels=arg)
        finally:
            self.eng.set_prescreen(True)
        return (np.asarray(ids).copy(), np.asarray(d).copy(), self.eng.last_query_counters(),
                self.eng.last_query_rows_read())


_cases = {}


@pytest.fixture(scope="module")
def case():
    def get(name, d=128, n=N, kbuild=KBUILD):
        key = (name, d) if (n, kbuild) == (N, KBUILD) else (name, d, n, kbuild)
        if key not in _cases:
            base, queries = dataset(name, d, n)
            _cases[key] = (Case(base, kbuild), queries)
        return _cases[key]
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


# ---- the filters of the filtered cells: a bitset of 30 %, a table of two rows (50 % and 5 %) with
# ---- filter ids in {-1, 0, 1}, four labels with query labels in {-1 .. 3} --------------------------
def bitset_filter(n):
    return np.random.default_rng(1).random(n) < 0.3


def table_filter(n, nq=NQ):
    """(masks [2, n], filter ids [nq] int32)"""
    rng = np.random.default_rng(2)
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.05])
    return masks, rng.integers(-1, 2, nq).astype(np.int32)


def label_filter(n, nq=NQ):
    """(labels [n] int32, query labels [nq] int32)"""
    rng = np.random.default_rng(4)
    labels = rng.integers(0, 4, n).astype(np.int32)
    return labels, rng.integers(-1, 4, nq).astype(np.int32)
