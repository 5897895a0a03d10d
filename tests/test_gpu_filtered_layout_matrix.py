"""The filtered, table and labelled kernels on every row layout: traversal and scan against plain
CPU references, bit for bit (ids equal, distances as bytes, counters equal; no tolerance).

pick_dist_config (ggnn_amd/csrc/traversal.hpp) gives every (D, element type) one of seven
<LPR, NCH> layouts, and query_filtered_kernel* / query_labeled_kernel* and the FILT / LAB forms of
bf_query_kernel / bf_query_lds_kernel are instantiated per layout, element type and measure.
MATRIX has a case for every (type, layout, measure) cell a D in [1, 4096] reaches, for float32,
float32 with the pre-screen (f32_ps), uint8, float16 and bfloat16;
tests/test_filtered_layout_coverage.py checks that on the CPU against the layout table itself.

Data: one integer base and one query set per (D, measure), shared by all types, values in [0, m]
with m = min(127, isqrt((2^24 - 1) // D)): exact in all four element types, and every float32 sum
(squared differences, dot products, norms) is an integer below 2^24, so it is exact in any order.
One label column per (D, measure); the filter table and the per-call bitsets are derived from it,
so one Python reference per query (tests/filtered_reference.py, py_query_filtered) serves every
entry point.  Before any GPU result is judged the reference itself is checked on the CPU
(`reference`): with the all-ones mask it equals the C++ oracle's orc.query in both summation
orders (ids, distance bytes, n_dist, n_pop), and the filtered rows have the shape the cases are
meant to have (an empty row, a row with fewer than K entries, full rows).

Data, graph and reference construction are plain functions that need no GPU."""
import math

import numpy as np
import pytest

from filtered_reference import bf_filtered_reference, pack_bits, py_query_filtered

pytestmark = pytest.mark.gpu

# one D per layout: {8,1} {8,2} {8,3} {16,2} {16,4} {64,4} {64,16} (uint8 does not reach the last)
F32_DIMS = (32, 64, 96, 128, 256, 1024, 4096)
HALF_DIMS = (64, 128, 192, 256, 512, 1024, 4096)
U8_DIMS = (64, 256, 384, 512, 1024, 4096)
TYPE_DIMS = {"f32": F32_DIMS, "f32_ps": F32_DIMS, "u8": U8_DIMS, "f16": HALF_DIMS,
             "bf16": HALF_DIMS}
# (type, D, measure); read as data by tests/test_filtered_layout_coverage.py
MATRIX = [(t, D, m) for t, dims in TYPE_DIMS.items() for D in dims for m in (0, 1)]
IDS = [f"{t}-D{D}-{'cos' if m else 'l2'}" for t, D, m in MATRIX]
SCAN_MATRIX = [c for c in MATRIX if c[0] != "f32_ps"]      # the scan has no pre-screen
SCAN_IDS = [f"{t}-D{D}-{'cos' if m else 'l2'}" for t, D, m in SCAN_MATRIX]

KB = 24
NQ = 8
# -1: unfiltered; 7: a label no row carries; 4: exactly six rows; label 0 twice (a sub-batch of two)
QLABELS = np.array([-1, 0, 1, 2, 3, 4, 7, 0], np.int32)
N_TABLE = 5                  # table rows = labels 0..4; id 7 is outside the table
RARE, RARE_ROWS, UNUSED = 4, 6, 7
BASE_POINT = (10, 0.6, 200)  # (K, tau, iterations)
R2_POINT = (100, 0.6, 300)   # sorted 128: the R = 2 register list
LDS_POINT = (2100, 0.5, 64)  # sorted 2144: the LDS list
TABLE_OFFSET, LABEL_OFFSET = 37, 5


def points_for(D):
    pts = [BASE_POINT]
    if D in (96, 128, 1024):
        pts.append(R2_POINT)
    if D == 128:
        pts.append(LDS_POINT)
    return pts


# ---- data, graph, reference: CPU only --------------------------------------------------------------
def n_rows(D):
    return 1100 if D <= 512 else 400


def max_value(D):
    return min(127, math.isqrt((2 ** 24 - 1) // D))


_data, _graphs, _refs = {}, {}, {}


def data(D, measure):
    """base [N, D], queries [8, D] (float32 integers in [0, m]) and the label column [N]"""
    key = (D, measure)
    if key not in _data:
        N, m = n_rows(D), max_value(D)
        assert D * m * m < 2 ** 24
        rng = np.random.default_rng(7000 + 2 * D + measure)
        base = rng.integers(0, m + 1, (N, D)).astype(np.float32)
        q = rng.integers(0, m + 1, (NQ, D)).astype(np.float32)
        assert (base.sum(1) > 0).all() and (q.sum(1) > 0).all()     # no zero-norm row
        labels = rng.choice(5, N, p=[.5, .3, .15, .04, .01]).astype(np.int32)
        had = labels == RARE
        forced = rng.choice(np.nonzero(~had)[0], RARE_ROWS, replace=False)
        labels[had] = 3
        labels[forced] = RARE
        assert int((labels == RARE).sum()) == RARE_ROWS and not (labels == UNUSED).any()
        _data[key] = base, q, labels
    return _data[key]


def graph(orc, D, measure):
    key = (D, measure)
    if key not in _graphs:
        base = data(D, measure)[0]
        N = base.shape[0]
        cfg, gr, tr, sel, stats = orc.build(base, KB, 0.5, 0, measure=measure,
                                            rng=orc.make_rng(N, 11))
        start = np.ascontiguousarray(tr[cfg.STs_offsets[3]:cfg.STs_offsets[3] + cfg.Ns[3]])
        _graphs[key] = dict(graph0=np.ascontiguousarray(gr[:N]), start=start,
                            stats=np.asarray(stats, np.float32))
    return _graphs[key]


def allowed_of(labels, L):
    """the whole contract: the rows that carry L; everything for -1"""
    return np.ones(len(labels), bool) if L == -1 else labels == L


def _stack(rows):
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
            np.array([r[2] for r in rows], np.int64), np.array([r[3] for r in rows], np.int64))


def reference(orc, D, measure, point):
    """(ids [8, K], dists [8, K], n_dist [8], n_pop [8]) of the Python reference under QLABELS,
    after the checks of the reference itself"""
    key = (D, measure, point)
    if key in _refs:
        return _refs[key]
    K, tau, iters = point
    base, q, labels = data(D, measure)
    g = graph(orc, D, measure)
    N = base.shape[0]

    def py(i, allowed):
        return py_query_filtered(base, q[i], g["graph0"], g["start"], g["stats"], K, tau, iters,
                                 allowed, cosine=bool(measure))

    rows = [py(i, allowed_of(labels, int(L))) for i, L in enumerate(QLABELS)]
    ref = _stack(rows)
    # 1. the all-ones mask is the oracle's unfiltered search, in both summation orders: every query
    # at the point all cells share, the unfiltered query (label -1) at the others
    unfiltered = np.nonzero(QLABELS == -1)[0]
    sel = np.arange(NQ) if point == BASE_POINT else unfiltered
    ones = _stack([rows[i] if i in unfiltered else py(i, np.ones(N, bool)) for i in sel])
    for wave in (False, True):
        orc.set_wave_order(wave)
        try:
            o = orc.query(base, q[sel], g["graph0"], g["start"], g["stats"], K, tau, iters, measure,
                          counters=True)
        finally:
            orc.set_wave_order(False)
        what = (D, measure, point, "wave order" if wave else "reference order")
        assert np.array_equal(ones[0], o[0]), what
        assert ones[1].tobytes() == o[1].tobytes(), what
        assert np.array_equal(ones[2], o[2]) and np.array_equal(ones[3], o[3]), what
    # 2. the rows are what the cases are meant to be
    ids, d = ref[0], ref[1]
    fin = np.isfinite(d)
    assert ((ids == -1) == ~fin).all()
    for i, L in enumerate(QLABELS):
        n_fin = int(fin[i].sum())
        size = N if L == -1 else int((labels == L).sum())
        assert not fin[i, n_fin:].any(), (key, i)
        assert L == -1 or (labels[ids[i, :n_fin]] == L).all(), (key, i)
        if L == UNUSED:
            assert n_fin == 0, (key, i)
        elif L == RARE:
            assert 1 <= n_fin <= RARE_ROWS, (key, i, n_fin)
        elif point == BASE_POINT or size >= K:
            assert n_fin == K, (key, i, n_fin)
        else:   # K = 100 / 2100 exceeds the smaller classes (and N): such a list cannot be full
            assert 1 <= n_fin <= size, (key, i, n_fin)
    _refs[key] = ref
    return ref


_bf_refs = {}


def bf_reference(orc, D, measure, K):
    """exact filtered K nearest under QLABELS: the oracle on the compacted rows, per label"""
    key = (D, measure, K)
    if key not in _bf_refs:
        base, q, labels = data(D, measure)
        ids = np.empty((NQ, K), np.int32)
        d = np.empty((NQ, K), np.float32)
        for L in np.unique(QLABELS):
            sel = np.nonzero(QLABELS == L)[0]
            ids[sel], d[sel] = bf_filtered_reference(orc, base, q[sel], K,
                                                     allowed_of(labels, int(L)), measure)
        n_fin = np.isfinite(d).sum(1)
        sizes = [base.shape[0] if L == -1 else int((labels == L).sum()) for L in QLABELS]
        assert n_fin.tolist() == [min(K, s) for s in sizes]
        _bf_refs[key] = ids, d
    return _bf_refs[key]


# ---- the GPU side ------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ops():
    assert _torch().cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def _cast(a, kind):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = {"f32": t.float(), "u8": t.to(torch.uint8), "f16": t.to(torch.float16),
         "bf16": t.to(torch.bfloat16)}[kind.split("_")[0]]
    return t.contiguous().cuda()


def _i32(a):
    return _torch().from_numpy(np.ascontiguousarray(np.asarray(a, np.int32))).cuda()


def _bits(mask):
    return _torch().from_numpy(pack_bits(mask).view(np.int32).copy()).cuda()


def _table(masks):
    return _torch().from_numpy(np.stack([pack_bits(m) for m in masks]).view(np.int32).copy()).cuda()


class Filters:
    """the three filter forms of one label column, on the device"""

    def __init__(self, labels, seed):
        N = len(labels)
        rng = np.random.default_rng(seed)
        masks = np.stack([labels == f for f in range(N_TABLE)])
        self.labels, self.qlabels = _i32(labels), _i32(QLABELS)
        self.table = _table(masks)
        wide = rng.random((N_TABLE, TABLE_OFFSET + N + 50)) < 0.5
        wide[:, TABLE_OFFSET:TABLE_OFFSET + N] = masks
        self.wide_table = _table(wide)
        self.wide_labels = _i32(np.concatenate([rng.integers(0, 5, LABEL_OFFSET), labels,
                                                rng.integers(0, 5, 9)]))
        self.by_label = {int(L): (np.nonzero(QLABELS == L)[0], _bits(allowed_of(labels, int(L))))
                         for L in np.unique(QLABELS)}


def assert_query_equals(res, ref, rows, what):
    ids, d, nd, npop = [x.cpu().numpy() for x in res]
    assert np.array_equal(ids, ref[0][rows]), (what, "ids")
    assert d.tobytes() == ref[1][rows].tobytes(), (what, "dists")
    assert np.array_equal(nd, ref[2][rows]), (what, "n_dist")
    assert np.array_equal(npop, ref[3][rows]), (what, "n_pop")


def run_traversal(ops, kind, D, measure, point, ref, tag):
    """every filtered entry point of the traversal at one point, against `ref`"""
    K, tau, iters = point
    base, q, labels = data(D, measure)
    g = _dev_graph(D, measure)
    f = _filters(D, measure)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    ps = ops.prescreen_encode(d_base, measure) if kind == "f32_ps" else None
    head = (d_base, d_q, g["graph0"], g["start"], g["stats"], K, tau)
    kw = dict(counters=True, prescreen=ps)
    every = np.arange(NQ)
    what = (kind, D, measure, point, tag)
    assert_query_equals(ops.query_labeled(*head, f.labels, f.qlabels, iters, measure, **kw),
                        ref, every, what + ("labels",))
    assert_query_equals(ops.query_filtered_by(*head, f.table, f.qlabels, iters, measure, **kw),
                        ref, every, what + ("table",))
    assert_query_equals(ops.query_filtered_by(*head, f.wide_table, f.qlabels, iters, measure,
                                              filter_bit_offset=TABLE_OFFSET, **kw),
                        ref, every, what + ("table window",))
    for L, (rows, bits) in f.by_label.items():
        sub = (d_base, d_q[_torch().from_numpy(rows).cuda()].contiguous()) + head[2:]
        assert_query_equals(ops.query_filtered(*sub, bits, iters, measure, **kw),
                            ref, rows, what + ("bitset", L))
    assert_query_equals(ops.query_labeled(*head, f.wide_labels, f.qlabels, iters, measure,
                                          bit_offset=LABEL_OFFSET, **kw),
                        ref, every, what + ("label window",))


_dev_graphs, _dev_filters = {}, {}


def _dev_graph(D, measure):
    return _dev_graphs[(D, measure)]


def _filters(D, measure):
    return _dev_filters[(D, measure)]


def _upload(orc, D, measure):
    key = (D, measure)
    if key not in _dev_graphs:
        g = graph(orc, D, measure)
        _dev_graphs[key] = {k: _torch().from_numpy(v).cuda() for k, v in g.items()}
        _dev_filters[key] = Filters(data(D, measure)[2], 90 + D + measure)


@pytest.mark.parametrize("kind,D,measure", MATRIX, ids=IDS)
def test_filtered_traversal(ops, orc, kind, D, measure):
    """query_labeled, query_filtered_by (at offset 0 and as a window at bit offset 37 of a wider
    random table), query_filtered per distinct label on its sub-batch, and query_labeled on a window
    at offset 5 of a longer column: each with counters, each equal to the Python reference.  K = 10
    in every cell; K = 100 (the R = 2 register list) at D = 96, 128 and 1024; at D = 128 also
    K = 2100 (the LDS list), and float32 with and without the pre-screen under QUERY_EARLY = 0
    (the round-1..4 order of the headline layout)."""
    from ggnn_amd import _lib
    _upload(orc, D, measure)
    for point in points_for(D):
        ref = reference(orc, D, measure, point)
        run_traversal(ops, kind, D, measure, point, ref, "default")
        if D == 128 and kind in ("f32", "f32_ps") and point != LDS_POINT:
            with _lib.hooks(QUERY_EARLY=0):
                run_traversal(ops, kind, D, measure, point, ref, "QUERY_EARLY=0")


@pytest.mark.parametrize("kind,D,measure", SCAN_MATRIX, ids=SCAN_IDS)
def test_filtered_scan(ops, orc, kind, D, measure):
    """bf_query_kernel<.., FILT, LAB> (8 queries: never the matrix cores) in the same cells: K = 10
    (register list) and K = 300 (bf_query_lds_kernel), labels, table and per-call bitsets, against
    the oracle on the compacted rows; the call reports the scan path"""
    _upload(orc, D, measure)
    base, q, labels = data(D, measure)
    f = _filters(D, measure)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    for K in (10, 300):
        r_ids, r_d = bf_reference(orc, D, measure, K)

        def check(res, rows, what):
            ids, d, resc, path = res
            assert (resc, path) == (0, 0), (what, resc, path)
            assert np.array_equal(ids.cpu().numpy(), r_ids[rows]), (kind, D, measure, K, what)
            assert d.cpu().numpy().tobytes() == r_d[rows].tobytes(), (kind, D, measure, K, what)

        every = np.arange(NQ)
        check(ops.bf_query_labeled(d_base, d_q, K, f.labels, f.qlabels, measure, rescanned=True),
              every, "labels")
        check(ops.bf_query_labeled(d_base, d_q, K, f.wide_labels, f.qlabels, measure,
                                   bit_offset=LABEL_OFFSET, rescanned=True), every, "label window")
        check(ops.bf_query_filtered_by(d_base, d_q, K, f.table, f.qlabels, measure, rescanned=True),
              every, "table")
        check(ops.bf_query_filtered_by(d_base, d_q, K, f.wide_table, f.qlabels, measure,
                                       filter_bit_offset=TABLE_OFFSET, rescanned=True),
              every, "table window")
        for L, (rows, bits) in f.by_label.items():
            sub = d_q[_torch().from_numpy(rows).cuda()].contiguous()
            check(ops.bf_query_filtered(d_base, sub, K, bits, measure, rescanned=True), rows,
                  ("bitset", L))
