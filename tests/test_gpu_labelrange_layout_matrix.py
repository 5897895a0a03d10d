"""The label-range kernels on every row layout: one traversal case and one scan case per (type,
layout, measure) cell, against plain CPU references, bit for bit (ids equal, distances as bytes,
counters equal; no tolerance).

query_labelrange_kernel* (query_labelrange.hip, query_labelrange_16.hip) and
bf_query_labelrange_kernel* (bf_query_labelrange.hip) are instantiated per row layout <LPR, NCH>,
element type and measure, next to the label-set kernels.  Data, graphs, label column and the cells
(MATRIX, SCAN_MATRIX) are those of tests/test_gpu_filtered_layout_matrix.py: integer data whose
float32 sums are exact in any order, one label column per (D, measure) with classes 0..4, RARE (4)
on exactly six rows, UNUSED on none.

The contract in one line:
    allowed[n] = any_j(lo_j <= labels <= hi_j) & row(filter_ids[n])
with row -1 all ones, an id outside the table empty and an interval with lo > hi empty, and the
reference is filtered_reference.py_query_filtered under that mask.

The traversal runs at the point all cells share (K 10, 200 iterations: the early-rows kernels where
the layout's first read is 8 lanes x one chunk, the R = 1 kernel elsewhere), the scan at K 10.  The
other rungs of the ladder (every list size and hook on every layout) are compared on layout {8,1} in
tests/test_gpu_label_ranges.py only."""
import numpy as np
import pytest

from filtered_reference import bf_filtered_reference, py_query_filtered
from test_gpu_filtered_layout_matrix import (BASE_POINT, IDS, MATRIX, NQ, RARE, SCAN_IDS, SCAN_MATRIX,
                                             UNUSED, _cast, _i32, _table, data, graph)
from test_gpu_filtered_layout_matrix import ops  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

MIN, MAX = -2 ** 31, 2 ** 31 - 1
# everything; two classes; two classes and a label no row carries; the six RARE rows; nothing (an
# empty interval and a label no row carries); RARE and class 3 under the 5 % row; one class between
# two empty intervals (what an unsigned span compare alone gets wrong); every class at once
RANGES = [[(MIN, MAX)], [(0, 1)], [(2, 3), (UNUSED, UNUSED)], [(RARE, RARE)], [(1, 0), (UNUSED, 9000)],
          [(RARE, RARE), (3, 3)], [(5, 4), (2, 2), (MAX, MIN)], [(0, 4)]]
FIDS = np.array([-1, -1, 0, -1, 2, 1, 2, 0], np.int32)
assert len(RANGES) == NQ and RARE == 4
SCAN_K = 10


def _torch():
    import torch
    return torch


def table(n, D, measure):
    """three rows: about 50 % random, about 5 % random, every id but every seventh"""
    u = np.random.default_rng(500 + D + measure).random((2, n))
    return np.stack([u[0] < 0.5, u[1] < 0.05, np.arange(n) % 7 != 0])


def _in_ranges(labels, r):
    lab = labels.astype(np.int64)
    out = np.zeros(len(lab), bool)
    for lo, hi in r:
        out |= (lab >= lo) & (lab <= hi)
    return out


def _row(tab, f):
    if f == -1:
        return np.ones(tab.shape[1], bool)
    return tab[f] if 0 <= f < len(tab) else np.zeros(tab.shape[1], bool)


def composed(D, measure):
    """the whole contract: one allowed array per query, [8, N]"""
    labels = data(D, measure)[2]
    tab = table(len(labels), D, measure)
    return np.stack([_in_ranges(labels, r) & _row(tab, int(FIDS[i])) for i, r in enumerate(RANGES)])


def padded(lists, width=4):
    """[Nq, width, 2] int32: every list padded with the empty interval (1, 0)"""
    return np.array([list(r) + [(1, 0)] * (width - len(r)) for r in lists],
                    np.int64).astype(np.int32).reshape(len(lists), width, 2)


_refs, _bf_refs = {}, {}


def reference(orc, D, measure):
    """(ids [8, K], dists [8, K], n_dist [8], n_pop [8]) of the Python reference under RANGES and
    FIDS at BASE_POINT, after a look at the rows: an empty one, the six RARE rows at most, full ones"""
    key = (D, measure)
    if key not in _refs:
        K, tau, iters = BASE_POINT
        base, q, labels = data(D, measure)
        g = graph(orc, D, measure)
        allowed = composed(D, measure)
        rows = [py_query_filtered(base, q[i], g["graph0"], g["start"], g["stats"], K, tau, iters,
                                  allowed[i], cosine=bool(measure)) for i in range(NQ)]
        ref = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
               np.array([r[2] for r in rows], np.int64), np.array([r[3] for r in rows], np.int64))
        n_fin = np.isfinite(ref[1]).sum(1)
        assert not allowed[4].any() and n_fin[4] == 0, key
        assert int(allowed[3].sum()) == 6 and 1 <= n_fin[3] <= 6, (key, n_fin)
        assert np.array_equal(allowed[6], (labels == 2) & table(len(labels), D, measure)[2]), key
        assert (n_fin == K).sum() >= 4 and n_fin[6] > 0, (key, n_fin)
        _refs[key] = ref
    return _refs[key]


def bf_reference(orc, D, measure):
    key = (D, measure)
    if key not in _bf_refs:
        base, q, labels = data(D, measure)
        allowed = composed(D, measure)
        rows = [bf_filtered_reference(orc, base, q[i:i + 1], SCAN_K, allowed[i], measure)
                for i in range(NQ)]
        ids, d = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
        assert np.isfinite(d).sum(1).tolist() == [min(SCAN_K, int(a.sum())) for a in allowed]
        assert (ids[3, :6] >= 0).all() and (ids[3, 6:] == -1).all() and (labels[ids[3, :6]] == RARE).all()
        _bf_refs[key] = ids, d
    return _bf_refs[key]


# ---- the GPU side ------------------------------------------------------------------------------------
_dev = {}


def _device(orc, D, measure):
    """(graph arguments, label column, table, ranges, ids) of one (D, measure) on the device"""
    key = (D, measure)
    if key not in _dev:
        g = graph(orc, D, measure)
        labels = data(D, measure)[2]
        _dev[key] = (tuple(_torch().from_numpy(g[k]).cuda() for k in ("graph0", "start", "stats")),
                     _i32(labels), _table(table(len(labels), D, measure)), _i32(padded(RANGES)),
                     _i32(FIDS))
    return _dev[key]


@pytest.mark.parametrize("kind,D,measure", MATRIX, ids=IDS)
def test_labelrange_traversal(ops, orc, kind, D, measure):
    """ops.query_labeled_range with four intervals, filter ids and the table, with counters, against
    the Python reference"""
    d_graph, d_labels, d_table, d_ranges, d_fids = _device(orc, D, measure)
    K, tau, iters = BASE_POINT
    ref = reference(orc, D, measure)
    base, q, _ = data(D, measure)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    ps = ops.prescreen_encode(d_base, measure) if kind == "f32_ps" else None
    ids, d, nd, npop = [x.cpu().numpy() for x in ops.query_labeled_range(
        d_base, d_q, *d_graph, K, tau, d_labels, d_ranges, d_table, d_fids, max_iterations=iters,
        measure=measure, counters=True, prescreen=ps)]
    assert np.array_equal(ids, ref[0])
    assert d.tobytes() == ref[1].tobytes()
    assert np.array_equal(nd, ref[2]) and np.array_equal(npop, ref[3])


@pytest.mark.parametrize("kind,D,measure", SCAN_MATRIX, ids=SCAN_IDS)
def test_labelrange_scan(ops, orc, kind, D, measure):
    """ops.bf_query_labeled_range at K = 10 with four intervals, filter ids and the table, against
    the oracle on the compacted rows of every query"""
    _, d_labels, d_table, d_ranges, d_fids = _device(orc, D, measure)
    r_ids, r_d = bf_reference(orc, D, measure)
    base, q, _ = data(D, measure)
    ids, d = ops.bf_query_labeled_range(_cast(base, kind), _cast(q, kind), SCAN_K, d_labels, d_ranges,
                                        d_table, d_fids, measure)
    ids, d = ids.cpu().numpy(), d.cpu().numpy()
    assert np.array_equal(ids, r_ids)
    assert d.tobytes() == r_d.tobytes()
