"""The label-mask kernels on every row layout: one traversal cell and one scan cell per (type, D,
measure), bit for bit (ids equal, distances as bytes, counters equal; no tolerance).

query_labelmask_kernel* (query_labelmask.hip, query_labelmask_16.hip) and bf_query_labelmask_kernel*
(bf_query_labelmask.hip) are instantiated per row layout <LPR, NCH>, element type and measure, next
to the label-range kernels.  Data, graphs, classes and the cells (MATRIX, SCAN_MATRIX) are those of
tests/test_gpu_filtered_layout_matrix.py; the tag column gives every class 0..4 a bit, two random
tags, bit 31 to the six RARE rows and label 0 to three rows.

The contract in one line:
    allowed[n] = any_j(((labels & mask_j) == value_j) & ((any_j == 0) | ((labels & any_j) != 0)))
                 & row(filter_ids[n])
with row -1 all ones and an id outside the table empty.  The reference is the EXISTING GPU entry
point ops.query_filtered_by / ops.bf_query_filtered_by on the table of those masks, composed on the
CPU: tests/test_gpu_filtered_layout_matrix.py pins those kernels to the CPU references in the same
cells.

The traversal runs at the point all cells share (K 10, 200 iterations) and, at the D values where
points_for adds them, at the R = 2 and LDS-list points; the scan at K 10, and at K 300 where the
traversal has its LDS point."""
import numpy as np
import pytest

from test_gpu_filtered_layout_matrix import (BASE_POINT, IDS, LDS_POINT, MATRIX, NQ, RARE, SCAN_IDS,
                                             SCAN_MATRIX, _cast, _i32, _table, data, graph, n_rows,
                                             points_for)
from test_gpu_filtered_layout_matrix import ops  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

T8, T9, B31 = 1 << 8, 1 << 9, 0x80000000
# everything; class 0 or class 1 (two clauses); any of class 2, 3 under the 50 % row; the six RARE
# rows by bit 31; a value with a bit outside its mask (nothing); RARE or class 3 under the 5 % row;
# class 2 without tag 8 and with tag 9, next to a clause no row satisfies; none of tag 8
MASKS = [[(0, 0, 0)], [(1, 1, 0), (2, 2, 0)], [(0, 0, 4 | 8)], [(B31, B31, 0)], [(1, 1 | T8, 0)],
         [(0, 0, B31 | 8)], [(4 | T8, 4, T9), (1 | 2, 1 | 2, 0)], [(T8, 0, 0)]]
FIDS = np.array([-1, -1, 0, -1, 2, 1, 2, 0], np.int32)
assert len(MASKS) == NQ and RARE == 4
ZERO_ROWS = 3


def _torch():
    import torch
    return torch


def tags(D, measure):
    """the int32 tag column of one (D, measure): bit c for class c, two random tags at a share of
    0.3, bit 31 on the RARE rows, 0 on the first three rows of class 0"""
    classes = data(D, measure)[2]
    assert len(classes) == n_rows(D)
    rs = np.random.default_rng(900 + D + measure)
    lab = np.int64(1) << classes.astype(np.int64)
    lab[rs.random(len(lab)) < 0.3] |= T8
    lab[rs.random(len(lab)) < 0.3] |= T9
    lab[classes == RARE] |= B31
    lab[np.nonzero(classes == 0)[0][:ZERO_ROWS]] = 0
    return lab.astype(np.uint32).view(np.int32)


def table(n, D, measure):
    """three rows: about 50 % random, about 5 % random, every id but every seventh"""
    u = np.random.default_rng(500 + D + measure).random((2, n))
    return np.stack([u[0] < 0.5, u[1] < 0.05, np.arange(n) % 7 != 0])


def _passes(labels, clauses):
    """the definition, in bool / int64 numpy"""
    lab = labels.astype(np.int64) & 0xffffffff
    out = np.zeros(len(lab), bool)
    for mask, value, any_ in clauses:
        out |= ((lab & mask) == value) & ((any_ == 0) | ((lab & any_) != 0))
    return out


def _row(tab, f):
    if f == -1:
        return np.ones(tab.shape[1], bool)
    return tab[f] if 0 <= f < len(tab) else np.zeros(tab.shape[1], bool)


def composed(D, measure):
    """the whole contract: one allowed array per query, [8, N], after a look at what it selects"""
    labels, classes = tags(D, measure), data(D, measure)[2]
    tab = table(len(labels), D, measure)
    allowed = np.stack([_passes(labels, r) & _row(tab, int(FIDS[i])) for i, r in enumerate(MASKS)])
    live = np.ones(len(labels), bool)
    live[np.nonzero(classes == 0)[0][:ZERO_ROWS]] = False
    assert allowed[0].all() and not allowed[4].any()
    assert np.array_equal(allowed[1], (classes <= 1) & live)
    assert np.array_equal(allowed[2], ((classes == 2) | (classes == 3)) & tab[0])
    assert np.array_equal(allowed[3], classes == RARE) and allowed[3].sum() == 6
    assert np.array_equal(allowed[5], (classes >= 3) & tab[1])
    assert np.array_equal(allowed[6], (classes == 2) & ((labels & T8) == 0) & ((labels & T9) != 0) & tab[2])
    assert allowed[6].any() and allowed[7].any() and not allowed[7].all()
    return allowed


def padded(lists, width=2):
    """[Nq, width, 3] int32: every list padded by repeating its first clause"""
    wrap = lambda v: v - (1 << 32) if v >= (1 << 31) else v  # noqa: E731
    return np.array([[[wrap(v) for v in c] for c in list(r) + [r[0]] * (width - len(r))] for r in lists],
                    np.int32).reshape(len(lists), width, 3)


_dev = {}


def _device(orc, D, measure):
    """(graph arguments, tag column, table, clauses, ids, composed table, its ids, the composed
    masks) of one (D, measure) on the device"""
    key = (D, measure)
    if key not in _dev:
        g = graph(orc, D, measure)
        labels = tags(D, measure)
        allowed = composed(D, measure)
        _dev[key] = (tuple(_torch().from_numpy(g[k]).cuda() for k in ("graph0", "start", "stats")),
                     _i32(labels), _table(table(len(labels), D, measure)), _i32(padded(MASKS)),
                     _i32(FIDS), _table(allowed), _i32(np.arange(NQ)), allowed)
    return _dev[key]


@pytest.mark.parametrize("kind,D,measure", MATRIX, ids=IDS)
def test_labelmask_traversal(ops, orc, kind, D, measure):  # noqa: F811
    """ops.query_labeled_mask with two clauses, filter ids and the table, with counters, against
    ops.query_filtered_by on the composed table"""
    d_graph, d_labels, d_table, d_masks, d_fids, c_table, c_fids, allowed = _device(orc, D, measure)
    base, q, _ = data(D, measure)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    ps = ops.prescreen_encode(d_base, measure) if kind == "f32_ps" else None
    for point in points_for(D):
        K, tau, iters = point
        kw = dict(max_iterations=iters, measure=measure, counters=True, prescreen=ps)
        ref = [x.cpu().numpy() for x in ops.query_filtered_by(d_base, d_q, *d_graph, K, tau, c_table,
                                                              c_fids, **kw)]
        n_fin = np.isfinite(ref[1]).sum(1)
        print(point, "finite entries per query:", n_fin.tolist())
        assert n_fin[4] == 0 and 1 <= n_fin[3] <= 6, (point, n_fin)
        if point != LDS_POINT:
            assert (n_fin == min(K, int(allowed[0].sum()))).any(), (point, n_fin)
        assert n_fin[6] > 0 and (ref[3] > 0).all(), (point, n_fin)
        got = [x.cpu().numpy() for x in ops.query_labeled_mask(d_base, d_q, *d_graph, K, tau, d_labels,
                                                               d_masks, d_table, d_fids, **kw)]
        assert np.array_equal(got[0], ref[0]), point
        assert got[1].tobytes() == ref[1].tobytes(), point
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), point


@pytest.mark.parametrize("kind,D,measure", SCAN_MATRIX, ids=SCAN_IDS)
def test_labelmask_scan(ops, orc, kind, D, measure):  # noqa: F811
    """ops.bf_query_labeled_mask with two clauses, filter ids and the table, against
    ops.bf_query_filtered_by on the composed table"""
    _, d_labels, d_table, d_masks, d_fids, c_table, c_fids, allowed = _device(orc, D, measure)
    base, q, _ = data(D, measure)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    for K in (10, 300) if LDS_POINT in points_for(D) else (10,):
        r_ids, r_d = ops.bf_query_filtered_by(d_base, d_q, K, c_table, c_fids, measure)
        ids, d = ops.bf_query_labeled_mask(d_base, d_q, K, d_labels, d_masks, d_table, d_fids, measure)
        assert _torch().equal(ids, r_ids), K
        assert d.cpu().numpy().tobytes() == r_d.cpu().numpy().tobytes(), K
        ids = ids.cpu().numpy()
        assert ((ids >= 0).sum(1) == np.minimum(allowed.sum(1), K)).all(), K
        assert (ids[4] == -1).all() and (ids[3, :6] >= 0).all() and (ids[3, 6:] == -1).all(), K
