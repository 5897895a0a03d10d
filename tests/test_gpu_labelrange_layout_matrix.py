"""The label-range kernels on every row layout, list size and kernel form: the traversal on every
rung of its launch ladder and the scan at every list size, against plain CPU references, bit for bit
(ids equal, distances as bytes, counters equal; no tolerance).

query_labelrange_kernel* (query_labelrange.hip, query_labelrange_16.hip) and
bf_query_labelrange_kernel* / bf_query_labelrange_lds_kernel (bf_query_labelrange.hip) are
instantiated per row layout <LPR, NCH>, element type, measure, list size and pre-screen, next to the
label-set kernels.  Data, graphs, label column and the cells (MATRIX, SCAN_MATRIX) are those of
tests/test_gpu_filtered_layout_matrix.py: integer data whose float32 sums are exact in any order, one
label column per (D, measure) with classes 0..4, RARE (4) on exactly six rows, UNUSED on none.

The contract in one line:
    allowed[n] = any_j(lo_j <= labels <= hi_j) & row(filter_ids[n])
with row -1 all ones, an id outside the table empty and an interval with lo > hi empty, and the
reference is filtered_reference.py_query_filtered under that mask.

Two columns, one set of masks.  RANGES on the plain column (labels 0..4) and EDGE_RANGES on the edge
column EDGE[labels] (INT32_MIN, -1, 0, 1, INT32_MAX: strictly increasing, so classes keep their
order) select, query by query, exactly the masks of SETS / FIDS of
tests/test_gpu_labelset_layout_matrix.py, with filter ids and without (`check_masks`, CPU).  The
ladder and the scan ladder therefore take their references from that module (`reference`,
`bf_reference`: the Python reference checked against the oracle in both summation orders, and the
shapes of its rows), computed once for both filters.  On the edge column every kernel sees the span
~0u, an interval that ends at INT32_MAX, one that starts at INT32_MIN, two that abut across the sign
change, an empty interval first, in the middle and last, and a query whose intervals are all empty.

test_labelrange_traversal and test_labelrange_scan are the base point (K 10) on the plain column.
test_labelrange_every_ladder_kernel runs every case of LADDER_CASES -- the points of the label-set
ladder -- in one form: filter ids and the table at bit offset 0, lists of width 4, on the long lists
(queries 0, 2, 4 and 6: at most three intervals) of width 3; the base point runs once more with
every list back to front (`reversed_lists`).  test_labelrange_scan_ladder runs the
scan at K 10 / 100 / 200 / 300 with ids and without, directly and through windows at bit offset 37.
The traversal through windows at a bit offset, on sub-batches without ids and against
query_filtered_by is NOT run on the wide layouts: those forms stay compared on layout {8,1} in
tests/test_gpu_label_ranges.py (their label-set twins once met an illegal memory access in a
whole-suite run whose cause was never found).

`labelrange_kernel` restates FilteredLadder<LabelRangeFilter>::launch (query_filtered.hip),
launch_query_cfg and launch_query_ladder (query_wave.hpp), `bf_labelrange_kernel`
launch_bf_labelrange_r (bf_query_labelrange.hip); tests/test_labelrange_coverage.py checks on the CPU
that the cases reach every label-range kernel of the built library.  Nothing reports which kernel a
launch ran: the guard is as good as the restatement, which follows the launchers as they read today.

Everything down to `the GPU side` is plain functions that need no GPU."""
import numpy as np
import pytest

import test_gpu_labelset_layout_matrix as labelset
from filtered_reference import bf_filtered_reference, py_query_filtered
from test_gpu_filtered_layout_matrix import (BASE_POINT, IDS, KB, MATRIX, NQ, RARE, SCAN_IDS, SCAN_MATRIX,
                                             UNUSED, _cast, _i32, data, graph)
from test_gpu_filtered_layout_matrix import ops  # noqa: F401  (the module fixture)
from test_gpu_labelset_layout_matrix import (BIT_OFFSET, HOOK_DEFAULTS, LONG_POINTS, LONG_QUERIES,
                                             SCAN_KS, TYPE_NAMES, _dtype, _np, _rows, assert_equals,
                                             assert_same, bf_list_regs, ladder_points, list_regs,
                                             prescreen_layout, queries_of, table, vis_hash_regs)

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

# the same masks on the edge column: class c carries EDGE[c]
EDGE = np.array([MIN, -1, 0, 1, MAX], np.int64)
EDGE_RANGES = [[(MIN, MAX)], [(MIN, -1)], [(0, 1), (1000, 1000)], [(MAX, MAX)], [(1, 0), (2, MAX - 1)],
               [(MAX, MAX), (1, 1)], [(5, 4), (0, 0), (MAX, MIN)], [(MIN, -1), (0, MAX)]]
LONG_WIDTH = 3                       # n_ranges of the long-list points
assert len(EDGE_RANGES) == NQ and (np.diff(EDGE) > 0).all()
assert max(len(EDGE_RANGES[i]) for i in LONG_QUERIES) == LONG_WIDTH


def _torch():
    import torch
    return torch


# ---- the launchers, restated -------------------------------------------------------------------------
def labelrange_kernel(kind, D, measure, K, iters, hooks=(), kbuild=KB):
    """demangled name of the kernel that ops.query_labeled_range launches: launch_query_labelrange,
    launch_query_cfg and FilteredLadder<LabelRangeFilter>::launch, restated (the launch itself does
    not report its kernel: the name is used in assertion messages and by the CPU guard)"""
    from ggnn_amd import ops
    h = dict(HOOK_DEFAULTS, **dict(hooks))
    lpr, nch = ops.dist_layout(D, _dtype(kind))
    cache, sorted_ = ops.query_sizing(D, K, iters)
    T = f"{TYPE_NAMES[kind.split('_')[0]]}, {lpr}, {nch}"
    # launch_query_cfg: the pre-screened kernels for a sorted part of at most 512
    ps = kind == "f32_ps" and sorted_ <= 512
    first = prescreen_layout(lpr, nch) if ps else (lpr, nch)
    psc = "Prescreen<%d, %d, %d>" % (*first, measure) if ps else "NoPrescreen"
    # FilteredLadder::launch: early rows and the hashed set, else the ladder
    hb = vis_hash_regs(cache - sorted_) if sorted_ <= 64 else 0
    if first == (8, 1) and hb != 0 and kbuild <= 24 and h["QUERY_EARLY"] != 0:
        return f"query_labelrange_kernel<{T}, 1, {measure}, {psc}, {hb}, true>"
    R = list_regs(sorted_, ps)
    if R == 0:
        return f"query_labelrange_kernel_lds<{T}, {measure}, {psc}>"
    return f"query_labelrange_kernel<{T}, {R}, {measure}, {psc}, 0, false>"


def bf_labelrange_kernel(kind, D, measure, K):
    """launch_bf_labelrange_r: K <= 64 / 128 / 256 is list registers 1 / 2 / 4, above that the list
    in LDS (the rule of launch_bf_labelset_r)"""
    from ggnn_amd import ops
    lpr, nch = ops.dist_layout(D, _dtype(kind))
    T = f"{TYPE_NAMES[kind]}, {lpr}, {nch}"
    R = bf_list_regs(K)
    if R == 0:
        return f"bf_query_labelrange_lds_kernel<{T}, {measure}>"
    return f"bf_query_labelrange_kernel<{T}, {R}, {measure}>"


# (kind, D, measure, K, tau, iterations, hooks): the points of the label-set ladder, cell by cell;
# read as data by tests/test_labelrange_coverage.py
LADDER_CASES = [(kind, D, m, *pt) for kind, D, m in MATRIX for pt in ladder_points(kind, D)]


# ---- masks and references: CPU only ------------------------------------------------------------------
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


def edge_column(labels):
    assert labels.min() >= 0 and labels.max() < len(EDGE)
    return EDGE[labels].astype(np.int32)


def masks_of(column, lists, tab=None, fids=None):
    """the whole contract: one allowed array per list, [n, N].  `lists`: per query a sequence of
    (lo, hi), ragged or an int32 array [n, width, 2] as the device takes it"""
    return np.stack([_in_ranges(column, [(int(lo), int(hi)) for lo, hi in r]) &
                     (_row(tab, int(fids[i])) if fids is not None else True)
                     for i, r in enumerate(lists)])


def composed_ranges(D, measure, with_ids=True, edge=False):
    """RANGES on the plain column, or EDGE_RANGES on the edge column, with FIDS or without"""
    labels = data(D, measure)[2]
    tab = table(len(labels), D, measure)
    return masks_of(edge_column(labels) if edge else labels, EDGE_RANGES if edge else RANGES,
                    tab if with_ids else None, FIDS if with_ids else None)


def padded(lists, width=4):
    """[Nq, width, 2] int32: every list padded with the empty interval (1, 0)"""
    assert all(1 <= len(r) <= width for r in lists)
    return np.array([list(r) + [(1, 0)] * (width - len(r)) for r in lists],
                    np.int64).astype(np.int32).reshape(len(lists), width, 2)


def long_lists():
    """the lists of the long-list points: queries 0, 2, 4 and 6 at width 3"""
    return padded([EDGE_RANGES[i] for i in LONG_QUERIES], LONG_WIDTH)


def reversed_lists():
    """EDGE_RANGES at width 4 with every list back to front, the padding first.  The masks do not
    depend on the order, the registers do: in order, no list of EDGE_RANGES puts a narrower interval
    in front of a wider one, and a verdict that took the first interval's span for all four would
    pass"""
    return np.ascontiguousarray(padded(EDGE_RANGES)[:, ::-1])


_masks_checked = set()


def check_masks(D, measure):
    """both columns select the masks of the label-set module, query by query, with filter ids and
    without; so do the int32 arrays the device is given, at width 4 and (the long lists) at width 3"""
    if (D, measure) in _masks_checked:
        return
    assert np.array_equal(FIDS, labelset.FIDS) and NQ == labelset.NQ
    labels = data(D, measure)[2]
    tab = table(len(labels), D, measure)
    for with_ids in (True, False):
        want = labelset.composed(D, measure, with_ids)
        what = (D, measure, with_ids)
        assert np.array_equal(composed_ranges(D, measure, with_ids), want), what
        assert np.array_equal(composed_ranges(D, measure, with_ids, edge=True), want), what
        t, f = (tab, FIDS) if with_ids else (None, None)
        assert np.array_equal(masks_of(labels, padded(RANGES), t, f), want), what
        assert np.array_equal(masks_of(edge_column(labels), padded(EDGE_RANGES), t, f), want), what
        assert np.array_equal(masks_of(edge_column(labels), reversed_lists(), t, f), want), what
        f = FIDS[LONG_QUERIES] if with_ids else None
        assert np.array_equal(masks_of(edge_column(labels), long_lists(), t, f),
                              want[LONG_QUERIES]), what
    # the shapes the lists are meant to have on the edge column
    only = masks_of(edge_column(labels), EDGE_RANGES)
    assert only[0].all() and only[7].all() and not only[4].any() and int(only[3].sum()) == 6
    assert np.array_equal(only[1], labels <= 1) and np.array_equal(only[6], labels == 2)
    _masks_checked.add((D, measure))


_refs, _bf_refs = {}, {}


def reference(orc, D, measure):
    """(ids [8, K], dists [8, K], n_dist [8], n_pop [8]) of the Python reference under RANGES and
    FIDS at BASE_POINT, after a look at the rows: an empty one, the six RARE rows at most, full ones"""
    key = (D, measure)
    if key not in _refs:
        K, tau, iters = BASE_POINT
        base, q, labels = data(D, measure)
        g = graph(orc, D, measure)
        allowed = composed_ranges(D, measure)
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
        allowed = composed_ranges(D, measure)
        rows = [bf_filtered_reference(orc, base, q[i:i + 1], SCAN_K, allowed[i], measure)
                for i in range(NQ)]
        ids, d = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
        assert np.isfinite(d).sum(1).tolist() == [min(SCAN_K, int(a.sum())) for a in allowed]
        assert (ids[3, :6] >= 0).all() and (ids[3, 6:] == -1).all() and (labels[ids[3, :6]] == RARE).all()
        _bf_refs[key] = ids, d
    return _bf_refs[key]


# ---- the GPU side ------------------------------------------------------------------------------------
_dev = {}


class Device:
    """graph and filter arguments of one (D, measure) on the device: graph, plain column, table, ids
    and the windows' table are those the label-set module uploaded; the edge column and its window
    are the plain ones class by class"""

    def __init__(self, orc, D, measure):
        ls = labelset._device(orc, D, measure)
        labels = data(D, measure)[2]
        self.graph, self.labels, self.table, self.fids = ls.graph, ls.labels, ls.table, ls.fids
        self.wide_table = ls.wide_table
        self.ranges = _i32(padded(RANGES))
        self.edge = _i32(edge_column(labels))
        self.edge_ranges, self.long_ranges = _i32(padded(EDGE_RANGES)), _i32(long_lists())
        self.reversed_ranges = _i32(reversed_lists())
        # what lies in front of the window and behind it are labels of the lists
        wide = edge_column(ls.wide_labels.cpu().numpy())
        assert np.array_equal(wide[BIT_OFFSET:BIT_OFFSET + len(labels)], edge_column(labels))
        self.wide_edge = _i32(wide)


def _device(orc, D, measure):
    key = (D, measure)
    if key not in _dev:
        _dev[key] = Device(orc, D, measure)
    return _dev[key]


@pytest.mark.parametrize("kind,D,measure", MATRIX, ids=IDS)
def test_labelrange_traversal(ops, orc, kind, D, measure):
    """ops.query_labeled_range with four intervals, filter ids and the table, with counters, against
    the Python reference"""
    dv = _device(orc, D, measure)
    K, tau, iters = BASE_POINT
    ref = reference(orc, D, measure)
    base, q, _ = data(D, measure)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    ps = ops.prescreen_encode(d_base, measure) if kind == "f32_ps" else None
    ids, d, nd, npop = [x.cpu().numpy() for x in ops.query_labeled_range(
        d_base, d_q, *dv.graph, K, tau, dv.labels, dv.ranges, dv.table, dv.fids, max_iterations=iters,
        measure=measure, counters=True, prescreen=ps)]
    assert np.array_equal(ids, ref[0])
    assert d.tobytes() == ref[1].tobytes()
    assert np.array_equal(nd, ref[2]) and np.array_equal(npop, ref[3])


@pytest.mark.parametrize("kind,D,measure", SCAN_MATRIX, ids=SCAN_IDS)
def test_labelrange_scan(ops, orc, kind, D, measure):
    """ops.bf_query_labeled_range at K = 10 with four intervals, filter ids and the table, against
    the oracle on the compacted rows of every query"""
    dv = _device(orc, D, measure)
    r_ids, r_d = bf_reference(orc, D, measure)
    base, q, _ = data(D, measure)
    ids, d = ops.bf_query_labeled_range(_cast(base, kind), _cast(q, kind), SCAN_K, dv.labels, dv.ranges,
                                        dv.table, dv.fids, measure)
    ids, d = ids.cpu().numpy(), d.cpu().numpy()
    assert np.array_equal(ids, r_ids)
    assert d.tobytes() == r_d.tobytes()


@pytest.mark.parametrize("kind,D,measure", MATRIX, ids=IDS)
def test_labelrange_every_ladder_kernel(ops, orc, kind, D, measure):
    """every case of LADDER_CASES in this cell: ops.query_labeled_range on the edge column with
    filter ids and the table, with counters, against the reference of the label-set ladder (all
    eight queries at width 4; 0, 2, 4 and 6 at width 3 on the long lists).  A case under hooks gives
    the bytes and counters of the same point without them; the base point runs once more with every
    list back to front."""
    from ggnn_amd import _lib
    check_masks(D, measure)
    dv = _device(orc, D, measure)
    base, q, _ = data(D, measure)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    ps = ops.prescreen_encode(d_base, measure) if kind == "f32_ps" else None
    plain, ran = {}, 0
    for kind_, D_, m_, K, tau, iters, hooks in LADDER_CASES:
        if (kind_, D_, m_) != (kind, D, measure):
            continue
        ran += 1
        point = (K, tau, iters)
        ref = labelset.reference(orc, D, measure, point)
        sel = queries_of(point)
        ranges = dv.long_ranges if point in LONG_POINTS else _rows(dv.edge_ranges, sel)
        assert ranges.shape == (len(sel), LONG_WIDTH if point in LONG_POINTS else 4, 2)
        what = (labelrange_kernel(kind, D, measure, K, iters, hooks), point, hooks)
        with _lib.hooks(**dict(hooks)):
            res = _np(ops.query_labeled_range(
                d_base, _rows(d_q, sel), *dv.graph, K, tau, dv.edge, ranges, dv.table,
                _rows(dv.fids, sel), max_iterations=iters, measure=measure, counters=True,
                prescreen=ps))
        assert_equals(res, ref, np.arange(len(sel)), what)
        if hooks:
            assert_same(res, plain[point], what)
        else:
            plain[point] = res
        if point == BASE_POINT and not hooks:
            res = _np(ops.query_labeled_range(
                d_base, d_q, *dv.graph, K, tau, dv.edge, dv.reversed_ranges, dv.table, dv.fids,
                max_iterations=iters, measure=measure, counters=True, prescreen=ps))
            assert_equals(res, ref, np.arange(NQ), what + ("back to front",))
    assert ran >= 7


@pytest.mark.parametrize("kind,D,measure", SCAN_MATRIX, ids=SCAN_IDS)
def test_labelrange_scan_ladder(ops, orc, kind, D, measure):
    """ops.bf_query_labeled_range on the edge column at K = 10, 100, 200 and 300 (list registers 1, 2,
    4 and bf_query_labelrange_lds_kernel): (a) four intervals with filter ids and the table, (b) the
    same with label column and table as windows at bit offset 37 of wider random arrays, and both
    without ids, and (a) once more with every list back to front, against the oracle on the
    compacted rows of every query.  Query 3 shows its six rows, then (-1, +inf)."""
    check_masks(D, measure)
    dv = _device(orc, D, measure)
    base, q, _ = data(D, measure)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    for K in SCAN_KS:
        for with_ids in (True, False):
            r_ids, r_d = labelset.bf_reference(orc, D, measure, K, with_ids)
            tab, fids = (dv.table, dv.fids) if with_ids else (None, None)
            wide = dv.wide_table if with_ids else None
            runs = {"(a)" if with_ids else "no ids":
                    ops.bf_query_labeled_range(d_base, d_q, K, dv.edge, dv.edge_ranges, tab, fids,
                                               measure),
                    "(b)" if with_ids else "no ids, window":
                    ops.bf_query_labeled_range(d_base, d_q, K, dv.wide_edge, dv.edge_ranges, wide, fids,
                                               measure, bit_offset=BIT_OFFSET)}
            if with_ids:
                runs["(a), back to front"] = ops.bf_query_labeled_range(
                    d_base, d_q, K, dv.edge, dv.reversed_ranges, tab, fids, measure)
            for name, (ids, d) in runs.items():
                ids, d = ids.cpu().numpy(), d.cpu().numpy()
                what = (bf_labelrange_kernel(kind, D, measure, K), name)
                assert np.array_equal(ids, r_ids), what
                assert d.tobytes() == r_d.tobytes(), what
                assert (ids[3, :6] >= 0).all() and (ids[3, 6:] == -1).all(), what
                assert np.isposinf(d[3, 6:]).all() and np.isfinite(d[3, :6]).all(), what


def test_labelrange_refuses_byte_rows_above_4096(ops):
    """uint8 layout {64,16} starts above 4096 elements, and both label-range entry points refuse such
    rows before any launch: why tests/test_labelrange_coverage.py lists the kernels of that layout
    as unreachable"""
    from ggnn_amd import _lib
    torch = _torch()
    N, D, nq = 64, 4112, 2
    assert ops.dist_layout(D, torch.uint8) == (64, 16)
    base = torch.zeros((N, D), dtype=torch.uint8, device="cuda")
    q = torch.zeros((nq, D), dtype=torch.uint8, device="cuda")
    graph0 = torch.zeros((N, KB), dtype=torch.int32, device="cuda")
    start = torch.zeros(4, dtype=torch.int32, device="cuda")
    stats = torch.ones(2, dtype=torch.float32, device="cuda")
    labels = torch.zeros(N, dtype=torch.int32, device="cuda")
    ranges = torch.zeros((nq, 1, 2), dtype=torch.int32, device="cuda")
    for call in (lambda: ops.query_labeled_range(base, q, graph0, start, stats, 10, 0.6, labels, ranges),
                 lambda: ops.bf_query_labeled_range(base, q, 10, labels, ranges)):
        with pytest.raises(_lib.GGNNError, match="4096") as e:
            call()
        assert e.value.status == _lib.INVALID_ARGUMENT
