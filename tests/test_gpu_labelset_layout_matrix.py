"""The label-set kernels on every row layout, list size and kernel form: the traversal on every rung
of its launch ladder and the scan, against plain CPU references, bit for bit (ids equal, distances
as bytes, counters equal; no tolerance).

query_labelset_kernel* (query_labelset.hip, query_labelset_16.hip) and bf_query_labelset_kernel* /
bf_query_labelset_lds_kernel (bf_query_labelset.hip) are instantiated per row layout <LPR, NCH>,
element type, measure, list size and pre-screen, next to the kernels of the bitset and the one-label
filters.  Data, graphs, label column and the cells (MATRIX, SCAN_MATRIX) are those of
tests/test_gpu_filtered_layout_matrix.py: integer data whose float32 sums are exact in any order,
one label column per (D, measure) with classes 0..4, RARE on exactly six rows, UNUSED on none.

The contract in one line:
    allowed[n] = isin(labels, set n) (everything if -1 in set n) & row(filter_ids[n])
with row -1 all ones and an id outside the table empty, and the reference is
filtered_reference.py_query_filtered under that mask.  Before any GPU result is judged the reference
itself is checked on the CPU (`reference`): with the set [-1] and row -1 it equals the C++ oracle's
orc.query in both summation orders, and the rows have the shape the cases are meant to have (an
empty row, a partly filled row, full rows).

The traversal runs in one form here, in test_labelset_every_ladder_kernel: sets of width 8 with
filter ids and the table at bit offset 0, the base point of every cell included.  (The traversal
through windows at a bit offset, on a sub-batch without ids, and against query_filtered_by is
compared in tests/test_gpu_label_sets.py, on layout {8,1}; the scan runs through windows and
without ids in every cell here.)

`labelset_kernel` restates FilteredLadder<LabelSetFilter>::launch (query_filtered.hip),
launch_query_cfg and launch_query_ladder (query_wave.hpp); LADDER_CASES holds a case for every
label-set traversal kernel a launch can reach, which tests/test_labelset_coverage.py checks on the
CPU against the built library.  Nothing reports which kernel a launch ran: as with int8_kernel of
tests/test_gpu_int8_parity.py, the guard is as good as the restatement, which follows the launchers
as they read today and has to follow them when they change.

Everything down to `the GPU side` is plain functions that need no GPU."""
import numpy as np
import pytest

from filtered_reference import bf_filtered_reference, py_query_filtered
from test_gpu_filtered_layout_matrix import (BASE_POINT, IDS, KB, MATRIX, RARE, SCAN_IDS, SCAN_MATRIX,
                                             UNUSED, _cast, _i32, _table, data, graph)
from test_gpu_filtered_layout_matrix import ops  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

INT32_MIN = -2 ** 31
NQ = 8
# everything; two classes; two classes and a label no row carries; the six RARE rows; nothing (no
# row carries either label); RARE and class 3 under the 5 % row; eight distinct values of which only
# the last is carried by any row; the wildcard in the middle
SETS = [[-1], [0, 1], [2, 3, UNUSED], [RARE], [UNUSED, 9000], [RARE, 3],
        [5000, 5001, 5002, 5003, INT32_MIN, 5005, 5006, 2], [1, -1, 2]]
FIDS = np.array([-1, -1, 0, -1, 2, 1, 2, 0], np.int32)
LONG_QUERIES = np.array([0, 2, 4, 6])       # the queries of the long lists
BIT_OFFSET = 37                             # of the label column and of the table; no multiple of 32

# (K, tau, iterations).  The long lists: sorted part 128 / 224 / 448 / 928 / 2048 / 2144 = list
# registers 2, 4, 8, 16, 32 and the LDS list (with the pre-screen: 2, 4, 8, then the kernels without)
LONG_POINTS = [(K, 0.6, 64) for K in (100, 200, 400, 900, 2000)] + [(2100, 0.5, 64)]
# rows whose first read is 8 lanes x one chunk: two bucket registers, and a ring too long for the
# hashed set (the R = 1 kernel without early rows)
EARLY_POINTS = [(10, 0.6, 400), (10, 0.6, 600)]
NO_EARLY = (("QUERY_EARLY", 0),)
# the stash of the hashed set, its overflow into the ring scan, and the two hooks that do nothing
# under a filter
VIS_HOOKS = [(("VIS_SLOTS", 1),), (("VIS_SLOTS", 1), ("QUERY_EARLY", 0)),
             (("QUERY_GLOBAL_RING", 0),), (("VIS_TAG_SET", 0),)]
HOOK_DEFAULTS = {"QUERY_EARLY": 1, "QUERY_GLOBAL_RING": 1, "VIS_TAG_SET": 1, "VIS_SLOTS": 8}
TYPE_NAMES = {"f32": "float", "u8": "unsigned char", "f16": "f16_t", "bf16": "bf16_t"}


def _torch():
    import torch
    return torch


def _dtype(kind):
    torch = _torch()
    return {"f32": torch.float32, "u8": torch.uint8, "f16": torch.float16,
            "bf16": torch.bfloat16}[kind.split("_")[0]]


# ---- the launchers, restated -------------------------------------------------------------------------
def vis_hash_regs(vis):
    return 1 if vis <= 192 else 2 if vis <= 480 else 0


def prescreen_layout(lpr, nch):
    """PsFor (traversal.hpp): <LPR, NCH> of the pre-screen in front of a float32 layout"""
    return {(16, 4): (16, 1), (64, 4): (32, 2), (64, 16): (64, 4)}.get((lpr, nch), (8, 1))


def list_regs(sorted_, prescreen):
    """launch_query_ladder: list registers per lane, 0 = the LDS list"""
    caps = ((1, 64), (2, 128), (4, 256), (8, 512)) + \
        (() if prescreen else ((16, 1024), (32, 2048)))
    for r, cap in caps:
        if sorted_ <= cap:
            return r
    return 0


def early_rows(kind, D):
    """early_rows_layout (query_wave.hpp): the first row read is 8 lanes x one 16-byte chunk, the
    pre-screen's (at a sorted part of at most 512) or the row's own"""
    from ggnn_amd import ops
    layout = ops.dist_layout(D, _dtype(kind))
    return (prescreen_layout(*layout) if kind == "f32_ps" else layout) == (8, 1)


def labelset_kernel(kind, D, measure, K, iters, hooks=(), kbuild=KB):
    """demangled name of the kernel that ops.query_labeled_in launches: launch_query_labelset,
    launch_query_cfg and FilteredLadder<LabelSetFilter>::launch, restated (the launch itself does
    not report its kernel: the name is used in assertion messages and by the CPU guard)"""
    from ggnn_amd import ops
    h = dict(HOOK_DEFAULTS, **dict(hooks))
    lpr, nch = ops.dist_layout(D, _dtype(kind))
    cache, sorted_ = ops.query_sizing(D, K, iters)
    vis = cache - sorted_
    T = f"{TYPE_NAMES[kind.split('_')[0]]}, {lpr}, {nch}"
    # launch_query_cfg: the pre-screened kernels for a sorted part of at most 512
    ps = kind == "f32_ps" and sorted_ <= 512
    first = prescreen_layout(lpr, nch) if ps else (lpr, nch)
    psc = "Prescreen<%d, %d, %d>" % (*first, measure) if ps else "NoPrescreen"
    hb = vis_hash_regs(vis) if sorted_ <= 64 else 0
    if first == (8, 1) and hb != 0 and kbuild <= 24 and h["QUERY_EARLY"] != 0:
        return f"query_labelset_kernel<{T}, 1, {measure}, {psc}, {hb}, true>"
    R = list_regs(sorted_, ps)
    if R == 0:
        return f"query_labelset_kernel_lds<{T}, {measure}, {psc}>"
    return f"query_labelset_kernel<{T}, {R}, {measure}, {psc}, 0, false>"


def bf_list_regs(K):
    """launch_bf_labelset_r: list registers per lane, 0 = bf_query_labelset_lds_kernel"""
    return 1 if K <= 64 else 2 if K <= 128 else 4 if K <= 256 else 0


SCAN_KS = (10, 100, 200, 300)        # list registers 1, 2, 4 and the list in LDS


def bf_labelset_kernel(kind, D, measure, K):
    from ggnn_amd import ops
    lpr, nch = ops.dist_layout(D, _dtype(kind))
    T = f"{TYPE_NAMES[kind]}, {lpr}, {nch}"
    R = bf_list_regs(K)
    if R == 0:
        return f"bf_query_labelset_lds_kernel<{T}, {measure}>"
    return f"bf_query_labelset_kernel<{T}, {R}, {measure}>"


# the D of MATRIX whose first row read is 8 lanes x one chunk (early_rows; checked against the layout
# table by tests/test_labelset_coverage.py)
EARLY_DIMS = {"f32": (32,), "f32_ps": (32, 64, 96, 128), "u8": (64,), "f16": (64,), "bf16": (64,)}


def ladder_points(kind, D):
    """[(K, tau, iterations, hooks)] of one cell"""
    pts = [BASE_POINT + ((),)] + [p + ((),) for p in LONG_POINTS]
    if D in EARLY_DIMS[kind]:
        pts += [p + ((),) for p in EARLY_POINTS]
        pts += [BASE_POINT + (NO_EARLY,), EARLY_POINTS[0] + (NO_EARLY,)]
        if kind in ("f32", "f32_ps"):
            pts += [p + (hk,) for hk in VIS_HOOKS for p in (BASE_POINT, EARLY_POINTS[0])]
    return pts


# (kind, D, measure, K, tau, iterations, hooks); read as data by tests/test_labelset_coverage.py
LADDER_CASES = [(kind, D, m, *pt) for kind, D, m in MATRIX for pt in ladder_points(kind, D)]


# ---- masks and references: CPU only ------------------------------------------------------------------
def table(n, D, measure):
    """three rows: about 50 % random, about 5 % random, every id but every seventh"""
    u = np.random.default_rng(500 + D + measure).random((2, n))
    return np.stack([u[0] < 0.5, u[1] < 0.05, np.arange(n) % 7 != 0])


def _in_set(labels, s):
    return np.ones(len(labels), bool) if -1 in s else np.isin(labels, np.array(s, np.int64))


def _row(tab, f):
    if f == -1:
        return np.ones(tab.shape[1], bool)
    return tab[f] if 0 <= f < len(tab) else np.zeros(tab.shape[1], bool)


def composed(D, measure, with_ids=True):
    """the whole contract: one allowed array per query, [8, N]"""
    labels = data(D, measure)[2]
    tab = table(len(labels), D, measure)
    return np.stack([_in_set(labels, s) & (_row(tab, int(FIDS[i])) if with_ids else True)
                     for i, s in enumerate(SETS)])


def padded(sets, width=8):
    """[Nq, width] int32: every set padded by repeating its first entry"""
    assert all(1 <= len(s) <= width for s in sets)
    return np.array([list(s) + [s[0]] * (width - len(s)) for s in sets], np.int64).astype(np.int32)


def _stack(rows):
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
            np.array([r[2] for r in rows], np.int64), np.array([r[3] for r in rows], np.int64))


def queries_of(point):
    return LONG_QUERIES if tuple(point) in LONG_POINTS else np.arange(NQ)


_refs = {}


def reference(orc, D, measure, point):
    """(ids [n, K], dists [n, K], n_dist [n], n_pop [n]) of the Python reference under SETS and FIDS
    for the queries of `point` (all eight; 0, 2, 4 and 6 on the long lists), after the checks of the
    reference itself"""
    point = tuple(point)
    key = (D, measure, point)
    if key in _refs:
        return _refs[key]
    K, tau, iters = point
    base, q, labels = data(D, measure)
    g = graph(orc, D, measure)
    N = base.shape[0]
    allowed = composed(D, measure)
    sel = queries_of(point)

    def py(i, mask):
        return py_query_filtered(base, q[i], g["graph0"], g["start"], g["stats"], K, tau, iters,
                                 mask, cosine=bool(measure))

    rows = {int(i): py(i, allowed[i]) for i in sel}
    ref = _stack([rows[int(i)] for i in sel])
    # 1. the set [-1] with row -1 (query 0) is the oracle's unfiltered search, in both summation
    # orders: every query at the point all cells share, query 0 at the others
    assert SETS[0] == [-1] and FIDS[0] == -1 and allowed[0].all()
    osel = np.arange(NQ) if point == BASE_POINT else np.array([0])
    ones = _stack([rows[0] if i == 0 else py(i, np.ones(N, bool)) for i in osel])
    for wave in (False, True):
        orc.set_wave_order(wave)
        try:
            o = orc.query(base, q[osel], g["graph0"], g["start"], g["stats"], K, tau, iters, measure,
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
    n_fin = fin.sum(1)
    for j, i in enumerate(sel):
        assert not fin[j, n_fin[j]:].any(), (key, i)
        assert allowed[i][ids[j, :n_fin[j]]].all(), (key, i)
        assert n_fin[j] <= allowed[i].sum(), (key, i)
    filled = dict(zip(sel.tolist(), n_fin.tolist()))
    assert not allowed[4].any() and filled[4] == 0, key
    if point == BASE_POINT:
        assert int(allowed[3].sum()) == 6 and 1 <= filled[3] <= 6, (key, filled)
        assert (n_fin == 0).any() and ((n_fin >= 1) & (n_fin <= K - 1)).any(), (key, filled)
        assert (n_fin == K).sum() >= 4, (key, filled)
    elif point == (100, 0.6, 64) and D in (128, 4096):
        assert (n_fin == K).any() and ((n_fin >= 1) & (n_fin < K)).any() and (n_fin == 0).any(), \
            (key, filled)
    else:
        # (a search of 64 iterations visits fewer than 400 points: no full row above K = 400)
        assert (n_fin == 0).any() and (n_fin > 0).any(), (key, filled)
    _refs[key] = ref
    return ref


_bf_refs = {}


def bf_reference(orc, D, measure, K, with_ids):
    """exact K nearest under SETS (and FIDS): the oracle on the compacted rows, per query"""
    key = (D, measure, K, with_ids)
    if key not in _bf_refs:
        base, q, labels = data(D, measure)
        allowed = composed(D, measure, with_ids)
        rows = [bf_filtered_reference(orc, base, q[i:i + 1], K, allowed[i], measure)
                for i in range(NQ)]
        ids, d = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
        n_fin = np.isfinite(d).sum(1)
        assert n_fin.tolist() == [min(K, int(a.sum())) for a in allowed]
        # the six RARE rows, then padding
        assert int(allowed[3].sum()) == 6 and (ids[3, :6] >= 0).all() and (ids[3, 6:] == -1).all()
        assert np.isposinf(d[3, 6:]).all() and (labels[ids[3, :6]] == RARE).all()
        _bf_refs[key] = ids, d
    return _bf_refs[key]


# ---- the GPU side ------------------------------------------------------------------------------------
_dev = {}


class Device:
    """graph and filter arguments of one (D, measure) on the device"""

    def __init__(self, orc, D, measure):
        g = graph(orc, D, measure)
        labels = data(D, measure)[2]
        N = len(labels)
        tab = table(N, D, measure)
        rng = np.random.default_rng(900 + D + measure)
        self.graph = tuple(_torch().from_numpy(g[k]).cuda() for k in ("graph0", "start", "stats"))
        self.labels, self.table = _i32(labels), _table(tab)
        self.sets, self.fids = _i32(padded(SETS)), _i32(FIDS)
        # the same rows as windows at BIT_OFFSET of a longer column and of wider rows: what lies in
        # front of the window and behind it are labels of the sets and random bits
        self.wide_labels = _i32(np.concatenate([rng.integers(0, 5, BIT_OFFSET), labels,
                                                rng.integers(0, 5, 50)]))
        wide = rng.random((len(tab), BIT_OFFSET + N + 50)) < 0.5
        wide[:, BIT_OFFSET:BIT_OFFSET + N] = tab
        self.wide_table = _table(wide)


def _device(orc, D, measure):
    key = (D, measure)
    if key not in _dev:
        _dev[key] = Device(orc, D, measure)
    return _dev[key]


def _np(res):
    return [x.cpu().numpy() for x in res]


def assert_equals(res, ref, rows, what):
    ids, d, nd, npop = res
    assert np.array_equal(ids, ref[0][rows]), (what, "ids")
    assert d.tobytes() == ref[1][rows].tobytes(), (what, "dists")
    assert np.array_equal(nd, ref[2][rows]), (what, "n_dist")
    assert np.array_equal(npop, ref[3][rows]), (what, "n_pop")


def assert_same(a, b, what):
    for x, y, name in zip(a, b, ("ids", "dists", "n_dist", "n_pop")):
        assert x.tobytes() == y.tobytes(), (what, name)


def _rows(t, sel):
    return t[_torch().from_numpy(np.asarray(sel)).cuda()].contiguous()


@pytest.mark.parametrize("kind,D,measure", SCAN_MATRIX, ids=SCAN_IDS)
def test_labelset_scan(ops, orc, kind, D, measure):
    """ops.bf_query_labeled_in at K = 10, 100, 200 and 300 (list registers 1, 2, 4 and
    bf_query_labelset_lds_kernel): (a) sets of width 8 with filter ids and the table, (b) the same
    with label column and table as windows at bit offset 37 of wider random arrays, and both without
    ids, against the oracle on the compacted rows of every query.  Query 3 shows its six rows, then
    (-1, +inf)."""
    dv = _device(orc, D, measure)
    base, q, _ = data(D, measure)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    for K in SCAN_KS:
        for with_ids in (True, False):
            r_ids, r_d = bf_reference(orc, D, measure, K, with_ids)
            tab, fids = (dv.table, dv.fids) if with_ids else (None, None)
            wide = dv.wide_table if with_ids else None
            runs = {"(a)" if with_ids else "no ids":
                    ops.bf_query_labeled_in(d_base, d_q, K, dv.labels, dv.sets, tab, fids, measure),
                    "(b)" if with_ids else "no ids, window":
                    ops.bf_query_labeled_in(d_base, d_q, K, dv.wide_labels, dv.sets, wide, fids,
                                            measure, bit_offset=BIT_OFFSET)}
            for name, (ids, d) in runs.items():
                ids, d = ids.cpu().numpy(), d.cpu().numpy()
                what = (bf_labelset_kernel(kind, D, measure, K), name)
                assert np.array_equal(ids, r_ids), what
                assert d.tobytes() == r_d.tobytes(), what
                assert (ids[3, :6] >= 0).all() and (ids[3, 6:] == -1).all(), what
                assert np.isposinf(d[3, 6:]).all() and np.isfinite(d[3, :6]).all(), what


@pytest.mark.parametrize("kind,D,measure", MATRIX, ids=IDS)
def test_labelset_every_ladder_kernel(ops, orc, kind, D, measure):
    """every case of LADDER_CASES in this cell: ops.query_labeled_in with sets of width 8, filter ids
    and the table, with counters, against the Python reference (all eight queries; 0, 2, 4 and 6 on
    the long lists).  A case under hooks gives the bytes and
    counters of the same point without them."""
    from ggnn_amd import _lib
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
        ref = reference(orc, D, measure, point)
        sel = queries_of(point)
        what = (labelset_kernel(kind, D, measure, K, iters, hooks), point, hooks)
        with _lib.hooks(**dict(hooks)):
            res = _np(ops.query_labeled_in(
                d_base, _rows(d_q, sel), *dv.graph, K, tau, dv.labels, _rows(dv.sets, sel), dv.table,
                _rows(dv.fids, sel), max_iterations=iters, measure=measure, counters=True,
                prescreen=ps))
        assert_equals(res, ref, np.arange(len(sel)), what)
        if hooks:
            assert_same(res, plain[point], what)
        else:
            plain[point] = res
    assert ran >= 7


def test_labelset_refuses_byte_rows_above_4096(ops):
    """uint8 layout {64,16} starts above 4096 elements, and both label-set entry points refuse such
    rows before any launch: why tests/test_labelset_coverage.py lists the kernels of that layout as
    unreachable"""
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
    sets = torch.zeros((nq, 1), dtype=torch.int32, device="cuda")
    for call in (lambda: ops.query_labeled_in(base, q, graph0, start, stats, 10, 0.6, labels, sets),
                 lambda: ops.bf_query_labeled_in(base, q, 10, labels, sets)):
        with pytest.raises(_lib.GGNNError, match="4096") as e:
            call()
        assert e.value.status == _lib.INVALID_ARGUMENT
