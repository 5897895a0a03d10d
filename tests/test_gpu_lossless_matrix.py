"""Every kernel variant of "Distances from lossless codes" that the engine can launch, on the GPU.

The query kernels of PrescreenExact<8, 1, kL2> are picked by QueryLadder::launch
(ggnn_amd/csrc/query.hip) and FilteredLadder::launch (query_filtered.hip) when the caller knows the
base's lossless-grid flag -- the engine handle only; the operator seam never sets it, so no oracle
comparison made through ggnn_amd.ops runs them.  CASES lists cells (how, D, KBuild, K, tau,
iterations, hooks) that between them launch every reachable variant: ring-less hashed sets of one
and two bucket registers, the ring-less tag sets of 8 and 9 bucket bits (513..2016 iterations), the
filtered and labelled kernels with one and two bucket registers, with rings in LDS that wrap, on
row lengths that fill their float layout and code row and on ones that do not, under shrunken
buckets (hook VIS_SLOTS), and on either side of every condition by which the launchers choose
between these kernels and the previous ones.  tests/test_lossless_coverage.py checks on the CPU,
against the kernels in the built library, that no variant is left without a cell.

Per cell (test_cell), on the mixed batch (on grid, a copy of a base row, clamped on either side,
fractional rows) and on the all-on-grid batch: the default kernels against hook PS_EXACT = 0 and
against set_prescreen(False) -- ids, distance bytes, n_dist and n_pop equal, code rows equal
between the first two; distances of the integral rows equal to float64 truth on the unpadded data;
no denied id; the search ran its iterations.  `exact_variant` restates the launchers' choice; on
the grid batch fewer float rows are read than with PS_EXACT = 0 exactly when it names a variant,
and otherwise the rows read are the same, so "the exact kernel ran" is asserted, not assumed.

One cell of every family is also held to the CPU oracle on the engine's own graph
(test_against_the_oracle).  Data are integers in [0, 255]: every float32 sum is exact, and there
is no tolerance anywhere in this file."""
import contextlib

import numpy as np
import pytest

from lossless_helpers import (F, INTEGRAL_ROWS, KBUILD, N, NQ, TAU, assert_same, bitset_filter,
                              case, label_filter, mixed_queries, table_filter, three_way, true_l2)

pytestmark = pytest.mark.gpu

N_SMALL = 8000      # D = 64, 70, 100, 132 and the extra KBuild builds: short builds


def n_rows(D, kbuild):
    return N if D in (128, 96) and kbuild == KBUILD else N_SMALL


# ---- the launchers' choice, restated ---------------------------------------------------------------
def vis_hash_regs(vis):
    return 1 if vis <= 192 else 2 if vis <= 480 else 0


def tag_set_bucket_bits(vis):
    """buckets (log2) of seven 16-bit tags for a ring of `vis` keys: load factor <= 4/7"""
    b = 5
    while (7 << b) * 4 < 7 * vis:
        b += 1
    return b


HOOK_DEFAULTS = {"QUERY_EARLY": 1, "QUERY_GLOBAL_RING": 1, "VIS_TAG_SET": 1, "PS_EXACT": 1}


def exact_variant(how, D, KBuild, K, iters, hooks=None):
    """(family, HB) of the PrescreenExact kernel that a search of an engine with a lossless copy
    launches -- family "query_kernel" / "query_filtered_kernel" / "query_labeled_kernel", HB the
    bucket registers of the hashed set or minus the bucket bits of the tag set -- or None where the
    launchers keep the kernels of Prescreen (launch_query and QueryLadder::launch in query.hip,
    FilteredLadder::launch in query_filtered.hip; bases of at most 2^24 rows, which the tag set
    takes whole)."""
    import torch
    from ggnn_amd import ops
    h = dict(HOOK_DEFAULTS, **(hooks or {}))
    pad_d = (D + 3) // 4 * 4
    if pad_d < 64 or not h["PS_EXACT"]:             # ensure_prescreen: no copy of short rows
        return None
    cache, sorted_ = ops.query_sizing(pad_d, K, iters)
    if sorted_ > 512:                               # launch_query_cfg: no pre-screened kernel
        return None
    if ops.dist_layout(pad_d, torch.float32) in ((16, 4), (64, 4), (64, 16)):
        return None                                 # PsFor: code rows that are not Prescreen<8, 1>
    vis = cache - sorted_
    hb = vis_hash_regs(vis) if sorted_ <= 64 else 0
    early = KBuild <= 24 and sorted_ <= 64 and h["QUERY_EARLY"] != 0
    if how != "plain":
        family = "query_labeled_kernel" if how == "labels" else "query_filtered_kernel"
        return (family, hb) if hb != 0 and early else None
    cannot_wrap = iters <= vis and h["QUERY_GLOBAL_RING"] != 0
    if hb != 0:                                     # ring-less hashed set
        return ("query_kernel", hb) if early and cannot_wrap else None
    tagged = sorted_ <= 64 and 481 <= vis <= 2016 and h["VIS_TAG_SET"] != 0 and \
        tag_set_bucket_bits(vis) in (8, 9)
    if tagged and early and cannot_wrap:            # ring-less tag set
        return ("query_kernel", -tag_set_bucket_bits(vis))
    return None


# ---- the cells ---------------------------------------------------------------------------------------
# tau: chosen on the CPU (orc.build with KBuild, 0.5, 1 refinement and orc.query with counters on the
# same data, 256 grid queries) so that the searches run their iterations; the comment of a group
# gives the oracle's mean pops per query.  On uniform integers of 96 to 132 dimensions no search of
# K >= 10 ends before its last iteration at tau = 0.7; at D = 64 and 70 some do (1500 iterations:
# 1208.7 and 1378.7 pops), and none does at tau = 1.
TAU_SHORT_ROWS = 1.0


def tau_of(D):
    return TAU if D >= 96 else TAU_SHORT_ROWS


def _cells():
    c = []

    def add(how, D, iters, K=10, kbuild=KBUILD, **hooks):
        cell = (how, D, kbuild, K, tau_of(D), iters, tuple(sorted(hooks.items())))
        if cell not in c:
            c.append(cell)

    # unfiltered: ring-less hashed sets (175: HB 1, 400: HB 2) and long searches; D = 128, 96, 100
    # are layouts {16,2}, {8,3} and {16,2} with a partly filled last chunk, D = 64 is {8,2}
    # oracle, every D (64 at tau = 1): 175.0 / 400.0 / 600.0 / 1500.0 / 700.0 (K = 47) / 992.0 /
    # 993.0 / 1000.0 pops
    for D in (128, 96, 100, 64):
        add("plain", D, 175)
        add("plain", D, 400)
        add("plain", D, 600)                      # ring 992, tag bits 8
        add("plain", D, 1500)                     # ring 2016, tag bits 9
    for D in (128, 96, 100):
        add("plain", D, 700, K=47)                # ring 960
        add("plain", D, 992)                      # the last ring-less one for K = 10
        add("plain", D, 993)                      # the ring may wrap: previous kernels
        add("plain", D, 1000)
        # shrunken buckets: stash, stash overflow and the scan of the ring inside the exact kernels
        for slots in (1, 2, 4):
            add("plain", D, 600, VIS_SLOTS=slots)
            add("plain", D, 1500, VIS_SLOTS=slots)
        for slots in (1, 2):
            add("plain", D, 175, VIS_SLOTS=slots)
            add("plain", D, 400, VIS_SLOTS=slots)
    # filtered: 400 (HB 2), 256 (HB 1, 192-key ring in LDS that wraps), 512 (HB 2, 480 keys, wraps),
    # 600 (no exact variant: the register ladder)
    # oracle (tests/filtered_reference.py, 8 queries under each filter at D = 128): 400.0 / 256.0 /
    # 512.0 / 600.0 pops -- a denied point is popped and expanded like any other
    for D in (128, 96):
        for how in ("bitset", "table", "labels"):
            for iters in (400, 256, 512, 600):
                add(how, D, iters)
    for how in ("bitset", "labels"):              # layout {8,2}
        add(how, 64, 256)
        add(how, 64, 400)
    # partial rows: D = 70 is padded to 72, layout {8,3}; D = 100 is {16,2}; code rows of 128 bytes
    # of which 56 / 28 are padding
    # oracle: 175.0 / 600.0 pops at both D (D = 70 at tau = 1)
    for D in (70, 100):
        for how in ("plain", "labels"):
            add(how, D, 175)
            add(how, D, 600)
    # boundaries of the launchers
    # oracle at D = 128: K = 1 at 600 iterations: 597.9 pops (a few queries end early); K = 47 and
    # 48 at 700: 700.0
    for K in (1, 47, 48):                         # sorted part 32 or 64 / 64 / 96
        add("plain", 128, 175, K=K)
        add("plain", 128, 700 if K > 1 else 600, K=K)
        add("bitset", 128, 256, K=K)
    # oracle, N = 8 000: KBuild 20 and 40: 175.0 / 400.0 / 600.0 pops
    for kb in (20, 40):                           # 20: lanes past the row masked; 40: no early rows
        add("plain", 128, 175, kbuild=kb)
        add("plain", 128, 600, kbuild=kb)
        add("labels", 128, 400, kbuild=kb)
    # oracle: 175.0 / 400.0 / 600.0 pops
    for how, iters in (("plain", 175), ("plain", 600), ("labels", 400)):
        add(how, 132, iters)                      # {16,4}: code rows of Prescreen<16, 1>, flag set
    for hook in ("QUERY_GLOBAL_RING", "QUERY_EARLY"):
        for how, iters in (("plain", 175), ("plain", 400), ("plain", 600), ("bitset", 400)):
            add(how, 128, iters, **{hook: 0})
    return c


CASES = _cells()


def cell_id(cell):
    how, D, kb, K, tau, iters, hooks = cell
    return "-".join([how, f"D{D}", f"kb{kb}", f"K{K}", f"it{iters}"] +
                    [f"{k}={v}" for k, v in hooks])


def ring_of(D, K, iters):
    from ggnn_amd import ops
    cache, sorted_ = ops.query_sizing((D + 3) // 4 * 4, K, iters)
    return cache - sorted_


# one cell per exact family at D = 128 -- hashed set HB 1 and 2, tag set -8 and -9 --, the tag set
# on the other layouts, and a bitset and a labels cell with HB 2 and with the HB 1 ring that wraps
ORACLE_CELLS = [
    ("plain", 128, KBUILD, 10, TAU, 175, ()), ("plain", 128, KBUILD, 10, TAU, 400, ()),
    ("plain", 128, KBUILD, 10, TAU, 600, ()), ("plain", 128, KBUILD, 10, TAU, 1500, ()),
    ("plain", 96, KBUILD, 10, TAU, 600, ()), ("plain", 100, KBUILD, 10, TAU, 600, ()),
    ("plain", 64, KBUILD, 10, TAU_SHORT_ROWS, 600, ()),
    ("bitset", 128, KBUILD, 10, TAU, 400, ()), ("bitset", 128, KBUILD, 10, TAU, 256, ()),
    ("labels", 128, KBUILD, 10, TAU, 400, ()), ("labels", 128, KBUILD, 10, TAU, 256, ()),
]
N_ORACLE = 64


# ---- filters ---------------------------------------------------------------------------------------
@contextlib.contextmanager
def filter_of(c, how):
    """the filter of the existing lossless tests on this engine: (argument of the search for the
    first nq queries, allowed [nq, N] of those queries), both as functions of nq"""
    n = len(c.base)
    if how == "plain":
        yield (lambda nq: None), (lambda nq: np.ones((nq, n), bool))
    elif how == "bitset":
        mask = bitset_filter(n)
        yield (lambda nq: mask), (lambda nq: np.broadcast_to(mask, (nq, n)))
    elif how == "table":
        masks, fid = table_filter(n)
        rows = np.concatenate([masks, np.ones((1, n), bool)])      # id -1: the last row
        c.eng.set_filters(masks)
        try:
            yield (lambda nq: fid[:nq]), (lambda nq: rows[fid[:nq]])
        finally:
            c.eng.set_filters(None)
    else:
        labels, ql = label_filter(n)
        c.eng.set_labels(labels)
        try:
            yield (lambda nq: ql[:nq]), \
                (lambda nq: (ql[:nq, None] < 0) | (labels[None, :] == ql[:nq, None]))
        finally:
            c.eng.set_labels(None)


def assert_allowed(res, allowed):
    ids = res[0]
    hit = ids >= 0
    assert np.take_along_axis(allowed, np.maximum(ids, 0), 1)[hit].all(), "a denied id is returned"


# ---- the tests ---------------------------------------------------------------------------------------
_default_slots = {}


@pytest.fixture(scope="module")
def default_slots():
    """(default result, rows read) of the cells that are also run with shrunken buckets"""
    yield _default_slots
    _default_slots.clear()


@pytest.mark.parametrize("cell", CASES, ids=cell_id)
def test_cell(case, default_slots, cell):
    how, D, kb, K, tau, iters, hooks = cell
    c, grid_q = case("int", D, n_rows(D, kb), kb)
    assert c.flag() == 1.0
    variant = exact_variant(how, D, kb, K, iters, dict(hooks))
    ring = ring_of(D, K, iters)
    kw = dict(iters=iters, k=K, tau=tau, how=how)
    with filter_of(c, how) as (arg, allowed):
        for batch, q in (("mixed", mixed_queries(c.base, grid_q, F(1))), ("grid", grid_q)):
            on, off = three_way(c, q, arg=arg(NQ), hooks=dict(hooks), **kw)
            rows = INTEGRAL_ROWS if batch == "mixed" else np.ones(NQ, bool)
            assert np.array_equal(on[1][rows], true_l2(c.base, q[rows], on[0][rows]))
            assert_allowed(on, allowed(NQ))
            # the search was as long as the cell means it to be
            pops = on[2]["n_pop"] / NQ
            print(f"{cell_id(cell)} {batch}: {pops:.1f} pops per query, ring {ring}")
            assert pops >= 0.8 * iters
            if how != "plain" and iters in (256, 512):
                assert iters > ring and pops > ring, "the ring in LDS was meant to wrap"
            # which kernel ran
            if batch == "grid":
                if variant:
                    assert on[3]["float_rows"] < off[3]["float_rows"], variant
                else:
                    assert on[3] == off[3]
            # the visited set is exact: nothing depends on the size of its buckets
            if any(k == "VIS_SLOTS" for k, _ in hooks):
                rest = {k: v for k, v in hooks if k != "VIS_SLOTS"}
                key = (how, D, kb, K, tau, iters, tuple(sorted(rest.items())), batch)
                if key not in default_slots:
                    default_slots[key] = c.search(q, arg=arg(NQ), hooks=rest, **kw)
                assert_same(on, default_slots[key])
                assert on[3] == default_slots[key][3]


@pytest.mark.parametrize("cell", ORACLE_CELLS, ids=cell_id)
def test_against_the_oracle(case, orc, cell):
    """the first 64 integral queries of the mixed batch (on grid, a copy of a base row, clamped on
    either side) against the CPU oracle on the engine's own graph: orc.query, and under a filter
    tests/filtered_reference.py -- ids and distance bytes per query, counter sums against the
    handle's totals of the launch"""
    from filtered_reference import py_query_filtered
    how, D, kb, K, tau, iters, hooks = cell
    c, grid_q = case("int", D, n_rows(D, kb), kb)
    q = np.ascontiguousarray(mixed_queries(c.base, grid_q, F(1))[INTEGRAL_ROWS][:N_ORACLE])
    g = c.eng.get_graph(0)
    graph0 = g.graph[0].view.numpy()
    start = g.translation[3].view.numpy().reshape(-1)
    stats = g.nn1_stats.view.numpy().reshape(-1)
    with filter_of(c, how) as (arg, allowed):
        got = c.search(q, iters=iters, k=K, tau=tau, how=how, arg=arg(N_ORACLE), hooks=dict(hooks))
        if how == "plain":
            o_ids, o_d, o_nd, o_np = orc.query(c.base, q, graph0, start, stats, K, tau, iters,
                                               counters=True)
        else:
            ok = allowed(N_ORACLE)
            ref = [py_query_filtered(c.base, q[i], graph0, start, stats, K, tau, iters, ok[i])
                   for i in range(N_ORACLE)]
            o_ids, o_d = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
            o_nd, o_np = np.array([r[2] for r in ref]), np.array([r[3] for r in ref])
    differ = np.nonzero((got[0] != o_ids).any(1) |
                        (got[1].view(np.uint32) != o_d.view(np.uint32)).any(1))[0]
    if len(differ):
        i = int(differ[0])
        raise AssertionError(f"{cell_id(cell)}: query {i} differs: kernel {got[0][i]} {got[1][i]}, "
                             f"oracle {o_ids[i]} {o_d[i]}")
    assert got[2] == {"n_dist": int(o_nd.sum()), "n_pop": int(o_np.sum())}
