"""GPU tests of the label-set filters: up to eight labels per query, combined with a filter id into
the resident filter table (ggnn_*_labeled_in and their operators).  The contract is one sentence --
query n is the per-call filtered search of that query with the bitset
isin(base_labels, set n) & row(filter_ids[n]) -- and every comparison here is bit for bit:
array_equal on ids, tobytes() on distances, equal counters.  Base, graphs and label classes are
those of tests/test_gpu_labels.py."""
import numpy as np
import pytest

from filtered_reference import bf_filtered_reference, py_query_filtered
from test_gpu_labels import (D, INT32_MAX, INT32_MIN, N, QLABELS, SEAM_CASES, STARTS, UNUSED,
                             VARIANTS, _base_labels, _cast, _dev, _same, _table_bits, _torch,
                             graphs)  # noqa: F401  (graphs: the module fixture)

pytestmark = pytest.mark.gpu

# the ten label sets: one class, the wildcard, a label no row carries, two and three classes, a
# repeated entry, a class with an unused label, a class with the wildcard, eight distinct values of
# which only STARTS is carried by any row, and the two ends of int32
SETS = [[1], [-1], [UNUSED], [0, 1], [2, 3, -7], [1, 1, 1], [3, UNUSED], [0, -1],
        [5000, 5001, STARTS, 5003, INT32_MIN, 5005, 5006, 5007], [INT32_MAX, INT32_MIN]]
FIDS = np.array([-1, 0, 1, 2, 99] * 2, np.int32)


def _padded(sets, width):
    """[Nq, width] int32: every set padded by repeating its first entry"""
    assert all(1 <= len(s) <= width for s in sets)
    return np.array([list(s) + [s[0]] * (width - len(s)) for s in sets], np.int32)


def _table(n=N, seed=56):
    """three rows: about 50 % random, about 5 % random, every id but every seventh (the seed: row 0
    leaves fewer than ten of the 3000-row base's class 3, a partly filled row at K = 10)"""
    u = np.random.default_rng(seed).random((2, n))
    return np.stack([u[0] < 0.5, u[1] < 0.05, np.arange(n) % 7 != 0])


def _in_set(labels, s):
    return np.ones(len(labels), bool) if -1 in s else np.isin(labels, np.array(s, np.int32))


def _row(table, f):
    if f == -1:
        return np.ones(table.shape[1], bool)
    return table[f] if 0 <= f < len(table) else np.zeros(table.shape[1], bool)


def _composed(labels, sets, table=None, fids=None):
    """the whole contract: one allowed array per query"""
    return np.stack([_in_set(labels, s) & (_row(table, int(fids[i])) if fids is not None else True)
                     for i, s in enumerate(sets)])


@pytest.mark.parametrize("KB,K,iters", SEAM_CASES, ids=[f"kb{c[0]}-k{c[1]}-it{c[2]}" for c in SEAM_CASES])
def test_seam_query_labeled_in(graphs, KB, K, iters):
    """every kernel form and element type, width 8, without filter ids and with them, against the
    CPU reference on the composed masks and against the filter table of those masks.

    Not vacuous: the reference rows of the ten queries (under both id arrays) hold an empty one, a
    partly filled one and -- wherever a search can fill a row at all -- a full one.  A search visits
    at most num_start + iters * KBuild points, which for K 2100 at 64 iterations of a KBuild 24
    graph is below K: that case can have no full row, and asks for one with more than K / 4 entries
    instead.  (Without ids no set of the ten admits between 1 and 9 rows -- the smallest classes have
    22 and 32 -- so at K = 10 the partly filled row is one under the ids.)"""
    from ggnn_amd import ops
    g, base = graphs[KB], graphs["base"]
    tau = 0.6
    labels = _base_labels(g)
    table = _table()
    assert 0.45 < table[0].mean() < 0.55 and 0.03 < table[1].mean() < 0.07
    nq = len(SETS)
    q = np.random.default_rng(K + iters).integers(0, 128, (nq, D)).astype(np.float32)
    runs = []
    for fids in (None, FIDS):
        allowed = _composed(labels, SETS, table, fids)
        ref = [py_query_filtered(base, q[i], g["graph"], g["start"], g["stats"], K, tau, iters,
                                 allowed[i]) for i in range(nq)]
        runs.append((fids, allowed, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]),
                     np.array([r[2] for r in ref]), np.array([r[3] for r in ref])))
    filled = np.concatenate([np.isfinite(r[3]).sum(1) for r in runs])
    print("finite entries per query:", filled.tolist())
    assert (filled == 0).any() and ((filled > 0) & (filled < K)).any()
    if K <= len(g["start"]) + iters * KB:
        assert (filled == K).any()
    else:
        assert (filled > K // 4).any()
    d_labels, d_sets = _dev(labels), _dev(_padded(SETS, 8))
    c_fids = _dev(np.arange(nq))
    for variant in VARIANTS:
        d_base, d_q = _cast(base, variant), _cast(q, variant)
        ps = ops.prescreen_encode(d_base, 0) if variant == "f32_ps" else None
        common = (g["d_graph"], g["d_start"], g["d_stats"], K, tau)
        for fids, allowed, r_ids, r_d, r_nd, r_pop in runs:
            what = (variant, fids is not None)
            d_table, d_fids = (_table_bits(table), _dev(fids)) if fids is not None else (None, None)
            ids, d, nd, npop = [x.cpu().numpy() for x in ops.query_labeled_in(
                d_base, d_q, *common, d_labels, d_sets, d_table, d_fids, iters, counters=True,
                prescreen=ps)]
            assert np.array_equal(ids, r_ids), what
            assert d.tobytes() == r_d.tobytes(), what
            assert np.array_equal(nd, r_nd) and np.array_equal(npop, r_pop), what
            empty = ~allowed.any(1)
            assert (ids[empty] == -1).all() and np.isinf(d[empty]).all() and (d[empty] > 0).all()
            # ... and the filter table of the composed masks on the same device arrays
            t_ids, t_d, t_nd, t_pop = [x.cpu().numpy() for x in ops.query_filtered_by(
                d_base, d_q, *common, _table_bits(allowed), c_fids, iters, counters=True,
                prescreen=ps)]
            assert np.array_equal(ids, t_ids) and d.tobytes() == t_d.tobytes(), what
            assert np.array_equal(nd, t_nd) and np.array_equal(npop, t_pop), what


@pytest.mark.parametrize("variant", ["f32", "f32_ps", "u8", "bf16"])
def test_seam_widths(graphs, variant):
    """width 1 without ids is query_labeled, width 3 equals width 8 on sets of at most three
    entries, an all -1 set with ids is query_filtered_by (ids 99 and -1 included; once more without
    any table, where an id is -1 or admits nothing); every width 1 .. 8 equals width 8 padded, a set
    whose -1 stands last of eight or in the middle is query_filtered_by, and widths and wildcard
    once more under cosine"""
    from ggnn_amd import ops
    g, base = graphs[24], graphs["base"]
    K, tau, iters = 10, 0.6, 400
    labels, table = _base_labels(g), _table()
    nq = len(QLABELS)
    q = np.random.default_rng(5).integers(0, 128, (nq, D)).astype(np.float32)
    d_base, d_q = _cast(base, variant), _cast(q, variant)
    ps = ops.prescreen_encode(d_base, 0) if variant == "f32_ps" else None
    args = (d_base, d_q, g["d_graph"], g["d_start"], g["d_stats"], K, tau)
    kw = dict(max_iterations=iters, counters=True, prescreen=ps)
    d_labels, d_table, d_fids = _dev(labels), _table_bits(table), _dev(FIDS)

    def same(a, b, what):
        for x, y in zip(a, b):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), what

    one = ops.query_labeled_in(*args, d_labels, _dev(QLABELS.reshape(-1, 1)), **kw)
    same(one, ops.query_labeled(*args, d_labels, _dev(QLABELS), **kw), "width 1")
    short = [s for s in SETS if len(s) <= 3] + [[3], [-7, 2]]
    short = (short * 2)[:nq]
    for ids in (None, d_fids):
        tab = d_table if ids is not None else None
        w3 = ops.query_labeled_in(*args, d_labels, _dev(_padded(short, 3)), tab, ids, **kw)
        w8 = ops.query_labeled_in(*args, d_labels, _dev(_padded(short, 8)), tab, ids, **kw)
        same(w3, w8, "width 3 == width 8")
    assert np.isfinite(w3[1].cpu().numpy()).any()
    for width in (1, 8):
        wild = _dev(np.full((nq, width), -1))
        same(ops.query_labeled_in(*args, d_labels, wild, d_table, d_fids, **kw),
             ops.query_filtered_by(*args, d_table, d_fids, **kw), "all -1 with ids")
    # no table at all: id -1 is the labelled search, every other id an empty result
    no_table = ops.query_labeled_in(*args, d_labels, _dev(QLABELS.reshape(-1, 1)), None, d_fids, **kw)
    sel = FIDS == -1
    assert sel.any() and not sel.all()
    for x, y in zip(no_table[:2], one[:2]):
        assert x.cpu().numpy()[sel].tobytes() == y.cpu().numpy()[sel].tobytes()
    assert (no_table[0].cpu().numpy()[~sel] == -1).all()
    assert np.isinf(no_table[1].cpu().numpy()[~sel]).all()
    # every width 1 .. 8, on sets of at most that many entries, is width 8 padded: entry j of a set
    # is read at [n * width + j], and the entries beyond the width repeat the first
    pool = SETS + [[3], [-7, 2], [2, 1, 0, 3], [-7, 3, 2, 1, UNUSED], [9, 8, 7, 6, 5, 1],
                   [9, 8, 7, 6, 5, 4, 2]]
    assert {len(s) for s in pool} == set(range(1, 9))
    for width in range(1, 9):
        fit = [s for s in pool if len(s) <= width]
        longest = [s for s in fit if len(s) == width]
        sets = (longest + fit * nq)[:nq]                   # the sets of exactly this width first
        for ids in (None, d_fids):
            tab = d_table if ids is not None else None
            w = ops.query_labeled_in(*args, d_labels, _dev(_padded(sets, width)), tab, ids, **kw)
            w8 = ops.query_labeled_in(*args, d_labels, _dev(_padded(sets, 8)), tab, ids, **kw)
            same(w, w8, ("width", width, ids is not None))
            assert np.isfinite(w[1].cpu().numpy()).any(), width
    # the wildcard last of eight and in the middle, next to labels no row carries: with ids that is
    # query_filtered_by, whatever the other entries are
    last = [[5000 + j for j in range(7)] + [-1]] * nq
    middle = [[UNUSED, 1, 5002, -1, 5004, 0, INT32_MIN, 5007]] * nq
    by_ids = ops.query_filtered_by(*args, d_table, d_fids, **kw)
    assert np.isfinite(by_ids[1].cpu().numpy()).any()
    for name, wild in (("last", last), ("middle", middle)):
        same(ops.query_labeled_in(*args, d_labels, _dev(wild), d_table, d_fids,
                                  **kw), by_ids, ("-1 " + name, "with ids"))
    # ... and under cosine (query_labelset_kernel<.., kCos, ..> of this layout at K = 10): widths 3
    # and 5 against width 8, the wildcard in the middle against query_filtered_by.  Graph and nn1
    # statistics are those built for squared L2 on the unclamped base: sound only because both
    # sides of each comparison are GPU runs on the same inputs -- no reference stands behind this
    # block (cosine against py_query_filtered: tests/test_gpu_labelset_layout_matrix.py, width 8)
    base_c = np.maximum(base, 1.0)                         # (no zero row)
    c_base, c_q = _cast(base_c, variant), _cast(np.maximum(q, 1.0), variant)
    c_args = (c_base, c_q) + args[2:]
    c_kw = dict(kw, measure=1, prescreen=ops.prescreen_encode(c_base, 1) if variant == "f32_ps" else None)
    for width in (3, 5):
        fit = [s for s in pool if len(s) <= width]
        sets = ([s for s in fit if len(s) == width] + fit * nq)[:nq]
        w = ops.query_labeled_in(*c_args, d_labels, _dev(_padded(sets, width)), d_table, d_fids, **c_kw)
        w8 = ops.query_labeled_in(*c_args, d_labels, _dev(_padded(sets, 8)), d_table, d_fids, **c_kw)
        same(w, w8, ("cosine, width", width))
        assert np.isfinite(w[1].cpu().numpy()).any()
    same(ops.query_labeled_in(*c_args, d_labels, _dev(middle), d_table, d_fids,
                              **c_kw),
         ops.query_filtered_by(*c_args, d_table, d_fids, **c_kw), "cosine, -1 in the middle")


def test_seam_shard_offset(graphs):
    """second shard of two per GPU: labels and bits read at offset N of a column and a table over
    2 N ids, result columns and the -1 of empty slots offset as the unfiltered kernel writes them"""
    from ggnn_amd import ops
    g, base = graphs[24], graphs["base"]
    K, tau, iters = 10, 0.6, 200
    labels, table = _base_labels(g), _table()
    # this shard's labels and bits are the upper half; the lower half carries other values
    wide = np.concatenate([np.roll(labels, 17), labels])
    wide_table = np.concatenate([np.roll(table, 29, axis=1), table], axis=1)
    allowed = _composed(labels, SETS, table, FIDS)
    nq = len(SETS)
    q = np.random.default_rng(9).integers(0, 128, (nq, D)).astype(np.float32)
    d_base, d_q = _cast(base, "f32"), _cast(q, "f32")
    args = (d_base, d_q, g["d_graph"], g["d_start"], g["d_stats"], K, tau)
    ids, d = ops.query_labeled_in(*args, _dev(wide), _dev(_padded(SETS, 8)), _table_bits(wide_table),
                                  _dev(FIDS), iters, bit_offset=N, shards_per_gpu=2, on_gpu_shard=1)
    wide_allowed = np.concatenate([np.zeros_like(allowed), allowed], axis=1)
    t_ids, t_d = ops.query_filtered_by(*args, _table_bits(wide_allowed), _dev(np.arange(nq)), iters,
                                       filter_bit_offset=N, shards_per_gpu=2, on_gpu_shard=1)
    assert np.array_equal(ids.cpu().numpy()[:, K:], t_ids.cpu().numpy()[:, K:])
    assert d.cpu().numpy()[:, K:].tobytes() == t_d.cpu().numpy()[:, K:].tobytes()
    ids, d = ids.cpu().numpy()[:, K:], d.cpu().numpy()[:, K:]
    some_empty = False
    for i in range(nq):
        r = py_query_filtered(base, q[i], g["graph"], g["start"], g["stats"], K, tau, iters,
                              allowed[i])
        assert np.array_equal(ids[i], r[0] + N) and d[i].tobytes() == r[1].tobytes(), i
        if not allowed[i].any():
            some_empty = True
            assert (ids[i] == N - 1).all() and np.isinf(d[i]).all()
    assert some_empty


@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("variant", ["f32", "u8", "f16", "bf16"])
def test_seam_bf_query_labeled_in(orc, graphs, variant, measure):
    """k 10 (register list) and k 300 (the LDS scan kernel), both above the size of the smallest
    classes, so slots are padded; N = 3000 is no multiple of 64; with and without filter ids, and
    once more with labels and bits at offset N of a column and a table over 2 N ids"""
    from ggnn_amd import ops
    base = np.maximum(graphs["base"], 1.0)                # (no zero row: cosine)
    labels, table = _base_labels(graphs[24]), _table()
    labels[np.nonzero(labels == 3)[0][5:]] = 2            # a class of exactly five rows
    assert (labels == 3).sum() == 5
    sets = SETS[:6] + [[3]] + SETS[7:]
    nq = len(sets)
    q = np.maximum(np.random.default_rng(61 + measure).integers(0, 128, (nq, D)), 1)
    q = q.astype(np.float32)
    d_base, d_q = _cast(base, variant), _cast(q, variant)
    d_labels, d_sets = _dev(labels), _dev(_padded(sets, 8))
    wide = np.concatenate([np.roll(labels, 5), labels])
    wide_table = np.concatenate([np.roll(table, 3, axis=1), table], axis=1)
    for fids in (None, FIDS):
        allowed = _composed(labels, sets, table, fids)
        d_table, d_fids = (_table_bits(table), _dev(fids)) if fids is not None else (None, None)
        for K in (10, 300):
            ids, d = ops.bf_query_labeled_in(d_base, d_q, K, d_labels, d_sets, d_table, d_fids, measure)
            t_ids, t_d = ops.bf_query_filtered_by(d_base, d_q, K, _table_bits(allowed),
                                                  _dev(np.arange(nq)), measure)
            assert _torch().equal(ids, t_ids)
            assert d.cpu().numpy().tobytes() == t_d.cpu().numpy().tobytes()
            o_ids, o_d = ops.bf_query_labeled_in(
                d_base, d_q, K, _dev(wide), d_sets,
                _table_bits(wide_table) if fids is not None else None, d_fids, measure, bit_offset=N)
            assert _torch().equal(ids, o_ids)
            assert d.cpu().numpy().tobytes() == o_d.cpu().numpy().tobytes()
            ids, d = ids.cpu().numpy(), d.cpu().numpy()
            for i in range(nq):
                r_ids, r_d = bf_filtered_reference(orc, base, q[i:i + 1], K, allowed[i], measure)
                assert np.array_equal(ids[i], r_ids[0]) and d[i].tobytes() == r_d[0].tobytes(), (K, i)
            if fids is None:                              # five rows, then padding
                assert (ids[6, :5] >= 0).all() and (ids[6, 5:] == -1).all() and np.isinf(d[6, 5:]).all()


@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("variant", ["f32", "u8"])
def test_seam_bf_query_labeled_in_sliced_base(orc, variant, measure):
    """few queries on a base large enough for several slices: with five queries launch_bf_query_labelset
    splits 20011 rows into four slices of 5056, every (query, slice) wave reads labels and bitset
    words from its slice's first row on, and the partial lists are merged lower slice first.  A block
    of 40 rows is repeated across the first slice boundary (ties come out by lower base index, and
    two queries are rows of that block), one query's rows lie in the third slice only, one query
    admits nothing; label column and table are windows at bit offset 37.  The one-label scan
    (ops.bf_query_labeled) runs on the same base."""
    from ggnn_amd import ops
    Nb, nq, off, SLICE = 20011, 5, 37, 5056
    # launch_bf_query_labelset: below 4096 waves the base is split, into at most Nb / 4096 slices;
    # bf_slice_rows: their rows rounded up to a multiple of 64
    slices = min(-(-(256 * 16) // nq), max(1, Nb // 4096)) if nq < 256 * 16 else 1
    assert slices == 4 and ((Nb + slices - 1) // slices + 63) // 64 * 64 == SLICE
    assert -(-Nb // SLICE) == slices
    rs = np.random.default_rng(151 + measure)
    base = rs.integers(1, 5, (Nb, D)).astype(np.float32)        # many equal distances, no zero row
    base[SLICE:SLICE + 40] = base[SLICE - 40:SLICE]
    q = rs.integers(1, 5, (nq, D)).astype(np.float32)
    q[0], q[3] = base[SLICE - 26], base[SLICE - 36]
    labels = rs.integers(0, 4, Nb).astype(np.int32)
    third = np.arange(Nb) // SLICE == 2
    labels[third & (rs.random(Nb) < 0.1)] = 5                   # label 5: the third slice only
    labels[SLICE - 40:SLICE + 40] = 0
    table = np.stack([rs.random(Nb) < 0.3, rs.random(Nb) < 0.05])
    table[0, SLICE - 40:SLICE + 40] = True
    sets = [[0, 1], [5], [UNUSED, 77], [-1], [2, 5, 3]]
    fids = np.array([0, -1, 1, -1, 1], np.int32)
    qlabels = np.array([0, 5, UNUSED, -1, 2], np.int32)
    allowed = _composed(labels, sets, table, fids)
    where = [np.unique(np.nonzero(a)[0] // SLICE).tolist() for a in allowed]
    assert where == [[0, 1, 2, 3], [2], [], [0, 1, 2, 3], [0, 1, 2, 3]]
    wide_labels = np.concatenate([rs.integers(0, 6, off), labels, rs.integers(0, 6, 60)])
    wide_table = rs.random((2, off + Nb + 60)) < 0.5
    wide_table[:, off:off + Nb] = table
    d_base, d_q = _cast(base, variant), _cast(q, variant)
    d_sets, d_fids = _dev(_padded(sets, 8)), _dev(fids)
    for K in (10, 300):
        ref = [bf_filtered_reference(orc, base, q[i:i + 1], K, allowed[i], measure) for i in range(nq)]
        r_ids, r_d = np.concatenate([r[0] for r in ref]), np.concatenate([r[1] for r in ref])
        # both copies of the queries' own rows lead their lists, the lower slice's first
        assert r_ids[0, :2].tolist() == [SLICE - 26, SLICE + 14] and r_d[0, 0] == r_d[0, 1]
        assert r_ids[3, :2].tolist() == [SLICE - 36, SLICE + 4] and r_d[3, 0] == r_d[3, 1]
        assert (r_ids[2] == -1).all() and (r_ids[1] >= 2 * SLICE).all() and (r_ids[1] < 3 * SLICE).all()
        runs = {
            "offset 0": ops.bf_query_labeled_in(d_base, d_q, K, _dev(labels), d_sets,
                                                _table_bits(table), d_fids, measure),
            "windows": ops.bf_query_labeled_in(d_base, d_q, K, _dev(wide_labels), d_sets,
                                               _table_bits(wide_table), d_fids, measure, bit_offset=off),
            "table of the composed masks": ops.bf_query_filtered_by(
                d_base, d_q, K, _table_bits(allowed), _dev(np.arange(nq)), measure)}
        for name, (ids, d) in runs.items():
            assert np.array_equal(ids.cpu().numpy(), r_ids), (K, name)
            assert d.cpu().numpy().tobytes() == r_d.tobytes(), (K, name)
        # one label per query
        one = [bf_filtered_reference(orc, base, q[i:i + 1], K,
                                     np.ones(Nb, bool) if L == -1 else labels == L, measure)
               for i, L in enumerate(qlabels)]
        o_ids, o_d = np.concatenate([r[0] for r in one]), np.concatenate([r[1] for r in one])
        assert o_ids[0, :2].tolist() == [SLICE - 26, SLICE + 14]
        assert (o_ids[2] == -1).all() and (o_ids[1] >= 2 * SLICE).all() and (o_ids[1] < 3 * SLICE).all()
        for name, (ids, d) in {
                "offset 0": ops.bf_query_labeled(d_base, d_q, K, _dev(labels), _dev(qlabels), measure),
                "window": ops.bf_query_labeled(d_base, d_q, K, _dev(wide_labels), _dev(qlabels),
                                               measure, bit_offset=off)}.items():
            assert np.array_equal(ids.cpu().numpy(), o_ids), (K, name, "one label")
            assert d.cpu().numpy().tobytes() == o_d.tobytes(), (K, name, "one label")


# ---- the handle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ctx", [1, 4])
def test_handle_label_sets(n_ctx):
    """two shards per GPU on one GPU and on a handle of four device contexts; 37 queries with mixed
    sets and filter ids through every path of the blocking driver and two asynchronous slots.  The
    expectation comes from the same handle and graph: the table of the composed masks and
    query_filtered_by first, then the user's table and query_labeled_in."""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    torch = _torch()
    Nb, Dh, K, tau, iters, nq = 8000, 64, 10, 0.7, 200, 37
    NSH = Nb // (2 * n_ctx)
    base = np.random.default_rng(187).integers(0, 256, (Nb, Dh)).astype(np.float32)
    q = np.random.default_rng(188).integers(0, 256, (nq, Dh)).astype(np.float32)
    rs = np.random.default_rng(5)
    labels = _base_labels(None, Nb, seed=6)
    pool = SETS[:8] + [[5000, 5001, 3, 5003, INT32_MIN, 5005, 5006, 5007], SETS[9]]
    sets = [pool[i] for i in list(range(len(pool))) + rs.integers(0, len(pool), nq - len(pool)).tolist()]
    sets2 = sets[11:] + sets[:11]
    table = _table(Nb)
    fids = rs.integers(-1, 3, nq).astype(np.int32)
    fids[:4] = [-1, 0, 1, 2]
    fids2 = np.roll(fids, 5)
    all_rows = np.arange(nq, dtype=np.int32)
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_labels(labels)
    if n_ctx > 1:
        eng.set_gpus([0] * n_ctx)
    eng.set_shard_size(NSH)
    eng.build(24, 0.5, 1)
    modes = [{}, {"SHARD_OVERLAP": 0}, {"EXCHANGE": 1, "QUERY_SPLIT": 1}] if n_ctx == 1 else \
        [{}, {"QUERY_SPLIT": 1}, {"EXCHANGE": 3, "QUERY_SPLIT": 1}, {"EXCHANGE": 2, "QUERY_SPLIT": 0}]

    def expect(labels, table, sets, fids, hooks={}, k=K, bf=False, counters=False):
        """the composed masks as the resident table, searched by query_filtered_by"""
        eng.set_filters(_composed(labels, sets, table, fids))
        with _lib.hooks(**hooks):
            want = eng.bf_query_filtered_by(q, k, filter_ids=all_rows) if bf else \
                eng.query_filtered_by(q, K, tau, iters, filter_ids=all_rows)
        c = eng.last_query_counters() if counters else None
        eng.set_filters(table)
        return (want, c) if counters else want

    def check_all(labels, table, what):
        want = expect(labels, table, sets, fids)
        want2 = expect(labels, table, sets2, fids2)
        want_l = expect(labels, table, sets, None)
        w_d = want[1].numpy()
        filled = np.isfinite(w_d).sum(1)
        assert (filled == 0).any() and (filled == K).any(), what
        ragged = eng.query_labeled_in(q, K, tau, iters, label_sets=sets, filter_ids=fids)
        _same(ragged, want, (what, "ragged"))
        for hooks in modes[1:]:
            w = expect(labels, table, sets, fids, hooks)
            with _lib.hooks(**hooks):
                _same(eng.query_labeled_in(q, K, tau, iters, label_sets=sets, filter_ids=fids), w,
                      (what, hooks))
        # 2-D, int64 and device forms; ids on the host and on the device
        p8 = _padded(sets, 8)
        for form in (p8, p8.astype(np.int64), torch.from_numpy(p8), torch.from_numpy(p8).cuda()):
            _same(eng.query_labeled_in(q, K, tau, iters, label_sets=form,
                                       filter_ids=torch.from_numpy(fids).cuda()), want, what)
        _same(eng.query_labeled_in(q, K, tau, iters, label_sets=sets), want_l, (what, "no ids"))
        # two asynchronous slots in flight with different sets and ids
        if n_ctx == 1:
            qd = torch.from_numpy(q).cuda()
            t0 = eng.query_async_labeled_in(qd, K, tau, iters, slot=0, label_sets=torch.from_numpy(p8).cuda(),
                                            filter_ids=torch.from_numpy(fids).cuda())
            t1 = eng.query_async_labeled_in(qd, K, tau, iters, slot=1, label_sets=sets2, filter_ids=fids2)
        else:
            t0 = eng.query_async_labeled_in(torch.from_numpy(q).cuda(), K, tau, iters, slot=0,
                                            label_sets=sets, filter_ids=fids)
            t1 = eng.query_async_labeled_in(torch.from_numpy(q), K, tau, iters, slot=1,
                                            label_sets=torch.from_numpy(_padded(sets2, 8)).cuda(),
                                            filter_ids=torch.from_numpy(fids2).cuda())
        assert t0.label_sets is not None and t1.filter_ids is not None
        eng.synchronize()
        for t, w in ((t0, want), (t1, want2)):
            _same((t.ids[:, :K], t.dists[:, :K]), w, (what, "async"))
        t2 = eng.query_async_labeled_in(torch.from_numpy(q).cuda(), K, tau, iters, slot=2, label_sets=sets)
        eng.synchronize()
        _same((t2.ids[:, :K], t2.dists[:, :K]), want_l, (what, "async, no ids"))
        _same(eng.query_labeled_in(q, K, tau, iters, label_sets=sets, filter_ids=fids), want,
              (what, "blocking again"))
        return want[0].numpy(), w_d

    first = check_all(labels, table, "as set")
    if n_ctx == 1:
        # results on the GPU: the sorted [Nq, K * shards] rows
        eng.set_return_results_on_gpu(True)
        ids_g, d_g = eng.query_labeled_in(torch.from_numpy(q).cuda(), K, tau, iters, label_sets=sets,
                                          filter_ids=fids)
        eng.set_return_results_on_gpu(False)
        assert ids_g.is_cuda and tuple(ids_g.shape) == (nq, 2 * K)
        _same((ids_g[:, :K], d_g[:, :K]), first, "results on the GPU")
        # counters equal to the composed table's
        eng.set_collect_counters(True)
        _, c_table = expect(labels, table, sets, fids, counters=True)
        eng.query_labeled_in(q, K, tau, iters, label_sets=sets, filter_ids=fids)
        c = eng.last_query_counters()
        eng.set_collect_counters(False)
        assert (c["n_dist"], c["n_pop"]) == (c_table["n_dist"], c_table["n_pop"]) and c["n_pop"] > 0
        # the exact search through the handle: always the scan
        for f in (fids, None):
            b = eng.bf_query_labeled_in(q, 100, label_sets=sets, filter_ids=f)
            assert eng.last_bf_query_matrix_path() == 0
            _same(b, expect(labels, table, sets, f, k=100, bf=True), "bf")
        _same(eng.bf_query_labeled_in(q, 100, label_sets=torch.from_numpy(_padded(sets, 8)).cuda()), b,
              "bf, device")
        # both arguments None: the unfiltered call; sets None: query_filtered_by
        _same(eng.query_labeled_in(q, K, tau, iters), eng.query(q, K, tau, iters), "both None")
        _same(eng.bf_query_labeled_in(q, 20), eng.bf_query(q, 20), "bf, both None")
        _same(eng.query_labeled_in(q, K, tau, iters, filter_ids=fids),
              eng.query_filtered_by(q, K, tau, iters, filter_ids=fids), "sets None")
        # errors that need the handle
        with pytest.raises(_lib.GGNNError) as e:
            eng.query_labeled_in(q, K, tau, iters, label_sets=sets, filter_ids=np.full(nq, 3))
        assert e.value.status == _lib.INVALID_ARGUMENT
        with pytest.raises(ValueError):
            eng.query_labeled_in(q, K, tau, iters, label_sets=np.zeros((nq, 9), np.int32))
        with pytest.raises(ValueError):
            eng.query_labeled_in(q, K, tau, iters, label_sets=[[1]] * (nq - 1) + [[]])

    # update_labels and update_filter change what the same arguments select
    labels2 = labels.copy()
    big = np.arange(Nb) % 3 == 0
    labels2[big] = 1
    eng.update_labels(np.nonzero(big)[0], np.full(big.sum(), 1, np.int32))
    table2 = table.copy()
    table2[0] = np.arange(Nb) % 5 < 2
    eng.update_filter(0, table2[0])
    second = check_all(labels2, table2, "relabelled, row 0 replaced")
    assert not np.array_equal(first[0], second[0])

    # ids without a table, then no labels
    eng.set_filters(None)
    with pytest.raises(_lib.GGNNError) as e:
        eng.query_labeled_in(q, K, tau, iters, label_sets=sets, filter_ids=fids)
    assert e.value.status == _lib.INVALID_STATE
    with pytest.raises(_lib.GGNNError) as e:
        eng.query_async_labeled_in(torch.from_numpy(q).cuda(), K, tau, iters, label_sets=sets,
                                   filter_ids=fids)
    assert e.value.status == _lib.INVALID_STATE
    _same(eng.query_labeled_in(q, K, tau, iters, label_sets=sets), expect(labels2, None, sets, None),
          "labels only, no table resident")
    eng.set_filters(None)
    eng.set_labels(None)
    for call in (lambda: eng.query_labeled_in(q, K, tau, iters, label_sets=sets),
                 lambda: eng.bf_query_labeled_in(q, K, label_sets=sets),
                 lambda: eng.query_async_labeled_in(torch.from_numpy(q).cuda(), K, tau, iters,
                                                    label_sets=sets)):
        with pytest.raises(_lib.GGNNError, match="labels") as e:
            call()
        assert e.value.status == _lib.INVALID_STATE


def test_handle_int8_base_is_unsupported():
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    Nb, Dh = 2000, 64
    base = np.random.default_rng(3).integers(-100, 100, (Nb, Dh)).astype(np.int8)
    q = base[:8].copy()
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_labels(np.arange(Nb, dtype=np.int32) % 4)
    sets = [[0, 1]] * 8
    with pytest.raises(_lib.GGNNError) as e:
        eng.bf_query_labeled_in(q, 10, label_sets=sets)
    assert e.value.status == _lib.UNSUPPORTED
    eng.build(24, 0.5, 1)
    with pytest.raises(_lib.GGNNError) as e:
        eng.query_labeled_in(q, 10, 0.6, 200, label_sets=sets)
    assert e.value.status == _lib.UNSUPPORTED
    # (the one-label form is built for int8 rows)
    ids, _ = eng.query_labeled(q, 10, 0.6, 200, labels=np.zeros(8, np.int32))
    assert (ids.numpy() >= 0).any()
