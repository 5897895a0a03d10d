"""GPU tests of the label-range filters: up to four closed intervals of signed int32 labels per
query, combined with a filter id into the resident filter table (ggnn_*_labeled_range and their
operators).  The contract is one sentence -- query n is the per-call filtered search of that query
with the bitset any_j(lo_j <= base_labels <= hi_j) & row(filter_ids[n]) -- and every comparison here
is bit for bit: array_equal on ids, tobytes() on distances, equal counters.  Base, graphs and label
classes are those of tests/test_gpu_labels.py; the column also carries the two ends of int32."""
import numpy as np
import pytest

from filtered_reference import bf_filtered_reference, py_query_filtered
from test_gpu_labels import (D, N, QLABELS, SEAM_CASES, STARTS, UNUSED, VARIANTS, _base_labels,
                             _cast, _dev, _same, _table_bits, _torch,
                             graphs)  # noqa: F401  (graphs: the module fixture)

pytestmark = pytest.mark.gpu

MIN, MAX = -2 ** 31, 2 ** 31 - 1
EMPTY = (1, 0)

# one interval list per query.  [(1, 0)], [(MAX, MIN)] and the ninth list are the ones an unsigned
# span compare without normalisation gets wrong: it admits every row for (1, 0) and (5, 4), and both
# ends of int32 for (MAX, MIN), where the contract admits none.  (-100, 0) spans the classes -7 and 0
# and contains -1, which is no wildcard here.
RANGES = [[(1, 1)], [(MIN, MAX)], [(UNUSED, UNUSED)], [(0, 1)], [(-7, -7), (2, 3)], [(-100, 0)],
          [(1, 0)], [(MAX, MIN)], [(3, 3), (1, 0), (STARTS, STARTS), (5, 4)], [(MIN, MIN), (MAX, MAX)],
          [(2, MAX)], [(MIN, -1)], [(MAX, MAX)]]
assert STARTS == 1000 and UNUSED == 4242
FIDS = np.array(([-1, 0, 1, 2, 99] * 3)[:len(RANGES)], np.int32)


def _labels(g, n=N, seed=3):
    """the classes of _base_labels; the first six rows of class -7 carry INT32_MIN, the next six
    INT32_MAX"""
    lab = _base_labels(g, n, seed)
    rest = np.nonzero(lab == -7)[0]
    assert len(rest) > 24
    lab[rest[:6]] = MIN
    lab[rest[6:12]] = MAX
    return lab


def _padded(lists, width=4, pad=EMPTY):
    """[Nq, width, 2] int32: every list padded with `pad` (an interval, or None: its first one)"""
    assert all(1 <= len(r) <= width for r in lists)
    return np.array([list(r) + [pad if pad is not None else r[0]] * (width - len(r)) for r in lists],
                    np.int64).astype(np.int32).reshape(len(lists), width, 2)


def _table(n=N, seed=56):
    """three rows: about 50 % random, about 5 % random, every id but every seventh"""
    u = np.random.default_rng(seed).random((2, n))
    return np.stack([u[0] < 0.5, u[1] < 0.05, np.arange(n) % 7 != 0])


def _in_ranges(labels, r):
    """the signed definition, in int64: lo <= label <= hi for some interval"""
    lab = labels.astype(np.int64)
    out = np.zeros(len(lab), bool)
    for lo, hi in r:
        out |= (lab >= int(lo)) & (lab <= int(hi))
    return out


def _row(table, f):
    if f == -1:
        return np.ones(table.shape[1], bool)
    return table[f] if 0 <= f < len(table) else np.zeros(table.shape[1], bool)


def _composed(labels, lists, table=None, fids=None):
    """the whole contract: one allowed array per query"""
    return np.stack([_in_ranges(labels, r) & (_row(table, int(fids[i])) if fids is not None else True)
                     for i, r in enumerate(lists)])


def test_the_interval_lists_select_what_they_are_meant_to(graphs):
    labels = _labels(graphs[24])
    counts = _composed(labels, RANGES).sum(1).tolist()
    print("admitted rows per list:", counts)
    cls = {L: int((labels == L).sum()) for L in (0, 1, 2, 3, -7, STARTS, MIN, MAX)}
    assert sum(cls.values()) == N and cls[MIN] == cls[MAX] == 6
    assert counts == [cls[1], N, 0, cls[0] + cls[1], cls[-7] + cls[2] + cls[3],
                      cls[-7] + cls[0], 0, 0, cls[3] + cls[STARTS], 12,
                      cls[2] + cls[3] + cls[STARTS] + 6, cls[-7] + 6, 6]
    # what the span compare alone would admit for the three lists that need the normalisation
    u = labels.astype(np.uint32)
    for i, wrong in ((6, N), (7, 12), (8, N)):
        got = np.zeros(N, bool)
        for lo, hi in RANGES[i]:
            got |= (u - np.uint32(lo & 0xffffffff)) <= np.uint32((hi - lo) & 0xffffffff)
        assert got.sum() == wrong != counts[i]


@pytest.mark.parametrize("KB,K,iters", SEAM_CASES, ids=[f"kb{c[0]}-k{c[1]}-it{c[2]}" for c in SEAM_CASES])
def test_seam_query_labeled_range(graphs, KB, K, iters):
    """every kernel form and element type, four intervals, without filter ids and with them, against
    the CPU reference on the composed masks and against the filter table of those masks.

    Not vacuous: the reference rows of the queries hold an empty one, a partly filled one and --
    wherever a search can fill a row at all -- a full one.  A search visits at most num_start +
    iters * KBuild points, which for K 2100 at 64 iterations of a KBuild 24 graph is below K: that
    case can have no full row, and asks for one with more than K / 4 entries instead."""
    from ggnn_amd import ops
    g, base = graphs[KB], graphs["base"]
    tau = 0.6
    labels = _labels(g)
    table = _table()
    assert 0.45 < table[0].mean() < 0.55 and 0.03 < table[1].mean() < 0.07
    nq = len(RANGES)
    q = np.random.default_rng(K + iters).integers(0, 128, (nq, D)).astype(np.float32)
    runs = []
    for fids in (None, FIDS):
        allowed = _composed(labels, RANGES, table, fids)
        ref = [py_query_filtered(base, q[i], g["graph"], g["start"], g["stats"], K, tau, iters,
                                 allowed[i]) for i in range(nq)]
        runs.append((fids, allowed, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]),
                     np.array([r[2] for r in ref]), np.array([r[3] for r in ref])))
    for r in runs:                                         # without ids, and with them
        filled = np.isfinite(r[3]).sum(1)
        print("finite entries per query:", filled.tolist())
        assert (filled == 0).any() and ((filled > 0) & (filled < K)).any()
    filled = np.concatenate([np.isfinite(r[3]).sum(1) for r in runs])
    if K <= len(g["start"]) + iters * KB:
        assert (filled == K).any()
    else:
        assert (filled > K // 4).any()
    d_labels, d_ranges = _dev(labels), _dev(_padded(RANGES))
    c_fids = _dev(np.arange(nq))
    for variant in VARIANTS:
        d_base, d_q = _cast(base, variant), _cast(q, variant)
        ps = ops.prescreen_encode(d_base, 0) if variant == "f32_ps" else None
        common = (g["d_graph"], g["d_start"], g["d_stats"], K, tau)
        for fids, allowed, r_ids, r_d, r_nd, r_pop in runs:
            what = (variant, fids is not None)
            d_table, d_fids = (_table_bits(table), _dev(fids)) if fids is not None else (None, None)
            ids, d, nd, npop = [x.cpu().numpy() for x in ops.query_labeled_range(
                d_base, d_q, *common, d_labels, d_ranges, d_table, d_fids, iters, counters=True,
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
def test_seam_equivalences(graphs, variant):
    """(L, L) without ids is query_labeled; degenerate intervals are query_labeled_in on sets without
    -1; (MIN, MAX) with ids is query_filtered_by (ids 99 and -1 included; once more without any
    table); every n_ranges 1 .. 4 equals the list padded to four, by repetition and by (1, 0); the
    order of the intervals does not matter; the paddings once more under cosine"""
    from ggnn_amd import ops
    g, base = graphs[24], graphs["base"]
    K, tau, iters = 10, 0.6, 400
    labels, table = _labels(g), _table()
    qlab = QLABELS.copy()
    qlab[qlab == -1] = -7                                  # (-1 is the wildcard of query_labeled)
    nq = len(qlab)
    fids = FIDS[:nq]
    q = np.random.default_rng(5).integers(0, 128, (nq, D)).astype(np.float32)
    d_base, d_q = _cast(base, variant), _cast(q, variant)
    ps = ops.prescreen_encode(d_base, 0) if variant == "f32_ps" else None
    args = (d_base, d_q, g["d_graph"], g["d_start"], g["d_stats"], K, tau)
    kw = dict(max_iterations=iters, counters=True, prescreen=ps)
    d_labels, d_table, d_fids = _dev(labels), _table_bits(table), _dev(fids)

    def same(a, b, what):
        for x, y in zip(a, b):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), what

    def filled(r):
        return np.isfinite(r[1].cpu().numpy()).any()

    one = ops.query_labeled_range(*args, d_labels, _dev(np.stack([qlab, qlab], 1).reshape(nq, 1, 2)), **kw)
    same(one, ops.query_labeled(*args, d_labels, _dev(qlab), **kw), "(L, L)")
    assert filled(one)
    sets = ([[1], [0, 1], [2, 3, -7], [3, UNUSED], [MAX, MIN], [STARTS, 5000, 2, MIN], [UNUSED]] * 2)[:nq]
    deg = [[(v, v) for v in s] for s in sets]
    for ids in (None, d_fids):
        tab = d_table if ids is not None else None
        as_sets = np.array([s + s[:1] * (4 - len(s)) for s in sets], np.int32)
        r = ops.query_labeled_range(*args, d_labels, _dev(_padded(deg)), tab, ids, **kw)
        same(r, ops.query_labeled_in(*args, d_labels, _dev(as_sets), tab, ids, **kw), "degenerate")
        assert filled(r)
    for n in (1, 4):
        every = _dev(np.tile(np.array([MIN, MAX], np.int32), (nq, n, 1)))
        r = ops.query_labeled_range(*args, d_labels, every, d_table, d_fids, **kw)
        same(r, ops.query_filtered_by(*args, d_table, d_fids, **kw), "(MIN, MAX) with ids")
        assert filled(r)
    # no table at all: id -1 is the search under the intervals alone, every other id an empty result
    no_table = ops.query_labeled_range(*args, d_labels, _dev(_padded(deg)), None, d_fids, **kw)
    alone = ops.query_labeled_range(*args, d_labels, _dev(_padded(deg)), **kw)
    sel = fids == -1
    assert sel.any() and not sel.all()
    for x, y in zip(no_table[:2], alone[:2]):
        assert x.cpu().numpy()[sel].tobytes() == y.cpu().numpy()[sel].tobytes()
    assert (no_table[0].cpu().numpy()[~sel] == -1).all()
    assert np.isinf(no_table[1].cpu().numpy()[~sel]).all()
    # every n_ranges 1 .. 4, on lists of at most that many intervals, is the list padded to four:
    # interval j of a query is read at [(n * n_ranges + j) * 2]
    pool = RANGES + [[(0, 0), (2, 2)], [(-7, -7), (MIN, MIN), (3, 3)], [(5, 4), (2, 3), (MAX, MAX)]]
    assert {len(r) for r in pool} == {1, 2, 3, 4}
    for width in range(1, 5):
        fit = [r for r in pool if len(r) <= width]
        lists = ([r for r in fit if len(r) == width] + fit * nq)[:nq]
        for ids in (None, d_fids):
            tab = d_table if ids is not None else None
            w = ops.query_labeled_range(*args, d_labels, _dev(_padded(lists, width)), tab, ids, **kw)
            for pad in (None, EMPTY):
                w4 = ops.query_labeled_range(*args, d_labels, _dev(_padded(lists, 4, pad)), tab, ids, **kw)
                same(w, w4, ("n_ranges", width, pad, ids is not None))
            assert filled(w), width
    # the order of the intervals
    lists = (RANGES + pool)[:nq]
    fwd = ops.query_labeled_range(*args, d_labels, _dev(_padded(lists)), d_table, d_fids, **kw)
    rev = ops.query_labeled_range(*args, d_labels, _dev(_padded(lists)[:, ::-1].copy()), d_table, d_fids, **kw)
    same(fwd, rev, "order")
    assert filled(fwd)
    if variant != "f32":
        return
    # ... and under cosine: n_ranges 2 against four both ways, (MIN, MAX) against query_filtered_by.
    # Graph and nn1 statistics are those built for squared L2 on the unclamped base: sound only
    # because both sides of each comparison are GPU runs on the same inputs (cosine against the CPU
    # reference: tests/test_gpu_labelrange_layout_matrix.py)
    c_base, c_q = _cast(np.maximum(base, 1.0), variant), _cast(np.maximum(q, 1.0), variant)
    c_args = (c_base, c_q) + args[2:]
    c_kw = dict(kw, measure=1, prescreen=None)
    fit = [r for r in pool if len(r) <= 2]
    lists = ([r for r in fit if len(r) == 2] + fit * nq)[:nq]
    w = ops.query_labeled_range(*c_args, d_labels, _dev(_padded(lists, 2)), d_table, d_fids, **c_kw)
    for pad in (None, EMPTY):
        same(w, ops.query_labeled_range(*c_args, d_labels, _dev(_padded(lists, 4, pad)), d_table,
                                        d_fids, **c_kw), ("cosine", pad))
    assert filled(w)
    every = _dev(np.tile(np.array([MIN, MAX], np.int32), (nq, 1, 1)))
    same(ops.query_labeled_range(*c_args, d_labels, every, d_table, d_fids, **c_kw),
         ops.query_filtered_by(*c_args, d_table, d_fids, **c_kw), "cosine, (MIN, MAX)")


def test_seam_shard_offset(graphs):
    """second shard of two per GPU: labels and bits read at offset N of a column and a table over
    2 N ids, result columns and the -1 of empty slots offset as the unfiltered kernel writes them"""
    from ggnn_amd import ops
    g, base = graphs[24], graphs["base"]
    K, tau, iters = 10, 0.6, 200
    labels, table = _labels(g), _table()
    # this shard's labels and bits are the upper half; the lower half carries other values
    wide = np.concatenate([np.roll(labels, 17), labels])
    wide_table = np.concatenate([np.roll(table, 29, axis=1), table], axis=1)
    allowed = _composed(labels, RANGES, table, FIDS)
    nq = len(RANGES)
    q = np.random.default_rng(9).integers(0, 128, (nq, D)).astype(np.float32)
    d_base, d_q = _cast(base, "f32"), _cast(q, "f32")
    args = (d_base, d_q, g["d_graph"], g["d_start"], g["d_stats"], K, tau)
    ids, d = ops.query_labeled_range(*args, _dev(wide), _dev(_padded(RANGES)), _table_bits(wide_table),
                                     _dev(FIDS), iters, bit_offset=N, shards_per_gpu=2, on_gpu_shard=1)
    wide_allowed = np.concatenate([np.zeros_like(allowed), allowed], axis=1)
    t_ids, t_d = ops.query_filtered_by(*args, _table_bits(wide_allowed), _dev(np.arange(nq)), iters,
                                       filter_bit_offset=N, shards_per_gpu=2, on_gpu_shard=1)
    assert np.array_equal(ids.cpu().numpy()[:, K:], t_ids.cpu().numpy()[:, K:])
    assert d.cpu().numpy()[:, K:].tobytes() == t_d.cpu().numpy()[:, K:].tobytes()
    ids, d = ids.cpu().numpy()[:, K:], d.cpu().numpy()[:, K:]
    some_empty = some_found = False
    for i in range(nq):
        r = py_query_filtered(base, q[i], g["graph"], g["start"], g["stats"], K, tau, iters,
                              allowed[i])
        assert np.array_equal(ids[i], r[0] + N) and d[i].tobytes() == r[1].tobytes(), i
        some_found |= bool(np.isfinite(r[1]).any())
        if not allowed[i].any():
            some_empty = True
            assert (ids[i] == N - 1).all() and np.isinf(d[i]).all()
    assert some_empty and some_found


@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("variant", ["f32", "u8", "f16", "bf16"])
def test_seam_bf_query_labeled_range(orc, graphs, variant, measure):
    """k 10 (register list) and k 2100 (the LDS scan kernel), both above the size of the smallest
    classes, so slots are padded; N = 3000 is no multiple of 64; with and without filter ids, and
    once more through a window: labels and bits at offset 37 of a longer column and table"""
    from ggnn_amd import ops
    OFF = 37
    base = np.maximum(graphs["base"], 1.0)                # (no zero row: cosine)
    labels, table = _labels(graphs[24]), _table()
    nq = len(RANGES)
    q = np.maximum(np.random.default_rng(61 + measure).integers(0, 128, (nq, D)), 1)
    q = q.astype(np.float32)
    d_base, d_q = _cast(base, variant), _cast(q, variant)
    d_labels, d_ranges = _dev(labels), _dev(_padded(RANGES))
    rs = np.random.default_rng(8)
    wide = np.concatenate([rs.integers(-8, 4, OFF).astype(np.int32), labels,
                           rs.integers(-8, 4, 60).astype(np.int32)])
    wide_table = rs.random((3, OFF + N + 60)) < 0.5
    wide_table[:, OFF:OFF + N] = table
    for fids in (None, FIDS):
        allowed = _composed(labels, RANGES, table, fids)
        d_table, d_fids = (_table_bits(table), _dev(fids)) if fids is not None else (None, None)
        for K in (10, 2100):
            ids, d = ops.bf_query_labeled_range(d_base, d_q, K, d_labels, d_ranges, d_table, d_fids,
                                                measure)
            t_ids, t_d = ops.bf_query_filtered_by(d_base, d_q, K, _table_bits(allowed),
                                                  _dev(np.arange(nq)), measure)
            assert _torch().equal(ids, t_ids)
            assert d.cpu().numpy().tobytes() == t_d.cpu().numpy().tobytes()
            o_ids, o_d = ops.bf_query_labeled_range(
                d_base, d_q, K, _dev(wide), d_ranges,
                _table_bits(wide_table) if fids is not None else None, d_fids, measure, bit_offset=OFF)
            assert _torch().equal(ids, o_ids)
            assert d.cpu().numpy().tobytes() == o_d.cpu().numpy().tobytes()
            ids, d = ids.cpu().numpy(), d.cpu().numpy()
            for i in range(nq):
                r_ids, r_d = bf_filtered_reference(orc, base, q[i:i + 1], K, allowed[i], measure)
                assert np.array_equal(ids[i], r_ids[0]) and d[i].tobytes() == r_d[0].tobytes(), (K, i)
            filled = (ids >= 0).sum(1)
            assert np.array_equal(filled, np.minimum(allowed.sum(1), K))
            assert (filled == 0).any() and ((filled > 0) & (filled < K)).any()
            assert (filled == K).any() or allowed.sum(1).max() < K
            if fids is None:                              # six rows, then padding
                assert (ids[12, :6] >= 0).all() and (ids[12, 6:] == -1).all() and np.isinf(d[12, 6:]).all()
                ends = labels[ids[9, :min(K, 12)]].tolist()      # the twelve rows at the two ends
                assert set(ends) <= {MIN, MAX} and (ids[9, 12:] == -1).all()
                assert K < 12 or sorted(ends) == [MIN] * 6 + [MAX] * 6


# ---- the handle ----------------------------------------------------------------------------------
def test_handle_label_ranges():
    """two shards on one GPU; 26 queries with the interval lists and mixed filter ids through the
    blocking driver (also as two half-batches: DeviceFilter::from with first > 0), the exact search
    and two asynchronous slots, each query against query_filtered / bf_query_filtered of the same
    handle with the composed bitset"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    torch = _torch()
    Nb, Dh, K, tau, iters = 6000, 64, 10, 0.7, 200
    base = np.random.default_rng(187).integers(0, 256, (Nb, Dh)).astype(np.float32)
    lists = RANGES + RANGES[::-1]
    lists = [[(3, 3) if p == (STARTS, STARTS) else p for p in r] for r in lists]
    nq = len(lists)
    q = np.random.default_rng(188).integers(0, 256, (nq, Dh)).astype(np.float32)
    labels = _labels(None, Nb, seed=6)
    table = _table(Nb)
    fids = np.random.default_rng(5).integers(-1, 3, nq).astype(np.int32)
    fids[:4] = [-1, 0, 1, 2]
    p4 = _padded(lists)
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_labels(labels)
    eng.set_filters(table)
    eng.set_shard_size(Nb // 2)
    eng.build(24, 0.5, 1)

    def expect(labels, f, bf=False, k=K):
        """every query on its own: the per-call filtered search with the composed bitset"""
        allowed = _composed(labels, lists, table, f)
        out = [eng.bf_query_filtered(q[i:i + 1], k, filter=allowed[i]) if bf else
               eng.query_filtered(q[i:i + 1], K, tau, iters, filter=allowed[i]) for i in range(nq)]
        return (np.concatenate([o[0].numpy() for o in out]), np.concatenate([o[1].numpy() for o in out]))

    def check_all(labels, what):
        want, want_l = expect(labels, fids), expect(labels, None)
        filled = np.isfinite(want_l[1]).sum(1)
        assert (filled == 0).any() and (filled == K).any(), what
        # ragged lists and ids on the host
        _same(eng.query_labeled_range(q, K, tau, iters, label_ranges=lists, filter_ids=fids), want,
              (what, "ragged"))
        # as two half-batches
        with _lib.hooks(EXCHANGE=1, QUERY_SPLIT=1):
            r = eng.query_labeled_range(q, K, tau, iters, label_ranges=lists, filter_ids=fids)
            assert eng.last_query_parts() == 2
            _same(r, want, (what, "half-batches"))
            _same(eng.query_labeled_range(q, K, tau, iters, label_ranges=torch.from_numpy(p4).cuda(),
                                          filter_ids=torch.from_numpy(fids).cuda()), want,
                  (what, "half-batches, device"))
        # 3-D, int64 and device forms; ids on the host and on the device
        for form in (p4, p4.astype(np.int64), torch.from_numpy(p4), torch.from_numpy(p4).cuda()):
            _same(eng.query_labeled_range(q, K, tau, iters, label_ranges=form,
                                          filter_ids=torch.from_numpy(fids).cuda()), want, what)
        _same(eng.query_labeled_range(q, K, tau, iters, label_ranges=torch.from_numpy(p4).cuda(),
                                      filter_ids=fids), want, (what, "device ranges, host ids"))
        _same(eng.query_labeled_range(q, K, tau, iters, label_ranges=lists), want_l, (what, "no ids"))
        # results on the GPU: the sorted [Nq, K * shards] rows
        eng.set_return_results_on_gpu(True)
        ids_g, d_g = eng.query_labeled_range(torch.from_numpy(q).cuda(), K, tau, iters,
                                             label_ranges=lists, filter_ids=fids)
        eng.set_return_results_on_gpu(False)
        assert ids_g.is_cuda and tuple(ids_g.shape) == (nq, 2 * K)
        _same((ids_g[:, :K], d_g[:, :K]), want, (what, "results on the GPU"))
        # two asynchronous slots in flight
        qd = torch.from_numpy(q).cuda()
        t0 = eng.query_async_labeled_range(qd, K, tau, iters, slot=0,
                                           label_ranges=torch.from_numpy(p4).cuda(),
                                           filter_ids=torch.from_numpy(fids).cuda())
        t1 = eng.query_async_labeled_range(qd, K, tau, iters, slot=1, label_ranges=lists)
        assert t0.label_ranges is not None and t0.filter_ids is not None and t1.filter_ids is None
        eng.synchronize()
        _same((t0.ids[:, :K], t0.dists[:, :K]), want, (what, "async"))
        _same((t1.ids[:, :K], t1.dists[:, :K]), want_l, (what, "async, no ids"))
        # the exact search: always the scan
        for f in (fids, None):
            b = eng.bf_query_labeled_range(q, 100, label_ranges=lists, filter_ids=f)
            assert eng.last_bf_query_matrix_path() == 0
            _same(b, expect(labels, f, bf=True, k=100), (what, "bf"))
        _same(eng.bf_query_labeled_range(q, 100, label_ranges=torch.from_numpy(p4).cuda()), b,
              (what, "bf, device"))
        return want_l

    first = check_all(labels, "as set")
    # counters equal to those of the composed table
    eng.set_collect_counters(True)
    eng.query_labeled_range(q, K, tau, iters, label_ranges=lists, filter_ids=fids)
    c = eng.last_query_counters()
    eng.set_filters(_composed(labels, lists, table, fids))
    eng.query_filtered_by(q, K, tau, iters, filter_ids=np.arange(nq, dtype=np.int32))
    c_table = eng.last_query_counters()
    eng.set_filters(table)
    eng.set_collect_counters(False)
    assert (c["n_dist"], c["n_pop"]) == (c_table["n_dist"], c_table["n_pop"]) and c["n_pop"] > 0
    # both arguments None: the unfiltered call; ranges None: query_filtered_by
    _same(eng.query_labeled_range(q, K, tau, iters), eng.query(q, K, tau, iters), "both None")
    _same(eng.bf_query_labeled_range(q, 20), eng.bf_query(q, 20), "bf, both None")
    _same(eng.query_labeled_range(q, K, tau, iters, filter_ids=fids),
          eng.query_filtered_by(q, K, tau, iters, filter_ids=fids), "ranges None")
    with pytest.raises(_lib.GGNNError) as e:
        eng.query_labeled_range(q, K, tau, iters, label_ranges=lists, filter_ids=np.full(nq, 3))
    assert e.value.status == _lib.INVALID_ARGUMENT
    with pytest.raises(ValueError):
        eng.query_labeled_range(q, K, tau, iters, label_ranges=np.zeros((nq, 5, 2), np.int32))

    # update_labels moves rows into and out of the ranges: class 1 leaves (1, 1) for 2, and rows of
    # class 0 enter (MAX, MAX)
    labels2 = labels.copy()
    moved = np.nonzero(labels == 1)[0][::2]
    entered = np.nonzero(labels == 0)[0][::3]
    labels2[moved], labels2[entered] = 2, MAX
    rows = np.concatenate([moved, entered])
    eng.update_labels(rows, labels2[rows])
    second = check_all(labels2, "relabelled")
    assert not np.array_equal(first[0], second[0])
    assert not np.array_equal(first[0][12], second[0][12])    # [(MAX, MAX)]

    # ids without a table, then no labels
    eng.set_filters(None)
    with pytest.raises(_lib.GGNNError) as e:
        eng.query_labeled_range(q, K, tau, iters, label_ranges=lists, filter_ids=fids)
    assert e.value.status == _lib.INVALID_STATE
    eng.set_labels(None)
    for call in (lambda: eng.query_labeled_range(q, K, tau, iters, label_ranges=lists),
                 lambda: eng.bf_query_labeled_range(q, K, label_ranges=lists),
                 lambda: eng.query_async_labeled_range(torch.from_numpy(q).cuda(), K, tau, iters,
                                                       label_ranges=lists)):
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
    lists = [[(0, 1)]] * 8
    with pytest.raises(_lib.GGNNError) as e:
        eng.bf_query_labeled_range(q, 10, label_ranges=lists)
    assert e.value.status == _lib.UNSUPPORTED
