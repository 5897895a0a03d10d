"""GPU tests of the label-mask filters: the int32 label read as 32 tag bits, one or two clauses
(mask, value, any) per query, combined with a filter id into the resident filter table
(ggnn_*_labeled_mask and their operators).  The contract is one sentence -- query n is the per-call
filtered search of that query with the bitset
    any_j(((labels & mask_j) == value_j) & ((any_j == 0) | ((labels & any_j) != 0))) & row(filter_ids[n])
-- and every comparison here is bit for bit: array_equal on ids, tobytes() on distances, equal
counters.  Base, graphs and classes are those of tests/test_gpu_labels.py.

To stay at seconds per test the reference is the EXISTING GPU entry point ops.query_filtered_by /
ops.bf_query_filtered_by on a filter table built from the composed masks on the CPU: those kernels
are pinned to the CPU reference by their own suites.  One small case goes through py_query_filtered,
one through bf_filtered_reference."""
import numpy as np
import pytest

from filtered_reference import bf_filtered_reference, py_query_filtered
from test_gpu_labels import (D, N, SEAM_CASES, STARTS, VARIANTS, _base_labels, _cast, _dev, _same,
                             _table_bits, _torch, graphs)  # noqa: F401  (graphs: the module fixture)

pytestmark = pytest.mark.gpu

# one bit per class of _base_labels, three independent random tags, a three-bit tenant field and
# bit 31
C0, C1, C2, C3, CREST, CSTART = (1 << b for b in range(6))
R8, R9, R10 = 1 << 8, 1 << 9, 1 << 10
FIELD_SHIFT, FIELD = 16, 7 << 16
B31 = 0x80000000
CLASS_BIT = {0: C0, 1: C1, 2: C2, 3: C3, -7: CREST, STARTS: CSTART}


def _parts(g, n=N, seed=3):
    """what the tag column is made of, each on its own: the class of every row, the three random
    tags (share 0.3), the tenant 0..7, the six bit-31 rows (of the rest class) and the five rows
    whose label is 0 altogether (of class 0)"""
    cls = _base_labels(g, n, seed)
    rs = np.random.default_rng(seed + 100)
    tags = rs.random((3, n)) < 0.3
    tenant = rs.integers(0, 8, n)
    rest, zero_of = np.nonzero(cls == -7)[0], np.nonzero(cls == 0)[0]
    assert len(rest) > 24 and len(zero_of) > 24
    b31 = np.zeros(n, bool)
    b31[rest[:6]] = True
    zero = np.zeros(n, bool)
    zero[zero_of[:5]] = True
    return dict(cls=cls, tags=tags, tenant=tenant, b31=b31, zero=zero)


def _labels(g, n=N, seed=3):
    """the int32 tag column of _parts"""
    p = _parts(g, n, seed)
    lab = np.zeros(n, np.int64)
    for c, bit in CLASS_BIT.items():
        lab[p["cls"] == c] |= bit
    for t, bit in zip(p["tags"], (R8, R9, R10)):
        lab[t] |= bit
    lab |= p["tenant"].astype(np.int64) << FIELD_SHIFT
    lab[p["b31"]] |= B31
    lab[p["zero"]] = 0
    return lab.astype(np.uint32).view(np.int32)


# one clause list per query, values written as they read (0x80000000 is bit 31)
MASKS = [
    [(0, 0, 0)],                                   # 0  every row
    [(C1 | R8, C1 | R8, 0)],                       # 1  all of: class 1 and tag 8
    [(C0 | R9, 0, 0)],                             # 2  none of: not class 0, not tag 9
    [(0, 0, B31 | C3)],                            # 3  any of, bit 31 among them; mask 0
    [(FIELD, 5 << FIELD_SHIFT, 0)],                # 4  field equality: tenant 5
    [(B31, B31, 0)],                               # 5  exactly the six bit-31 rows
    [(C0 | C1, C0 | C1, 0)],                       # 6  no row is in two classes
    [(C1, C1 | R8, 0)],                            # 7  value has a bit outside mask: nothing
    [(C0, C0, 0), (R8, R8, 0)],                    # 8  two clauses that overlap
    [(C2, C2, R9 | R10), (C0 | C1, C0 | C1, 0)],   # 9  the second clause is unsatisfiable
    [(0, 0, R10)],                                 # 10 any non-zero with mask 0
    [(C1 | R8, C1, R9 | B31)],                     # 11 all of A, none of B, any of C
    [(0xffffffff, 0, 0)],                          # 12 the label is 0: five rows
]
FIDS = np.array(([-1, 0, 1, 2, 99] * 3)[:len(MASKS)], np.int32)


def _wrap(v):
    return v - (1 << 32) if v >= (1 << 31) else v


def _padded(lists, width=2):
    """[Nq, width, 3] int32: every list padded by repeating its first clause"""
    assert all(1 <= len(r) <= width for r in lists)
    return np.array([[[_wrap(v) for v in c] for c in list(r) + [r[0]] * (width - len(r))]
                     for r in lists], np.int32).reshape(len(lists), width, 3)


def _table(n=N, seed=56):
    """three rows: about 50 % random, about 5 % random, every id but every seventh"""
    u = np.random.default_rng(seed).random((2, n))
    return np.stack([u[0] < 0.5, u[1] < 0.05, np.arange(n) % 7 != 0])


def _passes(labels, clauses):
    """the definition, in bool / int64 numpy, independent of the engine"""
    lab = labels.astype(np.int64) & 0xffffffff
    out = np.zeros(len(lab), bool)
    for mask, value, any_ in clauses:
        mask, value, any_ = (int(v) & 0xffffffff for v in (mask, value, any_))
        out |= ((lab & mask) == value) & ((any_ == 0) | ((lab & any_) != 0))
    return out


def _row(table, f):
    if f == -1:
        return np.ones(table.shape[1], bool)
    return table[f] if 0 <= f < len(table) else np.zeros(table.shape[1], bool)


def _composed(labels, lists, table=None, fids=None):
    """the whole contract: one allowed array per query"""
    return np.stack([_passes(labels, r) & (_row(table, int(fids[i])) if fids is not None else True)
                     for i, r in enumerate(lists)])


def test_the_clause_lists_select_what_they_are_meant_to(graphs):
    g = graphs[24]
    labels, p = _labels(g), _parts(graphs[24])
    assert labels.dtype == np.int32 and (labels < 0).sum() == 6 and (labels == 0).sum() == 5
    counts = _composed(labels, MASKS).sum(1).tolist()
    print("admitted rows per list:", counts)
    # class arithmetic on the parts, never on the packed word
    live = ~p["zero"]
    cls = {c: (p["cls"] == c) & live for c in CLASS_BIT}
    t8, t9, t10 = (t & live for t in p["tags"])
    b31 = p["b31"] & live
    assert sum(int(c.sum()) for c in cls.values()) == N - 5 and b31.sum() == 6
    assert all(0.25 < t.mean() < 0.35 for t in p["tags"])
    several = np.array([bin(int(v) & 0xffffffff).count("1") for v in labels])
    assert (several >= 3).mean() > 0.5                     # most rows carry several tags
    want = [N, (cls[1] & t8).sum(), (~cls[0] & ~t9).sum(), (cls[3] | b31).sum(),
            ((p["tenant"] == 5) & live).sum(), 6, 0, 0, (cls[0] | t8).sum(),
            (cls[2] & (t9 | t10)).sum(), t10.sum(), (cls[1] & ~t8 & (t9 | b31)).sum(), 5]
    assert counts == [int(w) for w in want]
    assert all(c > 0 for i, c in enumerate(counts) if i not in (6, 7))
    # the clause whose value has a bit outside its mask admits nothing; with value pre-masked it would
    # admit class 1
    mask, value, any_ = MASKS[7][0]
    assert value & ~mask and counts[7] == 0
    premasked = int(_passes(labels, [(mask, value & mask, any_)]).sum())
    assert premasked == int(cls[1].sum()) and premasked > 0
    # the two overlapping clauses do overlap, and each alone is narrower than their union
    a, b = (_passes(labels, [c]) for c in MASKS[8])
    assert (a & b).any() and a.sum() < counts[8] > b.sum()
    assert not _passes(labels, MASKS[9][1:]).any() and _passes(labels, MASKS[9][:1]).any()


@pytest.mark.parametrize("KB,K,iters", SEAM_CASES, ids=[f"kb{c[0]}-k{c[1]}-it{c[2]}" for c in SEAM_CASES])
def test_seam_query_labeled_mask(graphs, KB, K, iters):
    """every kernel form and element type, two clauses, without filter ids and with them, against
    the filter table of the composed masks (ops.query_filtered_by), with counters.

    Not vacuous, asserted on the reference's output: the rows of the queries hold an empty one, a
    partly filled one and -- wherever a search can fill a row at all -- a full one.  A search visits
    at most num_start + iters * KBuild points, which for K 2100 at 64 iterations of a KBuild 24 graph
    is below K: that case can have no full row, and asks for one with more than K / 4 entries
    instead."""
    from ggnn_amd import ops
    g, base = graphs[KB], graphs["base"]
    tau = 0.6
    labels, table = _labels(g), _table()
    assert 0.45 < table[0].mean() < 0.55 and 0.03 < table[1].mean() < 0.07
    nq = len(MASKS)
    q = np.random.default_rng(K + iters).integers(0, 128, (nq, D)).astype(np.float32)
    d_labels, d_masks = _dev(labels), _dev(_padded(MASKS))
    c_fids = _dev(np.arange(nq))
    for variant in VARIANTS:
        d_base, d_q = _cast(base, variant), _cast(q, variant)
        ps = ops.prescreen_encode(d_base, 0) if variant == "f32_ps" else None
        common = (g["d_graph"], g["d_start"], g["d_stats"], K, tau)
        fills = []
        for fids in (None, FIDS):
            what = (variant, fids is not None)
            allowed = _composed(labels, MASKS, table, fids)
            t_ids, t_d, t_nd, t_pop = [x.cpu().numpy() for x in ops.query_filtered_by(
                d_base, d_q, *common, _table_bits(allowed), c_fids, iters, counters=True,
                prescreen=ps)]
            filled = np.isfinite(t_d).sum(1)
            print(what, "finite entries per query:", filled.tolist())
            assert (filled == 0).any() and ((filled > 0) & (filled < K)).any(), what
            fills.append(filled)
            d_table, d_fids = (_table_bits(table), _dev(fids)) if fids is not None else (None, None)
            ids, d, nd, npop = [x.cpu().numpy() for x in ops.query_labeled_mask(
                d_base, d_q, *common, d_labels, d_masks, d_table, d_fids, iters, counters=True,
                prescreen=ps)]
            assert np.array_equal(ids, t_ids), what
            assert d.tobytes() == t_d.tobytes(), what
            assert np.array_equal(nd, t_nd) and np.array_equal(npop, t_pop), what
            assert (npop > 0).all(), what
            empty = ~allowed.any(1)
            assert empty.any(), what
            assert (ids[empty] == -1).all() and np.isinf(d[empty]).all() and (d[empty] > 0).all()
        filled = np.concatenate(fills)
        if K <= len(g["start"]) + iters * KB:
            assert (filled == K).any(), variant
        else:
            assert (filled > K // 4).any(), variant


def test_seam_against_the_cpu_reference(graphs):
    """the one case that goes through py_query_filtered directly: (KB 24, K 10, 200 iterations),
    float32, with filter ids, every query on its own"""
    from ggnn_amd import ops
    g, base = graphs[24], graphs["base"]
    K, tau, iters = 10, 0.6, 200
    labels, table = _labels(g), _table()
    allowed = _composed(labels, MASKS, table, FIDS)
    nq = len(MASKS)
    q = np.random.default_rng(K + iters).integers(0, 128, (nq, D)).astype(np.float32)
    ids, d, nd, npop = [x.cpu().numpy() for x in ops.query_labeled_mask(
        _cast(base, "f32"), _cast(q, "f32"), g["d_graph"], g["d_start"], g["d_stats"], K, tau,
        _dev(labels), _dev(_padded(MASKS)), _table_bits(table), _dev(FIDS), iters, counters=True)]
    filled = []
    for i in range(nq):
        r = py_query_filtered(base, q[i], g["graph"], g["start"], g["stats"], K, tau, iters, allowed[i])
        assert np.array_equal(ids[i], r[0]) and d[i].tobytes() == r[1].tobytes(), i
        assert (nd[i], npop[i]) == (r[2], r[3]), i
        filled.append(int(np.isfinite(r[1]).sum()))
    print("finite entries per query:", filled)
    assert 0 in filled and K in filled and any(0 < f < K for f in filled)


@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("variant", ["f32", "u8", "f16", "bf16"])
def test_seam_bf_query_labeled_mask(orc, graphs, variant, measure):
    """k 10 (register list) and k 300 (the LDS scan kernel), both above the size of the smallest
    selections, so slots are padded; N = 3000 is no multiple of 64; with and without filter ids,
    against ops.bf_query_filtered_by on the composed table; the float32 squared-L2 case with ids at
    k 10 also against bf_filtered_reference"""
    from ggnn_amd import ops
    base = np.maximum(graphs["base"], 1.0)                # (no zero row: cosine)
    labels, table = _labels(graphs[24]), _table()
    nq = len(MASKS)
    q = np.maximum(np.random.default_rng(61 + measure).integers(0, 128, (nq, D)), 1)
    q = q.astype(np.float32)
    d_base, d_q = _cast(base, variant), _cast(q, variant)
    d_labels, d_masks = _dev(labels), _dev(_padded(MASKS))
    for fids in (None, FIDS):
        allowed = _composed(labels, MASKS, table, fids)
        d_table, d_fids = (_table_bits(table), _dev(fids)) if fids is not None else (None, None)
        for K in (10, 300):
            ids, d = ops.bf_query_labeled_mask(d_base, d_q, K, d_labels, d_masks, d_table, d_fids,
                                               measure)
            t_ids, t_d = ops.bf_query_filtered_by(d_base, d_q, K, _table_bits(allowed),
                                                  _dev(np.arange(nq)), measure)
            assert _torch().equal(ids, t_ids), (K, fids is not None)
            assert d.cpu().numpy().tobytes() == t_d.cpu().numpy().tobytes(), (K, fids is not None)
            ids, d = ids.cpu().numpy(), d.cpu().numpy()
            filled = (ids >= 0).sum(1)
            assert np.array_equal(filled, np.minimum(allowed.sum(1), K))
            assert (filled == 0).any() and ((filled > 0) & (filled < K)).any() and (filled == K).any()
            if fids is None:                              # six rows with bit 31, then padding
                assert (ids[5, :6] >= 0).all() and (ids[5, 6:] == -1).all() and np.isinf(d[5, 6:]).all()
                assert (labels[ids[5, :6]] < 0).all()
                assert (labels[ids[12, :5]] == 0).all() and (ids[12, 5:] == -1).all()
            if K == 10 and fids is not None and variant == "f32" and measure == 0:
                for i in range(nq):
                    r_ids, r_d = bf_filtered_reference(orc, base, q[i:i + 1], K, allowed[i], measure)
                    assert np.array_equal(ids[i], r_ids[0]) and d[i].tobytes() == r_d[0].tobytes(), i


def test_seam_shard_offset(graphs):
    """second shard of two per GPU: labels and bits read at offset N of a column and a table over
    2 N ids, result columns and the -1 of empty slots offset as the unfiltered kernel writes them;
    the scan through the same window"""
    from ggnn_amd import ops
    g, base = graphs[24], graphs["base"]
    K, tau, iters = 10, 0.6, 200
    labels, table = _labels(g), _table()
    # this shard's labels and bits are the upper half; the lower half carries other values
    wide = np.concatenate([np.roll(labels, 17), labels])
    wide_table = np.concatenate([np.roll(table, 29, axis=1), table], axis=1)
    allowed = _composed(labels, MASKS, table, FIDS)
    assert not np.array_equal(_composed(np.roll(labels, 17), MASKS, np.roll(table, 29, axis=1), FIDS),
                              allowed)
    nq = len(MASKS)
    q = np.random.default_rng(9).integers(0, 128, (nq, D)).astype(np.float32)
    d_base, d_q = _cast(base, "f32"), _cast(q, "f32")
    args = (d_base, d_q, g["d_graph"], g["d_start"], g["d_stats"], K, tau)
    ids, d, nd, npop = ops.query_labeled_mask(*args, _dev(wide), _dev(_padded(MASKS)),
                                              _table_bits(wide_table), _dev(FIDS), iters, bit_offset=N,
                                              shards_per_gpu=2, on_gpu_shard=1, counters=True)
    wide_allowed = np.concatenate([np.zeros_like(allowed), allowed], axis=1)
    t_ids, t_d, t_nd, t_pop = ops.query_filtered_by(*args, _table_bits(wide_allowed),
                                                    _dev(np.arange(nq)), iters, filter_bit_offset=N,
                                                    shards_per_gpu=2, on_gpu_shard=1, counters=True)
    assert np.array_equal(ids.cpu().numpy()[:, K:], t_ids.cpu().numpy()[:, K:])
    assert d.cpu().numpy()[:, K:].tobytes() == t_d.cpu().numpy()[:, K:].tobytes()
    assert _torch().equal(nd, t_nd) and _torch().equal(npop, t_pop)
    ids, d = ids.cpu().numpy()[:, K:], d.cpu().numpy()[:, K:]
    # ... which is the search of the shard alone, ids moved by N
    a_ids, a_d = ops.query_filtered_by(*args, _table_bits(allowed), _dev(np.arange(nq)), iters)
    a_ids, a_d = a_ids.cpu().numpy(), a_d.cpu().numpy()
    assert np.array_equal(ids, a_ids + N) and d.tobytes() == a_d.tobytes()
    empty = ~allowed.any(1)
    assert empty.any() and np.isfinite(d[~empty]).any()
    assert (ids[empty] == N - 1).all() and np.isinf(d[empty]).all()
    assert ((ids[~empty] >= N) | (ids[~empty] == N - 1)).all()
    # the scan at the same offset
    b_ids, b_d = ops.bf_query_labeled_mask(d_base, d_q, K, _dev(wide), _dev(_padded(MASKS)),
                                           _table_bits(wide_table), _dev(FIDS), bit_offset=N)
    s_ids, s_d = ops.bf_query_filtered_by(d_base, d_q, K, _table_bits(allowed), _dev(np.arange(nq)))
    assert _torch().equal(b_ids, s_ids) and b_d.cpu().numpy().tobytes() == s_d.cpu().numpy().tobytes()


def test_seam_one_clause_is_the_clause_repeated(graphs):
    """n_masks 1 reads clause 0 of a query at [n * 3]; it equals the same clause given twice, and
    the order of two clauses does not matter"""
    from ggnn_amd import ops
    g, base = graphs[24], graphs["base"]
    K, tau, iters = 10, 0.6, 400
    labels, table = _labels(g), _table()
    ones = [r for r in MASKS if len(r) == 1]
    nq = len(ones)
    q = np.random.default_rng(5).integers(0, 128, (nq, D)).astype(np.float32)
    args = (_cast(base, "f32"), _cast(q, "f32"), g["d_graph"], g["d_start"], g["d_stats"], K, tau)
    tail = (_table_bits(table), _dev(FIDS[:nq]), iters)
    one = ops.query_labeled_mask(*args, _dev(labels), _dev(_padded(ones, 1)), *tail, counters=True)
    two = ops.query_labeled_mask(*args, _dev(labels), _dev(_padded(ones, 2)), *tail, counters=True)
    for x, y in zip(one, two):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert np.isfinite(one[1].cpu().numpy()).any()
    both = (MASKS * 2)[:nq]
    fwd = ops.query_labeled_mask(*args, _dev(labels), _dev(_padded(both)), *tail, counters=True)
    rev = ops.query_labeled_mask(*args, _dev(labels), _dev(_padded(both)[:, ::-1].copy()), *tail,
                                 counters=True)
    for x, y in zip(fwd, rev):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ---- the handle ----------------------------------------------------------------------------------
def test_handle_label_masks():
    """two shards on one GPU; the clause lists with mixed filter ids through the blocking driver, the
    exact search and the asynchronous call, each query against query_filtered / bf_query_filtered of
    the same handle with the composed bitset (the merged result of both shards); update_labels;
    label_masks=None"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    torch = _torch()
    Nb, Dh, K, tau, iters = 6000, 64, 10, 0.7, 200
    base = np.random.default_rng(187).integers(0, 256, (Nb, Dh)).astype(np.float32)
    lists = MASKS
    nq = len(lists)
    q = np.random.default_rng(188).integers(0, 256, (nq, Dh)).astype(np.float32)
    labels = _labels(None, Nb, seed=6)
    table = _table(Nb)
    fids = FIDS.copy()
    fids[fids == 99] = -1                                  # (host ids outside the table are refused)
    p2 = _padded(lists)
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
        assert (want_l[0] >= Nb // 2).any() and ((want_l[0] >= 0) & (want_l[0] < Nb // 2)).any()
        # ragged lists written as they read, and ids on the host
        _same(eng.query_labeled_mask(q, K, tau, iters, label_masks=lists, filter_ids=fids), want,
              (what, "ragged"))
        # 3-D, int64 and device forms; ids on the device
        for form in (p2, p2.astype(np.int64) & 0xffffffff, torch.from_numpy(p2),
                     torch.from_numpy(p2).cuda()):
            _same(eng.query_labeled_mask(q, K, tau, iters, label_masks=form,
                                         filter_ids=torch.from_numpy(fids).cuda()), want, what)
        _same(eng.query_labeled_mask(q, K, tau, iters, label_masks=lists), want_l, (what, "no ids"))
        # [Nq, 3]: one clause per query
        first = np.ascontiguousarray(p2[:, 0])
        one = eng.query_labeled_mask(q, K, tau, iters, label_masks=first)
        _same(one, eng.query_labeled_mask(q, K, tau, iters, label_masks=[r[:1] for r in lists]),
              (what, "[Nq, 3]"))
        # the asynchronous call, two slots in flight
        qd = torch.from_numpy(q).cuda()
        t0 = eng.query_async_labeled_mask(qd, K, tau, iters, slot=0,
                                          label_masks=torch.from_numpy(p2).cuda(),
                                          filter_ids=torch.from_numpy(fids).cuda())
        t1 = eng.query_async_labeled_mask(qd, K, tau, iters, slot=1, label_masks=lists)
        assert t0.label_masks is not None and t0.filter_ids is not None and t1.filter_ids is None
        eng.synchronize()
        _same((t0.ids[:, :K], t0.dists[:, :K]), want, (what, "async"))
        _same((t1.ids[:, :K], t1.dists[:, :K]), want_l, (what, "async, no ids"))
        # the exact search: always the scan
        for f in (fids, None):
            b = eng.bf_query_labeled_mask(q, 100, label_masks=lists, filter_ids=f)
            assert eng.last_bf_query_matrix_path() == 0
            _same(b, expect(labels, f, bf=True, k=100), (what, "bf"))
        return want_l

    first = check_all(labels, "as set")
    # both arguments None: the unfiltered call; masks None: query_filtered_by
    _same(eng.query_labeled_mask(q, K, tau, iters), eng.query(q, K, tau, iters), "both None")
    _same(eng.bf_query_labeled_mask(q, 20), eng.bf_query(q, 20), "bf, both None")
    _same(eng.query_labeled_mask(q, K, tau, iters, filter_ids=fids),
          eng.query_filtered_by(q, K, tau, iters, filter_ids=fids), "masks None")
    t = eng.query_async_labeled_mask(torch.from_numpy(q).cuda(), K, tau, iters)
    eng.synchronize()
    assert t.label_masks is None
    _same((t.ids[:, :K], t.dists[:, :K]), eng.query(q, K, tau, iters), "async, both None")
    with pytest.raises(_lib.GGNNError) as e:
        eng.query_labeled_mask(q, K, tau, iters, label_masks=lists, filter_ids=np.full(nq, 3))
    assert e.value.status == _lib.INVALID_ARGUMENT
    with pytest.raises(ValueError):
        eng.query_labeled_mask(q, K, tau, iters, label_masks=np.zeros((nq, 3, 3), np.int32))

    # update_labels grants and revokes tags: every other bit-31... rows of class 1 lose their class
    # bit for class 2's, and a few rows of class 0 gain bit 31
    labels2 = labels.copy()
    moved = np.nonzero((labels & C1) != 0)[0][::2]
    granted = np.nonzero((labels & C0) != 0)[0][::3]
    labels2[moved] = (labels2[moved] & ~np.int32(C1)) | np.int32(C2)
    labels2[granted] |= np.int32(-2 ** 31)
    rows = np.concatenate([moved, granted])
    eng.update_labels(rows, labels2[rows])
    second = check_all(labels2, "relabelled")
    assert not np.array_equal(first[0], second[0])
    assert not np.array_equal(first[0][5], second[0][5])      # [(B31, B31, 0)]
    assert np.isfinite(second[1][5]).sum() == K > np.isfinite(first[1][5]).sum() > 0

    # ids without a table, then no labels
    eng.set_filters(None)
    with pytest.raises(_lib.GGNNError) as e:
        eng.query_labeled_mask(q, K, tau, iters, label_masks=lists, filter_ids=fids)
    assert e.value.status == _lib.INVALID_STATE
    eng.set_labels(None)
    for call in (lambda: eng.query_labeled_mask(q, K, tau, iters, label_masks=lists),
                 lambda: eng.bf_query_labeled_mask(q, K, label_masks=lists),
                 lambda: eng.query_async_labeled_mask(torch.from_numpy(q).cuda(), K, tau, iters,
                                                      label_masks=lists)):
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
    lists = [[(3, 1, 0)]] * 8
    for call in (lambda: eng.bf_query_labeled_mask(q, 10, label_masks=lists),
                 lambda: eng.query_labeled_mask(q, 10, 0.5, label_masks=lists)):
        with pytest.raises(_lib.GGNNError, match="int8") as e:
            call()
        assert e.value.status == _lib.UNSUPPORTED
