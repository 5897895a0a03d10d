"""GPU tests of the per-query filters: a filter table and one filter id per query
(ggnn_set_filters / ggnn_*_filtered_by and their operators).  The contract is one sentence --
query n with id f is the per-call filtered search of that query with row f, id -1 the unfiltered
search, any other id an empty result -- and every comparison here is bit for bit: array_equal on
ids, tobytes() on distances, equal counters.  Integer-valued data (values 0..127: exact in every
dtype) as in tests/test_gpu_filtered.py."""
import numpy as np
import pytest

from filtered_reference import bf_filtered_reference, pack_bits, py_query_filtered

pytestmark = pytest.mark.gpu

N, D = 3000, 32
VARIANTS = ["f32", "f32_ps", "u8", "f16", "bf16"]
TABLE = ["100", "50", "10", "1", "0", "starts"]          # F = 6
INVALID = 6 + 3                                          # names no row (direct seam calls only)


def _torch():
    import torch
    return torch


def _cast(a, variant):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a))
    kind = variant.split("_")[0]
    t = {"f32": t.float(), "u8": t.to(torch.uint8), "f16": t.to(torch.float16),
         "bf16": t.to(torch.bfloat16)}[kind]
    return t.contiguous().cuda()


def _table_bits(masks):
    words = np.stack([pack_bits(m) for m in masks]).view(np.int32)
    return _torch().from_numpy(np.ascontiguousarray(words)).cuda()


@pytest.fixture(scope="module")
def graphs(orc):
    """the 3000 x 32 integer base with a KBuild = 24 and a KBuild = 40 graph of the oracle,
    uploaded once (as tests/test_gpu_filtered.py builds them)"""
    torch = _torch()
    base = np.random.default_rng(77).integers(0, 128, (N, D)).astype(np.float32)
    out = {"base": base}
    for KB in (24, 40):
        cfg, graph, tr, sel, stats = orc.build(base, KB, 0.5, 1, rng=orc.make_rng(N, 5))
        start = np.ascontiguousarray(tr[cfg.STs_offsets[3]:cfg.STs_offsets[3] + cfg.Ns[3]])
        g0 = np.ascontiguousarray(graph[:N])
        out[KB] = dict(graph=g0, start=start, stats=stats,
                       d_graph=torch.from_numpy(g0).cuda(), d_start=torch.from_numpy(start).cuda(),
                       d_stats=torch.from_numpy(np.asarray(stats, np.float32)).cuda())
    return out


def _table(g):
    rs = np.random.default_rng(3)
    rows = []
    for name in TABLE:
        if name == "starts":
            m = np.ones(N, bool)
            m[g["start"]] = False
        else:
            m = rs.random(N) < float(name) / 100.0 if float(name) < 100 else np.ones(N, bool)
        rows.append(m)
    return np.stack(rows)


def _allowed_of(table, f):
    """the whole contract: row f, all ones for -1, all zeros for anything else"""
    return table[f] if 0 <= f < len(table) else np.full(table.shape[1], f == -1)


# every kernel form, from CASES of tests/test_gpu_filtered.py: early rows (K 10 / 400 iterations),
# the ring scan (2048 iterations), R > 1 (K 300), the LDS list (K 2100), the non-early order of a
# KBuild = 40 graph
SEAM_CASES = [(24, 10, 400), (24, 10, 2048), (24, 300, 1000), (24, 2100, 64), (40, 10, 400)]


@pytest.mark.parametrize("KB,K,iters", SEAM_CASES, ids=[f"kb{c[0]}-k{c[1]}-it{c[2]}" for c in SEAM_CASES])
def test_seam_query_filtered_by(graphs, KB, K, iters):
    from ggnn_amd import ops
    torch = _torch()
    g, base = graphs[KB], graphs["base"]
    tau = 0.6
    table = _table(g)
    F = len(table)
    # every row, -1 and one invalid value, not grouped
    fids = np.array([2, -1, 0, INVALID, 5, 1, 3, 4], np.int32)
    nq = len(fids)
    q = np.random.default_rng(K + iters).integers(0, 128, (nq, D)).astype(np.float32)
    ref = [py_query_filtered(base, q[i], g["graph"], g["start"], g["stats"], K, tau, iters,
                             _allowed_of(table, int(fids[i]))) for i in range(nq)]
    r_ids = np.stack([r[0] for r in ref])
    r_d = np.stack([r[1] for r in ref])
    r_nd = np.array([r[2] for r in ref])
    r_pop = np.array([r[3] for r in ref])
    bad = np.nonzero(fids == INVALID)[0]
    assert (r_ids[bad] == -1).all() and np.isinf(r_d[bad]).all()
    d_table, d_fids = _table_bits(table), torch.from_numpy(fids).cuda()
    for variant in VARIANTS:
        d_base, d_q = _cast(base, variant), _cast(q, variant)
        ps = ops.prescreen_encode(d_base, 0) if variant == "f32_ps" else None
        common = (g["d_graph"], g["d_start"], g["d_stats"], K, tau)
        ids, d, nd, npop = [x.cpu().numpy() for x in ops.query_filtered_by(
            d_base, d_q, *common, d_table, d_fids, iters, counters=True, prescreen=ps)]
        assert np.array_equal(ids, r_ids), variant
        assert d.tobytes() == r_d.tobytes(), variant
        assert np.array_equal(nd, r_nd) and np.array_equal(npop, r_pop), variant
        # ... and the per-call kernel path, once per table row on that row's queries
        for f in range(F):
            sel = np.nonzero(fids == f)[0]
            one = [x.cpu().numpy() for x in ops.query_filtered(
                d_base, d_q[torch.from_numpy(sel).cuda()].contiguous(), *common,
                d_table[f].contiguous(), iters, counters=True, prescreen=ps)]
            what = (variant, f)
            assert np.array_equal(ids[sel], one[0]) and d[sel].tobytes() == one[1].tobytes(), what
            assert np.array_equal(nd[sel], one[2]) and np.array_equal(npop[sel], one[3]), what
        sel = np.nonzero(fids == -1)[0]
        one = [x.cpu().numpy() for x in ops.query(
            d_base, d_q[torch.from_numpy(sel).cuda()].contiguous(), *common, iters, counters=True,
            prescreen=ps)]
        assert np.array_equal(ids[sel], one[0]) and d[sel].tobytes() == one[1].tobytes(), variant
        assert np.array_equal(nd[sel], one[2]) and np.array_equal(npop[sel], one[3]), variant


def test_seam_shard_offsets_and_wild_ids(graphs):
    """second shard of two per GPU: bits read at offset N in a table over 2 N ids, result columns
    and the -1 of empty slots offset as the unfiltered kernel writes them; id values far outside
    the table (INT32_MIN / MAX, -2) give empty results"""
    from ggnn_amd import ops
    torch = _torch()
    g, base = graphs[24], graphs["base"]
    K, tau, iters = 10, 0.6, 200
    table = _table(g)
    wide = np.concatenate([~table, table], axis=1)        # this shard's bits are the upper half
    fids = np.array([1, -2, 2 ** 31 - 1, -2 ** 31, -1, 3, len(table)], np.int32)
    q = np.random.default_rng(9).integers(0, 128, (len(fids), D)).astype(np.float32)
    d_base, d_q = _cast(base, "f32"), _cast(q, "f32")
    ids, d = ops.query_filtered_by(d_base, d_q, g["d_graph"], g["d_start"], g["d_stats"], K, tau,
                                   _table_bits(wide), torch.from_numpy(fids).cuda(), iters,
                                   filter_bit_offset=N, shards_per_gpu=2, on_gpu_shard=1)
    ids, d = ids.cpu().numpy()[:, K:], d.cpu().numpy()[:, K:]
    for i, f in enumerate(fids):
        r = py_query_filtered(base, q[i], g["graph"], g["start"], g["stats"], K, tau, iters,
                              _allowed_of(table, int(f)))
        assert np.array_equal(ids[i], r[0] + N) and d[i].tobytes() == r[1].tobytes(), (i, f)
        if not -1 <= f < len(table):
            assert (ids[i] == N - 1).all() and np.isinf(d[i]).all()


@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("variant", ["f32", "u8", "f16", "bf16"])
def test_seam_bf_query_filtered_by(orc, graphs, variant, measure):
    """k 10 (register list) and k 300 (the LDS scan kernel); N is no multiple of 64"""
    from ggnn_amd import ops
    torch = _torch()
    base = np.maximum(graphs["base"], 1.0)                # (no zero row: cosine)
    table = _table(graphs[24])
    fids = np.array([2, -1, 0, INVALID, 5, 1, 3, 4, 2, -5], np.int32)
    q = np.maximum(np.random.default_rng(61 + measure).integers(0, 128, (len(fids), D)), 1)
    q = q.astype(np.float32)
    d_base, d_q = _cast(base, variant), _cast(q, variant)
    d_table, d_fids = _table_bits(table), torch.from_numpy(fids).cuda()
    for K in (10, 300):
        ids, d = ops.bf_query_filtered_by(d_base, d_q, K, d_table, d_fids, measure)
        ids, d = ids.cpu().numpy(), d.cpu().numpy()
        for i, f in enumerate(fids):
            r_ids, r_d = bf_filtered_reference(orc, base, q[i:i + 1], K, _allowed_of(table, int(f)),
                                               measure)
            assert np.array_equal(ids[i], r_ids[0]) and d[i].tobytes() == r_d[0].tobytes(), (K, i, f)


def test_seam_bf_query_filtered_by_sliced_base(orc):
    """few queries on a base large enough for several slices: every (query, slice) wave picks the
    row of its query"""
    from ggnn_amd import ops
    torch = _torch()
    Nb = 20011
    rs = np.random.default_rng(51)
    base = rs.integers(0, 4, (Nb, D)).astype(np.float32)        # many equal distances
    q = rs.integers(0, 4, (5, D)).astype(np.float32)
    table = np.stack([rs.random(Nb) < 0.3, rs.random(Nb) < 0.05])
    fids = np.array([1, 0, -1, 7, 0], np.int32)
    ids, d = ops.bf_query_filtered_by(_cast(base, "f32"), _cast(q, "f32"), 100, _table_bits(table),
                                      torch.from_numpy(fids).cuda())
    for i, f in enumerate(fids):
        r_ids, r_d = bf_filtered_reference(orc, base, q[i:i + 1], 100, _allowed_of(table, int(f)))
        assert np.array_equal(ids[i].cpu().numpy(), r_ids[0]), (i, f)
        assert d[i].cpu().numpy().tobytes() == r_d[0].tobytes(), (i, f)


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("Nb", [1, 31, 32, 33, 63, 64, 65, 3000])
def test_pack_filters_on_the_gpu_equals_the_host_packing(Nb, F):
    import ggnn_amd
    torch = _torch()
    masks = np.random.default_rng(Nb + F).random((F, Nb)) < 0.4
    masks[F - 1, Nb - 1] = True
    got = ggnn_amd.pack_filters(torch.from_numpy(masks).cuda())
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (F, (Nb + 31) // 32)
    want = np.stack([pack_bits(m) for m in masks])
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)      # (padding bits zero)
    assert np.array_equal(ggnn_amd.pack_filters(masks).numpy().view(np.uint32), want)


# ---- the handle ----------------------------------------------------------------------------------
def _expected(eng, q, fids, table, K, tau, iters, query_filtered=None):
    """per table row what GGNN.query_filtered(filter=row) returns for that row's queries on this
    handle (pinned against the oracle by tests/test_gpu_filtered.py), GGNN.query for the -1 rows"""
    ids = np.empty((len(q), K), np.int32)
    d = np.empty((len(q), K), np.float32)
    for f in np.unique(fids):
        sel = np.nonzero(fids == f)[0]
        sub = np.ascontiguousarray(q[sel])
        r = eng.query(sub, K, tau, iters) if f == -1 else \
            eng.query_filtered(sub, K, tau, iters, filter=table[f])
        ids[sel], d[sel] = r[0].numpy(), r[1].numpy()
    return ids, d


def _same(got, want, what):
    ids, d = (x.cpu().numpy() for x in got)
    assert np.array_equal(ids, want[0]), what
    assert d.tobytes() == want[1].tobytes(), what


@pytest.mark.parametrize("n_ctx", [1, 4])
def test_handle_filter_table(n_ctx):
    """two shards per GPU on one GPU and on a handle of four device contexts; 37 queries with
    mixed ids through every path of the blocking driver and two asynchronous slots"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    torch = _torch()
    Nb, Dh, K, tau, iters = 8000, 64, 10, 0.7, 200
    NSH = Nb // (2 * n_ctx)
    base = np.random.default_rng(187).integers(0, 256, (Nb, Dh)).astype(np.float32)
    q = np.random.default_rng(188).integers(0, 256, (37, Dh)).astype(np.float32)
    rs = np.random.default_rng(5)
    table = np.stack([rs.random(Nb) < 0.3, rs.random(Nb) < 0.02, np.ones(Nb, bool),
                      np.zeros(Nb, bool), np.arange(Nb) >= Nb // 2])
    F = len(table)
    fids = rs.integers(-1, F, 37).astype(np.int32)
    fids[:F + 1] = np.arange(-1, F)                       # every row and -1 at least once
    fids2 = np.roll(fids, 11)
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_filters(table)                                # before there is any GPU context
    assert eng.num_filters == F
    if n_ctx > 1:
        eng.set_gpus([0] * n_ctx)
    eng.set_shard_size(NSH)
    eng.build(24, 0.5, 1)

    def check_all(table, what):
        want, want2 = (_expected(eng, q, f, table, K, tau, iters) for f in (fids, fids2))
        for i, f in enumerate(fids):                      # never a denied id
            fin = np.isfinite(want[1][i])
            assert f == -1 or table[f][want[0][i][fin]].all(), (what, i)
        modes = [{}, {"SHARD_OVERLAP": 0}, {"EXCHANGE": 1, "QUERY_SPLIT": 1}] if n_ctx == 1 else \
            [{}, {"QUERY_SPLIT": 1}, {"EXCHANGE": 3, "QUERY_SPLIT": 1},
             {"EXCHANGE": 2, "QUERY_SPLIT": 0}]
        for hooks in modes:
            with _lib.hooks(**hooks):
                # (the expectation under the same hooks: the exchange decides the order of ties)
                w = _expected(eng, q, fids, table, K, tau, iters) if hooks else want
                _same(eng.query_filtered_by(q, K, tau, iters, filter_ids=fids), w, (what, hooks))
        # ids as int64, as a torch tensor, in device memory
        for form in (fids.astype(np.int64), torch.from_numpy(fids), torch.from_numpy(fids).cuda()):
            _same(eng.query_filtered_by(q, K, tau, iters, filter_ids=form), want, what)
        # two asynchronous slots in flight with different id arrays
        if n_ctx == 1:
            qd = torch.from_numpy(q).cuda()
            t0 = eng.query_async(qd, K, tau, iters, slot=0, filter_ids=torch.from_numpy(fids).cuda())
            t1 = eng.query_async(qd, K, tau, iters, slot=1, filter_ids=fids2)
        else:
            t0 = eng.query_async(torch.from_numpy(q).cuda(), K, tau, iters, slot=0, filter_ids=fids)
            t1 = eng.query_async(torch.from_numpy(q), K, tau, iters, slot=1,
                                 filter_ids=torch.from_numpy(fids2).cuda())
        assert t0.filter_ids is not None and t1.filter_ids is not None
        eng.synchronize()
        for t, w in ((t0, want), (t1, want2)):
            _same((t.ids[:, :K], t.dists[:, :K]), w, (what, "async"))
        return want

    first = check_all(table, "as set")
    if n_ctx == 1:
        # results on the GPU: the sorted [Nq, K * shards] rows
        eng.set_return_results_on_gpu(True)
        ids_g, d_g = eng.query_filtered_by(torch.from_numpy(q).cuda(), K, tau, iters, filter_ids=fids)
        eng.set_return_results_on_gpu(False)
        assert ids_g.is_cuda and tuple(ids_g.shape) == (37, 2 * K)
        _same((ids_g[:, :K], d_g[:, :K]), first, "results on the GPU")
        # counters: the sums over the per-row calls
        eng.set_collect_counters(True)
        tot = {"n_dist": 0, "n_pop": 0}
        for f in np.unique(fids):
            sub = np.ascontiguousarray(q[fids == f])
            eng.query(sub, K, tau, iters) if f == -1 else \
                eng.query_filtered(sub, K, tau, iters, filter=table[f])
            c = eng.last_query_counters()
            tot = {k: tot[k] + c[k] for k in tot}
        eng.query_filtered_by(q, K, tau, iters, filter_ids=fids)
        c = eng.last_query_counters()
        eng.set_collect_counters(False)
        assert (c["n_dist"], c["n_pop"]) == (tot["n_dist"], tot["n_pop"]) and tot["n_pop"] > 0
        # the exact search through the handle
        b_ids, b_d = eng.bf_query_filtered_by(q, 20, filter_ids=fids)
        for f in np.unique(fids):
            sel = np.nonzero(fids == f)[0]
            sub = np.ascontiguousarray(q[sel])
            r = eng.bf_query(sub, 20) if f == -1 else eng.bf_query_filtered(sub, 20, filter=table[f])
            assert np.array_equal(b_ids.numpy()[sel], r[0].numpy()), f
            assert b_d.numpy()[sel].tobytes() == r[1].numpy().tobytes(), f

    # update_filter: the changed row's queries change accordingly, the others do not
    new_row = np.arange(Nb) % 3 == 0
    eng.update_filter(1, new_row)
    table2 = table.copy()
    table2[1] = new_row
    second = check_all(table2, "row 1 replaced")
    changed = fids == 1
    assert first[1][~changed].tobytes() == second[1][~changed].tobytes()
    assert np.array_equal(first[0][~changed], second[0][~changed])
    assert not np.array_equal(first[0][changed], second[0][changed])
    eng.update_filter(0, ggnn.pack_filter(table[1]).cuda())      # a packed row in device memory
    table2[0] = table[1]
    _same(eng.query_filtered_by(q, K, tau, iters, filter_ids=fids),
          _expected(eng, q, fids, table2, K, tau, iters), "row 0 replaced from the GPU")

    # host-side ids outside [-1, F) raise
    for bad in (F, -2):
        wrong = fids.copy()
        wrong[5] = bad
        with pytest.raises(RuntimeError, match="filter id"):
            eng.query_filtered_by(q, K, tau, iters, filter_ids=wrong)
        with pytest.raises(RuntimeError, match="filter id"):
            eng.bf_query_filtered_by(q, K, filter_ids=wrong)
    # ... in device memory they give an empty result and nothing else changes
    wrong = fids.copy()
    wrong[5] = F + 100
    got = eng.query_filtered_by(q, K, tau, iters, filter_ids=torch.from_numpy(wrong).cuda())
    want = _expected(eng, q, fids, table2, K, tau, iters)
    want[0][5], want[1][5] = -1, np.inf
    _same(got, want, "invalid id in device memory")

    # a table given as packed words on the GPU replaces the old one; None drops it
    eng.set_filters(ggnn.pack_filters(torch.from_numpy(table).cuda()))
    _same(eng.query_filtered_by(q, K, tau, iters, filter_ids=fids), first, "table from the GPU")
    eng.set_filters(None)
    assert eng.num_filters == 0
    with pytest.raises(RuntimeError, match="filter table"):
        eng.query_filtered_by(q, K, tau, iters, filter_ids=fids)


def test_handle_filter_table_follows_the_contexts(tmp_path):
    """the table is placed on whatever contexts the handle gets: the one an exact search creates
    before there is a graph, those of the build that follows, those a load creates in a new layout"""
    import ggnn_amd as ggnn
    Nb, Dh, K, tau, iters = 4000, 64, 10, 0.7, 200
    base = np.random.default_rng(31).integers(0, 256, (Nb, Dh)).astype(np.float32)
    q = np.random.default_rng(32).integers(0, 256, (12, Dh)).astype(np.float32)
    table = np.stack([np.random.default_rng(33).random(Nb) < 0.2, np.arange(Nb) < Nb // 2])
    fids = np.array([0, 1, -1] * 4, np.int32)
    eng = ggnn.GGNN()
    eng.set_working_directory(tmp_path)
    eng.set_base(base)
    eng.set_filters(table)
    b_ids, b_d = eng.bf_query_filtered_by(q, 20, filter_ids=fids)   # no graph yet: a context of its own
    for f in (0, 1):
        r = eng.bf_query_filtered(np.ascontiguousarray(q[fids == f]), 20, filter=table[f])
        assert np.array_equal(b_ids.numpy()[fids == f], r[0].numpy())
    eng.set_shard_size(Nb // 2)
    eng.build(24, 0.5, 1)
    before = eng.query_filtered_by(q, K, tau, iters, filter_ids=fids)
    _same(before, _expected(eng, q, fids, table, K, tau, iters), "before")
    eng.store()
    again = ggnn.GGNN()
    again.set_working_directory(tmp_path)
    again.set_base(base)
    again.set_filters(table)
    again.set_gpus([0, 0])                                # one shard on each of two contexts
    again.set_shard_size(Nb // 2)
    again.load(24)
    after = again.query_filtered_by(q, K, tau, iters, filter_ids=fids)
    _same(after, _expected(again, q, fids, table, K, tau, iters), "after load")
    assert after[1].numpy().tobytes() == before[1].numpy().tobytes()


def test_handle_filter_table_out_of_core():
    """shards that take turns in GPU memory (hook RESIDENT_SHARDS below the shards per GPU)"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    Nb, Dh, K, NSH = 8000, 64, 10, 2000
    base = np.random.default_rng(7).integers(0, 256, (Nb, Dh)).astype(np.float32)
    q = np.random.default_rng(8).integers(0, 256, (20, Dh)).astype(np.float32)
    table = np.stack([np.random.default_rng(9).random(Nb) < 0.2, np.arange(Nb) % 2 == 0])
    fids = np.array([0, 1, -1, 1, 0] * 4, np.int32)
    with _lib.hooks(RESIDENT_SHARDS=2):
        eng = ggnn.GGNN()
        eng.set_base(base)
        eng.set_filters(table)
        eng.set_shard_size(NSH)
        eng.build(24, 0.5, 1)
        got = eng.query_filtered_by(q, K, 0.7, 200, filter_ids=fids)
        want = _expected(eng, q, fids, table, K, 0.7, 200)
        del eng
    _same(got, want, "out of core")
    fin = np.isfinite(want[1])
    assert fin.any()
