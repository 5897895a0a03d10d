"""GPU tests of the label filters: one int32 label per base vector, one per query
(ggnn_set_labels / ggnn_*_labeled and their operators).  The contract is one sentence -- query n
with label L is the per-call filtered search of that query with the bitset base_labels == L, label
-1 the unfiltered search -- and every comparison here is bit for bit: array_equal on ids, tobytes()
on distances, equal counters.  Integer-valued data (values 0..127: exact in every dtype) and the
graphs of tests/test_gpu_filter_table.py."""
import numpy as np
import pytest

from filtered_reference import bf_filtered_reference, pack_bits, py_query_filtered

pytestmark = pytest.mark.gpu

N, D = 3000, 32
VARIANTS = ["f32", "f32_ps", "u8", "f16", "bf16"]
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
STARTS, UNUSED = 1000, 4242          # the class of the start points; a label no row carries


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


def _dev(a, dtype=np.int32):
    return _torch().from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _table_bits(masks):
    words = np.stack([pack_bits(m) for m in masks]).view(np.int32)
    return _torch().from_numpy(np.ascontiguousarray(words)).cuda()


@pytest.fixture(scope="module")
def graphs(orc):
    """the 3000 x 32 integer base with a KBuild = 24 and a KBuild = 40 graph of the oracle,
    uploaded once (as tests/test_gpu_filter_table.py builds them)"""
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


def _base_labels(g, n=N, seed=3):
    """skewed classes: about 50 % label 0, 25 % label 1, 10 % label 2, 1 % label 3, the rest -7;
    the start points (and nothing else) are the class STARTS"""
    u = np.random.default_rng(seed).random(n)
    lab = np.full(n, -7, np.int32)
    lab[u < 0.86] = 3
    lab[u < 0.85] = 2
    lab[u < 0.75] = 1
    lab[u < 0.50] = 0
    if g is not None:
        lab[g["start"]] = STARTS
    return lab


def _allowed_of(labels, L):
    """the whole contract: the rows that carry L; everything for -1"""
    return np.ones(len(labels), bool) if L == -1 else labels == L


def _as_table(labels, qlabels):
    """the same filters as a filter table: one row per distinct query label, and the id of each
    query's row (-1 stays -1)"""
    rows = [L for L in dict.fromkeys(int(x) for x in qlabels) if L != -1]
    table = np.stack([labels == L for L in rows])
    fids = np.array([-1 if L == -1 else rows.index(int(L)) for L in qlabels], np.int32)
    return table, fids


# every class, -1, a label no row carries and the two ends of int32, not grouped
QLABELS = np.array([1, -1, UNUSED, 0, INT32_MIN, STARTS, 2, -7, INT32_MAX, 3], np.int32)

# every kernel form, as SEAM_CASES of tests/test_gpu_filter_table.py: early rows (K 10 / 400
# iterations), the ring scan (2048 iterations), R > 1 (K 300), the LDS list (K 2100), the non-early
# order of a KBuild = 40 graph
SEAM_CASES = [(24, 10, 400), (24, 10, 2048), (24, 300, 1000), (24, 2100, 64), (40, 10, 400)]


@pytest.mark.parametrize("KB,K,iters", SEAM_CASES, ids=[f"kb{c[0]}-k{c[1]}-it{c[2]}" for c in SEAM_CASES])
def test_seam_query_labeled(graphs, KB, K, iters):
    from ggnn_amd import ops
    g, base = graphs[KB], graphs["base"]
    tau = 0.6
    labels = _base_labels(g)
    shares = [np.mean(labels == L) for L in (0, 1, 2, 3)]
    assert 0.45 < shares[0] < 0.55 and 0.2 < shares[1] < 0.3 and 0.07 < shares[2] < 0.13
    assert 0.003 < shares[3] < 0.02 and (labels == -7).any()
    assert np.array_equal(np.sort(np.nonzero(labels == STARTS)[0]), np.sort(g["start"]))
    nq = len(QLABELS)
    q = np.random.default_rng(K + iters).integers(0, 128, (nq, D)).astype(np.float32)
    ref = [py_query_filtered(base, q[i], g["graph"], g["start"], g["stats"], K, tau, iters,
                             _allowed_of(labels, int(QLABELS[i]))) for i in range(nq)]
    r_ids = np.stack([r[0] for r in ref])
    r_d = np.stack([r[1] for r in ref])
    r_nd = np.array([r[2] for r in ref])
    r_pop = np.array([r[3] for r in ref])
    table, fids = _as_table(labels, QLABELS)
    d_labels, d_qlabels = _dev(labels), _dev(QLABELS)
    d_table, d_fids = _table_bits(table), _dev(fids)
    for variant in VARIANTS:
        d_base, d_q = _cast(base, variant), _cast(q, variant)
        ps = ops.prescreen_encode(d_base, 0) if variant == "f32_ps" else None
        common = (g["d_graph"], g["d_start"], g["d_stats"], K, tau)
        ids, d, nd, npop = [x.cpu().numpy() for x in ops.query_labeled(
            d_base, d_q, *common, d_labels, d_qlabels, iters, counters=True, prescreen=ps)]
        assert np.array_equal(ids, r_ids), variant
        assert d.tobytes() == r_d.tobytes(), variant
        assert np.array_equal(nd, r_nd) and np.array_equal(npop, r_pop), variant
        # a label no row carries: all (-1, +inf)
        for L in (UNUSED, INT32_MIN, INT32_MAX):
            sel = QLABELS == L
            assert (ids[sel] == -1).all() and np.isinf(d[sel]).all() and (d[sel] > 0).all(), variant
        # ... and the filter table of those masks on the same device arrays
        t_ids, t_d, t_nd, t_pop = [x.cpu().numpy() for x in ops.query_filtered_by(
            d_base, d_q, *common, d_table, d_fids, iters, counters=True, prescreen=ps)]
        assert np.array_equal(ids, t_ids) and d.tobytes() == t_d.tobytes(), variant
        assert np.array_equal(nd, t_nd) and np.array_equal(npop, t_pop), variant


def test_seam_shard_offset(graphs):
    """second shard of two per GPU: labels read at offset N in a column over 2 N ids, result
    columns and the -1 of empty slots offset as the unfiltered kernel writes them"""
    from ggnn_amd import ops
    g, base = graphs[24], graphs["base"]
    K, tau, iters = 10, 0.6, 200
    labels = _base_labels(g)
    # this shard's labels are the upper half; the lower half carries other values of the same set
    wide = np.concatenate([np.roll(labels, 17), labels])
    q = np.random.default_rng(9).integers(0, 128, (len(QLABELS), D)).astype(np.float32)
    d_base, d_q = _cast(base, "f32"), _cast(q, "f32")
    args = (d_base, d_q, g["d_graph"], g["d_start"], g["d_stats"], K, tau)
    ids, d = ops.query_labeled(*args, _dev(wide), _dev(QLABELS), iters, bit_offset=N,
                               shards_per_gpu=2, on_gpu_shard=1)
    table, fids = _as_table(wide, QLABELS)
    t_ids, t_d = ops.query_filtered_by(*args, _table_bits(table), _dev(fids), iters,
                                       filter_bit_offset=N, shards_per_gpu=2, on_gpu_shard=1)
    assert np.array_equal(ids.cpu().numpy()[:, K:], t_ids.cpu().numpy()[:, K:])
    assert d.cpu().numpy()[:, K:].tobytes() == t_d.cpu().numpy()[:, K:].tobytes()
    ids, d = ids.cpu().numpy()[:, K:], d.cpu().numpy()[:, K:]
    for i, L in enumerate(QLABELS):
        r = py_query_filtered(base, q[i], g["graph"], g["start"], g["stats"], K, tau, iters,
                              _allowed_of(labels, int(L)))
        assert np.array_equal(ids[i], r[0] + N) and d[i].tobytes() == r[1].tobytes(), (i, L)
        if L in (UNUSED, INT32_MIN, INT32_MAX):
            assert (ids[i] == N - 1).all() and np.isinf(d[i]).all()


@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("variant", ["f32", "u8", "f16", "bf16"])
def test_seam_bf_query_labeled(orc, graphs, variant, measure):
    """k 10 (register list) and k 300 (the LDS scan kernel), both above the size of the smallest
    classes, so slots are padded; N = 3000 is no multiple of 64; once more with the labels at
    offset N of a column over 2 N ids"""
    from ggnn_amd import ops
    base = np.maximum(graphs["base"], 1.0)                # (no zero row: cosine)
    labels = _base_labels(graphs[24])
    labels[np.nonzero(labels == 3)[0][5:]] = 2            # a class of exactly five rows
    assert (labels == 3).sum() == 5
    q = np.maximum(np.random.default_rng(61 + measure).integers(0, 128, (len(QLABELS), D)), 1)
    q = q.astype(np.float32)
    d_base, d_q = _cast(base, variant), _cast(q, variant)
    table, fids = _as_table(labels, QLABELS)
    d_table, d_fids = _table_bits(table), _dev(fids)
    wide = np.concatenate([np.roll(labels, 5), labels])
    for K in (10, 300):
        ids, d = ops.bf_query_labeled(d_base, d_q, K, _dev(labels), _dev(QLABELS), measure)
        t_ids, t_d = ops.bf_query_filtered_by(d_base, d_q, K, d_table, d_fids, measure)
        assert _torch().equal(ids, t_ids)
        assert d.cpu().numpy().tobytes() == t_d.cpu().numpy().tobytes()
        o_ids, o_d = ops.bf_query_labeled(d_base, d_q, K, _dev(wide), _dev(QLABELS), measure,
                                          bit_offset=N)
        assert _torch().equal(ids, o_ids)
        assert d.cpu().numpy().tobytes() == o_d.cpu().numpy().tobytes()
        ids, d = ids.cpu().numpy(), d.cpu().numpy()
        for i, L in enumerate(QLABELS):
            r_ids, r_d = bf_filtered_reference(orc, base, q[i:i + 1], K,
                                               _allowed_of(labels, int(L)), measure)
            assert np.array_equal(ids[i], r_ids[0]) and d[i].tobytes() == r_d[0].tobytes(), (K, i, L)
        i = int(np.nonzero(QLABELS == 3)[0][0])           # five rows, then padding
        assert (ids[i, :5] >= 0).all() and (ids[i, 5:] == -1).all() and np.isinf(d[i, 5:]).all()


# ---- the handle ----------------------------------------------------------------------------------
def _same(got, want, what):
    ids, d = (x.cpu().numpy() for x in got)
    w_ids, w_d = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in want)
    assert np.array_equal(ids, w_ids), what
    assert d.tobytes() == w_d.tobytes(), what


@pytest.mark.parametrize("n_ctx", [1, 4])
def test_handle_labels(n_ctx):
    """two shards per GPU on one GPU and on a handle of four device contexts; 37 queries with
    mixed labels through every path of the blocking driver and two asynchronous slots, each
    against the filter table of the same masks on the same handle"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    torch = _torch()
    Nb, Dh, K, tau, iters = 8000, 64, 10, 0.7, 200
    NSH = Nb // (2 * n_ctx)
    base = np.random.default_rng(187).integers(0, 256, (Nb, Dh)).astype(np.float32)
    q = np.random.default_rng(188).integers(0, 256, (37, Dh)).astype(np.float32)
    rs = np.random.default_rng(5)
    labels = _base_labels(None, Nb, seed=6)
    pool = np.array([0, 1, 2, 3, -7, -1, UNUSED, INT32_MIN, INT32_MAX], np.int32)
    qlab = rs.choice(pool, 37).astype(np.int32)
    qlab[:len(pool)] = pool                               # every value at least once
    qlab2 = np.roll(qlab, 11)
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_labels(labels)                                # before there is any GPU context
    assert eng.num_labels == Nb
    if n_ctx > 1:
        eng.set_gpus([0] * n_ctx)
    eng.set_shard_size(NSH)
    eng.build(24, 0.5, 1)

    def check_all(labels, what):
        table, fids = _as_table(labels, qlab)
        fids2 = np.roll(fids, 11)                         # (the rows of the same table)
        eng.set_filters(table)
        want = eng.query_filtered_by(q, K, tau, iters, filter_ids=fids)
        want2 = eng.query_filtered_by(q, K, tau, iters, filter_ids=fids2)
        w_ids, w_d = want[0].numpy(), want[1].numpy()
        for i, L in enumerate(qlab):                      # never another label's row
            fin = np.isfinite(w_d[i])
            assert L == -1 or (labels[w_ids[i][fin]] == L).all(), (what, i)
        assert np.isfinite(w_d[qlab == 0]).all() and np.isinf(w_d[qlab == UNUSED]).all()
        modes = [{}, {"SHARD_OVERLAP": 0}, {"EXCHANGE": 1, "QUERY_SPLIT": 1}] if n_ctx == 1 else \
            [{}, {"QUERY_SPLIT": 1}, {"EXCHANGE": 3, "QUERY_SPLIT": 1},
             {"EXCHANGE": 2, "QUERY_SPLIT": 0}]
        for hooks in modes:
            with _lib.hooks(**hooks):
                # (the expectation under the same hooks: the exchange decides the order of ties)
                w = eng.query_filtered_by(q, K, tau, iters, filter_ids=fids) if hooks else want
                _same(eng.query_labeled(q, K, tau, iters, labels=qlab), w, (what, hooks))
        # labels as int64, as a torch tensor, in device memory
        for form in (qlab.astype(np.int64), torch.from_numpy(qlab), torch.from_numpy(qlab).cuda()):
            _same(eng.query_labeled(q, K, tau, iters, labels=form), want, what)
        # two asynchronous slots in flight with different label arrays
        if n_ctx == 1:
            qd = torch.from_numpy(q).cuda()
            t0 = eng.query_async_labeled(qd, K, tau, iters, slot=0, labels=torch.from_numpy(qlab).cuda())
            t1 = eng.query_async_labeled(qd, K, tau, iters, slot=1, labels=qlab2)
        else:
            t0 = eng.query_async_labeled(torch.from_numpy(q).cuda(), K, tau, iters, slot=0, labels=qlab)
            t1 = eng.query_async_labeled(torch.from_numpy(q), K, tau, iters, slot=1,
                                 labels=torch.from_numpy(qlab2).cuda())
        assert t0.filter_ids is not None and t1.filter_ids is not None
        eng.synchronize()
        for t, w in ((t0, want), (t1, want2)):
            _same((t.ids[:, :K], t.dists[:, :K]), w, (what, "async"))
        _same(eng.query_labeled(q, K, tau, iters, labels=qlab), want, (what, "blocking again"))
        return w_ids, w_d, fids

    first = check_all(labels, "as set")
    if n_ctx == 1:
        fids = first[2]
        # results on the GPU: the sorted [Nq, K * shards] rows
        eng.set_return_results_on_gpu(True)
        ids_g, d_g = eng.query_labeled(torch.from_numpy(q).cuda(), K, tau, iters, labels=qlab)
        eng.set_return_results_on_gpu(False)
        assert ids_g.is_cuda and tuple(ids_g.shape) == (37, 2 * K)
        _same((ids_g[:, :K], d_g[:, :K]), first[:2], "results on the GPU")
        # counters
        eng.set_collect_counters(True)
        eng.query_filtered_by(q, K, tau, iters, filter_ids=fids)
        c_table = eng.last_query_counters()
        eng.query_labeled(q, K, tau, iters, labels=qlab)
        c = eng.last_query_counters()
        eng.set_collect_counters(False)
        assert (c["n_dist"], c["n_pop"]) == (c_table["n_dist"], c_table["n_pop"]) and c["n_pop"] > 0
        # the exact search through the handle; k above the size of the 1 % class' shard share
        b = eng.bf_query_labeled(q, 100, labels=qlab)
        _same(b, eng.bf_query_filtered_by(q, 100, filter_ids=fids), "bf")
        _same(eng.bf_query_labeled(q, 100, labels=torch.from_numpy(qlab).cuda()), b, "bf, device")
        # labels=None is the unfiltered call
        _same(eng.query_labeled(q, K, tau, iters), eng.query(q, K, tau, iters), "labels=None")

    # update_labels with a repeated id equals set_labels of the final array
    ids_u = np.array([5, 900, 5, 4001, 7999, 900, 0], np.int64)
    val_u = np.array([1, 2, 3, 0, -7, INT32_MAX, 2], np.int32)
    labels2 = labels.copy()
    for i, v in zip(ids_u, val_u):
        labels2[i] = v
    assert labels2[5] == 3 and labels2[900] == INT32_MAX
    with pytest.raises(IndexError):                       # refused whole: nothing changes
        eng.update_labels(np.array([1, Nb]), np.array([3, 3]))
    _same(eng.query_labeled(q, K, tau, iters, labels=qlab), first[:2], "after a refused update")
    big = (np.arange(Nb) % 3 == 0)                        # enough rows to change results
    eng.update_labels(np.concatenate([np.nonzero(big)[0], ids_u]),
                      np.concatenate([np.full(big.sum(), 1, np.int32), val_u]))
    labels2 = labels.copy()
    labels2[big] = 1
    for i, v in zip(ids_u, val_u):
        labels2[i] = v
    updated = eng.query_labeled(q, K, tau, iters, labels=qlab)
    b_updated = eng.bf_query_labeled(q, 50, labels=qlab) if n_ctx == 1 else None
    eng.set_labels(torch.from_numpy(labels2).cuda())      # the final array, from device memory
    _same(eng.query_labeled(q, K, tau, iters, labels=qlab), updated, "update == set")
    if n_ctx == 1:
        _same(eng.bf_query_labeled(q, 50, labels=qlab), b_updated, "update == set, bf")
    second = check_all(labels2, "relabelled")
    assert not np.array_equal(first[0][qlab == 1], second[0][qlab == 1])
    same = qlab == -1
    assert np.array_equal(first[0][same], second[0][same])

    # None drops them: a labeled call without labels raises
    eng.set_labels(None)
    assert eng.num_labels == 0
    with pytest.raises(RuntimeError, match="labels"):
        eng.query_labeled(q, K, tau, iters, labels=qlab)
    with pytest.raises(RuntimeError, match="labels"):
        eng.query_async_labeled(torch.from_numpy(q).cuda(), K, tau, iters, labels=qlab)
    with pytest.raises(RuntimeError, match="labels"):
        eng.bf_query_labeled(q, K, labels=qlab)


def test_handle_labels_follow_the_contexts():
    """the column is placed on the context an exact search creates before there is a graph, and on
    those of the build that follows"""
    import ggnn_amd as ggnn
    Nb, Dh, K, tau, iters = 4000, 64, 10, 0.7, 200
    base = np.random.default_rng(31).integers(0, 256, (Nb, Dh)).astype(np.float32)
    q = np.random.default_rng(32).integers(0, 256, (12, Dh)).astype(np.float32)
    labels = _base_labels(None, Nb, seed=33)
    qlab = np.array([0, 1, -1, 3] * 3, np.int32)
    table, fids = _as_table(labels, qlab)
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_labels(labels)
    eng.set_filters(table)
    b = eng.bf_query_labeled(q, 20, labels=qlab)          # no graph yet: a context of its own
    _same(b, eng.bf_query_filtered_by(q, 20, filter_ids=fids), "bf without a graph")
    # set_base drops the labels (the base can be set again until a graph is built), GPU copy included
    eng.set_base(base)
    assert eng.num_labels == 0
    with pytest.raises(RuntimeError, match="labels"):
        eng.bf_query_labeled(q, 20, labels=qlab)
    eng.set_labels(labels)
    eng.set_filters(table)
    _same(eng.bf_query_labeled(q, 20, labels=qlab), b, "labels set again")
    eng.update_labels(np.array([3, 4]), np.array([1, 1]))
    eng.update_labels(np.array([3, 4]), labels[[3, 4]])   # ... and back
    eng.set_shard_size(Nb // 2)
    eng.build(24, 0.5, 1)
    _same(eng.query_labeled(q, K, tau, iters, labels=qlab),
          eng.query_filtered_by(q, K, tau, iters, filter_ids=fids), "after the build")


def test_labels_survive_a_second_build():
    """a handle builds once, unless the build fails: that rolls its GPU contexts back, the label
    copy of an earlier exact search included, and the build that follows places the column again"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    Nb, Dh, K, tau, iters = 4000, 64, 10, 0.7, 200
    base = np.random.default_rng(41).integers(0, 256, (Nb, Dh)).astype(np.float32)
    q = np.random.default_rng(42).integers(0, 256, (12, Dh)).astype(np.float32)
    labels = _base_labels(None, Nb, seed=43)
    qlab = np.array([0, 1, -1, 2] * 3, np.int32)
    table, fids = _as_table(labels, qlab)
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_labels(labels)
    eng.set_filters(table)
    b = eng.bf_query_labeled(q, 20, labels=qlab)          # the column is on a GPU now
    eng.set_build_hooks(rng=np.zeros(1, np.float32))      # too few numbers: the build refuses
    with pytest.raises(_lib.GGNNError) as e:
        eng.build(24, 0.5, 1)
    assert e.value.status == _lib.INVALID_ARGUMENT
    assert eng.num_labels == Nb
    eng.set_build_hooks()
    eng.build(24, 0.5, 1)                                 # the second build
    assert eng.num_labels == Nb
    _same(eng.query_labeled(q, K, tau, iters, labels=qlab),
          eng.query_filtered_by(q, K, tau, iters, filter_ids=fids), "after the second build")
    _same(eng.bf_query_labeled(q, 20, labels=qlab), b, "bf after the second build")
    with pytest.raises(RuntimeError, match="already been built"):
        eng.build(24, 0.5, 1)


def test_handle_labels_out_of_core():
    """shards that take turns in GPU memory (hook RESIDENT_SHARDS below the shards per GPU)"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    Nb, Dh, K, NSH = 8000, 64, 10, 2000
    base = np.random.default_rng(7).integers(0, 256, (Nb, Dh)).astype(np.float32)
    q = np.random.default_rng(8).integers(0, 256, (20, Dh)).astype(np.float32)
    labels = _base_labels(None, Nb, seed=9)
    qlab = np.array([0, 1, -1, 2, UNUSED] * 4, np.int32)
    table, fids = _as_table(labels, qlab)
    with _lib.hooks(RESIDENT_SHARDS=2):
        eng = ggnn.GGNN()
        eng.set_base(base)
        eng.set_labels(labels)
        eng.set_filters(table)
        eng.set_shard_size(NSH)
        eng.build(24, 0.5, 1)
        got = eng.query_labeled(q, K, 0.7, 200, labels=qlab)
        want = eng.query_filtered_by(q, K, 0.7, 200, filter_ids=fids)
        del eng
    _same(got, want, "out of core")
    assert np.isfinite(want[1].numpy()[qlab == 0]).all()
