"""GPU tests of the filtered search (ggnn_query_filtered / ggnn_bf_query_filtered and their
operators).  Integer-valued data (squared L2 exact in float32: D * max^2 < 2^24) so that the
kernels equal the Python reference of tests/filtered_reference.py bit for bit, counters included;
float data and the cosine measure are carried by the all-ones filter (== the unfiltered kernels,
which are pinned to the oracle) and by the kernel variants checking each other.  Nothing here is
statistical."""
import numpy as np
import pytest

from filtered_reference import (bf_filtered_reference, check_filtered_invariants, l2_exact,
                                pack_bits, py_query_filtered)
from parity_helpers import RTOL, assert_rows_consistent, cos_atol, true_distances

pytestmark = pytest.mark.gpu

N, D = 3000, 32
VARIANTS = ["f32", "f32_ps", "u8", "f16", "bf16"]


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


def _bits(mask):
    return _torch().from_numpy(pack_bits(mask).view(np.int32).copy()).cuda()


@pytest.fixture(scope="module")
def graphs(orc):
    """one integer base (values 0..127: exact in every dtype) with a KBuild = 24 and a KBuild = 40
    graph of the oracle, uploaded once"""
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


def _filters(g, which):
    rs = np.random.default_rng(3)
    out = {}
    for name in which:
        if name == "starts":
            m = np.ones(N, bool)
            m[g["start"]] = False
        elif name == "single":
            m = np.zeros(N, bool)
            m[1234] = True
        else:
            m = rs.random(N) < float(name) / 100.0 if float(name) < 100 else np.ones(N, bool)
        out[name] = m
    return out


def _gpu_query(ops, graphs, KB, variant, q, K, tau, iters, bits, base=None, measure=0,
               filtered=True):
    g = graphs[KB]
    base = graphs["base"] if base is None else base
    d_base, d_q = _cast(base, variant), _cast(q, variant)
    ps = ops.prescreen_encode(d_base, measure) if variant == "f32_ps" else None
    if filtered:
        r = ops.query_filtered(d_base, d_q, g["d_graph"], g["d_start"], g["d_stats"], K, tau, bits,
                               iters, measure, counters=True, prescreen=ps)
    else:
        r = ops.query(d_base, d_q, g["d_graph"], g["d_start"], g["d_stats"], K, tau, iters, measure,
                      counters=True, prescreen=ps)
    return [x.cpu().numpy() for x in r]


ALL_FILTERS = ["100", "50", "10", "1", "0", "starts", "single"]
# (KBuild, K, iterations, queries, filters): every list form -- one register (sorted 32 / 64, early
# rows with one and two bucket registers; 2048 iterations: the ring scan), R = 2, 8, 16, 32, the
# LDS list (sorted > 2048) and the non-early order of a KBuild > 24 graph
CASES = [
    (24, 1, 64, 8, ALL_FILTERS),
    (24, 10, 400, 8, ALL_FILTERS),
    (24, 40, 64, 8, ALL_FILTERS),
    (24, 10, 2048, 3, ["10", "1"]),
    (24, 100, 400, 4, ["100", "10", "0", "starts"]),
    (24, 300, 1000, 3, ["50", "1"]),
    (24, 600, 2048, 2, ["50", "1"]),
    (24, 1200, 2048, 2, ["50"]),
    (24, 2100, 64, 2, ["50"]),
    (40, 10, 400, 6, ["100", "10", "0", "starts"]),
]


@pytest.mark.parametrize("KB,K,iters,nq,which", CASES,
                         ids=[f"kb{c[0]}-k{c[1]}-it{c[2]}" for c in CASES])
def test_query_filtered_equals_python_reference(orc, graphs, KB, K, iters, nq, which):
    from ggnn_amd import ops
    g, base = graphs[KB], graphs["base"]
    tau = 0.6
    q = np.random.default_rng(K + iters).integers(0, 128, (nq, D)).astype(np.float32)
    for name, allowed in _filters(g, which).items():
        ref = [py_query_filtered(base, q[i], g["graph"], g["start"], g["stats"], K, tau, iters,
                                 allowed) for i in range(nq)]
        r_ids = np.stack([r[0] for r in ref])
        r_d = np.stack([r[1] for r in ref])
        r_nd = np.array([r[2] for r in ref])
        r_pop = np.array([r[3] for r in ref])
        check_filtered_invariants(orc, base, q, r_ids, r_d, allowed, l2_exact(base), K)
        bits = _bits(allowed)
        for variant in VARIANTS:
            ids, d, nd, npop = _gpu_query(ops, graphs, KB, variant, q, K, tau, iters, bits)
            what = (name, variant)
            assert np.array_equal(ids, r_ids), what
            assert d.tobytes() == r_d.tobytes(), what
            assert np.array_equal(nd, r_nd) and np.array_equal(npop, r_pop), what


def _float_bases():
    rs = np.random.default_rng(11)
    centres = rs.normal(size=(12, D)) * 2
    frac = (centres[rs.integers(0, 12, N)] + rs.normal(size=(N, D))).astype(np.float32)
    q_frac = (centres[rs.integers(0, 12, 40)] + rs.normal(size=(40, D))).astype(np.float32)
    return frac, q_frac


@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("variant", VARIANTS)
def test_all_ones_filter_equals_the_unfiltered_kernels(graphs, variant, measure):
    """bit for bit with counters: L2 and cosine, fractional data (integers for uint8), every list
    form the unfiltered dispatch picks for these shapes"""
    from ggnn_amd import ops
    frac, q_frac = _float_bases()
    if variant == "u8":
        base = np.random.default_rng(5).integers(0, 256, (N, D)).astype(np.float32)
        q = np.random.default_rng(6).integers(0, 256, (40, D)).astype(np.float32)
    else:
        base, q = frac, q_frac
    ones = _bits(np.ones(N, bool))
    for KB, K, tau, iters in ((24, 10, 0.7, 400), (24, 1, 0.5, 64), (24, 40, 0.8, 128),
                              (24, 100, 0.7, 400), (24, 300, 0.6, 600), (24, 600, 0.6, 1100),
                              (24, 10, 0.9, 2048), (40, 10, 0.7, 400), (24, 2100, 0.5, 64)):
        a = _gpu_query(ops, graphs, KB, variant, q, K, tau, iters, ones, base, measure)
        b = _gpu_query(ops, graphs, KB, variant, q, K, tau, iters, None, base, measure,
                       filtered=False)
        what = (variant, measure, KB, K, iters)
        assert np.array_equal(a[0], b[0]), what
        assert a[1].tobytes() == b[1].tobytes(), what
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), what
        assert a[3].sum() > 0


@pytest.mark.parametrize("measure", [0, 1])
def test_variants_agree_under_real_filters(orc, graphs, measure):
    """cosine and fractional L2 with 50 % / 10 % / 1 % filters: the kernel variants a hook selects
    (early rows or not, pre-screen or not, small buckets: stash and ring-scan fallback) give the
    same bytes, and the result has the invariants of a filtered search"""
    from ggnn_amd import _lib, ops
    base, q = _float_bases()
    q = q[:16]
    rs = np.random.default_rng(21)
    t = true_distances(base, q, measure)
    atol = cos_atol(D) if measure else 1e-9 * float(np.abs(t).max())
    for share, K, iters in ((0.5, 10, 400), (0.1, 10, 400), (0.01, 10, 200), (0.5, 40, 100)):
        allowed = rs.random(N) < share
        bits = _bits(allowed)
        first = None
        for variant in ("f32_ps", "f32"):
            for hooks in ({}, {"QUERY_EARLY": 0}, {"VIS_SLOTS": 1}, {"VIS_SLOTS": 1, "QUERY_EARLY": 0},
                          {"QUERY_GLOBAL_RING": 0}, {"VIS_TAG_SET": 0}):
                with _lib.hooks(**hooks):
                    r = _gpu_query(ops, graphs, 24, variant, q, K, 0.7, iters, bits, base, measure)
                if first is None:
                    first = r
                what = (share, K, variant, hooks)
                assert np.array_equal(r[0], first[0]) and r[1].tobytes() == first[1].tobytes(), what
                # counters: evaluations and pops do not depend on the variant
                assert np.array_equal(r[2], first[2]) and np.array_equal(r[3], first[3]), what
        ids, d = first[0], first[1]
        assert_rows_consistent(base, q, ids, d, measure, (share, K))
        fin = np.isfinite(d)
        assert allowed[ids[fin]].all()
        assert (fin.sum(1) <= allowed.sum()).all()
        # the exact filtered K nearest are a lower bound entry by entry (float64 truth)
        ta = np.sort(np.where(allowed[None, :], t, np.inf), axis=1)[:, :K]
        assert np.all(ta <= d.astype(np.float64) * (1 + RTOL) + atol)


@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("variant", ["f32", "u8", "f16", "bf16"])
def test_bf_query_filtered_equals_compacted_oracle(orc, variant, measure):
    """N not a multiple of 32 or 64, duplicated rows across the allowed / denied boundary (tie
    order: lower base index first), fewer allowed rows than K (tail (-1, +inf)), a bit offset"""
    from ggnn_amd import ops
    Nb = 1003
    rs = np.random.default_rng(41 + measure)
    base = rs.integers(1, 16, (Nb, D)).astype(np.float32)
    base[500:540] = base[100:140]
    base[900:903] = base[0:3]
    q = rs.integers(1, 16, (9, D)).astype(np.float32)
    q[0] = base[101]
    filters = {}
    for share in (100, 50, 10, 1, 0):
        filters[str(share)] = rs.random(Nb) < share / 100.0 if share < 100 else np.ones(Nb, bool)
    m = np.zeros(Nb, bool)
    m[777] = True
    filters["single"] = m
    m = np.zeros(Nb, bool)
    m[[100, 101, 501, 502, 900, 1002]] = True          # six rows: fewer than K = 10, 100, 300
    filters["few"] = m
    m = np.ones(Nb, bool)
    m[100:140:2] = False                               # one copy of a duplicated pair denied ...
    m[501:540:2] = False                               # ... alternating between the two copies
    filters["dups"] = m
    d_base, d_q = _cast(base, variant), _cast(q, variant)
    for name, allowed in filters.items():
        bits = _bits(allowed)
        for K in (1, 10, 100, 300):
            r_ids, r_d = bf_filtered_reference(orc, base, q, K, allowed, measure)
            ids, d = ops.bf_query_filtered(d_base, d_q, K, bits, measure)
            what = (name, K)
            assert np.array_equal(ids.cpu().numpy(), r_ids), what
            assert d.cpu().numpy().tobytes() == r_d.tobytes(), what
    # the same rows as a window of a longer bitset
    allowed = filters["50"]
    off = 37
    wide = np.zeros(off + Nb, bool)
    wide[off:] = allowed
    r_ids, r_d = bf_filtered_reference(orc, base, q, 10, allowed, measure)
    ids, d = ops.bf_query_filtered(d_base, d_q, 10, _bits(wide), measure, filter_bit_offset=off)
    assert np.array_equal(ids.cpu().numpy(), r_ids) and d.cpu().numpy().tobytes() == r_d.tobytes()


def test_bf_query_filtered_sliced_base(orc):
    """few queries on a base large enough for several slices (their merge keeps the tie order)"""
    from ggnn_amd import ops
    Nb = 20011
    rs = np.random.default_rng(51)
    base = rs.integers(0, 4, (Nb, D)).astype(np.float32)        # many equal distances
    q = rs.integers(0, 4, (5, D)).astype(np.float32)
    allowed = rs.random(Nb) < 0.3
    r_ids, r_d = bf_filtered_reference(orc, base, q, 100, allowed)
    ids, d = ops.bf_query_filtered(_cast(base, "f32"), _cast(q, "f32"), 100, _bits(allowed))
    assert np.array_equal(ids.cpu().numpy(), r_ids) and d.cpu().numpy().tobytes() == r_d.tobytes()


def _handle_reference(orc, eng, base, q, K, tau, iters, allowed, n_ctx, spg, n_shard):
    """per-shard ops.query_filtered (checked against the Python reference in this file) merged the
    way the engine merges: per-GPU sort, then ResultMerger"""
    from ggnn_amd import ops
    torch = _torch()
    bits = _bits(allowed)
    d_q = torch.from_numpy(q).cuda()
    parts_i, parts_d = [], []
    n_dist = n_pop = 0
    for ctx in range(n_ctx):
        rows_i, rows_d = [], []
        for s in range(spg):
            gs = ctx * spg + s
            g = eng.get_graph(gs)
            lo = gs * n_shard
            ids, d, nd, npop = ops.query_filtered(
                torch.from_numpy(base[lo:lo + n_shard]).cuda(), d_q, g.graph[0].view.cuda(),
                g.translation[3].view.reshape(-1).contiguous().cuda(),
                g.nn1_stats.view.reshape(-1).contiguous().cuda(), K, tau, bits, iters,
                filter_bit_offset=lo, counters=True)
            rows_i.append(ids.cpu().numpy() + s * n_shard)
            rows_d.append(d.cpu().numpy())
            n_dist += int(nd.sum())
            n_pop += int(npop.sum())
        si, sd = orc.sort_shard_results(np.concatenate(rows_i, 1), np.concatenate(rows_d, 1))
        parts_i.append(si)
        parts_d.append(sd)
    r_ids, r_d = orc.merge_results(parts_i, parts_d, K, spg, n_shard)
    return r_ids, r_d, n_dist, n_pop


@pytest.mark.parametrize("n_ctx", [1, 4])
def test_handle_query_filtered(orc, n_ctx):
    """GGNN.query_filtered on a 4-shard base on one GPU and on a handle of four device contexts:
    the merged per-shard operator results, global ids, every form of the filter argument"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    torch = _torch()
    Nb, Dh, K, NSH, tau, iters = 8000, 64, 10, 2000 if n_ctx == 1 else 1000, 0.7, 200
    base = np.random.default_rng(187).integers(0, 256, (Nb, Dh)).astype(np.float32)
    q = np.random.default_rng(188).integers(0, 256, (37, Dh)).astype(np.float32)
    eng = ggnn.GGNN()
    eng.set_base(base)
    if n_ctx > 1:
        eng.set_gpus([0] * n_ctx)
    eng.set_shard_size(NSH)
    eng.build(24, 0.5, 1)
    spg = Nb // NSH // n_ctx
    plain = eng.query(q, K, tau, iters)
    none = eng.query_filtered(q, K, tau, iters, filter=None)
    assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1])
    for share in (0.3, 0.02):
        allowed = np.random.default_rng(int(share * 100)).random(Nb) < share
        r_ids, r_d, r_nd, r_pop = _handle_reference(orc, eng, base, q, K, tau, iters, allowed, n_ctx,
                                                    spg, NSH)
        uniq = np.ones_like(r_d, bool)
        uniq[:, 1:] &= r_d[:, 1:] != r_d[:, :-1]
        uniq[:, :-1] &= r_d[:, :-1] != r_d[:, 1:]
        uniq[:, -1] = False
        uniq &= np.isfinite(r_d)
        packed = ggnn.pack_filter(allowed)
        forms = [allowed, torch.from_numpy(allowed), packed, packed.numpy().view(np.uint32),
                 packed.cuda()]
        modes = [{}] if n_ctx == 1 else [{}, {"EXCHANGE": 3, "QUERY_SPLIT": 1},
                                         {"EXCHANGE": 2, "QUERY_SPLIT": 0}]
        for hooks in modes + ([{"SHARD_OVERLAP": 0}] if n_ctx == 1 else []):
            for f in forms if not hooks else forms[:1]:
                with _lib.hooks(**hooks):
                    ids, d = eng.query_filtered(q, K, tau, iters, filter=f)
                ids, d = ids.numpy(), d.numpy()
                assert np.array_equal(d, r_d), (share, hooks)
                assert np.array_equal(ids[uniq], r_ids[uniq]), (share, hooks)
                fin = np.isfinite(d)
                assert allowed[ids[fin]].all() and (ids[fin] < Nb).all()
        eng.set_collect_counters(True)
        ids, d = eng.query_filtered(q, K, tau, iters, filter=allowed)
        c = eng.last_query_counters()
        eng.set_collect_counters(False)
        assert np.array_equal(d.numpy(), r_d)
        assert (c["n_dist"], c["n_pop"]) == (r_nd, r_pop) and r_pop > 0
        assert eng.last_timing_ms()["query_ms"] > 0
    if n_ctx == 1:
        # results on the GPU: the sorted [Nq, K * shards] rows of every shard
        eng.set_return_results_on_gpu(True)
        ids_g, d_g = eng.query_filtered(torch.from_numpy(q).cuda(), K, tau, iters, filter=allowed)
        eng.set_return_results_on_gpu(False)
        assert ids_g.is_cuda and tuple(ids_g.shape) == (37, K * spg)
        assert np.array_equal(d_g[:, :K].cpu().numpy(), r_d)
        # the whole base: exact filtered brute force, host and device filters
        b_ids, b_d = bf_filtered_reference(orc, base, q, 20, allowed)
        for f in (allowed, ggnn.pack_filter(allowed).cuda()):
            ids, d = eng.bf_query_filtered(q, 20, filter=f)
            assert np.array_equal(ids.numpy(), b_ids) and np.array_equal(d.numpy(), b_d)
        ids, d = eng.bf_query_filtered(q, 20, filter=None)
        o_ids, o_d = orc.bf_query(base, q, 20)
        assert np.array_equal(ids.numpy(), o_ids) and np.array_equal(d.numpy(), o_d)
        with pytest.raises(RuntimeError, match="n_bits|one bit per base"):
            _lib.check(_lib.lib().ggnn_query_filtered(
                eng._h, q.ctypes.data, 37, Dh, _lib.F32, _lib.CPU, 0, K, tau, iters, 0,
                ids.data_ptr(), d.data_ptr(), _lib.CPU, packed.data_ptr(), Nb - 1, _lib.CPU, 0),
                eng._h)


def test_handle_query_filtered_out_of_core(orc):
    """shards that take turns in GPU memory (hook RESIDENT_SHARDS below the shards per GPU): the
    filtered call works, and equals the merged per-shard operator results"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    Nb, Dh, K, NSH = 8000, 64, 10, 2000
    base = np.random.default_rng(7).integers(0, 256, (Nb, Dh)).astype(np.float32)
    q = np.random.default_rng(8).integers(0, 256, (20, Dh)).astype(np.float32)
    allowed = np.random.default_rng(9).random(Nb) < 0.2
    with _lib.hooks(RESIDENT_SHARDS=2):
        eng = ggnn.GGNN()
        eng.set_base(base)
        eng.set_shard_size(NSH)
        eng.build(24, 0.5, 1)
        ids, d = eng.query_filtered(q, K, 0.7, 200, filter=allowed)
        r_ids, r_d, _, _ = _handle_reference(orc, eng, base, q, K, 0.7, 200, allowed, 1, 4, NSH)
        del eng
    ids, d = ids.numpy(), d.numpy()
    assert np.array_equal(d, r_d)
    fin = np.isfinite(d)
    assert fin.any() and allowed[ids[fin]].all()


def test_calls_of_one_handle_do_not_leak_into_one_another(tmp_path):
    """Every query mode in turn on ONE handle, a failing filtered call and an asynchronous batch in
    flight among them: each filtered result equals, bit for bit, the same call made alone on a
    freshly loaded handle of the same graph, and the plain query before and after them is
    untouched -- whether a search is filtered depends on its own arguments only."""
    import ggnn_amd as ggnn
    torch = _torch()
    K, tau, iters, nq, F = 10, 0.7, 200, 50, 3
    rs = np.random.default_rng(4711)
    base = rs.integers(0, 128, (N, D)).astype(np.float32)
    q = rs.integers(0, 128, (nq, D)).astype(np.float32)
    mask = rs.random(N) < 0.3
    table = rs.random((F, N)) < 0.4
    fids = rs.integers(-1, F, nq).astype(np.int32)
    labels = rs.integers(0, 4, N).astype(np.int32)
    qlabels = rs.integers(0, 4, nq).astype(np.int32)

    def handle(load):
        e = ggnn.GGNN()
        e.set_base(base)
        e.set_working_directory(str(tmp_path))
        if load:
            e.load(24)
        else:
            e.build(24, 0.5, 1)
            e.store()
        e.set_filters(table)
        e.set_labels(labels)
        return e

    def same(a, b):
        return torch.equal(a[0].cpu(), b[0].cpu()) and torch.equal(a[1].cpu(), b[1].cpu())

    eng = handle(load=False)
    plain = eng.query(q, K, tau, iters)
    by_mask = eng.query_filtered(q, K, tau, iters, filter=mask)
    by_ids = eng.query_filtered_by(q, K, tau, iters, filter_ids=fids)
    by_label = eng.query_labeled(q, K, tau, iters, labels=qlabels)
    bf_ids, bf_d = eng.bf_query_filtered(q, K, filter=mask)
    assert mask[bf_ids.numpy()].all() and np.isfinite(bf_d.numpy()).all()
    with pytest.raises(RuntimeError, match="query dimension does not match the base"):
        eng.query_filtered(q[:, :D - 16].copy(), K, tau, iters, filter=mask)
    plain_again = eng.query(q, K, tau, iters)
    d_q = torch.from_numpy(q).cuda()
    ticket = eng.query_async_labeled(d_q, K, tau, iters, slot=0, labels=qlabels)
    by_ids_meanwhile = eng.query_filtered_by(q, K, tau, iters, filter_ids=fids)
    eng.synchronize()

    alone = handle(load=True)
    assert same(by_mask, alone.query_filtered(q, K, tau, iters, filter=mask))
    alone = handle(load=True)
    assert same(by_ids, alone.query_filtered_by(q, K, tau, iters, filter_ids=fids))
    assert same(by_ids_meanwhile, by_ids)
    alone = handle(load=True)
    assert same(by_label, alone.query_labeled(q, K, tau, iters, labels=qlabels))
    alone.set_return_results_on_gpu(True)
    on_gpu = alone.query_labeled(d_q, K, tau, iters, labels=qlabels)
    assert ticket.ids.is_cuda and ticket.ids.shape == on_gpu[0].shape
    assert same((ticket.ids, ticket.dists), on_gpu)
    assert same(plain, plain_again)
    for filtered in (by_mask, by_ids, by_label):
        assert not same(plain, filtered)      # (or the above would hold vacuously)
