"""float16 / bfloat16 rows (GGNN_F16, GGNN_BF16) against the unchanged oracle on their float32 copy.

The 16-bit kernels widen every element exactly to float32 and then run the float32 arithmetic of
the float path (include/ggnn_c.h, ggnn_dtype).  The oracle has no 16-bit type: it is fed the
exactly widened float32 copy.  On integer data -- multiples of 5 in [0, 255] for D <= 256, in
[0, 15] above (15^2 * 4096 < 2^24) -- every value is exact in both 16-bit types and every float32
sum the kernels and the oracle form is exact, sym's half point included (0.4f * 5m rounds to 2m,
tests/test_gpu_build_parity.py), so results must match BIT FOR BIT in any summation order, the
reference's own included (the 16-bit layouts differ from the float32 ones: 8 elements per chunk).

Per (type, layout, measure) cell: query (with counters, at the two points of
test_gpu_layout_matrix.POINTS), top on layers 0 and 1, merge (3, 0) and (2, 1), serial sym, the bf
scan, and the matrix-core bf path equal to the scan.  The float32 kernels on the widened copy give
identical outputs.  Then: the whole deterministic build, fractional data (tolerance track), and the
handle-level API (copy / reference bases, query_async, store / load, out-of-core, two contexts)."""
import os
import sys

import numpy as np
import pytest

from parity_helpers import RTOL, assert_rows_consistent, assert_topk_parity, cos_atol

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
# one D per layout of 16-bit rows (8 elements per chunk): {8,1} {8,2} {8,3} {16,2} {16,4} {64,4}
# {64,16}; read as data by tests/test_half_dtypes.py
HALF_DIMS = (48, 128, 192, 256, 384, 1024, 4096)
MATRIX = [(t, D, m) for t in TYPES for D in HALF_DIMS for m in (0, 1)]
IDS = [f"{t}-D{D}-{'cos' if m else 'l2'}" for t, D, m in MATRIX]

KB = 24
N_GRAPH = 1100
POINTS = ((10, 0.6, 200), (10, 3.0, 255))   # = test_gpu_layout_matrix.POINTS


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def int_data(N, D, seed):
    """float32 integers exact in float16 and bfloat16, with exact float32 sums"""
    hi = 52 if D <= 256 else 4
    return (np.random.default_rng(seed).integers(0, hi, (N, D)) * 5).astype(np.float32)


def half(a, t):
    """device tensor of a float32 array converted to the 16-bit type `t`"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(TYPES[t]).cuda()


def widened(x):
    """the exact float32 copy of a 16-bit tensor, on the host"""
    return x.float().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def np_(*ts):
    return [t.cpu().numpy() for t in ts]


_graphs = {}


def graph_for(orc, D, measure):
    key = (D, measure)
    if key not in _graphs:
        N = N_GRAPH if D < 1024 else 700
        base = int_data(N, D, 500 + D)
        cfg, graph, tr, sel, stats = orc.build(base, KB, 0.5, 0, measure=measure,
                                               rng=orc.make_rng(N, 11))
        _graphs[key] = dict(N=N, D=D, base=base, cfg=cfg, graph=graph, tr=tr, sel=sel, stats=stats)
    return _graphs[key]


def run_traversal_ops(ops, b, g, q, measure):
    """query at both points, top on layers 0/1, merge (3,0) / (2,1) on base tensor b"""
    c = g["cfg"]
    graph0 = dev(g["graph"][:g["N"]])
    start = dev(g["tr"][c.STs_offsets[3]:c.STs_offsets[3] + c.Ns[3]])
    out = []
    for K, tau, iters in POINTS:
        res = np_(*ops.query(b, q, graph0, start, dev(g["stats"]), K, tau, iters, measure,
                             counters=True))
        out.append(("query", K, tau, iters, [res[0], res[1]] + [x.astype(np.uint32) for x in res[2:]]))
    for layer in (0, 1):
        tr_l = None if layer == 0 else dev(g["tr"][c.STs_offsets[layer]:c.STs_offsets[layer] + c.Ns[layer]])
        S, S_off = (c.S0, c.S0_off) if layer == 0 else (c.S, 0)
        out.append(("top", layer, np_(*ops.top(b, KB, tr_l, c.Ns[layer], S, S_off, layer, measure))))
    for top, btm in ((3, 0), (2, 1)):
        gb, nn1, nd = np_(*ops.merge(b, c, dev(g["graph"]), dev(g["tr"]), dev(g["sel"]),
                                     dev(g["stats"]), 0.5, top, btm, measure, counters=True))
        out.append(("merge", top, btm, [gb, nn1 if btm == 0 else None, nd.astype(np.uint32)]))
    return out


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------
# every (type, layout, measure) cell: traversal and construction kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,D,measure", MATRIX, ids=IDS)
def test_half_query_top_merge(ops, orc, t, D, measure):
    g = graph_for(orc, D, measure)
    c, base = g["cfg"], g["base"]
    q = int_data(48, D, 900 + D)
    b16, q16 = half(base, t), half(q, t)
    assert np.array_equal(widened(b16), base) and np.array_equal(widened(q16), q), "exact data"
    mine = run_traversal_ops(ops, b16, g, q16, measure)
    # the float32 kernels on the widened copy: identical outputs
    f32 = run_traversal_ops(ops, dev(base), g, dev(q), measure)
    for a, b in zip(mine, f32):
        assert same(a[-1], b[-1]), ("16-bit != float32 kernels", t, D, measure, a[:-1])
    # the oracle in the reference's own order
    graph0 = g["graph"][:g["N"]]
    start = g["tr"][c.STs_offsets[3]:c.STs_offsets[3] + c.Ns[3]]
    for (_, K, tau, iters, res) in mine[:2]:
        o = orc.query(base, q, graph0, start, g["stats"], K, tau, iters, measure, counters=True)
        for x, y, name in zip(res, o, ("ids", "dists", "n_dist", "n_pop")):
            assert np.array_equal(x, y), (t, D, measure, tau, iters, name)
        assert_rows_consistent(base, q, res[0], res[1], measure, (t, D, measure, tau, iters))
        if iters == 255:
            assert int(o[3].max()) > 192 + 16, "the case is meant to wrap the visited ring"
    for (_, layer, (gr, nn1)) in mine[2:4]:
        tr_l = None if layer == 0 else g["tr"][c.STs_offsets[layer]:c.STs_offsets[layer] + c.Ns[layer]]
        S, S_off = (c.S0, c.S0_off) if layer == 0 else (c.S, 0)
        o_gr, o_nn1 = orc.top(base, KB, tr_l, c.Ns[layer], S, S_off, layer, measure)
        assert np.array_equal(gr, o_gr) and np.array_equal(nn1, o_nn1), ("top", t, layer)
    for (_, top, btm, (gb, nn1, nd)) in mine[4:]:
        o_gb, o_nn1, o_nd = orc.merge(base, c, g["graph"], g["tr"], g["sel"], g["stats"], 0.5,
                                      top, btm, measure, counters=True)
        assert np.array_equal(gb, o_gb), ("merge", t, top, btm)
        assert np.array_equal(nd, o_nd), ("merge n_dist", t, top, btm)
        if btm == 0:
            assert np.array_equal(nn1, o_nn1), ("merge nn1", t, top, btm)


def serial_sym(ops, b, g, measure, Nl):
    c = g["cfg"]
    sb = torch.full((c.N, KB // 2), -1, dtype=torch.int32, device="cuda")
    sa = torch.zeros(c.N, dtype=torch.int32, device="cuda")
    gr, st = dev(g["graph"][:c.N].copy()), dev(g["stats"])
    for n in range(Nl):
        ops.sym(b, KB, gr, None, st, 0.5, sb, sa, measure, first_n=n, count=1)
    return sb.cpu().numpy(), sa.cpu().numpy().astype(np.uint32)


@pytest.mark.parametrize("t,D,measure", MATRIX, ids=IDS)
def test_half_sym(ops, orc, t, D, measure):
    g = graph_for(orc, D, measure)
    c, Nl = g["cfg"], 150
    sb, sa = serial_sym(ops, half(g["base"], t), g, measure, Nl)
    o_sb = np.full((c.N, KB // 2), -1, np.int32)
    o_sa = np.zeros(c.N, np.uint32)
    orc.sym(g["base"], KB, g["graph"][:c.N].copy(), None, g["stats"], 0.5, o_sb, o_sa, first_n=0,
            count=Nl, measure=measure)
    assert np.array_equal(sb, o_sb) and np.array_equal(sa, o_sa), "reference order"
    assert int(sa.sum()) > 0, "some inverse links are requested at all"


# ---------------------------------------------------------------------------------------------
# brute force: scan kernel and matrix-core path
# ---------------------------------------------------------------------------------------------
def scan_answer(ops, b, q, K, measure):
    """the scan kernel (batches of < 256 queries never take the matrix-core path)"""
    ids, dists = [], []
    for i in range(0, q.shape[0], 128):
        a, d = ops.bf_query(b, q[i:i + 128].contiguous(), K, measure)
        ids.append(a)
        dists.append(d)
    return torch.cat(ids).cpu().numpy(), torch.cat(dists).cpu().numpy()


@pytest.mark.parametrize("t,D,measure", MATRIX, ids=IDS)
def test_half_bf(ops, orc, t, D, measure):
    N, Nq, K = (4096 if D == 4096 else 5000), 256, 10
    base, q = int_data(N, D, 700 + D), int_data(Nq, D, 800 + D)
    b, qq = half(base, t), half(q, t)
    s_ids, s_d = scan_answer(ops, b, qq, K, measure)
    m_ids, m_d, rescanned = ops.bf_query(b, qq, K, measure, rescanned=True)
    m_ids, m_d = m_ids.cpu().numpy(), m_d.cpu().numpy()
    print(f"bf matrix path {t} D={D} {'cosine' if measure else 'L2'}: "
          f"{rescanned} of {Nq} queries rescanned")
    assert np.array_equal(m_ids, s_ids) and np.array_equal(m_d, s_d), "matrix path != scan"
    sub = slice(0, 64)
    r_ids, r_d = orc.bf_query(base, q[sub], K, measure)
    assert np.array_equal(s_ids[sub], r_ids) and np.array_equal(s_d[sub], r_d), "reference order"
    f_ids, f_d = scan_answer(ops, dev(base), dev(q), K, measure)
    assert np.array_equal(s_ids, f_ids) and np.array_equal(s_d, f_d), "16-bit != float32 scan"
    assert_topk_parity(base, q, m_ids, m_d, s_ids, K, measure, "matrix path")


# ---------------------------------------------------------------------------------------------
# whole build: deterministic schedule against orc.build on the float32 copy
# ---------------------------------------------------------------------------------------------
def mult5_data(N, D, seed):
    """multiples of 5 in [0, 255]: exact in both 16-bit types, and sym's half point is exact too
    (see tests/test_gpu_build_parity.py)"""
    return (np.random.default_rng(seed).integers(0, 52, (N, D)) * 5).astype(np.float32)


def graph_arrays(eng, K):
    g = eng.get_graph(0)
    graph = np.concatenate([g.graph[l].view.numpy().reshape(-1, K) for l in range(4)])
    tr = np.concatenate([g.translation[l].view.numpy().reshape(-1) for l in range(1, 4)])
    sel = np.concatenate([g.selection[l].view.numpy().reshape(-1) for l in range(1, 4)])
    return g.config, graph, tr, sel, g.nn1_stats.view.numpy().reshape(-1).copy()


@pytest.mark.parametrize("t,D,N,refine", [("f16", 128, 6000, 1), ("bf16", 96, 7777, 2)])
def test_half_build_bit_exact(orc, t, D, N, refine):
    import ggnn_amd as ggnn
    K = 24
    base = mult5_data(N, D, 1357 + D)
    rng = orc.make_rng(N, 19)
    o_cfg, o_graph, o_tr, o_sel, o_stats = orc.build(base, K, 0.5, refine, rng=rng)
    eng = ggnn.GGNN()
    eng.set_base(torch.from_numpy(base).to(TYPES[t]))
    eng.set_build_hooks(rng[:3], serial_sym=True)
    eng.build(K, 0.5, refine)
    cfg, graph, tr, sel, stats = graph_arrays(eng, K)
    assert cfg["Ns"] == list(o_cfg.Ns) and cfg["G"] == o_cfg.G and cfg["SG"] == o_cfg.SG
    assert stats.tobytes() == o_stats.tobytes(), (stats, o_stats)
    assert np.array_equal(tr, o_tr[:tr.size]), "translation differs"
    assert np.array_equal(sel, o_sel[:sel.size]), "selection differs"
    for l in range(4):
        a, b = o_cfg.Ns_offsets[l], o_cfg.Ns_offsets[l] + o_cfg.Ns[l]
        bad = np.nonzero((graph[a:b] != o_graph[a:b]).any(1))[0]
        assert bad.size == 0, f"layer {l}: {bad.size} of {b - a} rows differ, first {bad[:5]}"


# ---------------------------------------------------------------------------------------------
# fractional data: the 16-bit values are rounded, the widened copy is what the oracle sees
# ---------------------------------------------------------------------------------------------
def fractional(t, N, D, seed):
    r = np.random.default_rng(seed)
    a = r.standard_normal((N, D)) if t == "f16" else r.random((N, D))
    return torch.from_numpy(a.astype(np.float32)).to(TYPES[t])


@pytest.mark.parametrize("t", list(TYPES))
@pytest.mark.parametrize("measure", [0, 1])
def test_half_fractional_query_and_bf(ops, orc, t, measure):
    N, D, K = 3000, 128, 10
    b16 = fractional(t, N, D, 61)
    q16 = fractional(t, 300, D, 62)
    base, q = widened(b16), widened(q16)
    cfg, graph, tr, sel, stats = orc.build(base, KB, 0.5, 1, measure=measure,
                                           rng=orc.make_rng(N, 23))
    start = tr[cfg.STs_offsets[3]:cfg.STs_offsets[3] + cfg.Ns[3]]
    ids, d = np_(*ops.query(b16.cuda(), q16.cuda(), dev(graph[:N]), dev(start), dev(stats), K, 0.6,
                            300, measure))
    o_ids, o_d = orc.query(base, q, graph[:N], start, stats, K, 0.6, 300, measure)
    atol = cos_atol(D) if measure else 0.0
    shared = 0
    for r in range(q.shape[0]):
        theirs = dict(zip(o_ids[r].tolist(), o_d[r].tolist()))
        for i, x in zip(ids[r].tolist(), d[r].tolist()):
            if i in theirs:
                shared += 1
                assert abs(x - theirs[i]) <= RTOL * abs(theirs[i]) + atol, (r, i)
    assert shared >= 0.95 * ids.size, (shared, ids.size)
    assert_rows_consistent(base, q, ids, d, measure, (t, "query"))
    # bf: exact against float64 up to near-ties (tests/test_gpu_bf_exact.py)
    bf_ids, bf_d = np_(*ops.bf_query(b16.cuda(), q16.cuda(), K, measure))
    ob_ids, _ = orc.bf_query(base, q, K, measure)
    assert_topk_parity(base, q, bf_ids, bf_d, ob_ids, K, measure, (t, "bf"))


def test_bf16_cosine_zero_rows_and_zero_query(ops):
    N, D, K = 5000, 128, 10
    r = np.random.default_rng(71)
    base = r.random((N, D)).astype(np.float32)
    base[[3, 70, 1234]] = 0.0
    q = r.random((256, D)).astype(np.float32)
    q[0] = 0.0
    b, qq = half(base, "bf16"), half(q, "bf16")
    for ids, d in (scan_answer(ops, b, qq, K, 1), np_(*ops.bf_query(b, qq, K, 1))):
        # the zero query: every row at exactly 1.0, the lowest indices first
        assert np.all(d[0] == np.float32(1.0)) and np.array_equal(ids[0], np.arange(K))
        # non-negative data: every other pair is below 1.0, so no zero row (1.0) is returned
        assert np.all(d[1:] < 1.0) and not np.isin(ids[1:], [3, 70, 1234]).any()
    zq = half(np.zeros((1, D), np.float32), "bf16")
    ids, d = np_(*ops.bf_query(b[[3, 70, 1234]].contiguous(), zq, 3, 1))
    assert np.all(d == np.float32(1.0)) and np.array_equal(ids[0], [0, 1, 2])


# ---------------------------------------------------------------------------------------------
# handle level
# ---------------------------------------------------------------------------------------------
def recall(a, b):
    return np.mean([len(set(x) & set(y)) / len(y) for x, y in zip(a, b)])


@pytest.mark.parametrize("t", list(TYPES))
def test_half_handle_api(orc, t, tmp_path):
    import ggnn_amd as ggnn
    N, D, K = 8000, 64, 10
    base32, q32 = int_data(N, D, 171), int_data(700, D, 172)
    base, q = torch.from_numpy(base32).to(TYPES[t]), torch.from_numpy(q32).to(TYPES[t])
    rng = orc.make_rng(4000, 3)[:3]
    results = []
    for where in ("cpu", "gpu"):
        eng = ggnn.GGNN()
        if where == "cpu":
            eng.set_base(base)
        else:
            eng.set_base_reference(base.cuda())
        eng.set_working_directory(str(tmp_path))
        eng.set_shard_size(4000)
        eng.set_build_hooks(rng, serial_sym=True)
        eng.build(24, 0.5, 1)
        results.append(eng.query(q, K, 0.7, 200))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    ids, d = results[0]
    assert d.dtype == torch.float32 and ids.dtype == torch.int32
    # float32 handle on the widened copy, same deterministic build: same results
    f = ggnn.GGNN()
    f.set_base(base32)
    f.set_shard_size(4000)
    f.set_build_hooks(rng, serial_sym=True)
    f.build(24, 0.5, 1)
    f_ids, f_d = f.query(q32, K, 0.7, 200)
    assert torch.equal(ids, f_ids) and torch.equal(d, f_d)
    gt, gd = eng.bf_query(q, K)
    o_ids, o_d = orc.bf_query(base32, q32, K)
    assert np.array_equal(gt.numpy(), o_ids) and np.array_equal(gd.numpy(), o_d)
    assert recall(ids.numpy(), o_ids) > 0.9
    # query_async on two slots equals the blocking query
    eng.set_return_results_on_gpu(True)
    qd, qd2 = q.cuda(), q.flip(0).contiguous().cuda()
    ref, ref2 = eng.query(qd, K, 0.7, 200), eng.query(qd2, K, 0.7, 200)
    outs = [eng.query_async(qd if i % 2 == 0 else qd2, K, 0.7, 200, slot=i % 2) for i in range(4)]
    eng.synchronize()
    for i, (a, b) in enumerate(outs):
        want = ref if i % 2 == 0 else ref2
        assert torch.equal(a, want[0]) and torch.equal(b, want[1])
    # store / load
    eng.store()
    e2 = ggnn.GGNN()
    e2.set_base(base)
    e2.set_working_directory(str(tmp_path))
    e2.set_shard_size(4000)
    e2.load(24)
    l_ids, l_d = e2.query(q, K, 0.7, 200)
    assert torch.equal(l_ids, ids) and torch.equal(l_d, d)


@pytest.mark.parametrize("t", list(TYPES))
def test_half_out_of_core_equals_resident(orc, t):
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    N, D, K, NS = 12000, 64, 24, 3000
    base = torch.from_numpy(mult5_data(N, D, 901)).to(TYPES[t])
    q = torch.from_numpy(mult5_data(300, D, 902)).to(TYPES[t])
    rng = orc.make_rng(NS, 5)[:3]

    def build(slots):
        eng = ggnn.GGNN()
        eng.set_base(base)
        eng.set_shard_size(NS)
        eng.set_build_hooks(rng, serial_sym=True)
        with _lib.hooks(RESIDENT_SHARDS=slots):
            eng.build(K, 0.5, 1)
        return eng

    ref, ooc = build(0), build(2)
    for s in range(4):
        a, b = ref.get_graph(s), ooc.get_graph(s)
        for l in range(4):
            assert np.array_equal(a.graph[l].view.numpy(), b.graph[l].view.numpy()), (s, l)
    for nq in (300, 1):
        r, o = ref.query(q[:nq], 10, 0.7, 200), ooc.query(q[:nq], 10, 0.7, 200)
        assert torch.equal(r[0], o[0]) and torch.equal(r[1], o[1])
    rb, ob = ref.bf_query(q, 10), ooc.bf_query(q, 10)
    assert torch.equal(rb[0], ob[0]) and torch.equal(rb[1], ob[1])


@pytest.mark.parametrize("t", list(TYPES))
def test_half_two_contexts_equal_one(orc, t):
    import ggnn_amd as ggnn
    N, D, K, NS = 8000, 64, 10, 2000
    base = torch.from_numpy(mult5_data(N, D, 87)).to(TYPES[t])
    q = torch.from_numpy(mult5_data(120, D, 88)).to(TYPES[t])
    rng = orc.make_rng(NS, 9)[:3]
    out = []
    for gpus in ([0, 0], [0]):
        eng = ggnn.GGNN()
        eng.set_base(base)
        eng.set_gpus(gpus)
        eng.set_shard_size(NS)
        eng.set_build_hooks(rng, serial_sym=True)
        eng.build(24, 0.5, 1)
        out.append(eng.query(q, K, 0.7, 400))
    (i2, d2), (i1, d1) = out
    assert torch.equal(d2, d1)
    d = d1.numpy()
    uniq = np.ones_like(d, bool)   # ids of tied distances may come in either order
    uniq[:, 1:] &= d[:, 1:] != d[:, :-1]
    uniq[:, :-1] &= d[:, :-1] != d[:, 1:]
    assert np.array_equal(i2.numpy()[uniq], i1.numpy()[uniq])


def test_half_recall_matches_float32_path():
    """200k x 128 lowrank base (bench.synthetic), one fixed point: recall@10 of each 16-bit build
    within 0.005 of the float32 path on the widened copy (ground truth: each base's own bf_query)"""
    import bench
    import ggnn_amd as ggnn
    base32 = bench.synthetic("lowrank16", 200_000, 128, 5, "cuda").cpu().numpy()
    q32 = bench.synthetic("lowrank16", 2000, 128, 6, "cuda").cpu().numpy()
    rec = {}
    for t in ("f32", "f16", "bf16"):
        b = torch.from_numpy(np.ascontiguousarray(base32))
        q = torch.from_numpy(np.ascontiguousarray(q32))
        if t != "f32":
            b, q = b.to(TYPES[t]), q.to(TYPES[t])
        eng = ggnn.GGNN()
        eng.set_base(b)
        eng.build(24, 0.5, 2)
        ids, _ = eng.query(q, 10, 0.64, 400)
        gt, _ = eng.bf_query(q, 10)
        rec[t] = recall(ids.numpy(), gt.numpy())
    print("recall@10", rec)
    assert abs(rec["f16"] - rec["f32"]) <= 0.005 and abs(rec["bf16"] - rec["f32"]) <= 0.005, rec
