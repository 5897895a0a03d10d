"""The reference's stated limits, executed (round-4 verdict: "claimed in DESIGN 6, never run"):
  * KQuery up to 6000 and max_iterations up to 8192 -- the largest cache the reference sizes,
    8192 keys (query_kernels.cu:66-110; README.md:138-140),
  * D = 4096, the widest row (`<.,64,16>` float layout, `<.,64,4>` for uint8): query, top, merge,
    sym and both brute-force paths.
Everything is compared with the oracle bit for bit (ids, distances, n_dist / n_pop), through the
operator seam of the C-ABI (ggnn_op_*)."""
import numpy as np
import pytest

from parity_helpers import assert_rows_consistent

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def start_points(g):
    c = g["cfg"]
    return g["tr"][c.STs_offsets[3]:c.STs_offsets[3] + c.Ns[3]]


@pytest.fixture(scope="module")
def wide_graph(orc):
    """10 000 points so that searches of 4096 / 8192 iterations really pop that often"""
    N, D, K = 10000, 32, 24
    base = np.random.default_rng(2001).integers(0, 256, (N, D)).astype(np.float32)
    cfg, graph, tr, sel, stats = orc.build(base, K, 0.5, 0, rng=orc.make_rng(N, 3))
    return dict(N=N, D=D, K=K, base=base, cfg=cfg, graph=graph, tr=tr, sel=sel, stats=stats)


def _query_vs_oracle(ops, orc, g, q, K, tau, iters, prescreen=False):
    graph0 = g["graph"][:g["N"]]
    b = dev(g["base"])
    ids, d, nd, npop = ops.query(b, dev(q), dev(graph0), dev(start_points(g)), dev(g["stats"]), K,
                                 tau, iters, counters=True,
                                 prescreen=ops.prescreen_encode(b) if prescreen else None)
    o_ids, o_d, o_nd, o_np = orc.query(g["base"], q, graph0, start_points(g), g["stats"], K, tau,
                                       iters, counters=True)
    assert np.array_equal(ids.cpu().numpy(), o_ids)
    assert np.array_equal(d.cpu().numpy(), o_d)
    assert np.array_equal(npop.cpu().numpy().astype(np.uint32), o_np)
    assert np.array_equal(nd.cpu().numpy().astype(np.uint32), o_nd)
    return o_np


@pytest.mark.parametrize("tau,iters", [(8.0, 4096), (12.0, 8192), (12.0, 8191), (6.0, 2049)])
def test_query_max_iterations_up_to_8192(ops, orc, wide_graph, tau, iters):
    """caches of 4096 / 8192 keys (visited rings of 4064 / 8160): beyond the tag set's 2016 keys the
    ring is scanned in LDS (query_kernels.cu:98-110: cache = bit_ceil(max_iterations))"""
    sz = orc.query_sizing(wide_graph["D"], 10, iters)
    assert sz.cache_size == (8192 if iters > 4096 else 4096) and sz.sorted_size == 32
    q = np.random.default_rng(2002).integers(0, 256, (6, wide_graph["D"])).astype(np.float32)
    pops = _query_vs_oracle(ops, orc, wide_graph, q, 10, tau, iters)
    assert int(pops.min()) > 0.9 * iters, "the case is meant to run (nearly) all its iterations"


@pytest.mark.parametrize("K,iters", [(3000, 4096), (6000, 8192), (5999, 6000), (2048, 4096)])
def test_query_kquery_up_to_6000(ops, orc, wide_graph, K, iters):
    """KQuery 2048..6000: the LDS-resident list (sorted part up to 6048 entries in a cache of 8192:
    57 KB of LDS); K = 6000 / 8192 iterations is the largest case the reference allows
    (query_kernels.cu:66-75)"""
    sz = orc.query_sizing(wide_graph["D"], K, iters)
    assert sz.cache_size <= 8192 and sz.sorted_size >= K + 17
    q = np.random.default_rng(2003).integers(0, 256, (4, wide_graph["D"])).astype(np.float32)
    _query_vs_oracle(ops, orc, wide_graph, q, K, 1.0, iters)


def test_limits_are_enforced(ops, wide_graph):
    """one past each limit fails loudly (GGNN_INVALID_ARGUMENT), like the reference's checks"""
    g = wide_graph
    q = dev(g["base"][:2])
    args = (dev(g["base"]), q, dev(g["graph"][:g["N"]]), dev(start_points(g)), dev(g["stats"]))
    with pytest.raises(Exception, match="KQuery"):
        ops.query(*args, 6001, 1.0, 8192)
    with pytest.raises(Exception, match="max_iterations"):
        ops.query(*args, 10, 1.0, 8193)


# ---- D = 4096 ------------------------------------------------------------------------------------
# small integer values: every squared distance stays below 2^24 (225 x 4096), so float sums are exact
# in any order and L2 results can be compared bit for bit; cosine runs the oracle in the kernels'
# summation order (orc.wave_order)
def _small_ints(dtype, N, D, seed):
    a = np.random.default_rng(seed).integers(0, 16, (N, D))
    return a.astype(np.uint8) if dtype == "u8" else a.astype(np.float32)


_graphs = {}


def _graph4096(orc, dtype, measure):
    key = (dtype, measure)
    if key not in _graphs:
        N, D, K = 700, 4096, 24
        base = _small_ints(dtype, N, D, 3001)
        cfg, graph, tr, sel, stats = orc.build(base, K, 0.5, 0, measure=measure,
                                               rng=orc.make_rng(N, 11))
        _graphs[key] = dict(N=N, D=D, K=K, base=base, cfg=cfg, graph=graph, tr=tr, sel=sel,
                            stats=stats)
    return _graphs[key]


@pytest.mark.parametrize("dtype,measure,ps", [("f32", 0, False), ("f32", 0, True), ("f32", 1, False),
                                              ("f32", 1, True), ("u8", 0, False)])
def test_d4096_query_top_merge(ops, orc, dtype, measure, ps):
    g = _graph4096(orc, dtype, measure)
    c, K = g["cfg"], g["K"]
    q = _small_ints(dtype, 40, g["D"], 3002)
    graph0 = g["graph"][:g["N"]]
    d_base = dev(g["base"])
    codes = ops.prescreen_encode(d_base, measure) if ps else None
    orc.set_wave_order(measure == 1)
    try:
        ids, d, nd, npop = ops.query(d_base, dev(q), dev(graph0), dev(start_points(g)),
                                     dev(g["stats"]), 10, 0.7, 300, measure, counters=True,
                                     prescreen=codes)
        o_ids, o_d, o_nd, o_np = orc.query(g["base"], q, graph0, start_points(g), g["stats"], 10,
                                           0.7, 300, measure, counters=True)
        assert np.array_equal(ids.cpu().numpy(), o_ids) and np.array_equal(d.cpu().numpy(), o_d)
        assert_rows_consistent(g["base"], q, ids.cpu().numpy(), d.cpu().numpy(), measure)
        assert np.array_equal(nd.cpu().numpy().astype(np.uint32), o_nd)
        assert np.array_equal(npop.cpu().numpy().astype(np.uint32), o_np)
        if ps:
            return   # (top has no pre-screen; merge with it is covered by the plain comparison below)
        for layer in (0, 1):
            tr_l = None if layer == 0 else g["tr"][c.STs_offsets[layer]:c.STs_offsets[layer] + c.Ns[layer]]
            S, S_off = (c.S0, c.S0_off) if layer == 0 else (c.S, 0)
            gr, nn1 = ops.top(d_base, K, None if tr_l is None else dev(tr_l), c.Ns[layer], S, S_off,
                              layer, measure)
            o_gr, o_nn1 = orc.top(g["base"], K, tr_l, c.Ns[layer], S, S_off, layer, measure)
            assert np.array_equal(gr.cpu().numpy(), o_gr) and np.array_equal(nn1.cpu().numpy(), o_nn1)
        for top, btm in ((3, 0), (2, 1)):
            gb, nn1 = ops.merge(d_base, c, dev(g["graph"]), dev(g["tr"]), dev(g["sel"]),
                                dev(g["stats"]), 0.5, top, btm, measure)
            o_gb, o_nn1 = orc.merge(g["base"], c, g["graph"], g["tr"], g["sel"], g["stats"], 0.5,
                                    top, btm, measure)
            assert np.array_equal(gb.cpu().numpy(), o_gb)
            if btm == 0:
                assert np.array_equal(nn1.cpu().numpy(), o_nn1)
    finally:
        orc.set_wave_order(False)


@pytest.mark.parametrize("dtype,measure", [("f32", 0), ("f32", 1), ("u8", 0)])
def test_d4096_sym(ops, orc, dtype, measure):
    """sym launched one point at a time in ascending order (the oracle's serialisation); cosine in
    the kernels' summation order, L2 with a decision margin on the inexact half-point distance"""
    g = _graph4096(orc, dtype, measure)
    c, K = g["cfg"], g["K"]
    KF, Nl = K // 2, 100
    graph_l = g["graph"][:c.N].copy()
    sb = np.full((c.N, KF), -1, np.int32)
    sa = np.zeros(c.N, np.uint32)
    orc.margin_reset()
    orc.set_wave_order(measure == 1)
    orc.sym(g["base"], K, graph_l, None, g["stats"], 0.5, sb, sa, first_n=0, count=Nl,
            measure=measure)
    orc.set_wave_order(False)
    if measure == 0:
        assert orc.margin_min() > 1e-5, "a half-point decision of this case hinges on a rounding"
    d_sb = torch.full((c.N, KF), -1, dtype=torch.int32, device="cuda")
    d_sa = torch.zeros(c.N, dtype=torch.int32, device="cuda")
    d_base, d_graph, d_stats = dev(g["base"]), dev(graph_l), dev(g["stats"])
    for n in range(Nl):
        ops.sym(d_base, K, d_graph, None, d_stats, 0.5, d_sb, d_sa, measure, first_n=n, count=1)
    assert np.array_equal(d_sa.cpu().numpy().astype(np.uint32), sa)
    assert np.array_equal(d_sb.cpu().numpy(), sb)


@pytest.mark.parametrize("dtype,N,Nq,K", [("f32", 3000, 300, 10), ("f32", 2000, 40, 10),
                                          ("u8", 3000, 256, 10), ("f32", 2500, 260, 100)])
def test_d4096_bf_query(ops, orc, dtype, N, Nq, K):
    """both brute-force paths at D = 4096: the matrix-core kernels (>= 256 queries: 32 chunks of
    128 columns) and the scan kernel"""
    base, q = _small_ints(dtype, N, 4096, 3003), _small_ints(dtype, Nq, 4096, 3004)
    ids, d = ops.bf_query(dev(base), dev(q), K)
    o_ids, o_d = orc.bf_query(base, q, K)
    assert np.array_equal(ids.cpu().numpy(), o_ids)
    assert np.array_equal(d.cpu().numpy(), o_d)
