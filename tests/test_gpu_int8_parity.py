"""int8 rows (GGNN_I8) against two yardsticks, neither of which is the code under test.

A. The uint8 kernels on `x ^ 0x80` (squared L2 only, full range -128..127).  x ^ 0x80 read as uint8
   is x + 128: every difference o - q is unchanged, so every output of an int8 op -- ids, distance
   bits, n_dist, n_pop, graphs -- must equal the output of the same op on the biased uint8 tensors.
   The uint8 kernels are pinned to the oracle by the existing suite.
B. The unchanged oracle on the float32 copy (both measures).  The oracle has no int8 type.  Values
   are chosen so that every float32 sum it forms is an exact integer below 2^24 (at most 2^24 under
   cosine), hence the same in any summation order, the reference's own included:
     squared L2   full range for D <= 256 (255^2 * 256 < 2^24), [-64, 63] for D <= 1024,
                  [-32, 31] at D = 4096
     cosine       full range for D <= 1024 (128^2 * 1024 = 2^24, still exact), [-32, 31] at 4096
     sym, builds  signed multiples of 5 (sym's half point stays exact: 0.4f * 5m rounds to 2m,
                  tests/test_gpu_build_parity.py): 5 * [-25, 25] for D <= 256, 5 * [-3, 3] above
   `assert_exact` checks these preconditions on the data of every case.

Per (D, measure) cell: query with counters at the two points of test_gpu_half_parity.POINTS, top on
layers 0 and 1, merge (3, 0) and (2, 1) with counters, serial sym, the bf scan.  Then filtered and
labelled queries, the whole deterministic build, bf_query on the matrix cores (both integer kernels,
the f32-staged tile kernels), filtered brute force, and the handle-level API."""
import os
import sys

import numpy as np
import pytest

from parity_helpers import assert_rows_consistent

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# one D per layout of 8-bit rows (16 elements per chunk): {8,1} {8,2} {8,3} {16,2} {16,4} {64,4},
# and D = 48: three chunks in the {8,1} layout; read as data by tests/test_int8_dtypes.py
DIMS = (48, 128, 256, 384, 512, 1024, 4096)
MATRIX = [(D, m) for D in DIMS for m in (0, 1)]
IDS = [f"D{D}-{'cos' if m else 'l2'}" for D, m in MATRIX]

KB = 24
N_GRAPH = 1100
POINTS = ((10, 0.6, 200), (10, 3.0, 255))   # = test_gpu_half_parity.POINTS
THREADS = min(16, len(os.sched_getaffinity(0)))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def value_range(D, measure):
    """[lo, hi] of yardstick B for the per-cell matrix (module docstring)"""
    if measure == 0:
        return (-128, 127) if D <= 256 else (-64, 63) if D <= 1024 else (-32, 31)
    return (-128, 127) if D <= 1024 else (-32, 31)


def assert_exact(D, measure, *arrays):
    """the precondition of yardstick B: max |sum| < 2^24 (<= 2^24 under cosine, exact as well)"""
    lo = min(int(a.min()) for a in arrays)
    hi = max(int(a.max()) for a in arrays)
    if measure == 0:
        assert (hi - lo) ** 2 * D < 2 ** 24, (D, lo, hi)       # sums of squared differences
    else:
        assert max(-lo, hi) ** 2 * D <= 2 ** 24, (D, lo, hi)   # dot products and norms


def ranged(N, D, measure, seed):
    lo, hi = value_range(D, measure)
    a = np.random.default_rng(seed).integers(lo, hi + 1, (N, D)).astype(np.int8)
    a[1, 0], a[1, 1] = lo, hi
    return a


def full_range(N, D, seed):
    a = np.random.default_rng(seed).integers(-128, 128, (N, D)).astype(np.int8)
    a[1, 0], a[1, 1] = -128, 127
    return a


def mult5(N, D, seed):
    m = 25 if D <= 256 else 3
    return (np.random.default_rng(seed).integers(-m, m + 1, (N, D)) * 5).astype(np.int8)


def f32(a):
    return a.astype(np.float32)


def biased(a):
    """the uint8 rows of yardstick A"""
    return a.view(np.uint8) ^ np.uint8(0x80)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def np_(*ts):
    return [t.cpu().numpy() for t in ts]


_graphs = {}


def graph_for(orc, D, measure, kind="ranged"):
    """an oracle-built graph over the float32 copy of int8 data of the given kind"""
    key = (D, measure, kind)
    if key not in _graphs:
        N = N_GRAPH if D < 1024 else 700
        base8 = {"ranged": lambda: ranged(N, D, measure, 500 + D),
                 "full": lambda: full_range(N, D, 600 + D),
                 "mult5": lambda: mult5(N, D, 650 + D)}[kind]()
        if measure == 1 and kind == "ranged":
            base8[77] = 0                      # one all-zero row: distance 1 to everything
        base = f32(base8)
        cfg, graph, tr, sel, stats = orc.build(base, KB, 0.5, 0, measure=measure,
                                               rng=orc.make_rng(N, 11))
        _graphs[key] = dict(N=N, D=D, base8=base8, base=base, cfg=cfg, graph=graph, tr=tr, sel=sel,
                            stats=stats)
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


def same_bits(a, b):
    return all((x is None and y is None) or (x.shape == y.shape and x.tobytes() == y.tobytes())
               for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------
# every (layout, measure) cell: traversal and construction kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,measure", MATRIX, ids=IDS)
def test_int8_query_top_merge_against_the_oracle(ops, orc, D, measure):
    g = graph_for(orc, D, measure)
    c, base = g["cfg"], g["base"]
    q8 = ranged(48, D, measure, 900 + D)
    if measure == 1:
        q8[5] = 0                              # one all-zero query
    q = f32(q8)
    assert_exact(D, measure, g["base8"], q8)
    mine = run_traversal_ops(ops, dev(g["base8"]), g, dev(q8), measure)
    graph0 = g["graph"][:g["N"]]
    start = g["tr"][c.STs_offsets[3]:c.STs_offsets[3] + c.Ns[3]]
    for (_, K, tau, iters, res) in mine[:2]:
        o = orc.query(base, q, graph0, start, g["stats"], K, tau, iters, measure, counters=True)
        for x, y, name in zip(res, o, ("ids", "dists", "n_dist", "n_pop")):
            assert np.array_equal(x, y), (D, measure, tau, iters, name)
        assert res[1].tobytes() == o[1].tobytes(), (D, measure, tau, iters, "distance bits")
        assert_rows_consistent(base, q, res[0], res[1], measure, (D, measure, tau, iters))
        if iters == 255:
            assert int(o[3].max()) > 192 + 16, "the case is meant to wrap the visited ring"
        if measure == 1:
            assert np.all(res[1][5] == np.float32(1.0)), "the zero query is at 1.0 from every row"
    for (_, layer, (gr, nn1)) in mine[2:4]:
        tr_l = None if layer == 0 else g["tr"][c.STs_offsets[layer]:c.STs_offsets[layer] + c.Ns[layer]]
        S, S_off = (c.S0, c.S0_off) if layer == 0 else (c.S, 0)
        o_gr, o_nn1 = orc.top(base, KB, tr_l, c.Ns[layer], S, S_off, layer, measure)
        assert np.array_equal(gr, o_gr) and nn1.tobytes() == o_nn1.tobytes(), ("top", D, layer)
    for (_, top, btm, (gb, nn1, nd)) in mine[4:]:
        o_gb, o_nn1, o_nd = orc.merge(base, c, g["graph"], g["tr"], g["sel"], g["stats"], 0.5,
                                      top, btm, measure, counters=True)
        assert np.array_equal(gb, o_gb), ("merge", D, top, btm)
        assert np.array_equal(nd, o_nd), ("merge n_dist", D, top, btm)
        if btm == 0:
            assert nn1.tobytes() == o_nn1.tobytes(), ("merge nn1", D, top, btm)


@pytest.mark.parametrize("D", DIMS)
def test_int8_query_top_merge_equal_uint8_on_biased_rows(ops, orc, D):
    """yardstick A: squared L2, full-range data at every D.  The graph is the oracle's over the
    float32 copy (its sums may round at D > 256: it is only a graph, both sides traverse it)"""
    g = graph_for(orc, D, 0, "full")
    q8 = full_range(48, D, 950 + D)
    mine = run_traversal_ops(ops, dev(g["base8"]), g, dev(q8), 0)
    theirs = run_traversal_ops(ops, dev(biased(g["base8"])), g, dev(biased(q8)), 0)
    for a, b in zip(mine, theirs):
        assert same_bits(a[-1], b[-1]), ("int8 != uint8 on x ^ 0x80", D, a[:-1])


def serial_sym(ops, b, g, measure, Nl):
    c = g["cfg"]
    sb = torch.full((c.N, KB // 2), -1, dtype=torch.int32, device="cuda")
    sa = torch.zeros(c.N, dtype=torch.int32, device="cuda")
    gr, st = dev(g["graph"][:c.N].copy()), dev(g["stats"])
    for n in range(Nl):
        ops.sym(b, KB, gr, None, st, 0.5, sb, sa, measure, first_n=n, count=1)
    return sb.cpu().numpy(), sa.cpu().numpy().astype(np.uint32)


@pytest.mark.parametrize("D,measure", MATRIX, ids=IDS)
def test_int8_sym(ops, orc, D, measure):
    g = graph_for(orc, D, measure, "mult5")
    c, Nl = g["cfg"], 150
    assert_exact(D, measure, g["base8"])
    sb, sa = serial_sym(ops, dev(g["base8"]), g, measure, Nl)
    o_sb = np.full((c.N, KB // 2), -1, np.int32)
    o_sa = np.zeros(c.N, np.uint32)
    orc.sym(g["base"], KB, g["graph"][:c.N].copy(), None, g["stats"], 0.5, o_sb, o_sa, first_n=0,
            count=Nl, measure=measure)
    assert np.array_equal(sb, o_sb) and np.array_equal(sa, o_sa), "reference order"
    assert int(sa.sum()) > 0, "some inverse links are requested at all"
    if measure == 0:
        # yardstick A (a common shift moves the half point with the rows: multiples of 5 plus 128,
        # 0.4f * 5m is still exact)
        u_sb, u_sa = serial_sym(ops, dev(biased(g["base8"])), g, 0, Nl)
        assert np.array_equal(sb, u_sb) and np.array_equal(sa, u_sa), "int8 != uint8 on x ^ 0x80"


# ---------------------------------------------------------------------------------------------
# brute force: the scan kernel
# ---------------------------------------------------------------------------------------------
def scan_answer(ops, b, q, K, measure):
    """the scan kernel (batches of < 256 queries never take the matrix-core path)"""
    ids, dists = [], []
    for i in range(0, q.shape[0], 128):
        a, d = ops.bf_query(b, q[i:i + 128].contiguous(), K, measure)
        ids.append(a)
        dists.append(d)
    return torch.cat(ids).cpu().numpy(), torch.cat(dists).cpu().numpy()


@pytest.mark.parametrize("D,measure", MATRIX, ids=IDS)
def test_int8_bf_scan(ops, orc, D, measure):
    N, Nq, K = 3000, 64, 10
    base8, q8 = ranged(N, D, measure, 700 + D), ranged(Nq, D, measure, 800 + D)
    if measure == 1:
        base8[[3, 70, 1234]] = 0
        q8[0] = 0
    assert_exact(D, measure, base8, q8)
    s_ids, s_d = scan_answer(ops, dev(base8), dev(q8), K, measure)
    r_ids, r_d = orc.bf_query(f32(base8), f32(q8), K, measure)
    assert np.array_equal(s_ids, r_ids) and s_d.tobytes() == r_d.tobytes(), "reference order"
    assert_rows_consistent(f32(base8), f32(q8), s_ids, s_d, measure, ("bf scan", D, measure))
    if measure == 1:
        assert np.all(s_d[0] == np.float32(1.0)) and np.array_equal(s_ids[0], np.arange(K))
    else:
        fb, fq = full_range(N, D, 710 + D), full_range(Nq, D, 810 + D)
        a_ids, a_d = scan_answer(ops, dev(fb), dev(fq), K, 0)
        u_ids, u_d = scan_answer(ops, dev(biased(fb)), dev(biased(fq)), K, 0)
        assert np.array_equal(a_ids, u_ids) and a_d.tobytes() == u_d.tobytes(), "yardstick A"


# ---------------------------------------------------------------------------------------------
# filtered and labelled query: bitset, filter table, labels (tests/filtered_reference.py)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,measure", [(128, 0), (256, 1)], ids=["D128-l2", "D256-cos"])
@pytest.mark.parametrize("how", ["bitset", "table", "labels"])
def test_int8_filtered_query(ops, orc, how, D, measure):
    """the way of tests/test_gpu_filtered_layout_matrix.py: one label column, the table and the
    bitsets derived from it, one Python reference per query; label 4 admits six rows (< K), label
    7 none"""
    from filtered_reference import py_query_filtered
    from test_gpu_filtered_layout_matrix import (NQ, QLABELS, RARE, RARE_ROWS, UNUSED, Filters,
                                                 _stack, allowed_of, assert_query_equals)
    K, tau, iters = 10, 0.6, 200
    g = graph_for(orc, D, measure)
    c, base, N = g["cfg"], g["base"], g["N"]
    q8 = ranged(NQ, D, measure, 970 + D)
    assert_exact(D, measure, g["base8"], q8)
    rng = np.random.default_rng(31 + D)
    labels = rng.choice(4, N, p=[.5, .3, .15, .05]).astype(np.int32)
    labels[rng.choice(N, RARE_ROWS, replace=False)] = RARE
    assert int((labels == RARE).sum()) == RARE_ROWS and not (labels == UNUSED).any()
    graph0 = np.ascontiguousarray(g["graph"][:N])
    start = np.ascontiguousarray(g["tr"][c.STs_offsets[3]:c.STs_offsets[3] + c.Ns[3]])
    stats = np.asarray(g["stats"], np.float32)
    ref = _stack([py_query_filtered(base, f32(q8)[i], graph0, start, stats, K, tau, iters,
                                    allowed_of(labels, int(L)), cosine=bool(measure))
                  for i, L in enumerate(QLABELS)])
    # the reference itself: its unfiltered row is the oracle's search
    o = orc.query(base, f32(q8)[:1], graph0, start, stats, K, tau, iters, measure, counters=True)
    assert QLABELS[0] == -1 and np.array_equal(ref[0][:1], o[0]) and \
        ref[1][:1].tobytes() == o[1].tobytes()
    fin = np.isfinite(ref[1]).sum(1)
    assert 1 <= fin[list(QLABELS).index(RARE)] <= RARE_ROWS < K and fin[list(QLABELS).index(UNUSED)] == 0
    f = Filters(labels, 90 + D)
    head = (dev(g["base8"]), dev(q8), dev(graph0), dev(start), dev(stats), K, tau)
    every = np.arange(NQ)
    what = (how, D, measure)
    if how == "labels":
        assert_query_equals(ops.query_labeled(*head, f.labels, f.qlabels, iters, measure,
                                              counters=True), ref, every, what)
    elif how == "table":
        assert_query_equals(ops.query_filtered_by(*head, f.table, f.qlabels, iters, measure,
                                                  counters=True), ref, every, what)
    else:
        for L, (rows, bits) in f.by_label.items():
            sub = (head[0], head[1][torch.from_numpy(rows).cuda()].contiguous()) + head[2:]
            assert_query_equals(ops.query_filtered(*sub, bits, iters, measure, counters=True),
                                ref, rows, what + (L,))


# ---------------------------------------------------------------------------------------------
# whole deterministic build
# ---------------------------------------------------------------------------------------------
def graph_arrays(eng, K):
    g = eng.get_graph(0)
    graph = np.concatenate([g.graph[l].view.numpy().reshape(-1, K) for l in range(4)])
    tr = np.concatenate([g.translation[l].view.numpy().reshape(-1) for l in range(1, 4)])
    sel = np.concatenate([g.selection[l].view.numpy().reshape(-1) for l in range(1, 4)])
    return g.config, graph, tr, sel, g.nn1_stats.view.numpy().reshape(-1).copy()


def det_build(rows, rng, K=24, refine=1):
    import ggnn_amd as ggnn
    eng = ggnn.GGNN()
    eng.set_base(torch.from_numpy(rows))
    eng.set_build_hooks(rng[:3], deterministic_sym=True)
    eng.build(K, 0.5, refine)
    return graph_arrays(eng, K)


def test_int8_build_bit_exact(orc):
    N, D, K = 6000, 128, 24
    base8 = mult5(N, D, 1357)
    assert_exact(D, 0, base8)
    rng = orc.make_rng(N, 19)
    o_cfg, o_graph, o_tr, o_sel, o_stats = orc.build(f32(base8), K, 0.5, 1, rng=rng,
                                                     threads=THREADS, deterministic_sym=True)
    cfg, graph, tr, sel, stats = det_build(base8, rng)
    assert cfg["Ns"] == list(o_cfg.Ns) and cfg["G"] == o_cfg.G and cfg["SG"] == o_cfg.SG
    assert stats.tobytes() == o_stats.tobytes(), (stats, o_stats)
    assert np.array_equal(tr, o_tr[:tr.size]), "translation differs"
    assert np.array_equal(sel, o_sel[:sel.size]), "selection differs"
    for l in range(4):
        a, b = o_cfg.Ns_offsets[l], o_cfg.Ns_offsets[l] + o_cfg.Ns[l]
        bad = np.nonzero((graph[a:b] != o_graph[a:b]).any(1))[0]
        assert bad.size == 0, f"layer {l}: {bad.size} of {b - a} rows differ, first {bad[:5]}"


def test_int8_build_equals_uint8_build_on_biased_rows(orc):
    """yardstick A on a whole build, full-range data: graph, translation, selection and nn1
    statistics of the engine's own builds, bit for bit"""
    N, D = 6000, 128
    base8 = full_range(N, D, 2468)
    rng = orc.make_rng(N, 21)
    mine, theirs = det_build(base8, rng), det_build(biased(base8), rng)
    assert mine[0]["Ns"] == theirs[0]["Ns"]
    for a, b, name in zip(mine[1:], theirs[1:], ("graph", "translation", "selection", "nn1_stats")):
        assert a.tobytes() == b.tobytes(), name


# ---------------------------------------------------------------------------------------------
# bf_query on the matrix cores
# ---------------------------------------------------------------------------------------------
def tie_heavy(N, D, Nq, seed):
    """the data of test_uint8_register_list_kernel_exact in signed bytes"""
    rng = np.random.default_rng(seed)
    base = rng.integers(-128, 128, (N, D)).astype(np.int8)
    base[::97] = 127
    base[5::101] = -128
    base[N // 2:N // 2 + 400] = base[:400]          # ties across slices: lower index first
    base[N - 300:] = base[100:400]                  # ... and at the very end of the base
    q = rng.integers(-128, 128, (Nq, D)).astype(np.int8)
    q[3] = -128
    q[4] = 127
    q[5:205] = base[100:300]                        # exact hits with three copies each
    return base, q


def handle_bf(d_base, d_q, K, measure):
    """bf_query through a handle over the device rows: (ids, dists, matrix path, rescanned)"""
    import ggnn_amd as ggnn
    eng = ggnn.GGNN()
    eng.set_base_reference(d_base)
    eng.set_return_results_on_gpu(True)
    ids, d = eng.bf_query(d_q, K, ggnn.DistanceMeasure(measure))
    return (ids.cpu().numpy(), d.cpu().numpy(), eng.last_bf_query_matrix_path(),
            eng.last_bf_query_rescanned())


# k <= 16: bf_i8v2_kernel<.., SIGNED> (register sets); k > 16: bf_mfma_i8_kernel<.., SIGNED>
@pytest.mark.parametrize("N,D,Nq,K", [(50_000, 128, 700, 10), (20_001, 96, 300, 16),
                                      (4_100, 32, 256, 4), (9000, 128, 300, 24),
                                      (6000, 112, 300, 100), (5000, 64, 257, 17)])
def test_int8_integer_matrix_kernels(ops, N, D, Nq, K, monkeypatch):
    base, q = tie_heavy(N, D, Nq, N + D + K)
    d_base, d_q = dev(base), dev(q)
    s_ids, s_d = scan_answer(ops, d_base, d_q, K, 0)
    for env in ({}, {"GGNN_BF_SLICES": "7"}, {"GGNN_BF_SLICES": "1"}):
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        ids, d, rescanned = ops.bf_query(d_base, d_q, K, 0, rescanned=True)
        for k_ in env:
            monkeypatch.delenv(k_)
        assert rescanned == 0, (env, rescanned)
        assert np.array_equal(ids.cpu().numpy(), s_ids), env
        assert d.cpu().numpy().tobytes() == s_d.tobytes(), env
    u_ids, u_d = ops.bf_query(dev(biased(base)), dev(biased(q)), K, 0)
    assert np.array_equal(u_ids.cpu().numpy(), s_ids) and u_d.cpu().numpy().tobytes() == s_d.tobytes()
    # through the handle: the path and the re-scan count are reported
    h_ids, h_d, path, rescanned = handle_bf(d_base, d_q, K, 0)
    assert path == 1 and rescanned == 0, (path, rescanned)
    assert np.array_equal(h_ids, s_ids) and h_d.tobytes() == s_d.tobytes()


@pytest.mark.parametrize("D,measure", [(128, 1), (256, 0)], ids=["D128-cos", "D256-l2"])
def test_int8_tile_kernels_equal_the_scan(ops, D, measure):
    """cosine, and squared L2 beyond 128 bytes per row: the f32-staged tile kernels"""
    N, Nq, K = 5000, 300, 10
    base, q = full_range(N, D, 41 + D), full_range(Nq, D, 43 + D)
    if measure == 1:
        base[[3, 70, 1234]] = 0
        q[0] = 0
    assert_exact(D, measure, base, q)
    s_ids, s_d = scan_answer(ops, dev(base), dev(q), K, measure)
    ids, d, rescanned = ops.bf_query(dev(base), dev(q), K, measure, rescanned=True)
    assert 0 <= rescanned <= Nq, rescanned
    assert np.array_equal(ids.cpu().numpy(), s_ids) and d.cpu().numpy().tobytes() == s_d.tobytes()
    h_ids, h_d, path, h_rescanned = handle_bf(dev(base), dev(q), K, measure)
    assert path == 1 and h_rescanned == rescanned, (path, h_rescanned, rescanned)
    assert np.array_equal(h_ids, s_ids) and h_d.tobytes() == s_d.tobytes()


@pytest.mark.parametrize("how", ["bits", "labels"])
def test_int8_filtered_bf_at_matrix_shapes(ops, orc, how):
    """D = 256, 300 queries (the shapes of tests/test_gpu_bf_filtered_mfma.py) under a bitset and
    under labels, against the oracle on the compacted rows.  A filtered call on int8 rows keeps the
    exact scan (the filtered tile kernels exist for the four other element types only, DESIGN.md
    section 6): the call reports that path."""
    from filtered_reference import bf_filtered_reference, pack_bits
    N, D, Nq, K = 5000, 256, 300, 10
    base, q = full_range(N, D, 61), full_range(Nq, D, 62)
    assert_exact(D, 0, base, q)
    rng = np.random.default_rng(63)
    labels = rng.integers(0, 3, N).astype(np.int32)
    labels[rng.choice(N, 6, replace=False)] = 5          # a class of six rows: fewer than K
    qlabels = rng.integers(0, 3, Nq).astype(np.int32)
    qlabels[:4] = (5, -1, 7, 5)                          # 7: no row
    d_base, d_q = dev(base), dev(q)
    if how == "labels":
        def call():
            return ops.bf_query_labeled(d_base, d_q, K, dev(labels), dev(qlabels), 0,
                                        rescanned=True)
        r_ids = np.empty((Nq, K), np.int32)
        r_d = np.empty((Nq, K), np.float32)
        for L in np.unique(qlabels):
            sel = np.nonzero(qlabels == L)[0]
            allowed = np.ones(N, bool) if L == -1 else labels == L
            r_ids[sel], r_d[sel] = bf_filtered_reference(orc, f32(base), f32(q)[sel], K, allowed, 0)
    else:
        mask = labels == 1
        bits = torch.from_numpy(pack_bits(mask).view(np.int32).copy()).cuda()

        def call():
            return ops.bf_query_filtered(d_base, d_q, K, bits, 0, rescanned=True)
        r_ids, r_d = bf_filtered_reference(orc, f32(base), f32(q), K, mask, 0)
    ids, d, rescanned, path = call()
    assert (rescanned, path) == (0, 0), "the filtered scan"
    assert np.array_equal(ids.cpu().numpy(), r_ids) and d.cpu().numpy().tobytes() == r_d.tobytes()


def test_int8_filtered_bf_keeps_the_scan_at_integer_shapes(ops):
    """squared L2, D <= 128, under a filter: the exact scan, as for uint8"""
    from filtered_reference import pack_bits
    N, D, Nq, K = 5000, 128, 300, 10
    base, q = full_range(N, D, 71), full_range(Nq, D, 72)
    mask = np.random.default_rng(73).random(N) < 0.3
    bits = torch.from_numpy(pack_bits(mask).view(np.int32).copy()).cuda()
    ids, d, rescanned, path = ops.bf_query_filtered(dev(base), dev(q), K, bits, 0, rescanned=True)
    assert (rescanned, path) == (0, 0)
    u = ops.bf_query_filtered(dev(biased(base)), dev(biased(q)), K, bits, 0)
    assert torch.equal(ids, u[0]) and torch.equal(d, u[1])
    assert mask[ids.cpu().numpy()].all()


# ---------------------------------------------------------------------------------------------
# handle level
# ---------------------------------------------------------------------------------------------
def test_int8_handle_api(orc, tmp_path):
    import ggnn_amd as ggnn
    N, D, K = 8000, 64, 10
    base8, q8 = full_range(N, D, 171), full_range(700, D, 172)
    assert_exact(D, 0, base8, q8)
    base, q = torch.from_numpy(base8), torch.from_numpy(q8)
    rng = orc.make_rng(4000, 3)[:3]

    def handle(rows, reference=False):
        eng = ggnn.GGNN()
        if reference:
            eng.set_base_reference(rows.cuda())
        else:
            eng.set_base(rows)
        eng.set_working_directory(str(tmp_path))
        eng.set_shard_size(4000)
        eng.set_build_hooks(rng, deterministic_sym=True)
        eng.set_prescreen(True)                 # accepted, no effect on 8-bit rows
        eng.build(24, 0.5, 1)
        return eng

    eng, eng_ref = handle(base), handle(base, reference=True)
    ids, d = eng.query(q, K, 0.7, 200)
    r_ids, r_d = eng_ref.query(q, K, 0.7, 200)
    assert torch.equal(ids, r_ids) and torch.equal(d, r_d), "copy != reference base"
    assert d.dtype == torch.float32 and ids.dtype == torch.int32
    # yardstick A through the handle: the biased uint8 base, same deterministic build
    u = handle(torch.from_numpy(biased(base8)))
    uq = torch.from_numpy(biased(q8))
    u_ids, u_d = u.query(uq, K, 0.7, 200)
    assert torch.equal(ids, u_ids) and torch.equal(d, u_d)
    gt, gd = eng.bf_query(q, K)
    o_ids, o_d = orc.bf_query(f32(base8), f32(q8), K)
    assert np.array_equal(gt.numpy(), o_ids) and gd.numpy().tobytes() == o_d.tobytes()
    # the Evaluator on the result: equal to the uint8-biased handle's (no statistical floor)
    ev = ggnn.Evaluator(base, q, gt, K).evaluate_results(ids)
    ev_u = ggnn.Evaluator(torch.from_numpy(biased(base8)), uq, u.bf_query(uq, K)[0],
                          K).evaluate_results(u_ids)
    assert repr(ev) == repr(ev_u) and ev.r_k_query == ev_u.r_k_query
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


def test_int8_padded_rows_equal_the_float32_handle(orc):
    """D = 100: the handle pads int8 rows to 112 bytes with zeros, float32 rows stay at 100; values
    in [-64, 63], where both are exact"""
    import ggnn_amd as ggnn
    N, D, K = 4000, 100, 10
    r = np.random.default_rng(181)
    base8 = r.integers(-64, 64, (N, D)).astype(np.int8)
    q8 = r.integers(-64, 64, (300, D)).astype(np.int8)
    assert_exact(D, 0, base8, q8)
    rng = orc.make_rng(N, 5)[:3]
    out = []
    for rows, qq in ((torch.from_numpy(base8), torch.from_numpy(q8)),
                     (torch.from_numpy(f32(base8)), torch.from_numpy(f32(q8)))):
        eng = ggnn.GGNN()
        eng.set_base(rows)
        eng.set_build_hooks(rng, deterministic_sym=True)
        eng.build(24, 0.5, 1)
        out.append((eng.query(qq, K, 0.7, 200), eng.bf_query(qq, K)))
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    o_ids, o_d = orc.bf_query(f32(base8), f32(q8), K)
    assert np.array_equal(out[0][1][0].numpy(), o_ids)
    assert out[0][1][1].numpy().tobytes() == o_d.tobytes()


def test_int8_out_of_core_equals_resident(orc):
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    N, D, K, NS = 12000, 64, 24, 3000
    base = torch.from_numpy(full_range(N, D, 901))
    q = torch.from_numpy(full_range(300, D, 902))
    rng = orc.make_rng(NS, 5)[:3]

    def build(slots):
        eng = ggnn.GGNN()
        eng.set_base(base)
        eng.set_shard_size(NS)
        eng.set_build_hooks(rng, deterministic_sym=True)
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


def test_int8_two_contexts_equal_one(orc):
    import ggnn_amd as ggnn
    N, D, K, NS = 8000, 64, 10, 2000
    base = torch.from_numpy(full_range(N, D, 87))
    q = torch.from_numpy(full_range(120, D, 88))
    rng = orc.make_rng(NS, 9)[:3]
    out = []
    for gpus in ([0, 0], [0]):
        eng = ggnn.GGNN()
        eng.set_base(base)
        eng.set_gpus(gpus)
        eng.set_shard_size(NS)
        eng.set_build_hooks(rng, deterministic_sym=True)
        eng.build(24, 0.5, 1)
        out.append(eng.query(q, K, 0.7, 400))
    (i2, d2), (i1, d1) = out
    assert torch.equal(d2, d1)
    d = d1.numpy()
    uniq = np.ones_like(d, bool)   # ids of tied distances may come in either order
    uniq[:, 1:] &= d[:, 1:] != d[:, :-1]
    uniq[:, :-1] &= d[:, :-1] != d[:, 1:]
    assert np.array_equal(i2.numpy()[uniq], i1.numpy()[uniq])


# ---------------------------------------------------------------------------------------------
# every int8 query kernel in the library: the launchers' ladder, restated, and a case per kernel
# (tests/test_int8_dtypes.py holds the mapping against the built library on the CPU)
# ---------------------------------------------------------------------------------------------
HOOK_DEFAULTS = {"QUERY_EARLY": 1, "QUERY_GLOBAL_RING": 1, "VIS_TAG_SET": 1}
FAMILIES = {"plain": "query_kernel", "bitset": "query_filtered_kernel", "labels": "query_labeled_kernel"}
N_MAX = 1100         # rows of the graphs above: every key fits the 16-bit tags of a tag set


def vis_hash_regs(vis):
    return 1 if vis <= 192 else 2 if vis <= 480 else 0


def tag_set_bucket_bits(vis):
    b = 5
    while (7 << b) * 4 < 7 * vis:
        b += 1
    return b


def list_regs(sorted_):
    """launch_query_ladder without pre-screen: list registers per lane, 0 = the LDS list"""
    for r, cap in ((1, 64), (2, 128), (4, 256), (8, 512), (16, 1024), (32, 2048)):
        if sorted_ <= cap:
            return r
    return 0


def int8_kernel(how, D, measure, K, iters, hooks=(), kbuild=KB):
    """demangled name of the kernel that an int8 launch through the operator seam runs: launch_query
    and QueryLadder::launch (query.hip), FilteredLadder::launch (query_filtered.hip), NoPrescreen"""
    from ggnn_amd import ops
    h = dict(HOOK_DEFAULTS, **dict(hooks))
    lpr, nch = ops.dist_layout(D, torch.int8)
    cache, sorted_ = ops.query_sizing(D, K, iters)
    vis = cache - sorted_
    T = f"signed char, {lpr}, {nch}"
    early_ok = kbuild <= 24 and sorted_ <= 64 and h["QUERY_EARLY"] != 0
    R = list_regs(sorted_)
    fam = FAMILIES[how]
    if how != "plain":
        hb = vis_hash_regs(vis) if sorted_ <= 64 else 0
        if (lpr, nch) == (8, 1) and hb != 0 and early_ok:
            return f"{fam}<{T}, 1, {measure}, NoPrescreen, {hb}, true>"
        if R == 0:
            return f"{fam}_lds<{T}, {measure}, NoPrescreen>"
        return f"{fam}<{T}, {R}, {measure}, NoPrescreen, 0, false>"
    fits = nch == 1
    hb = vis_hash_regs(vis) if sorted_ <= 64 and fits else 0
    one_chunk = (lpr, nch) == (8, 1)
    global_ring = sorted_ <= 64 and vis_hash_regs(vis) != 0 and iters <= vis and early_ok and \
        h["QUERY_GLOBAL_RING"] != 0 and one_chunk
    tag_ok = sorted_ <= 64 and fits and 481 <= vis <= 2016 and h["VIS_TAG_SET"] != 0
    ring = global_ring or tag_ok
    tag_bits = 0 if (global_ring or not ring) else tag_set_bucket_bits(vis)
    tagged = hb == 0 and fits and ring and tag_bits in (8, 9)
    if one_chunk and early_ok:
        if tagged and iters <= vis and h["QUERY_GLOBAL_RING"] != 0:
            return f"{fam}<{T}, 1, {measure}, NoPrescreen, -{tag_bits}, true, true>"
        if not tagged:
            ringless = "true" if ring and tag_bits == 0 else "false"
            if hb != 0:
                return f"{fam}<{T}, 1, {measure}, NoPrescreen, {hb}, true, {ringless}>"
            return f"{fam}<{T}, 1, {measure}, NoPrescreen, 0, true, false>"
    if tagged and sorted_ <= 64:
        return f"{fam}<{T}, 1, {measure}, NoPrescreen, -{tag_bits}, false, false>"
    if hb != 0:
        return f"{fam}<{T}, 1, {measure}, NoPrescreen, {hb}, false, false>"
    if R == 0:
        return f"{fam}_lds<{T}, {measure}, NoPrescreen>"
    return f"{fam}<{T}, {R}, {measure}, NoPrescreen, 0, false, false>"


# (K, tau, iterations, hooks).  Long lists: sorted part 128 / 224 / 448 / 928 / 2048 / 2144 = list
# registers 2, 4, 8, 16, 32 and the LDS list; K above the number of rows leaves (-1, +inf) slots
LONG_LISTS = [(K, 0.6, 64, ()) for K in (100, 200, 400, 900, 2000, 2100)]
NO_EARLY = (("QUERY_EARLY", 0),)
# the one-chunk layout {8, 1} (D <= 128): hashed sets with one / two bucket registers, ring-less
# (the search cannot wrap its ring) and with the ring in LDS; tag sets of 8 / 9 bucket bits,
# ring-less with early rows and with the ring in global memory; no set at all; and each without
# early rows (hook QUERY_EARLY = 0, the order a KBuild above 24 takes as well)
ONE_CHUNK_PLAIN = [(10, 0.6, 175, ()), (10, 0.6, 200, ()), (10, 0.6, 400, ()), (10, 3.0, 500, ()),
                   (10, 0.6, 600, ()), (10, 0.6, 1500, ()), (10, 3.0, 1000, ()), (10, 3.0, 2040, ()),
                   (10, 0.6, 600, (("VIS_TAG_SET", 0),)),
                   (10, 0.6, 200, NO_EARLY), (10, 0.6, 400, NO_EARLY),
                   (10, 0.6, 600, NO_EARLY + (("VIS_TAG_SET", 0),))]
ONE_CHUNK_FILTERED = [(10, 0.6, 200, ()), (10, 0.6, 400, ()), (10, 0.6, 600, ())]
LADDER_DIMS = (128, 256, 384, 512, 1024, 4096)      # one D per layout
# (how, D, measure, K, tau, iterations, hooks); read as data by tests/test_int8_dtypes.py


def ladder_points(how, D):
    pts = [(10, 0.6, 200, ())] + LONG_LISTS
    if D == 128:
        pts += [p for p in (ONE_CHUNK_PLAIN if how == "plain" else ONE_CHUNK_FILTERED)
                if p not in pts]
    return pts


LADDER_CASES = [(how, D, m, *pt) for how in FAMILIES for D in LADDER_DIMS for m in (0, 1)
                for pt in ladder_points(how, D)]
LADDER_GROUPS = sorted({(how, D, m) for how, D, m, *_ in LADDER_CASES})


def ladder_labels(N, nq, seed):
    """(labels [N], query labels [nq]): four classes; a query label of -1 is unfiltered"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, N).astype(np.int32), rng.integers(-1, 4, nq).astype(np.int32)


def run_ladder_case(ops, how, b, q, g, filt, measure, K, tau, iters, hooks):
    from ggnn_amd import _lib
    c = g["cfg"]
    head = (b, q, dev(g["graph"][:g["N"]]),
            dev(g["tr"][c.STs_offsets[3]:c.STs_offsets[3] + c.Ns[3]]), dev(g["stats"]), K, tau)
    with _lib.hooks(**dict(hooks)):
        if how == "plain":
            res = ops.query(*head, iters, measure, counters=True)
        elif how == "bitset":
            res = ops.query_filtered(*head, filt, iters, measure, counters=True)
        else:
            res = ops.query_labeled(*head, filt[0], filt[1], iters, measure, counters=True)
    return [x.astype(np.uint32) if i >= 2 else x for i, x in enumerate(np_(*res))]


@pytest.mark.parametrize("how,D,measure", LADDER_GROUPS,
                         ids=[f"{h}-D{D}-{'cos' if m else 'l2'}" for h, D, m in LADDER_GROUPS])
def test_int8_every_ladder_kernel(ops, orc, how, D, measure):
    """every case of LADDER_CASES in this (family, layout, measure) group.  Squared L2: yardstick A,
    full-range data, real filters (a bitset of 30 %, four labels with query labels in -1 .. 3).
    Cosine: yardstick B; the oracle has no filters, so the filtered and labelled kernels run under a
    filter that admits every row (the all-ones bitset, one label for all rows and queries), where
    they must give the oracle's unfiltered search, counters included -- the kernel is chosen by the
    presence of a filter, not by its content, and real filters on int8 rows are covered at K = 10
    above and under squared L2 here."""
    from filtered_reference import pack_bits
    g = graph_for(orc, D, measure, "full" if measure == 0 else "ranged")
    N, nq = g["N"], 16
    assert N <= N_MAX
    q8 = full_range(nq, D, 990 + D) if measure == 0 else ranged(nq, D, 1, 991 + D)
    if measure == 1:
        assert_exact(D, 1, g["base8"], q8)
    labels, qlabels = ladder_labels(N, nq, 77 + D)
    if measure == 1:
        labels[:], qlabels[:] = 2, 2
    mask = np.random.default_rng(78 + D).random(N) < 0.3 if measure == 0 else np.ones(N, bool)
    filt = None if how == "plain" else \
        torch.from_numpy(pack_bits(mask).view(np.int32).copy()).cuda() if how == "bitset" else \
        (dev(labels), dev(qlabels))
    c = g["cfg"]
    graph0 = g["graph"][:N]
    start = g["tr"][c.STs_offsets[3]:c.STs_offsets[3] + c.Ns[3]]
    ran = 0
    for h_, D_, m_, K, tau, iters, hooks in LADDER_CASES:
        if (h_, D_, m_) != (how, D, measure):
            continue
        ran += 1
        what = (int8_kernel(how, D, measure, K, iters, hooks), K, tau, iters, hooks)
        mine = run_ladder_case(ops, how, dev(g["base8"]), dev(q8), g, filt, measure, K, tau, iters,
                               hooks)
        if measure == 0:
            ref = run_ladder_case(ops, how, dev(biased(g["base8"])), dev(biased(q8)), g, filt, 0, K,
                                  tau, iters, hooks)
        else:
            ref = orc.query(g["base"], f32(q8), graph0, start, g["stats"], K, tau, iters, 1,
                            counters=True)
        for x, y, name in zip(mine, ref, ("ids", "dists", "n_dist", "n_pop")):
            y = np.asarray(y)
            assert np.array_equal(x, y.astype(x.dtype) if name[0] == "n" else y), (what, name)
        assert mine[1].tobytes() == np.asarray(ref[1]).tobytes(), (what, "distance bits")
        if how == "bitset":
            assert mask[mine[0][mine[0] >= 0]].all(), what
    assert ran >= 7


def test_int8_query_async_filtered_and_labeled(orc):
    """query_async with filter ids and query_async_labeled on two slots equal the blocking calls,
    and those equal the uint8 handle on the biased rows (yardstick A), under one deterministic build"""
    import ggnn_amd as ggnn
    N, D, K, nq = 4000, 64, 10, 200
    base8, q8 = full_range(N, D, 271), full_range(nq, D, 272)
    rng = orc.make_rng(N, 7)[:3]
    r = np.random.default_rng(273)
    masks = np.stack([r.random(N) < 0.5, r.random(N) < 0.05])
    fids = r.integers(-1, 2, nq).astype(np.int32)
    labels = r.integers(0, 4, N).astype(np.int32)
    qlabels = r.integers(-1, 4, nq).astype(np.int32)

    def handle(rows):
        eng = ggnn.GGNN()
        eng.set_base(torch.from_numpy(rows))
        eng.set_build_hooks(rng, deterministic_sym=True)
        eng.build(24, 0.5, 1)
        eng.set_filters(masks)
        eng.set_labels(labels)
        eng.set_return_results_on_gpu(True)
        return eng

    eng, u = handle(base8), handle(biased(base8))
    q, uq = torch.from_numpy(q8).cuda(), torch.from_numpy(biased(q8)).cuda()
    by = eng.query_filtered_by(q, K, 0.7, 200, filter_ids=fids)
    lab = eng.query_labeled(q, K, 0.7, 200, labels=qlabels)
    for mine, theirs in ((by, u.query_filtered_by(uq, K, 0.7, 200, filter_ids=fids)),
                         (lab, u.query_labeled(uq, K, 0.7, 200, labels=qlabels))):
        assert torch.equal(mine[0], theirs[0]) and torch.equal(mine[1], theirs[1])
    ids = by[0].cpu().numpy()
    for f in (0, 1):
        got = ids[fids == f]
        assert masks[f][got[got >= 0]].all()
    got = lab[0].cpu().numpy()
    rows = qlabels >= 0
    assert (labels[np.maximum(got[rows], 0)] == qlabels[rows, None])[got[rows] >= 0].all()
    d_fids, d_ql = torch.from_numpy(fids).cuda(), torch.from_numpy(qlabels).cuda()
    outs = [eng.query_async(q, K, 0.7, 200, slot=i % 2, filter_ids=d_fids) for i in range(2)] + \
           [eng.query_async_labeled(q, K, 0.7, 200, slot=i % 2, labels=d_ql) for i in range(2)]
    eng.synchronize()
    for i, (a, b) in enumerate(outs):
        want = by if i < 2 else lab
        assert torch.equal(a, want[0]) and torch.equal(b, want[1]), i


def test_int8_sharded_engine_one_rank_world():
    """ggnn_amd/distributed.py passes the element type through: a one-rank world over int8 rows
    (three resident shards) against a plain handle -- bf_query equal, blocking and pipelined
    queries equal to each other (the case of tests/test_gpu_distributed.py on signed bytes)"""
    import subprocess
    code = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["GGNN_ROOT"])
import ggnn_amd as ggnn
from ggnn_amd.distributed import ShardedGGNN
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", device_id=dev)
g = np.random.default_rng(5)
base = torch.from_numpy(g.integers(-128, 128, (12000, 64)).astype(np.int8)).to(dev)
q = torch.from_numpy(g.integers(-128, 128, (300, 64)).astype(np.int8)).to(dev)
s = ShardedGGNN()
s.set_base(base)
s.set_shard_size(4000)
s.build(24, 0.5, 1)
ids, d = s.query(q, 10, 0.9, 200)
gt, gd = s.bf_query(q, 10)
ids2, d2 = s.finish(s.query_async(q, 10, 0.9, 200, slot=1))
assert ids.is_cuda and tuple(ids.shape) == (300, 10) and d.dtype == torch.float32
assert torch.equal(ids, ids2) and torch.equal(d, d2)
ref = ggnn.GGNN(); ref.set_base_reference(base); ref.set_shard_size(4000)
ref.set_return_results_on_gpu(True); ref.build(24, 0.5, 1)
rg, rd = ref.bf_query(q, 10)
assert torch.equal(gd, rd[:, :10]) and torch.equal(gt, rg[:, :10])
dist.destroy_process_group()
print("OK")
'''
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29500 + (os.getpid() % 300) + 77),
               RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", GGNN_ROOT=ROOT,
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
