"""Every row layout of the distance kernels, for both element types and both measures, against
the oracle and against float64.

pick_dist_config (ggnn_amd/csrc/traversal.hpp) gives every (D, dtype) one of seven <LPR, NCH>
layouts; the kernels are instantiated per layout, element type and measure.  MATRIX below has a
case for every (dtype, layout, measure) cell that a D in [1, 4096] can reach --
tests/test_layout_coverage.py checks that on the CPU, against the layout table itself.

Per case, on full-range integer data ([0, 256) as uint8 or float32):
  * query (with counters, at two (tau, iterations) points, the second one wrapping the visited
    ring), top on layers 0 and 1, merge (3, 0) and (2, 1), serial sym on 150 points: bit for bit
    against the oracle in the kernels' summation order (orc.wave_order);
  * where every float sum is exact (D * 255^2 < 2^24, i.e. D <= 256), L2 and cosine: bit for bit
    against the oracle in the reference's own order as well -- this pins the kernels' formulas to
    the reference's, not only to the oracle's wave-order copy of them;
  * elsewhere the reference order differs in the last bits: the ids both results share must be
    most of them, and their distances agree within RTOL (+ cos_atol for cosine);
  * every query output: float64 consistency (assert_rows_consistent);
  * bf: the scan kernel (< 256 queries) against the oracle in wave order, the matrix-core path
    (>= 256 queries, >= 4096 rows) equal to the scan bit for bit, both against float64.

The degenerate cosine tests at the end use zero rows, a zero query, duplicated rows and scaled
copies, where the answer is decided by exact ties at distance 1.0."""
import numpy as np
import pytest

from parity_helpers import RTOL, assert_rows_consistent, assert_topk_parity, cos_atol

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U8_DIMS = (128, 144, 256, 384, 512, 1024, 4096)
F32_DIMS = (32, 64, 96, 128, 256, 1024, 4096)
# (dtype, D, measure); read as data by tests/test_layout_coverage.py
MATRIX = ([("u8", D, m) for D in U8_DIMS for m in (0, 1)] +
          [("f32", D, m) for D in F32_DIMS for m in (0, 1)])
IDS = [f"{t}-D{D}-{'cos' if m else 'l2'}" for t, D, m in MATRIX]

KB = 24                     # K_build
N_GRAPH = 1100              # graph points; 700 for D >= 1024, where the CPU oracle dominates
# (K, tau, iterations): the second point pops more keys than the 192-entry visited ring holds
POINTS = ((10, 0.6, 200), (10, 3.0, 255))
# Share of (query, id) pairs that the reference-order result shares with the kernel's where the
# sums are inexact (D > 256).  Measured with the CPU oracle (wave order against reference order)
# on these seeds: 1.0 for every case; the floor leaves room for a few near-ties.
SHARE_FLOOR = 0.95


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def exact_sums(D):
    """every partial sum of squared differences, dot products and norms of bytes is an integer
    below 2^24: float arithmetic is exact in every order"""
    return D * 255 * 255 < 2 ** 24


def data(dtype, N, D, seed):
    a = np.random.default_rng(seed).integers(0, 256, (N, D))
    return a.astype(np.uint8) if dtype == "u8" else a.astype(np.float32)


def start_points(g):
    c = g["cfg"]
    return g["tr"][c.STs_offsets[3]:c.STs_offsets[3] + c.Ns[3]]


_graphs = {}


def graph_for(orc, key, base, measure):
    if key not in _graphs:
        N = base.shape[0]
        cfg, graph, tr, sel, stats = orc.build(base, KB, 0.5, 0, measure=measure,
                                               rng=orc.make_rng(N, 11))
        _graphs[key] = dict(N=N, D=base.shape[1], base=base, cfg=cfg, graph=graph, tr=tr,
                            sel=sel, stats=stats)
    return _graphs[key]


def matrix_graph(orc, dtype, D, measure):
    N = N_GRAPH if D < 1024 else 700
    return graph_for(orc, (dtype, D, measure), data(dtype, N, D, 500 + D), measure)


def np_(*ts):
    return [t.cpu().numpy() for t in ts]


def assert_shared_ids_agree(ids, d, r_ids, r_d, D, measure, what):
    """reference-order result (r_ids, r_d) against the kernel's where the sums are inexact: the
    share of ids found in both rows is at least SHARE_FLOOR, and their distances agree"""
    atol = cos_atol(D) if measure else 0.0
    shared = total = 0
    for row in range(ids.shape[0]):
        mine = {int(i): float(x) for i, x in zip(ids[row], d[row]) if i >= 0}
        theirs = {int(i): float(x) for i, x in zip(r_ids[row], r_d[row]) if i >= 0}
        total += len(mine)
        for i in mine.keys() & theirs.keys():
            shared += 1
            assert abs(mine[i] - theirs[i]) <= RTOL * abs(theirs[i]) + atol, (what, row, i)
    assert shared >= SHARE_FLOOR * total, (what, shared, total)


# ---------------------------------------------------------------------------------------------
# traversal and construction kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,measure", MATRIX, ids=IDS)
def test_matrix_query_top_merge(ops, orc, dtype, D, measure):
    g = matrix_graph(orc, dtype, D, measure)
    c, base = g["cfg"], g["base"]
    exact = exact_sums(D)
    q = data(dtype, 48, D, 900 + D)
    graph0, start = g["graph"][:g["N"]], start_points(g)
    d_base = dev(base)
    for K, tau, iters in POINTS:
        what = (dtype, D, measure, tau, iters)
        res = np_(*ops.query(d_base, dev(q), dev(graph0), dev(start), dev(g["stats"]), K, tau,
                             iters, measure, counters=True))
        res[2:] = [x.astype(np.uint32) for x in res[2:]]
        with orc.wave_order():
            o = orc.query(base, q, graph0, start, g["stats"], K, tau, iters, measure, counters=True)
        for x, y, name in zip(res, o, ("ids", "dists", "n_dist", "n_pop")):
            assert np.array_equal(x, y), (what, name, "wave order")
        assert_rows_consistent(base, q, res[0], res[1], measure, what)
        r = orc.query(base, q, graph0, start, g["stats"], K, tau, iters, measure, counters=True)
        if exact:
            for x, y, name in zip(res, r, ("ids", "dists", "n_dist", "n_pop")):
                assert np.array_equal(x, y), (what, name, "reference order")
        else:
            assert_shared_ids_agree(res[0], res[1], r[0], r[1], D, measure, what)
        if iters == 255:
            assert int(o[3].max()) > 192 + 16, "the case is meant to wrap the visited ring"
    for layer in (0, 1):
        tr_l = None if layer == 0 else g["tr"][c.STs_offsets[layer]:c.STs_offsets[layer] + c.Ns[layer]]
        S, S_off = (c.S0, c.S0_off) if layer == 0 else (c.S, 0)
        gr, nn1 = np_(*ops.top(d_base, KB, None if tr_l is None else dev(tr_l), c.Ns[layer], S,
                               S_off, layer, measure))
        with orc.wave_order():
            o_gr, o_nn1 = orc.top(base, KB, tr_l, c.Ns[layer], S, S_off, layer, measure)
        assert np.array_equal(gr, o_gr) and np.array_equal(nn1, o_nn1), ("top", layer)
        if exact:
            r_gr, r_nn1 = orc.top(base, KB, tr_l, c.Ns[layer], S, S_off, layer, measure)
            assert np.array_equal(gr, r_gr) and np.array_equal(nn1, r_nn1), ("top ref", layer)
    for top, btm in ((3, 0), (2, 1)):
        args = (dev(g["graph"]), dev(g["tr"]), dev(g["sel"]), dev(g["stats"]), 0.5, top, btm)
        gb, nn1, nd = np_(*ops.merge(d_base, c, *args, measure, counters=True))
        o_args = (base, c, g["graph"], g["tr"], g["sel"], g["stats"], 0.5, top, btm, measure)
        with orc.wave_order():
            o_gb, o_nn1, o_nd = orc.merge(*o_args, counters=True)
        assert np.array_equal(gb, o_gb), ("merge", top, btm)
        assert np.array_equal(nd.astype(np.uint32), o_nd), ("merge n_dist", top, btm)
        if btm == 0:
            assert np.array_equal(nn1, o_nn1), ("merge nn1", top, btm)
        if exact:
            r_gb, r_nn1, r_nd = orc.merge(*o_args, counters=True)
            assert np.array_equal(gb, r_gb), ("merge ref", top, btm)
            assert np.array_equal(nd.astype(np.uint32), r_nd), ("merge ref n_dist", top, btm)
            if btm == 0:
                assert np.array_equal(nn1, r_nn1), ("merge ref nn1", top, btm)


def serial_sym(ops, g, measure, Nl, prescreen=None):
    """sym launched one point at a time in ascending order: the oracle's serialisation"""
    c = g["cfg"]
    KF = KB // 2
    sb = torch.full((c.N, KF), -1, dtype=torch.int32, device="cuda")
    sa = torch.zeros(c.N, dtype=torch.int32, device="cuda")
    b, gr, st = dev(g["base"]), dev(g["graph"][:c.N].copy()), dev(g["stats"])
    for n in range(Nl):
        ops.sym(b, KB, gr, None, st, 0.5, sb, sa, measure, first_n=n, count=1, prescreen=prescreen)
    return sb.cpu().numpy(), sa.cpu().numpy().astype(np.uint32)


def oracle_sym(orc, g, measure, Nl, wave):
    c = g["cfg"]
    sb = np.full((c.N, KB // 2), -1, np.int32)
    sa = np.zeros(c.N, np.uint32)
    orc.set_wave_order(wave)
    try:
        orc.sym(g["base"], KB, g["graph"][:c.N].copy(), None, g["stats"], 0.5, sb, sa, first_n=0,
                count=Nl, measure=measure)
    finally:
        orc.set_wave_order(False)
    return sb, sa


@pytest.mark.parametrize("dtype,D,measure", MATRIX, ids=IDS)
def test_matrix_sym(ops, orc, dtype, D, measure):
    g = matrix_graph(orc, dtype, D, measure)
    Nl = 150
    sb, sa = serial_sym(ops, g, measure, Nl)
    o_sb, o_sa = oracle_sym(orc, g, measure, Nl, True)
    assert np.array_equal(sb, o_sb) and np.array_equal(sa, o_sa), "wave order"
    assert int(sa.sum()) > 0, "some inverse links are requested at all"
    if exact_sums(D):
        r_sb, r_sa = oracle_sym(orc, g, measure, Nl, False)
        assert np.array_equal(sb, r_sb) and np.array_equal(sa, r_sa), "reference order"


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


N_SCAN_ORACLE = 64   # queries of the scan compared with the oracle (the wave-order restatement is slow)


@pytest.mark.parametrize("dtype,D,measure", MATRIX, ids=IDS)
def test_matrix_bf(ops, orc, dtype, D, measure):
    N, Nq, K = (4096 if D == 4096 else 5000), 256, 10
    base, q = data(dtype, N, D, 700 + D), data(dtype, Nq, D, 800 + D)
    b, qq = dev(base), dev(q)
    s_ids, s_d = scan_answer(ops, b, qq, K, measure)
    m_ids, m_d, rescanned = ops.bf_query(b, qq, K, measure, rescanned=True)
    m_ids, m_d = m_ids.cpu().numpy(), m_d.cpu().numpy()
    print(f"bf matrix path {dtype} D={D} {'cosine' if measure else 'L2'}: "
          f"{rescanned} of {Nq} queries rescanned")
    assert np.array_equal(m_ids, s_ids) and np.array_equal(m_d, s_d), "matrix path != scan"
    sub = slice(0, N_SCAN_ORACLE)
    with orc.wave_order():
        o_ids, o_d = orc.bf_query(base, q[sub], K, measure)
    assert np.array_equal(s_ids[sub], o_ids) and np.array_equal(s_d[sub], o_d), "wave order"
    if exact_sums(D):
        r_ids, r_d = orc.bf_query(base, q, K, measure)
        assert np.array_equal(s_ids, r_ids) and np.array_equal(s_d, r_d), "reference order"
    assert_topk_parity(base, q, s_ids, s_d, m_ids, K, measure, "scan")
    assert_topk_parity(base, q, m_ids, m_d, s_ids, K, measure, "matrix path")
    assert_rows_consistent(base, q, s_ids, s_d, measure, "scan")


# ---------------------------------------------------------------------------------------------
# degenerate cosine data: zero rows, a zero query, duplicates, scaled copies
# ---------------------------------------------------------------------------------------------
DEGENERATE = [("u8", 128), ("u8", 256), ("f32", 128)]


def degenerate(dtype, N, D, seed):
    """(base, queries): about 1 % all-zero base rows, duplicated rows (a later copy of an earlier
    row), a base row that is twice a query row; queries: all zero (0), an exact base row (1), an
    exact base row that has a duplicate of lower index (2), a row whose double is in the base (3),
    then random rows"""
    r = np.random.default_rng(seed)
    base = r.integers(0, 256, (N, D))
    q = r.integers(0, 256, (40, D))
    free = [i for i in range(60, N - 3) if not N // 2 <= i < N // 2 + 20]
    zero = r.choice(free, N // 100, replace=False)
    base[zero] = 0
    base[N // 2:N // 2 + 20] = base[40:60]         # duplicates: rows 40..59 again
    q[0] = 0
    q[1] = base[17]
    q[2] = base[N // 2 + 5]                         # = base[45], which comes first
    q[3] = r.integers(0, 128, D)
    base[N - 3] = 2 * q[3]
    cast = np.uint8 if dtype == "u8" else np.float32
    return base.astype(cast), q.astype(cast), np.sort(zero)


def check_degenerate_rows(ids, d, base, D, K, what):
    """oracle-free: the zero query ties everything at 1.0; an exact base row is found first (or
    right behind an identical row of lower index), at distance ~0"""
    assert len(set(ids[0].tolist())) == K and np.all(ids[0] >= 0), what
    assert np.all(d[0] == np.float32(1.0)), what
    for row, target in ((1, 17), (2, base.shape[0] // 2 + 5), (3, base.shape[0] - 3)):
        first = int(ids[row, 0])
        if first == target:
            assert abs(float(d[row, 0])) <= cos_atol(D), (what, row)
        else:
            assert first < target and np.array_equal(base[first], base[target]), (what, row, first)
            assert int(ids[row, 1]) == target and d[row, 1] == d[row, 0], (what, row)
            assert abs(float(d[row, 1])) <= cos_atol(D), (what, row)


@pytest.mark.parametrize("dtype,D", DEGENERATE)
def test_degenerate_cosine_bf(ops, orc, dtype, D):
    N, K = 5000, 10
    base, q, _ = degenerate(dtype, N, D, 31 + D)
    q = np.concatenate([q, data(dtype, 256 - q.shape[0], D, 32 + D)])
    b, qq = dev(base), dev(q)
    s_ids, s_d = scan_answer(ops, b, qq, K, 1)
    m_ids, m_d, rescanned = ops.bf_query(b, qq, K, 1, rescanned=True)
    m_ids, m_d = m_ids.cpu().numpy(), m_d.cpu().numpy()
    print(f"bf matrix path degenerate {dtype} D={D} cosine: {rescanned} of {q.shape[0]} rescanned")
    # the zero query ties every row at 1.0: no certificate can hold, the lowest indices win
    assert rescanned >= 1
    for ids, d, what in ((s_ids, s_d, "scan"), (m_ids, m_d, "matrix path")):
        assert np.array_equal(ids[0], np.arange(K)), what
        check_degenerate_rows(ids, d, base, D, K, what)
    assert np.array_equal(m_ids, s_ids) and np.array_equal(m_d, s_d)
    r_ids, r_d = orc.bf_query(base, q[:64], K, 1)
    assert np.array_equal(s_ids[:64], r_ids) and np.array_equal(s_d[:64], r_d)
    assert_topk_parity(base, q, s_ids, s_d, m_ids, K, 1, "scan")
    assert_rows_consistent(base, q, m_ids, m_d, 1, "matrix path")


@pytest.mark.parametrize("dtype,D", DEGENERATE)
def test_degenerate_cosine_traversal(ops, orc, dtype, D):
    base, q, zero = degenerate(dtype, N_GRAPH, D, 41 + D)
    g = graph_for(orc, ("degenerate", dtype, D), base, 1)
    c = g["cfg"]
    graph0, start = g["graph"][:g["N"]], start_points(g)
    d_base = dev(base)
    for K, tau, iters in POINTS:
        res = np_(*ops.query(d_base, dev(q), dev(graph0), dev(start), dev(g["stats"]), K, tau,
                             iters, 1, counters=True))
        res[2:] = [x.astype(np.uint32) for x in res[2:]]
        check_degenerate_rows(res[0], res[1], base, D, K, ("query", tau, iters))
        assert_rows_consistent(base, q, res[0], res[1], 1, ("query", tau, iters))
        with orc.wave_order():
            o = orc.query(base, q, graph0, start, g["stats"], K, tau, iters, 1, counters=True)
        for x, y, name in zip(res, o, ("ids", "dists", "n_dist", "n_pop")):
            assert np.array_equal(x, y), (tau, iters, name)
    for layer in (0, 1):
        tr_l = None if layer == 0 else g["tr"][c.STs_offsets[layer]:c.STs_offsets[layer] + c.Ns[layer]]
        S, S_off = (c.S0, c.S0_off) if layer == 0 else (c.S, 0)
        gr, nn1 = np_(*ops.top(d_base, KB, None if tr_l is None else dev(tr_l), c.Ns[layer], S,
                               S_off, layer, 1))
        with orc.wave_order():
            o_gr, o_nn1 = orc.top(base, KB, tr_l, c.Ns[layer], S, S_off, layer, 1)
        assert np.array_equal(gr, o_gr) and np.array_equal(nn1, o_nn1), ("top", layer)
    for top, btm in ((3, 0), (2, 1)):
        gb, nn1, nd = np_(*ops.merge(d_base, c, dev(g["graph"]), dev(g["tr"]), dev(g["sel"]),
                                     dev(g["stats"]), 0.5, top, btm, 1, counters=True))
        with orc.wave_order():
            o_gb, o_nn1, o_nd = orc.merge(base, c, g["graph"], g["tr"], g["sel"], g["stats"], 0.5,
                                          top, btm, 1, counters=True)
        assert np.array_equal(gb, o_gb) and np.array_equal(nd.astype(np.uint32), o_nd)
        if btm == 0:
            assert np.array_equal(nn1, o_nn1)
    sb, sa = serial_sym(ops, g, 1, 150)
    o_sb, o_sa = oracle_sym(orc, g, 1, 150, True)
    assert np.array_equal(sb, o_sb) and np.array_equal(sa, o_sa)


def test_degenerate_cosine_prescreen(ops, orc):
    """float32 cosine: the pre-screened query and merge equal the plain kernels on zero rows and a
    zero query, and the probe's bound never exceeds the float distance for them"""
    D = 128
    base, q, zero = degenerate("f32", N_GRAPH, D, 41 + D)
    g = graph_for(orc, ("degenerate", "f32", D), base, 1)
    c = g["cfg"]
    b, qq, ss = dev(base), dev(q), dev(g["stats"])
    g0, st = dev(g["graph"][:g["N"]]), dev(start_points(g))
    ps = ops.prescreen_encode(b, 1)
    assert ps[1].cpu().numpy()[4] == 1.0
    for K, tau, iters in POINTS + ((100, 0.5, 400),):
        plain = ops.query(b, qq, g0, st, ss, K, tau, iters, 1, counters=True)
        fast = ops.query(b, qq, g0, st, ss, K, tau, iters, 1, counters=True, prescreen=ps)
        for x, y in zip(plain, fast):
            assert torch.equal(x, y), (K, tau, iters)
    ga, ta, sa = dev(g["graph"]), dev(g["tr"]), dev(g["sel"])
    for top, btm in ((3, 0), (2, 1)):
        plain = ops.merge(b, c, ga, ta, sa, ss, 0.5, top, btm, 1, counters=True)
        fast = ops.merge(b, c, ga, ta, sa, ss, 0.5, top, btm, 1, counters=True, prescreen=ps)
        for x, y in zip(plain, fast):
            assert torch.equal(x, y), (top, btm)
    # the probe: every zero row against every query, and the zero query against everything
    M = 96
    cand = np.random.default_rng(73).integers(0, N_GRAPH, (q.shape[0], M)).astype(np.int32)
    cand[:, :len(zero)] = zero[None, :M]
    qn = np.sqrt((q.astype(np.float64) ** 2).sum(-1))[:, None]
    xn = np.sqrt((base[cand].astype(np.float64) ** 2).sum(-1))
    dot = (q[:, None, :].astype(np.float64) * base[cand].astype(np.float64)).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(qn * xn > 0, np.abs(1.0 - dot / (qn * xn)), 1.0)
    assert np.all(d[0] == 1.0) and np.all(d[:, :len(zero)] == 1.0)
    # a float32 evaluation lies within (D+8) * 2^-24 (absolute) of the exact value
    below = (d - 3.0 * (D + 8) * 2.0 ** -24).astype(np.float32)
    rej, _ = ops.prescreen_probe(ps[0], ps[1], qq, dev(cand), dev(below), 1)
    assert int(rej.sum()) == 0
    # and it is useful: at half the true distance nearly every ordinary pair is rejected
    rej, _ = ops.prescreen_probe(ps[0], ps[1], qq, dev(cand), dev((d * 0.5).astype(np.float32)), 1)
    assert rej.cpu().numpy()[4:, len(zero):].mean() > 0.9
