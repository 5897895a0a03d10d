"""The deterministic sym schedule (`set_build_hooks(deterministic_sym=True)`, ggnn_set_build_hooks
with serial_sym = 2) against the oracle, bit for bit: the graph that `bench.py --dump-outputs`
searches comes out of it.

Per layer the schedule is (include/ggnn_c.h; oracle/ggnn_oracle.hpp):
  1. request pass -- `sym_kernel` with `SymLaunch::requests`: the searches of sym with the pending
     inverse links counted as empty, candidate lists written to `requests`, nothing claimed;
  2. assign step -- `sym_assign_kernel`: slots handed out in ascending (point, neighbour) order;
  3. sym_buffer_merge as in every schedule.
Steps 1 and 2 are compared per kernel through ops.sym(requests=...) / ops.sym_assign with
orc.sym_requests / orc.sym_assign, whole builds with orc.build(deterministic_sym=True).

Data: integers for which sym's half point q + 0.4 (start - q) and every float32 sum are exact
(multiples of 5 in [0, 255], in [0, 15] for D > 256: tests/test_gpu_build_parity.py,
tests/test_gpu_half_parity.py), as float32, uint8, float16 or bfloat16.  No decision then depends
on a summation order, the oracle runs in the reference's own order, and equal inputs of different
element types have equal answers.  A half-point decision can therefore only tie exactly, on both
sides alike, so no case here needs the `orc.margin_min() > 1e-5` guard that the tests on general
integers carry (over the whole 3000-point layer of the large-K case, general integers in [0, 255]
do come within 2e-6 of a tie; that case uses multiples of 5 as well).  Every comparison is
np.array_equal."""
import os
import sys

import numpy as np
import pytest

import sym_assign_cases
from test_gpu_build_parity import mult5_data
from test_gpu_half_parity import HALF_DIMS, int_data
from test_gpu_layout_matrix import F32_DIMS, U8_DIMS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TORCH_TYPES = {"f32": torch.float32, "u8": torch.uint8, "f16": torch.float16,
               "bf16": torch.bfloat16}
# oracle threads: the CPUs this process may use, at most 16
THREADS = min(16, len(os.sched_getaffinity(0)))
KB = 24


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def typed(a, t):
    """device copy of exact float32 integers in element type t; every value survives"""
    out = torch.from_numpy(np.ascontiguousarray(a)).to(TORCH_TYPES[t]).cuda()
    assert np.array_equal(out.float().cpu().numpy(), a), "data is not exact in " + t
    return out


def host(a, t):
    """what the oracle is given: uint8 rows for uint8, the float32 values otherwise"""
    return a.astype(np.uint8) if t == "u8" else a


def layer_of(g, layer):
    c = g["cfg"]
    rows = g["graph"][c.Ns_offsets[layer]:c.Ns_offsets[layer] + c.Ns[layer]].copy()
    tr = None if layer == 0 else g["tr"][c.STs_offsets[layer]:c.STs_offsets[layer] + c.Ns[layer]].copy()
    return rows, tr


def gpu_requests(ops, b, K, rows, tr, stats, measure, prescreen=None, pieces=None, sb=None,
                 sa=None):
    """the request pass over a whole layer (pieces: points per launch); the table starts from a
    value no search writes, so every row must have been written.  sb / sa: cleared buffers as
    the build passes them unless given; the pass must leave them as they are."""
    Nl, KF = rows.shape[0], K // 2
    req = torch.full((Nl, K - KF, KF), -3, dtype=torch.int32, device="cuda")
    d_rows, d_stats = dev(rows), dev(stats)
    d_tr = None if tr is None else dev(tr)
    if sb is None:
        sb = torch.full((Nl, KF), -1, dtype=torch.int32, device="cuda")
        sa = torch.zeros(Nl, dtype=torch.int32, device="cuda")
    sb0, sa0 = sb.clone(), sa.clone()
    for first in range(0, Nl, pieces or Nl):
        ops.sym(b, K, d_rows, d_tr, d_stats, 0.5, sb, sa, measure, first_n=first,
                count=pieces or Nl, prescreen=prescreen, requests=req)
    assert torch.equal(sb, sb0) and torch.equal(sa, sa0), "the request pass wrote a slot buffer"
    return req.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# 1. request pass: every element type, row layout and measure, layer 0 and an upper layer
# ---------------------------------------------------------------------------------------------
REQ_MATRIX = ([("f32", D, m) for D in F32_DIMS for m in (0, 1)] +
              [("u8", D, m) for D in U8_DIMS for m in (0, 1)] +
              [(t, D, m) for t in ("f16", "bf16") for D in HALF_DIMS for m in (0, 1)])
REQ_IDS = [f"{t}-D{D}-{'cos' if m else 'l2'}" for t, D, m in REQ_MATRIX]

_graphs = {}
_oracle_requests = {}


def graph_for(orc, D, measure):
    """oracle-built graph (serial schedule, no refinement: rows as a merge + sym left them) on
    exact integers; equal for every element type"""
    key = (D, measure)
    if key not in _graphs:
        N = 1100 if D < 1024 else 700
        base = int_data(N, D, 600 + D)
        cfg, graph, tr, sel, stats = orc.build(base, KB, 0.5, 0, measure=measure,
                                               rng=orc.make_rng(N, 11), threads=THREADS)
        _graphs[key] = dict(N=N, D=D, base=base, cfg=cfg, graph=graph, tr=tr, stats=stats)
    return _graphs[key]


def oracle_requests(orc, g, t, measure, layer):
    key = (g["D"], measure, layer, t == "u8")
    if key not in _oracle_requests:
        rows, tr = layer_of(g, layer)
        _oracle_requests[key] = orc.sym_requests(host(g["base"], t), KB, rows, tr, g["stats"], 0.5,
                                                 measure=measure, threads=THREADS)
    return _oracle_requests[key]


@pytest.mark.parametrize("t,D,measure", REQ_MATRIX, ids=REQ_IDS)
def test_request_pass_equals_oracle(ops, orc, t, D, measure):
    """one launch over all points of layer 0 and of layer 1 (ids through `translation`); float32
    also with the pre-screen, which changes nothing"""
    g = graph_for(orc, D, measure)
    b = typed(g["base"], t)
    ps = ops.prescreen_encode(b, measure) if t == "f32" else None
    if ps is not None:
        assert ps[1].cpu().numpy()[4] == 1.0
    for layer in (0, 1):
        rows, tr = layer_of(g, layer)
        want = oracle_requests(orc, g, t, measure, layer)
        got = gpu_requests(ops, b, KB, rows, tr, g["stats"], measure)
        assert np.array_equal(got, want), ("layer", layer)
        if ps is not None:
            fast = gpu_requests(ops, b, KB, rows, tr, g["stats"], measure, prescreen=ps)
            assert np.array_equal(fast, want), ("pre-screen, layer", layer)
        asking = int((want[:, :, 0] >= 0).sum())
        assert 0 < asking < want.shape[0] * want.shape[1], ("found and unfound searches", layer)


def test_request_pass_large_kbuild(ops, orc):
    """KBuild 120: the sorted list of the sym kernel takes two registers per lane (R = 2), a
    request row has 60 entries"""
    N, D, K = 3000, 32, 120      # shape of test_gpu_parity.test_large_kbuild_merge_sym_exact
    base = mult5_data(N, D, 93, np.float32)
    cfg, graph, tr, sel, stats = orc.build(base, K, 0.5, 0, rng=orc.make_rng(N, 3), threads=THREADS)
    rows = graph[:N].copy()
    want = orc.sym_requests(base, K, rows, None, stats, 0.5, threads=THREADS)
    got = gpu_requests(ops, dev(base), K, rows, None, stats, 0)
    assert np.array_equal(got, want)
    assert int((want[:, :, 0] >= 0).sum()) > 0


# ---------------------------------------------------------------------------------------------
# 2. the request pass is a pure function of graph, base and statistics
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pure_case(orc):
    N, D = 3000, 128
    base = mult5_data(N, D, 321, np.float32)
    cfg, graph, tr, sel, stats = orc.build(base, KB, 0.5, 0, rng=orc.make_rng(N, 23),
                                           threads=THREADS)
    g = dict(N=N, D=D, base=base, cfg=cfg, graph=graph, tr=tr, stats=stats)
    want = {layer: orc.sym_requests(base, KB, *layer_of(g, layer), stats, 0.5, threads=THREADS)
            for layer in (0, 1)}
    return g, want


@pytest.mark.parametrize("prescreen", [False, True], ids=["plain", "prescreen"])
def test_request_pass_ignores_pending_links(ops, orc, pure_case, prescreen):
    """sym_buffer / sym_atomic hold valid but arbitrary ids and counts instead of -1 / 0 -- among
    them, for every point, its own id in the row of each of its local neighbours, which a search
    that still read pending links would meet at its first pop.  Same requests as the oracle's,
    and both arrays come back untouched."""
    g, want = pure_case
    b = dev(g["base"])
    ps = ops.prescreen_encode(b, 0) if prescreen else None
    KF = KB // 2
    r = np.random.default_rng(5)
    for layer in (0, 1):
        rows, tr = layer_of(g, layer)
        Nl = rows.shape[0]
        sb = r.integers(0, Nl, (Nl, KF)).astype(np.int32)
        for n in range(Nl):                       # n is a pending link of its first neighbours
            for j, m in enumerate(rows[n, :KF // 2]):
                sb[m, (n + j) % KF] = n
        sa = r.integers(0, KF + 4, Nl).astype(np.int32)
        d_sb, d_sa = dev(sb), dev(sa)
        got = gpu_requests(ops, b, KB, rows, tr, g["stats"], 0, prescreen=ps, sb=d_sb, sa=d_sa)
        assert np.array_equal(got, want[layer]), ("layer", layer)
        assert np.array_equal(d_sb.cpu().numpy(), sb) and np.array_equal(d_sa.cpu().numpy(), sa)
        # the same filled buffers do change what the claiming kernel of the other schedules finds
        if layer == 0 and not prescreen:
            sa0 = torch.zeros(Nl, dtype=torch.int32, device="cuda")
            sb0 = torch.full((Nl, KF), -1, dtype=torch.int32, device="cuda")
            ops.sym(b, KB, dev(rows), None, dev(g["stats"]), 0.5, sb0, sa0, 0, first_n=0, count=64)
            sa1 = torch.zeros(Nl, dtype=torch.int32, device="cuda")
            ops.sym(b, KB, dev(rows), None, dev(g["stats"]), 0.5, dev(sb), sa1, 0, first_n=0,
                    count=64)
            assert int(sa1.sum()) < int(sa0.sum()), "the planted links are not on the search paths"


@pytest.mark.parametrize("pieces", [1, 64])
def test_request_pass_does_not_depend_on_launch_split(ops, orc, pure_case, pieces):
    g, want = pure_case
    b = dev(g["base"])
    for layer in (0, 1):
        rows, tr = layer_of(g, layer)
        got = gpu_requests(ops, b, KB, rows, tr, g["stats"], 0, pieces=pieces)
        assert np.array_equal(got, want[layer]), ("layer", layer)


@pytest.mark.parametrize("xcd_map", [0, 2])
def test_request_pass_does_not_depend_on_block_mapping(ops, orc, pure_case, xcd_map):
    """hook XCD_MAP bit 1: workgroup -> point mapping of the sym kernel"""
    from ggnn_amd import _lib
    g, want = pure_case
    b = dev(g["base"])
    with _lib.hooks(XCD_MAP=xcd_map):
        for layer in (0, 1):
            rows, tr = layer_of(g, layer)
            got = gpu_requests(ops, b, KB, rows, tr, g["stats"], 0)
            assert np.array_equal(got, want[layer]), ("layer", layer)


# ---------------------------------------------------------------------------------------------
# 3. assign step
# ---------------------------------------------------------------------------------------------
def gpu_assign(ops, K, req, atomic0, buffer0):
    d_sa, d_sb = dev(atomic0.astype(np.int32)), dev(buffer0)
    ops.sym_assign(K, dev(req), d_sa, d_sb)
    return d_sa.cpu().numpy().astype(np.uint32), d_sb.cpu().numpy()


def assign_both(ops, orc, K, req, atomic0, buffer0):
    sa, sb = gpu_assign(ops, K, req, atomic0, buffer0)
    o_sa, o_sb = atomic0.copy(), buffer0.copy()
    orc.sym_assign(K, req, o_sa, o_sb)
    assert np.array_equal(sa, o_sa), "sym_atomic"
    assert np.array_equal(sb, o_sb), "sym_buffer"
    return sa, sb


@pytest.mark.parametrize("case", sym_assign_cases.all_cases(), ids=lambda c: c[0])
def test_assign_known_answers(ops, orc, case):
    """the hand-written expectations of tests/sym_assign_cases.py"""
    name, K, req, atomic0, buffer0, atomic1, buffer1 = case
    sa, sb = assign_both(ops, orc, K, req, atomic0, buffer0)
    assert sa.tolist() == atomic1.tolist() and sb.tolist() == buffer1.tolist(), name


def test_assign_real_layer(ops, orc):
    """the requests of layer 0 of a 20 000-point graph (built by the engine's default schedule;
    the request table itself is the kernel's, compared with the oracle's in the tests above)"""
    import ggnn_amd as ggnn
    N, D = 20000, 128
    base = mult5_data(N, D, 2024, np.float32)
    eng = ggnn.GGNN()
    eng.set_base(torch.from_numpy(base))
    eng.build(KB, 0.5, 0)
    g = eng.get_graph(0)
    rows = g.graph[0].view.numpy().reshape(N, KB).copy()
    stats = g.nn1_stats.view.numpy().reshape(-1).copy()
    req = gpu_requests(ops, dev(base), KB, rows, None, stats, 0)
    KF = KB // 2
    sa, sb = assign_both(ops, orc, KB, req, np.zeros(N, np.uint32), np.full((N, KF), -1, np.int32))
    assert int(sa.sum()) > N // 20, "implausibly few inverse links were requested"


def test_assign_under_contention(ops, orc):
    """all 60 000 rows of 5 000 points ask among 40 targets: after the first 480 grants every row
    walks through full targets only, bumping each counter"""
    N, KF = 5000, KB // 2
    req = sym_assign_cases.contention_table(N, KB, 40, 9)
    sa, sb = assign_both(ops, orc, KB, req, np.zeros(N, np.uint32), np.full((N, KF), -1, np.int32))
    assert int((sa > KF).sum()) == 40 and int(sa.max()) > 10 * KF


# ---------------------------------------------------------------------------------------------
# 4. whole builds
# ---------------------------------------------------------------------------------------------
def graph_arrays(eng, K, shard=0):
    g = eng.get_graph(shard)
    graph = np.concatenate([g.graph[l].view.numpy().reshape(-1, K) for l in range(4)])
    tr = np.concatenate([g.translation[l].view.numpy().reshape(-1) for l in range(1, 4)])
    sel = np.concatenate([g.selection[l].view.numpy().reshape(-1) for l in range(1, 4)])
    return g.config, graph, tr, sel, g.nn1_stats.view.numpy().reshape(-1).copy()


def assert_same_build(mine, theirs):
    cfg, graph, tr, sel, stats = mine
    o_cfg, o_graph, o_tr, o_sel, o_stats = theirs
    assert cfg["Ns"] == list(o_cfg.Ns) and cfg["G"] == o_cfg.G and cfg["SG"] == o_cfg.SG
    assert stats.tobytes() == o_stats.tobytes(), (stats, o_stats)
    assert np.array_equal(tr, o_tr[:tr.size]), "translation differs"
    assert np.array_equal(sel, o_sel[:sel.size]), "selection differs"
    for l in range(4):
        a, b = o_cfg.Ns_offsets[l], o_cfg.Ns_offsets[l] + o_cfg.Ns[l]
        bad = np.nonzero((graph[a:b] != o_graph[a:b]).any(1))[0]
        assert bad.size == 0, f"layer {l}: {bad.size} of {b - a} rows differ, first {bad[:5]}"


def compare(orc, base, K, tau, refine, seed, t="f32", measure=0, prescreen=True):
    """engine build with the injected selection numbers and the deterministic sym schedule against
    orc.build(deterministic_sym=True) on the same numbers"""
    import ggnn_amd as ggnn
    rng = orc.make_rng(base.shape[0], seed)
    theirs = orc.build(host(base, t), K, tau, refine, measure=measure, rng=rng, threads=THREADS,
                       deterministic_sym=True)
    eng = ggnn.GGNN()
    eng.set_base(torch.from_numpy(base).to(TORCH_TYPES[t]))
    eng.set_prescreen(prescreen)
    eng.set_build_hooks(rng[:3], deterministic_sym=True)
    eng.build(K, tau, refine, ggnn.DistanceMeasure(measure))
    assert_same_build(graph_arrays(eng, K), theirs)
    return eng


@pytest.mark.parametrize("refine", [0, 1, 2])
def test_deterministic_build_bit_exact_f32(orc, refine):
    compare(orc, mult5_data(6000, 128, 1234 + refine, np.float32), 24, 0.5, refine, seed=7 + refine)


def test_deterministic_build_bit_exact_without_prescreen(orc):
    compare(orc, mult5_data(5000, 128, 77, np.float32), 24, 0.5, 1, seed=3, prescreen=False)


def test_deterministic_build_bit_exact_d96(orc):
    compare(orc, mult5_data(7777, 96, 4321, np.float32), 24, 0.5, 2, seed=11)


def test_deterministic_build_bit_exact_u8(orc):
    compare(orc, mult5_data(6000, 128, 99, np.float32), 24, 0.5, 2, seed=5, t="u8")


def test_deterministic_build_bit_exact_other_k_tau(orc):
    compare(orc, mult5_data(5000, 64, 31, np.float32), 20, 0.7, 1, seed=13)


@pytest.mark.parametrize("t,D,N,refine", [("f16", 128, 6000, 1), ("bf16", 96, 7777, 2)])
def test_deterministic_build_bit_exact_half(orc, t, D, N, refine):
    compare(orc, mult5_data(N, D, 1357 + D, np.float32), 24, 0.5, refine, seed=19, t=t)


def test_deterministic_build_bit_exact_cosine(orc):
    compare(orc, mult5_data(5000, 128, 808, np.float32), 24, 0.5, 1, seed=29, measure=1)


def test_deterministic_build_larger_graph_and_query(orc):
    """20k points (G = 9, SG = 3, SG_off = 5), then the oracle's traversal over the built graph
    equals the engine's query"""
    base = mult5_data(20000, 128, 2024, np.float32)
    eng = compare(orc, base, 24, 0.5, 2, seed=17)
    q = mult5_data(300, 128, 555, np.float32)
    ids, d = eng.query(torch.from_numpy(q), 10, 0.64, 400)
    g = eng.get_graph(0)
    o_ids, o_d = orc.query(base, q, g.graph[0].view.numpy(),
                           g.translation[3].view.numpy().reshape(-1),
                           g.nn1_stats.view.numpy().reshape(-1), 10, 0.64, 400)
    assert np.array_equal(ids.numpy(), o_ids) and np.array_equal(d.numpy(), o_d)


def test_deterministic_build_shards_and_two_contexts(orc):
    """four shards of 2000 points: each shard's graph is orc.build(deterministic_sym=True) of its
    rows (every shard reads the same injected numbers), whether one device context builds them
    or two contexts on the one GPU share them"""
    import ggnn_amd as ggnn
    N, D, K, NS = 8000, 64, 24, 2000
    base = mult5_data(N, D, 51, np.float32)
    rng = orc.make_rng(NS, 37)
    theirs = [orc.build(base[s * NS:(s + 1) * NS], K, 0.5, 1, rng=rng, threads=THREADS,
                        deterministic_sym=True) for s in range(N // NS)]
    for gpus in ([0], [0, 0]):
        eng = ggnn.GGNN()
        eng.set_base(torch.from_numpy(base))
        eng.set_gpus(gpus)
        eng.set_shard_size(NS)
        eng.set_build_hooks(rng[:3], deterministic_sym=True)
        eng.build(K, 0.5, 1)
        for s in range(N // NS):
            assert_same_build(graph_arrays(eng, K, s), theirs[s])
