"""The small kernels behind the searches -- result sort and merge (csrc/results.hip), the uniform
generator and the nn1 statistics (csrc/construction_misc.hip) -- against the numpy references of
tests/results_reference.py, bit for bit, on the inputs such kernels go wrong on: rows that mostly
tie, both zeros, infinities, row lengths around the wave size and at the LDS limits, parts that
run empty, the part limit, sizes on both sides of the statistics kernel's grid-stride threshold.

The merge's tie order ("lower part first, then position") is the project's own rule, so the
reference here is that rule; the oracle's heap merge (the reference implementation's) orders ties
as libstdc++'s heap happens to and is compared up to that order only
(tests/test_results_reference.py records that the two differ)."""
import numpy as np
import pytest

from results_reference import (NN1_SIZES, UNIFORM_STREAMS, bits, merge_input, merge_ref,
                               nn1_exact_input, nn1_generic_input, nn1_ref, same_up_to_tie_order,
                               sort_rows_input, sort_rows_ref, uniform_ref)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# sort_rows_kernel
# ---------------------------------------------------------------------------------------------
def _sort_case(ops, orc, Nq, row_len, seed):
    """sorts the middle Nq rows of an [Nq + 2, row_len] tensor in place; the rows around them
    must come back as they were"""
    ids, d = sort_rows_input(Nq + 2, row_len, seed)
    r_ids, r_d = sort_rows_ref(ids[1:-1], d[1:-1])
    o_ids, o_d = orc.sort_shard_results(ids[1:-1], d[1:-1])
    assert np.array_equal(r_ids, o_ids) and np.array_equal(bits(r_d), bits(o_d))
    assert np.array_equal(np.sort(r_ids, 1), np.sort(ids[1:-1], 1))   # a permutation of the row
    t_ids, t_d = dev(ids), dev(d)
    mid_i, mid_d = t_ids[1:-1], t_d[1:-1]
    assert mid_i.is_contiguous() and mid_d.is_contiguous()
    ops.sort_shard_results(mid_i, mid_d)
    g_ids, g_d = host(t_ids), host(t_d)
    assert np.array_equal(g_ids[1:-1], r_ids), (Nq, row_len)
    assert np.array_equal(bits(g_d[1:-1]), bits(r_d)), (Nq, row_len)
    for edge in (0, -1):
        assert np.array_equal(g_ids[edge], ids[edge]), (Nq, row_len, edge)
        assert np.array_equal(bits(g_d[edge]), bits(d[edge])), (Nq, row_len, edge)


# 64 lanes take the entries of a row 64 at a time: 63 / 64 / 65 and 127 / 128 / 129 are the
# boundaries of that loop; 3 * 4 * 5461 B is the last row that fits the default 64 KB of dynamic
# LDS, 5462 the first that has the limit raised
@pytest.mark.parametrize("Nq,row_len", [(200, 2), (200, 63), (200, 64), (200, 65), (1, 65),
                                        (200, 127), (200, 128), (200, 129), (200, 1000),
                                        (3, 5461), (3, 5462), (1, 5462)])
def test_sort_rows(ops, orc, Nq, row_len):
    _sort_case(ops, orc, Nq, row_len, 1000 * Nq + row_len)


def test_sort_rows_longest_row_then_a_short_one(ops, orc):
    """12000 entries (144 000 B of LDS, with the raised attribute), then 40: the raised limit must
    not break a small launch after it"""
    _sort_case(ops, orc, 3, 12000, 12000)
    _sort_case(ops, orc, 200, 40, 40)


def test_sort_rows_limit_and_no_ops(ops):
    ids, d = sort_rows_input(2, 12001, 12001)
    t_ids, t_d = dev(ids), dev(d)
    with pytest.raises(RuntimeError, match="longer than 12000"):
        ops.sort_shard_results(t_ids, t_d)
    assert np.array_equal(host(t_ids), ids) and np.array_equal(bits(host(t_d)), bits(d))
    # one entry per row and no rows: nothing to do
    ids, d = sort_rows_input(5, 1, 1)
    t_ids, t_d = dev(ids), dev(d)
    ops.sort_shard_results(t_ids, t_d)
    assert np.array_equal(host(t_ids), ids) and np.array_equal(bits(host(t_d)), bits(d))
    ops.sort_shard_results(torch.empty((0, 7), dtype=torch.int32, device="cuda"),
                           torch.empty((0, 7), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# merge_results_kernel
# ---------------------------------------------------------------------------------------------
MERGE_CASES = [(1, 10, 10), (2, 10, 10), (3, 10, 1), (8, 20, 10), (64, 10, 10), (64, 1, 64),
               (3, 4, 10),      # k > stride: parts run empty
               (4, 6, 24),      # takes everything
               (2, 24, 24)]
MERGE_NQ = (1, 127, 128, 129, 300)      # the workgroup has 128 threads


def _oracle_defined(stride, k, offset):
    """the reference's merger is written for rows of K * shards_per_gpu entries of which it never
    takes more than K from one part, and for id offsets part * shards_per_gpu * N_shard"""
    return k <= stride and stride % k == 0 and offset % (stride // k) == 0


@pytest.mark.parametrize("P,stride,k", MERGE_CASES)
def test_merge_results(ops, orc, P, stride, k):
    compared_with_oracle = 0
    for Nq in MERGE_NQ:
        ids, d = merge_input(P, Nq, stride, 31 * P + stride + Nq)
        t_ids, t_d = dev(ids), dev(d)
        for offset in (0, 1000):
            r_ids, r_d = merge_ref(ids, d, k, offset)
            m_ids, m_d = ops.merge_results(t_ids, t_d, k, offset)
            m_ids, m_d = host(m_ids), host(m_d)
            assert np.array_equal(m_ids, r_ids), (Nq, offset)
            assert np.array_equal(bits(m_d), bits(r_d)), (Nq, offset)
            if _oracle_defined(stride, k, offset):
                spg = stride // k
                o_ids, o_d = orc.merge_results(list(ids), list(d), k, spg, offset // spg)
                assert same_up_to_tie_order(m_ids, m_d, o_ids, o_d), (Nq, offset)
                compared_with_oracle += 1
    assert compared_with_oracle == (2 * len(MERGE_NQ) if k <= stride else 0)


@pytest.mark.parametrize("P,stride,k", [(2, 10, 10), (8, 20, 10), (3, 4, 10)])
def test_merge_results_signed_zero_heads(ops, P, stride, k):
    """-0.0 against +0.0 is a tie: the lower part goes first and each zero keeps its sign.  (Not
    compared with the oracle: which zero its heap emits first is not a rule.)"""
    for Nq in (129, 300):
        ids, d = merge_input(P, Nq, stride, 17 * P + Nq, signed_zeros=True)
        heads = bits(d[:, :, 0])
        both = ((heads == 0x80000000).any(0) & (heads == 0).any(0)).sum()
        assert both >= Nq // 10, "too few rows set a -0.0 head against a +0.0 head"
        r_ids, r_d = merge_ref(ids, d, k, 1000)
        m_ids, m_d = ops.merge_results(dev(ids), dev(d), k, 1000)
        assert np.array_equal(host(m_ids), r_ids), Nq
        assert np.array_equal(bits(host(m_d)), bits(r_d)), Nq


def test_merge_results_limits(ops):
    ids, d = merge_input(65, 4, 2, 65)
    with pytest.raises(RuntimeError, match=r"parts must be in \[1, 64\]"):
        ops.merge_results(dev(ids), dev(d), 2, 1000)
    ids, d = merge_input(3, 4, 3, 3)
    with pytest.raises(RuntimeError, match="not enough candidates"):
        ops.merge_results(dev(ids), dev(d), 10, 1000)


# ---------------------------------------------------------------------------------------------
# sort and merge inside the engine: tied distances, every position compared
# ---------------------------------------------------------------------------------------------
TIE_N, TIE_D, TIE_K, TIE_NQ, TIE_TAU, TIE_ITERS = 8000, 32, 10, 37, 0.7, 200


def _tied_data():
    base = np.random.default_rng(501).integers(0, 4, (TIE_N, TIE_D)).astype(np.float32)
    q = np.random.default_rng(502).integers(0, 4, (TIE_NQ, TIE_D)).astype(np.float32)
    return base, q


def _context_rows(ops, eng, base, q, n_ctx, spg, n_shard):
    """what each context holds before the merge: its shards' ops.query rows side by side, ids
    local to the context, put in order by sort_rows_ref (ops.query is pinned to the oracle in
    tests/test_gpu_parity.py and the layout matrices)"""
    d_q = dev(q)
    parts_i, parts_d = [], []
    for ctx in range(n_ctx):
        rows_i, rows_d = [], []
        for s in range(spg):
            gs = ctx * spg + s
            g = eng.get_graph(gs)
            lo = gs * n_shard
            ids, d = ops.query(dev(base[lo:lo + n_shard]), d_q, g.graph[0].view.cuda(),
                               g.translation[3].view.reshape(-1).contiguous().cuda(),
                               g.nn1_stats.view.reshape(-1).contiguous().cuda(), TIE_K, TIE_TAU,
                               TIE_ITERS)
            rows_i.append(host(ids) + s * n_shard)
            rows_d.append(host(d))
        si, sd = sort_rows_ref(np.concatenate(rows_i, 1), np.concatenate(rows_d, 1))
        parts_i.append(si)
        parts_d.append(sd)
    return np.stack(parts_i), np.stack(parts_d)


def _share_tied_across(r_ids, r_d, ids_per_part):
    """share of the rows in which two results of equal distance come from different parts"""
    part = r_ids // ids_per_part
    tied = 0
    for n in range(len(r_d)):
        tied += any(len(set(part[n][r_d[n] == v])) > 1 for v in np.unique(r_d[n]))
    return tied / len(r_d)


@pytest.fixture(scope="module")
def eight_contexts(ops):
    import ggnn_amd as ggnn
    n_shard, n_ctx = 500, 8
    base, q = _tied_data()
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_gpus([0] * n_ctx)
    eng.set_shard_size(n_shard)
    eng.build(24, 0.5, 1)
    spg = TIE_N // n_shard // n_ctx
    parts_i, parts_d = _context_rows(ops, eng, base, q, n_ctx, spg, n_shard)
    r_ids, r_d = merge_ref(parts_i, parts_d, TIE_K, spg * n_shard)
    share = _share_tied_across(r_ids, r_d, spg * n_shard)
    print(f"eight contexts: {share:.2f} of the rows tie across contexts")
    return dict(eng=eng, q=q, r_ids=r_ids, r_d=r_d, share=share)


@pytest.mark.parametrize("exchange,split", [(3, 0), (3, 1), (2, 0)])
def test_engine_merge_with_ties_every_position(eight_contexts, exchange, split):
    """8000 x 32 base of integers below 4 (squared distances are small integers), 16 shards on
    eight contexts of one GPU: every id and distance of the merged result, tied or not, is the
    one "lower context first, inside it lower shard first, then position" gives"""
    from ggnn_amd import _lib
    c = eight_contexts
    assert c["share"] >= 0.5, c["share"]
    with _lib.hooks(EXCHANGE=exchange, QUERY_SPLIT=split):
        ids, d = c["eng"].query(c["q"], TIE_K, TIE_TAU, TIE_ITERS)
    assert c["eng"].last_exchange() == ("gather" if exchange == 3 else "copy")
    assert c["eng"].last_query_parts() == (2 if split else 1)
    assert np.array_equal(bits(d.numpy()), bits(c["r_d"]))
    assert np.array_equal(ids.numpy(), c["r_ids"])


def test_engine_shard_sort_with_ties_every_position(ops):
    """one context with four shards: no merge, the sorted [Nq, 4 K] rows cut to K -- among equal
    distances the lower shard first"""
    import ggnn_amd as ggnn
    n_shard, spg = 2000, 4
    base, q = _tied_data()
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_shard_size(n_shard)
    eng.build(24, 0.5, 1)
    rows_i, rows_d = _context_rows(ops, eng, base, q, 1, spg, n_shard)
    r_ids, r_d = np.ascontiguousarray(rows_i[0][:, :TIE_K]), np.ascontiguousarray(rows_d[0][:, :TIE_K])
    share = _share_tied_across(r_ids, r_d, n_shard)
    print(f"four shards: {share:.2f} of the rows tie across shards")
    assert share >= 0.5, share
    ids, d = eng.query(q, TIE_K, TIE_TAU, TIE_ITERS)
    assert np.array_equal(bits(d.numpy()), bits(r_d))
    assert np.array_equal(ids.numpy(), r_ids)


# ---------------------------------------------------------------------------------------------
# nn1 statistics
# ---------------------------------------------------------------------------------------------
def _nn1_case(ops, orc, v):
    mean, mx = nn1_ref(v)
    o = orc.nn1_stats(v)
    out = host(ops.nn1_stats(dev(v)))
    assert bits(out[0]) == bits(mean) == bits(o[0]), (out[0], mean, o[0])
    assert bits(out[1]) == bits(mx) == bits(o[1]), (out[1], mx, o[1])


# the partial kernel's at most kStatsBlocks = 1024 blocks of 256 threads cover 262144 entries in
# one pass and stride over the rest; below 256 entries the one block is partly idle
@pytest.mark.parametrize("N", NN1_SIZES)
def test_nn1_stats_exact_sums(ops, orc, N):
    _nn1_case(ops, orc, nn1_exact_input(N, N))


def test_nn1_stats_max_of_mixed_and_negative_values(ops, orc):
    mixed = nn1_exact_input(1000, 1, shift=2.0 ** 16)
    assert mixed.min() < 0 < mixed.max()
    _nn1_case(ops, orc, mixed)
    negative = nn1_exact_input(1000, 2, shift=2.0 ** 18)
    assert negative.max() < 0
    _nn1_case(ops, orc, negative)


def test_nn1_stats_generic_floats_exact(ops, orc):
    """unconstrained floats: nn1_generic_input checks first that no summation order can move the
    mean across a float32 rounding boundary, so the comparison is exact here too"""
    _nn1_case(ops, orc, nn1_generic_input())


# ---------------------------------------------------------------------------------------------
# uniform
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,stream", UNIFORM_STREAMS)
def test_uniform_bits(ops, seed, stream):
    for n in (1, 255, 256, 257, 100003):
        u = host(ops.uniform(n, seed, stream))
        assert np.array_equal(bits(u), bits(uniform_ref(n, seed, stream))), n
    assert u.min() > 0.0 and u.max() <= 1.0


def test_uniform_streams_differ(ops):
    a, b = host(ops.uniform(1000, 1234, 0)), host(ops.uniform(1000, 1234, 3))
    assert not np.array_equal(a, b)
    assert np.array_equal(bits(a), bits(uniform_ref(1000, 1234, 0)))
    assert np.array_equal(bits(b), bits(uniform_ref(1000, 1234, 3)))
