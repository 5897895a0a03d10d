"""The filtered brute force on the matrix cores (bf_mfma.hip, filter modes kBfBits / kBfLabels):
a per-call bitset, a filter table with one id per query, and label filters.

Every test compares ids exactly and distances as bytes against
  * `bf_filtered_reference` (tests/filtered_reference.py: the CPU oracle on the compacted base), and
  * the same call under hook BF_SCAN = 1 (the scan kernels, which were the only filtered path),
and asserts `matrix_path == 1`: results are bit-identical on either path, so only the path getter
tells that the tile kernels ran.  Integer-valued data (1..15: exact in float32, float16, bfloat16
and uint8) so that the oracle agrees bit for bit; the shapes are the smallest that reach the tile
kernels (Nq >= 256, N >= 4096), odd in N and Nq, with a last tile partly past N.

The filtered single-chunk kernels exist with the constant list length 18 only (k <= 10; K = 1 is
rounded up to it); a filtered call with k > 10 at D <= 128 runs the chunked kernel with its one
chunk of 128 columns (bf_filtered_runs_chunked, bf_common.hpp): K = 100 here, and K = 30 at
D = 64 / 100 / 128 in test_longer_lists_run_the_chunked_kernel (columns past D are padding).

Labels run everything the bitset and the table run (section 4b): the chunked kernels at T = 2 / 3 /
4 tiles per group (the [2][T][32] row labels beside the group norms), several segments per
workgroup, the re-scan of uncertified queries, a column window at an offset that is no multiple of
32 (which, unlike a bitset's, stays on the tile kernels) and K = 30 on the one-chunk chunked kernel;
and the chunked kernels also run with uint8 (both measures) and float16 rows.
"""
import functools

import numpy as np
import pytest

from conftest import make_int_data
from filtered_reference import bf_filtered_reference, pack_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def _cast(a, kind):
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = {"f32": t.float(), "u8": t.to(torch.uint8), "f16": t.to(torch.float16),
         "bf16": t.to(torch.bfloat16)}[kind]
    return t.contiguous().cuda()


def _bits(mask):
    return torch.from_numpy(pack_bits(mask).view(np.int32).copy()).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def both_paths(call):
    """call(rescanned=True) on the default path and under BF_SCAN = 1: (ids, dists, rescanned) of the
    default path as numpy, after asserting that it ran the tile kernels, that the hook ran the scan
    and that both gave the same bytes"""
    from ggnn_amd import _lib
    ids, d, resc, path = call()
    with _lib.hooks(BF_SCAN=1):
        s_ids, s_d, s_resc, s_path = call()
    assert path == 1, "the filtered call did not take the matrix-core path"
    assert s_path == 0 and s_resc == 0
    assert torch.equal(ids, s_ids)
    assert d.cpu().numpy().tobytes() == s_d.cpu().numpy().tobytes()
    return ids.cpu().numpy(), d.cpu().numpy(), resc


def assert_same(ids, d, r_ids, r_d, what):
    assert np.array_equal(ids, r_ids), what
    assert d.tobytes() == r_d.tobytes(), what


# ---- 1. per-call bitset -------------------------------------------------------------------------
NB, NQ = 4500, 257   # 4500 = 140 tiles + 20 rows: the last tile is partly past N


@functools.lru_cache(maxsize=None)
def _bitset_data(D):
    rs = np.random.default_rng(41 + D)
    base = rs.integers(1, 16, (NB, D)).astype(np.float32)
    base[500:540] = base[100:140]      # duplicated rows across the allowed / denied boundary
    base[4490:4493] = base[0:3]        # ... and in the last, partial tile
    q = rs.integers(1, 16, (NQ, D)).astype(np.float32)
    q[0] = base[101]
    filters = {}
    for share in (100, 50, 10, 1, 0):
        filters[str(share)] = rs.random(NB) < share / 100.0 if share < 100 else np.ones(NB, bool)
    m = np.zeros(NB, bool)
    m[777] = True
    filters["single"] = m
    m = np.zeros(NB, bool)
    m[[100, 101, 501, 502, 900, 4499]] = True          # six rows: fewer than K = 10, 100
    filters["few"] = m
    m = np.ones(NB, bool)
    m[100:140:2] = False                               # one copy of a duplicated pair denied ...
    m[501:540:2] = False                               # ... alternating between the two copies
    filters["dups"] = m
    m = np.zeros(NB, bool)
    m[4480:] = rs.random(20) < 0.6                     # only rows of the last tile, partly past N
    filters["last tile"] = m
    return base, q, filters


@functools.lru_cache(maxsize=None)
def _bitset_reference(orc, D, measure, K, name):
    base, q, filters = _bitset_data(D)
    return bf_filtered_reference(orc, base, q, K, filters[name], measure)


# (uint8 under squared L2 at D <= 128 belongs to the integer kernels, which have no filtered form:
# uint8 runs on this kernel under cosine only)
BITSET_CASES = [(k, d, m) for k, d in (("f32", 64), ("f32", 96), ("f32", 100), ("f32", 128),
                                       ("f16", 128), ("bf16", 128)) for m in (0, 1)] + [("u8", 128, 1)]


@pytest.mark.parametrize("K", [1, 10, 100])
@pytest.mark.parametrize("kind,D,measure", BITSET_CASES,
                         ids=[f"{k}-D{d}-{'cos' if m else 'l2'}" for k, d, m in BITSET_CASES])
def test_per_call_bitset(ops, orc, kind, D, measure, K):
    """NU = 8 / 12 / 16 with and without the constant list length (K = 10), every element type of
    the tile kernel, both measures"""
    base, q, filters = _bitset_data(D)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    for name, allowed in filters.items():
        bits = _bits(allowed)
        ids, d, resc = both_paths(lambda: ops.bf_query_filtered(d_base, d_q, K, bits, measure,
                                                                rescanned=True))
        r_ids, r_d = _bitset_reference(orc, D, measure, K, name)
        assert_same(ids, d, r_ids, r_d, (kind, D, measure, name, K, resc))


@pytest.mark.parametrize("kind,D", [("f32", 64), ("f32", 100), ("bf16", 128)])
def test_longer_lists_run_the_chunked_kernel(ops, orc, kind, D):
    """K = 30 at D <= 128: the chunked kernel on a single chunk of 128 columns, half of them / 28 /
    none past the end of the row"""
    base, q, filters = _bitset_data(D)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    for name in ("50", "1", "few", "dups"):
        bits = _bits(filters[name])
        ids, d, resc = both_paths(lambda: ops.bf_query_filtered(d_base, d_q, 30, bits, 0,
                                                                rescanned=True))
        r_ids, r_d = _bitset_reference(orc, D, 0, 30, name)
        assert_same(ids, d, r_ids, r_d, (kind, D, name, resc))


@pytest.mark.parametrize("measure", [0, 1])
def test_per_call_bitset_offsets(ops, orc, measure):
    """the rows as a window of a longer bitset: offset 64 stays on the tile kernels; offset 37 is
    exact on the scan (a bitset offset that is not a multiple of 32 keeps the scan, for the per-call
    bitset as for the table: launch_bf_query)"""
    from ggnn_amd import _lib
    D, K = 128, 10
    base, q, filters = _bitset_data(D)
    allowed = filters["50"]
    d_base, d_q = _cast(base, "f32"), _cast(q, "f32")
    r_ids, r_d = _bitset_reference(orc, D, measure, K, "50")
    for off in (64, 37):
        wide = np.random.default_rng(off).random(off + NB) < 0.5
        wide[off:] = allowed
        bits = _bits(wide)

        def call():
            return ops.bf_query_filtered(d_base, d_q, K, bits, measure, filter_bit_offset=off,
                                         rescanned=True)
        if off % 32 == 0:
            ids, d, _ = both_paths(call)
        else:
            ids, d, _, path = call()
            assert path == 0   # the documented fallback
            ids, d = ids.cpu().numpy(), d.cpu().numpy()
        assert_same(ids, d, r_ids, r_d, (measure, off))


# ---- 2. chunked kernels -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chunked_data(D):
    rs = np.random.default_rng(300 + D)
    base = rs.integers(1, 16, (9100, D)).astype(np.float32)
    q = rs.integers(1, 16, (301, D)).astype(np.float32)
    return base, q, rs.random(9100) < 0.3


@functools.lru_cache(maxsize=None)
def _chunked_reference(orc, D, measure):
    base, q, allowed = _chunked_data(D)
    return bf_filtered_reference(orc, base, q, 10, allowed, measure)


@pytest.mark.parametrize("tiles", [2, 3, 4])
@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("kind,D", [("f32", 200), ("f32", 960), ("bf16", 200)])
def test_chunked_kernels(ops, orc, kind, D, measure, tiles):
    """D > 128: T = 2 / 3 / 4 tiles per accumulator group, one 30 % bitset; N = 9100 leaves the last
    group with padding tiles (their verdict word is the clamped one of the last row)"""
    from ggnn_amd import _lib
    base, q, allowed = _chunked_data(D)
    d_base, d_q, bits = _cast(base, kind), _cast(q, kind), _bits(allowed)
    with _lib.hooks(BF_TILES=tiles):
        ids, d, resc = both_paths(lambda: ops.bf_query_filtered(d_base, d_q, 10, bits, measure,
                                                                rescanned=True))
    r_ids, r_d = _chunked_reference(orc, D, measure)
    assert_same(ids, d, r_ids, r_d, (kind, D, measure, tiles, resc))


@pytest.mark.parametrize("tiles", [2, 3, 4])
def test_chunked_many_segments_per_workgroup_filtered(ops, tiles):
    """test_bf_mfma_chunked_many_segments_per_workgroup with a filter table: a workgroup runs several
    segments in one do/while and picks its 128 filter rows anew in each.  Of that test's shapes the
    one kept is (N, Nq, D) = (2100, 40 000, 132) with N raised to 4100, the smallest the tile
    kernels accept (N >= 4096); fractional data, compared with the scan on every query."""
    from ggnn_amd import _lib
    N, Nq, D, F = 4100, 40_000, 132, 4
    rng = np.random.default_rng(77)
    base = rng.normal(size=(N, D)).astype(np.float32)
    q = rng.normal(size=(Nq, D)).astype(np.float32)
    table = rng.random((F, N)) < np.array([0.5, 0.05, 0.9, 0.0])[:, None]
    fids = rng.integers(-1, F + 1, Nq).astype(np.int32)    # F: out of range -> empty result
    d_table = torch.stack([_bits(m) for m in table])
    d_base, d_q, d_fids = _cast(base, "f32"), _cast(q, "f32"), _i32(fids)
    with _lib.hooks(BF_TILES=tiles):
        ids, d, resc = both_paths(lambda: ops.bf_query_filtered_by(d_base, d_q, 10, d_table, d_fids,
                                                                   0, rescanned=True))
    # what the scan cannot tell: the rows obey each query's own filter
    full = np.concatenate([table, np.ones((1, N), bool)])   # row -1 = unfiltered
    for f in range(-1, F):
        sel = ids[fids == f]
        assert full[f][sel[sel >= 0]].all(), f
        assert (sel >= 0).sum(1).min() == min(10, int(full[f].sum())), f
    assert (ids[fids == F] == -1).all() and np.isinf(d[fids == F]).all()


# ---- 3. filter table ----------------------------------------------------------------------------
def _table_case(seed, Nq=300):
    rs = np.random.default_rng(seed)
    D = 128
    base = rs.integers(1, 16, (NB, D)).astype(np.float32)
    q = rs.integers(1, 16, (Nq, D)).astype(np.float32)
    table = rs.random((5, NB)) < np.array([0.5, 0.0, 1.0, 0.02, 0.2])[:, None]
    fids = rs.integers(-1, 5, Nq).astype(np.int32)     # mixed within every wave's 32 queries
    fids[[3, 40, 77, 130, 299]] = 7                    # outside the table: empty result
    fids[[5, 41, 200]] = -5
    return base, q, table, fids


def _table_reference(orc, base, q, K, table, fids, measure):
    r_ids = np.full((q.shape[0], K), -1, np.int32)
    r_d = np.full((q.shape[0], K), np.inf, np.float32)
    for f in np.unique(fids):
        if f < -1 or f >= table.shape[0]:
            continue
        allowed = np.ones(base.shape[0], bool) if f == -1 else table[f]
        sel = np.nonzero(fids == f)[0]
        r_ids[sel], r_d[sel] = bf_filtered_reference(orc, base, q[sel], K, allowed, measure)
    return r_ids, r_d


@pytest.mark.parametrize("K", [10, 100])
@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_filter_table(ops, orc, kind, measure, K):
    """five rows of different density (one all-zero, one all-ones), ids from {-1, 0..4} plus 7 and
    -5 (empty result: every slot (-1, +inf)), at offset 0 and as a window at offset 4512 of a
    longer table"""
    base, q, table, fids = _table_case(61)
    d_base, d_q, d_fids = _cast(base, kind), _cast(q, kind), _i32(fids)
    off = 4512
    wide = np.random.default_rng(62).random((5, off + NB + 100)) < 0.5
    wide[:, off:off + NB] = table
    d_tables = {0: torch.stack([_bits(m) for m in table]), off: torch.stack([_bits(m) for m in wide])}
    r_ids, r_d = _table_reference(orc, base, q, K, table, fids, measure)
    empty = (fids < -1) | (fids >= 5)
    assert (r_ids[empty] == -1).all() and np.isinf(r_d[empty]).all()
    for o, d_table in d_tables.items():
        ids, d, resc = both_paths(lambda: ops.bf_query_filtered_by(
            d_base, d_q, K, d_table, d_fids, measure, filter_bit_offset=o, rescanned=True))
        assert_same(ids, d, r_ids, r_d, (kind, measure, K, o, resc))


# ---- 4. labels ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 100])
@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_labels(ops, orc, kind, measure, K):
    """seven tenants of unequal size, a label no row carries (8), row label -1 on some rows, query
    label -1 (= the unfiltered ops.bf_query); K = 10 also reads a window at offset 4512 of a longer
    column"""
    rs = np.random.default_rng(71)
    D, Nq = 128, 300
    base = rs.integers(1, 16, (NB, D)).astype(np.float32)
    q = rs.integers(1, 16, (Nq, D)).astype(np.float32)
    labels = rs.choice(7, NB, p=[0.4, 0.25, 0.15, 0.1, 0.06, 0.03, 0.01]).astype(np.int32)
    labels[rs.random(NB) < 0.03] = -1
    qlabels = rs.integers(-1, 9, Nq).astype(np.int32)      # -1 .. 8, 7 and 8: few / no rows
    qlabels[qlabels == 7] = 8
    d_base, d_q, d_ql = _cast(base, kind), _cast(q, kind), _i32(qlabels)
    off = 4512
    wide = np.concatenate([rs.integers(-1, 9, off), labels, rs.integers(-1, 9, 100)]).astype(np.int32)
    r_ids = np.full((Nq, K), -1, np.int32)
    r_d = np.full((Nq, K), np.inf, np.float32)
    for L in np.unique(qlabels):
        sel = np.nonzero(qlabels == L)[0]
        allowed = np.ones(NB, bool) if L == -1 else labels == L
        r_ids[sel], r_d[sel] = bf_filtered_reference(orc, base, q[sel], K, allowed, measure)
    for o, column in ((0, labels), (off, wide)) if K == 10 else ((0, labels),):
        d_lab = _i32(column)
        ids, d, resc = both_paths(lambda: ops.bf_query_labeled(
            d_base, d_q, K, d_lab, d_ql, measure, bit_offset=o, rescanned=True))
        assert_same(ids, d, r_ids, r_d, (kind, measure, K, o, resc))
    # label -1 is the unfiltered call
    u_ids, u_d = ops.bf_query(d_base, d_q, K, measure)
    sel = qlabels == -1
    assert sel.any()
    assert np.array_equal(ids[sel], u_ids.cpu().numpy()[sel])
    assert d[sel].tobytes() == u_d.cpu().numpy()[sel].tobytes()


# ---- 4b. labels beyond D = 128, the default tile group and the aligned window -----------------------
QLABEL_CYCLE = (-1, 0, 1, 2, 3, 4, 7, 0)   # -1: unfiltered; 7: no row carries it; 4: six rows


def _label_column(n, seed):
    """the column of tests/test_gpu_filtered_layout_matrix.py: classes of about 50 / 30 / 15 / 5 %
    and label 4 on exactly six rows (fewer than K)"""
    rs = np.random.default_rng(seed)
    labels = rs.choice(5, n, p=[.5, .3, .15, .04, .01]).astype(np.int32)
    had = labels == 4
    forced = rs.choice(np.nonzero(~had)[0], 6, replace=False)
    labels[had] = 3
    labels[forced] = 4
    return labels


def _query_labels(nq):
    """every value within every 8 consecutive queries: mixed within each wave's 32"""
    return np.resize(np.array(QLABEL_CYCLE, np.int32), nq)


def _labels_reference(orc, base, q, K, labels, qlabels, measure):
    r_ids = np.full((q.shape[0], K), -1, np.int32)
    r_d = np.full((q.shape[0], K), np.inf, np.float32)
    for L in np.unique(qlabels):
        sel = np.nonzero(qlabels == L)[0]
        allowed = np.ones(base.shape[0], bool) if L == -1 else labels == L
        r_ids[sel], r_d[sel] = bf_filtered_reference(orc, base, q[sel], K, allowed, measure)
    fin = np.isfinite(r_d).sum(1)
    assert (fin[qlabels == 7] == 0).all() and (fin[qlabels == 4] == min(K, 6)).all()
    assert (fin[(qlabels != 7) & (qlabels != 4)] == K).all()
    return r_ids, r_d


@functools.lru_cache(maxsize=None)
def _chunked_labels(D):
    return _label_column(9100, 400 + D), _query_labels(301)


@functools.lru_cache(maxsize=None)
def _chunked_labels_reference(orc, D, measure):
    base, q, _ = _chunked_data(D)
    labels, qlabels = _chunked_labels(D)
    return _labels_reference(orc, base, q, 10, labels, qlabels, measure)


@pytest.mark.parametrize("tiles", [2, 3, 4])
@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("kind,D", [("f32", 200), ("f32", 960), ("bf16", 200)])
def test_chunked_kernels_labels(ops, orc, kind, D, measure, tiles):
    """test_chunked_kernels under labels: the [2][T][32] row labels beside the group norms
    (bf_filter_lds_words(kBfLabels, T > 1)) at T = 2 / 3 / 4, the padding tiles of the last group
    included"""
    from ggnn_amd import _lib
    base, q, _ = _chunked_data(D)
    labels, qlabels = _chunked_labels(D)
    d_base, d_q, d_lab, d_ql = _cast(base, kind), _cast(q, kind), _i32(labels), _i32(qlabels)
    with _lib.hooks(BF_TILES=tiles):
        ids, d, resc = both_paths(lambda: ops.bf_query_labeled(d_base, d_q, 10, d_lab, d_ql, measure,
                                                               rescanned=True))
    r_ids, r_d = _chunked_labels_reference(orc, D, measure)
    assert_same(ids, d, r_ids, r_d, (kind, D, measure, tiles, resc))


@pytest.mark.parametrize("kind,D,measure", [("u8", 256, 0), ("u8", 256, 1), ("f16", 256, 0)],
                         ids=["u8-D256-l2", "u8-D256-cos", "f16-D256-l2"])
def test_chunked_kernels_other_element_types(ops, orc, kind, D, measure):
    """the element types the chunked filtered kernels never ran with: uint8 beyond the integer
    kernels' D <= 128 under both measures, float16 beyond one chunk; the 30 % bitset and labels,
    at the default tiles per group"""
    base, q, allowed = _chunked_data(D)
    labels, qlabels = _chunked_labels(D)
    d_base, d_q = _cast(base, kind), _cast(q, kind)
    bits, d_lab, d_ql = _bits(allowed), _i32(labels), _i32(qlabels)
    ids, d, resc = both_paths(lambda: ops.bf_query_filtered(d_base, d_q, 10, bits, measure,
                                                            rescanned=True))
    r_ids, r_d = _chunked_reference(orc, D, measure)
    assert_same(ids, d, r_ids, r_d, (kind, D, measure, "bitset", resc))
    ids, d, resc = both_paths(lambda: ops.bf_query_labeled(d_base, d_q, 10, d_lab, d_ql, measure,
                                                           rescanned=True))
    r_ids, r_d = _chunked_labels_reference(orc, D, measure)
    assert_same(ids, d, r_ids, r_d, (kind, D, measure, "labels", resc))


@pytest.mark.parametrize("tiles", [2, 3, 4])
def test_chunked_many_segments_per_workgroup_labeled(ops, tiles):
    """test_chunked_many_segments_per_workgroup_filtered with labels in place of the table: a
    workgroup that runs several segments in one do/while stages the 128 query labels of each anew.
    Labels mixed within every 32 queries, -1 and a label no row carries (4) among them; compared
    with the scan on every query, and every reported row carries its query's label"""
    from ggnn_amd import _lib
    N, Nq, D = 4100, 40_000, 132
    rng = np.random.default_rng(77)
    base = rng.normal(size=(N, D)).astype(np.float32)
    q = rng.normal(size=(Nq, D)).astype(np.float32)
    labels = rng.choice(4, N, p=[0.5, 0.05, 0.449, 0.001]).astype(np.int32)
    qlabels = rng.integers(-1, 5, Nq).astype(np.int32)
    for w in range(0, Nq - 31, 32):                        # mixed within every 32 queries
        assert len(np.unique(qlabels[w:w + 32])) >= 3
    d_base, d_q, d_lab, d_ql = _cast(base, "f32"), _cast(q, "f32"), _i32(labels), _i32(qlabels)
    with _lib.hooks(BF_TILES=tiles):
        ids, d, resc = both_paths(lambda: ops.bf_query_labeled(d_base, d_q, 10, d_lab, d_ql, 0,
                                                               rescanned=True))
    for L in range(0, 4):
        sel = ids[qlabels == L]
        assert (labels[sel[sel >= 0]] == L).all(), L
        assert (sel >= 0).sum(1).min() == min(10, int((labels == L).sum())), L
    assert (ids[qlabels == -1] >= 0).all()
    assert (ids[qlabels == 4] == -1).all() and np.isinf(d[qlabels == 4]).all()


@pytest.mark.parametrize("measure", [0, 1])
def test_labels_unaligned_window(ops, orc, measure):
    """the label column as a window at offset 4517 of a longer one: labels are read per row, so an
    offset that is no multiple of 32 stays on the tile kernels (unlike a bitset) and is exact"""
    D, K, off = 128, 10, 4517
    base, q, _ = _bitset_data(D)
    labels, qlabels = _label_column(NB, 91), _query_labels(NQ)
    rs = np.random.default_rng(92)
    wide = np.concatenate([rs.integers(-1, 8, off), labels, rs.integers(-1, 8, 100)]).astype(np.int32)
    d_base, d_q, d_wide, d_ql = _cast(base, "f32"), _cast(q, "f32"), _i32(wide), _i32(qlabels)
    ids, d, resc = both_paths(lambda: ops.bf_query_labeled(d_base, d_q, K, d_wide, d_ql, measure,
                                                           bit_offset=off, rescanned=True))
    r_ids, r_d = _labels_reference(orc, base, q, K, labels, qlabels, measure)
    assert_same(ids, d, r_ids, r_d, (measure, off, resc))


@pytest.mark.parametrize("D", [64, 100])
def test_longer_lists_run_the_chunked_kernel_labels(ops, orc, D):
    """K = 30 at D <= 128 under labels: the chunked kernel on its one chunk of 128 columns, half of
    them / 28 past the end of the row"""
    K = 30
    base, q, _ = _bitset_data(D)
    labels, qlabels = _label_column(NB, 93 + D), _query_labels(NQ)
    d_base, d_q, d_lab, d_ql = _cast(base, "f32"), _cast(q, "f32"), _i32(labels), _i32(qlabels)
    ids, d, resc = both_paths(lambda: ops.bf_query_labeled(d_base, d_q, K, d_lab, d_ql, 0,
                                                           rescanned=True))
    r_ids, r_d = _labels_reference(orc, base, q, K, labels, qlabels, 0)
    assert_same(ids, d, r_ids, r_d, (D, resc))


# ---- 5. the certificate under a filter ------------------------------------------------------------
def _far_tight(N, D, seed):
    """the data of test_bf_mfma_uncertifiable_data_is_rescanned (tests/test_gpu_bf_exact.py)"""
    rng = np.random.default_rng(seed)
    centres = np.random.default_rng(99).normal(size=(8, D)) * 4.0
    x = centres[rng.integers(0, 8, N)] + 1e-3 * rng.normal(size=(N, D))
    return x.astype(np.float32)


def test_uncertifiable_data_is_rescanned_under_a_filter(ops):
    """tight far clusters with a 50 % bitset: the queries the certificate rejects are answered by
    the FILTERED scan over a query subset; then a filter table with ids mixed within that subset
    -- the re-scan must pick each query's filter by its real index, not by its place in the list"""
    N, Nq, K, D = 20000, 300, 10, 128
    base, q = _far_tight(N, D, 511), _far_tight(Nq, D, 512)
    rs = np.random.default_rng(513)
    allowed = rs.random(N) < 0.5
    d_base, d_q, bits = _cast(base, "f32"), _cast(q, "f32"), _bits(allowed)
    ids, d, resc = both_paths(lambda: ops.bf_query_filtered(d_base, d_q, K, bits, 0, rescanned=True))
    print(f"uncertifiable, 50 % bitset: {resc} of {Nq} queries rescanned")
    assert 0 < resc <= Nq
    assert allowed[ids].all()
    table = rs.random((3, N)) < np.array([0.5, 0.2, 0.8])[:, None]
    fids = rs.integers(-1, 4, Nq).astype(np.int32)       # 3: out of range -> empty
    d_table, d_fids = torch.stack([_bits(m) for m in table]), _i32(fids)
    ids, d, resc = both_paths(lambda: ops.bf_query_filtered_by(d_base, d_q, K, d_table, d_fids, 0,
                                                               rescanned=True))
    print(f"uncertifiable, mixed table ids: {resc} of {Nq} queries rescanned")
    assert resc > 0
    for f in range(3):
        assert table[f][ids[fids == f]].all(), f
    assert (ids[fids == 3] == -1).all()
    assert (ids[fids == -1] >= 0).all()
    # ... and labels mixed within the batch: the re-scan picks the label by the query's real index
    labels = rs.integers(0, 3, N).astype(np.int32)
    qlabels = rs.integers(-1, 4, Nq).astype(np.int32)    # 3: no row carries it -> empty
    d_lab, d_ql = _i32(labels), _i32(qlabels)
    ids, d, resc = both_paths(lambda: ops.bf_query_labeled(d_base, d_q, K, d_lab, d_ql, 0,
                                                           rescanned=True))
    print(f"uncertifiable, mixed labels: {resc} of {Nq} queries rescanned")
    assert resc > 0
    for L in range(3):
        assert (qlabels == L).any() and (labels[ids[qlabels == L]] == L).all(), L
    assert (ids[qlabels == 3] == -1).all() and np.isinf(d[qlabels == 3]).all()
    assert (ids[qlabels == -1] >= 0).all()


def test_certifiable_data_is_certified_under_a_filter(ops, orc):
    """integer data (test_bf_mfma_integer_data_certified_and_exact) at K = 10 with a 50 % bitset:
    at most a quarter of the queries may need the re-scan, so the result cannot come from the
    re-scan alone; the unfiltered tile kernels on the compacted allowed rows are the yardstick
    (the existing test holds them to <= 3)"""
    K = 10
    base, q = make_int_data(30000, 128, 531), make_int_data(300, 128, 532)
    allowed = np.random.default_rng(533).random(30000) < 0.5
    d_base, d_q, bits = _cast(base, "f32"), _cast(q, "f32"), _bits(allowed)
    ids, d, resc = both_paths(lambda: ops.bf_query_filtered(d_base, d_q, K, bits, 0, rescanned=True))
    _, _, plain = ops.bf_query(_cast(base[allowed], "f32"), d_q, K, 0, rescanned=True)
    print(f"certifiable, 50 % bitset: {resc} rescanned; unfiltered on the compacted rows: {plain}")
    r_ids, r_d = bf_filtered_reference(orc, base, q, K, allowed)
    assert_same(ids, d, r_ids, r_d, resc)
    assert resc <= q.shape[0] // 4


# ---- 6. handle level ----------------------------------------------------------------------------
def test_handle_filtered_bf_query_reports_its_path(ops, orc):
    """a GGNN handle over N = 8192 in two resident shards of 4096, Nq = 256: the three filtered
    brute-force calls are exact, report the matrix path and the re-scan count of the operator, and
    leave the unfiltered call as it was"""
    import ggnn_amd as ggnn
    Nb, D, Nq, K = 8192, 64, 256, 10
    rs = np.random.default_rng(81)
    base = rs.integers(0, 256, (Nb, D)).astype(np.float32)
    q = rs.integers(0, 256, (Nq, D)).astype(np.float32)
    allowed = rs.random(Nb) < 0.3
    table = rs.random((3, Nb)) < np.array([0.5, 0.1, 0.9])[:, None]
    fids = rs.integers(-1, 3, Nq).astype(np.int32)
    labels = rs.integers(0, 5, Nb).astype(np.int32)
    qlabels = rs.integers(-1, 5, Nq).astype(np.int32)
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_shard_size(4096)
    eng.build(24, 0.5, 1)
    eng.set_filters(table)
    eng.set_labels(labels)
    d_base, d_q = _cast(base, "f32"), _cast(q, "f32")

    plain0 = eng.bf_query(q, K)
    assert eng.last_bf_query_matrix_path() == 1
    o_ids, o_d = orc.bf_query(base, q, K)
    assert_same(plain0[0].numpy(), plain0[1].numpy(), o_ids, o_d, "unfiltered")

    ids, d = eng.bf_query_filtered(q, K, filter=allowed)
    assert eng.last_bf_query_matrix_path() == 1
    r = bf_filtered_reference(orc, base, q, K, allowed)
    assert_same(ids.numpy(), d.numpy(), *r, "bitset")
    op = ops.bf_query_filtered(d_base, d_q, K, _bits(allowed), 0, rescanned=True)
    assert op[3] == 1 and eng.last_bf_query_rescanned() == op[2]

    ids, d = eng.bf_query_filtered_by(q, K, filter_ids=fids)
    assert eng.last_bf_query_matrix_path() == 1
    r = _table_reference(orc, base, q, K, table, fids, 0)
    assert_same(ids.numpy(), d.numpy(), *r, "table")
    op = ops.bf_query_filtered_by(d_base, d_q, K, torch.stack([_bits(m) for m in table]), _i32(fids),
                                  0, rescanned=True)
    assert op[3] == 1 and eng.last_bf_query_rescanned() == op[2]

    ids, d = eng.bf_query_labeled(q, K, labels=qlabels)
    assert eng.last_bf_query_matrix_path() == 1
    r_ids = np.full((Nq, K), -1, np.int32)
    r_d = np.full((Nq, K), np.inf, np.float32)
    for L in np.unique(qlabels):
        sel = np.nonzero(qlabels == L)[0]
        a = np.ones(Nb, bool) if L == -1 else labels == L
        r_ids[sel], r_d[sel] = bf_filtered_reference(orc, base, q[sel], K, a)
    assert_same(ids.numpy(), d.numpy(), r_ids, r_d, "labels")
    op = ops.bf_query_labeled(d_base, d_q, K, _i32(labels), _i32(qlabels), 0, rescanned=True)
    assert op[3] == 1 and eng.last_bf_query_rescanned() == op[2]

    plain1 = eng.bf_query(q, K)
    assert eng.last_bf_query_matrix_path() == 1
    assert torch.equal(plain0[0], plain1[0]) and torch.equal(plain0[1], plain1[1])
    # a small batch takes the scan, and says so
    eng.bf_query_filtered(q[:40], K, filter=allowed)
    assert eng.last_bf_query_matrix_path() == 0
