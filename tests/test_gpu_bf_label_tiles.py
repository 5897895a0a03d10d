"""bf_query under label sets, label ranges and label masks on the float tile kernels
(bf_mfma_pred.hip: FilterStage<kBfPredicate>, hook BF_LABEL_TILES = 2).

Integer data 1..15 (exact in all four element types) at N = 4500, Nq = 257: a full 128-query block, a
ragged one, a last tile partly past N.  Squared L2: plain numpy int64 distances over the admitted
[Nq, N] mask, stable argsort (ties: lower id first), padded with -1 / +inf; ids equal, distances equal
as bytes.  Every case asserts path 1 under the hook, and path 0 with the same bytes under BF_SCAN = 1
(the cosine reference)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, NQ = 4500, 257
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
BIT31 = I32_MIN
FAMILIES = ("sets", "ranges", "masks")
CASES = [("f32", 64, 0), ("f32", 100, 0), ("f32", 128, 0), ("bf16", 128, 0), ("f16", 128, 1),
         ("u8", 128, 1), ("f32", 256, 0), ("u8", 272, 0)]

# one spec row per query, cycled with period 8 (table ids with period 5: every pairing occurs, and
# every 32 queries mix them all)
SETS = [[1] * 8, [0, 2, 3, 6, -9, 0x50, 2, 0], [5, -1, 5, 5, 5, 5, 5, 5], [12345] * 8, [77] * 8,
        [BIT31 + 3, 1, 1, 1, 1, 1, 1, 1], [-9, 6, 6, -9, 6, 6, 6, 6], [0, 1, 2, 3, 6, 0x50, -9, 77]]
RANGES = [[(5, 4), (1, 3), (9, 8), (1, 0)], [(1, 0)] * 4, [(I32_MIN, I32_MAX)] * 4,
          [(-10, -2), (77, 77), (3, 2), (0x50, 0x50)], [(77, 77)] * 4,
          [(I32_MIN, -8), (6, I32_MAX), (1, 0), (1, 0)], [(2, 2), (2, 2), (2, 2), (2, 2)],
          [(0, 0), (2, 3), (-1, -1), (I32_MAX, I32_MAX)]]
MASKS = [[(0, 0, 0)] * 2, [(3, 1, 0), (3, 2, 0)], [(1, 3, 0)] * 2, [(BIT31, BIT31, 0)] * 2,
         [(0, 0, 6)] * 2, [(-1, 77, 0)] * 2, [(BIT31, 0, 3), (7, 6, 0)], [(0x50, 0x50, 0), (1, 1, 2)]]
FID_CYCLE = [0, -1, 3, 1, 2]   # 3: one past the table


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def _cast(a, kind):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return {"f32": t.float(), "u8": t.to(torch.uint8), "f16": t.to(torch.float16),
            "bf16": t.to(torch.bfloat16)}[kind].contiguous().cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _bits(mask):
    m = np.zeros((mask.shape[0], (mask.shape[1] + 31) // 32 * 32), bool)
    m[:, :mask.shape[1]] = mask
    return _i32(np.packbits(m, axis=1, bitorder="little").view(np.int32))


@functools.lru_cache(maxsize=None)
def _column():
    """labels of the N rows (negative ones, bit 31, 77 on exactly six rows), the table, the ids"""
    rs = np.random.default_rng(7)
    values = np.array([-9, -1, 0, 1, 2, 3, 6, 0x50, BIT31 + 3], np.int64)
    labels = values[rs.integers(0, len(values), N)].astype(np.int32)
    labels[rs.choice(N, 6, replace=False)] = 77
    table = rs.random((3, N)) < np.array([0.5, 0.1, 1.0])[:, None]
    return labels, table, np.resize(np.array(FID_CYCLE, np.int32), NQ)


def _spec(family, width=None):
    rows = {"sets": SETS, "ranges": RANGES, "masks": MASKS}[family]
    a = np.array([rows[i % 8] for i in range(NQ)], np.int64).astype(np.int32)
    return a if width is None else np.ascontiguousarray(a[:, :width])


def _admitted(family, spec, labels, table=None, fids=None):
    """[Nq, N] bool: the predicate of common.hpp, written out"""
    lab = labels.astype(np.int64)[None, :]
    s = spec.astype(np.int64)
    if family == "sets":
        ok = (s == -1).any(1)[:, None] | (lab[:, :, None] == s[:, None, :]).any(2)
    elif family == "ranges":
        ok = ((s[:, None, :, 0] <= lab[:, :, None]) & (lab[:, :, None] <= s[:, None, :, 1])).any(2)
    else:
        u, su = lab & 0xffffffff, s & 0xffffffff
        m, v, a = su[:, None, :, 0], su[:, None, :, 1], su[:, None, :, 2]
        ok = (((u[:, :, None] & m) == v) & ((a == 0) | ((u[:, :, None] & a) != 0))).any(2)
    if fids is not None:
        rows = np.concatenate([table, np.ones((1, table.shape[1]), bool), np.zeros((1, table.shape[1]), bool)])
        pick = np.where(fids == -1, len(table), np.where((fids >= 0) & (fids < len(table)), fids, len(table) + 1))
        ok = ok & rows[pick]
    return ok


@functools.lru_cache(maxsize=None)
def _data(D):
    rs = np.random.default_rng(100 + D)
    base = rs.integers(1, 16, (N, D)).astype(np.int64)
    base[500:540] = base[100:140]    # equal distances: the tie rule decides
    q = rs.integers(1, 16, (NQ, D)).astype(np.int64)
    q[0] = base[101]
    d = (q * q).sum(1)[:, None] + (base * base).sum(1)[None, :] - 2 * q @ base.T
    return base, q, d


def _l2_reference(D, ok, K):
    d = np.where(ok, _data(D)[2], np.iinfo(np.int64).max)
    order = np.argsort(d, axis=1, kind="stable")[:, :K]
    found = np.take_along_axis(ok, order, 1)
    r_d = np.where(found, np.take_along_axis(d, order, 1), np.inf).astype(np.float32)
    return np.where(found, order, -1).astype(np.int32), r_d


def _call(ops, family):
    return getattr(ops, "bf_query_labeled_" + {"sets": "in", "ranges": "range", "masks": "mask"}[family])


def both_paths(call):
    """call() under BF_LABEL_TILES = 2 and under BF_SCAN = 1: path 1 against path 0, same bytes"""
    from ggnn_amd import _lib
    with _lib.hooks(BF_LABEL_TILES=2):
        ids, d, resc, path = call()
        with _lib.hooks(BF_SCAN=1):
            s_ids, s_d, s_resc, s_path = call()
    assert path == 1, "the predicate call did not take the tile kernels"
    assert s_path == 0 and s_resc == 0
    assert torch.equal(ids, s_ids)
    assert d.cpu().numpy().tobytes() == s_d.cpu().numpy().tobytes()
    return ids.cpu().numpy(), d.cpu().numpy(), resc


@pytest.mark.parametrize("with_table", [False, True], ids=["labels-only", "table"])
@pytest.mark.parametrize("K", [1, 10, 30])
@pytest.mark.parametrize("kind,D,measure", CASES,
                         ids=[f"{k}-D{d}-{'cos' if m else 'l2'}" for k, d, m in CASES])
@pytest.mark.parametrize("family", FAMILIES)
def test_predicate_on_the_tile_kernels(ops, family, kind, D, measure, K, with_table):
    """NU = 8 / 12 / 16 single chunk, the chunked kernel at D <= 128 (K = 30) and beyond; sets at
    width 1, 3 and 8, ranges with 1 and 4 intervals, masks with 1 and 2 clauses"""
    labels, table, fids = _column()
    base, q, _ = _data(D)
    d_base, d_q, d_lab = _cast(base, kind), _cast(q, kind), _i32(labels)
    tab = (_bits(table), _i32(fids)) if with_table else (None, None)
    for width in {"sets": (1, 3, 8), "ranges": (1, 4), "masks": (1, 2)}[family]:
        spec = _spec(family, width)
        d_spec = _i32(spec)
        ids, d, resc = both_paths(lambda: _call(ops, family)(
            d_base, d_q, K, d_lab, d_spec, *tab, measure, rescanned=True))
        ok = _admitted(family, spec, labels, table, fids if with_table else None)
        assert (np.take_along_axis(ok, np.maximum(ids, 0), 1) | (ids < 0)).all()
        assert ((ids >= 0).sum(1) == np.minimum(ok.sum(1), K)).all()
        if measure == 0:
            r_ids, r_d = _l2_reference(D, ok, K)
            assert np.array_equal(ids, r_ids), (width, resc)
            assert d.tobytes() == r_d.tobytes(), (width, resc)


@pytest.mark.parametrize("family", FAMILIES)
def test_windows(ops, family):
    """label column and table as windows of longer ones: at bit offset 32 * 141 path 1 and the results
    of offset 0; at 64 + 5 a call with a table keeps the scan, one without stays on the tiles"""
    from ggnn_amd import _lib
    D, K = 128, 10
    labels, table, fids = _column()
    base, q, _ = _data(D)
    spec = _spec(family)
    d_base, d_q, d_spec, d_fids = _cast(base, "f32"), _cast(q, "f32"), _i32(spec), _i32(fids)
    r_ids, r_d = _l2_reference(D, _admitted(family, spec, labels, table, fids), K)
    rs = np.random.default_rng(8)
    for off in (32 * 141, 64 + 5):
        wide_lab = np.concatenate([rs.integers(-9, 80, off), labels, rs.integers(-9, 80, 50)])
        wide_tab = rs.random((3, off + N + 50)) < 0.5
        wide_tab[:, off:off + N] = table

        def call(tab=(_bits(wide_tab), d_fids), lab=_i32(wide_lab)):
            return _call(ops, family)(d_base, d_q, K, lab, d_spec, *tab, 0, bit_offset=off,
                                      rescanned=True)
        if off % 32 == 0:
            ids, d, _ = both_paths(call)
        else:
            with _lib.hooks(BF_LABEL_TILES=2):
                ids, d, _, path = call()
                assert path == 0
                assert call(tab=(None, None))[3] == 1
            ids, d = ids.cpu().numpy(), d.cpu().numpy()
        assert np.array_equal(ids, r_ids) and d.tobytes() == r_d.tobytes(), off


@pytest.mark.parametrize("family", FAMILIES)
def test_uncertified_queries_are_rescanned_under_their_own_predicate(ops, family):
    """tight far clusters (test_uncertifiable_data_is_rescanned_under_a_filter), three-valued labels,
    every query selecting one value: the family's scan answers the rejected queries, each under the
    predicate of its real index"""
    Nb, Nq, K, D = 20000, 300, 10, 128

    def far_tight(n, seed):
        rng = np.random.default_rng(seed)
        centres = np.random.default_rng(99).normal(size=(8, D)) * 4.0
        return (centres[rng.integers(0, 8, n)] + 1e-3 * rng.normal(size=(n, D))).astype(np.float32)
    base, q = far_tight(Nb, 511), far_tight(Nq, 512)
    rs = np.random.default_rng(513)
    labels = rs.integers(0, 3, Nb).astype(np.int32)
    L = rs.integers(0, 3, Nq).astype(np.int32)
    spec = {"sets": L[:, None], "ranges": np.stack([L, L], 1)[:, None, :],
            "masks": np.stack([np.full(Nq, -1), L, np.zeros(Nq)], 1)[:, None, :]}[family]
    d_base, d_q, d_lab, d_spec = _cast(base, "f32"), _cast(q, "f32"), _i32(labels), _i32(spec)
    ids, d, resc = both_paths(lambda: _call(ops, family)(d_base, d_q, K, d_lab, d_spec, None, None,
                                                         0, rescanned=True))
    assert 0 < resc <= Nq, resc
    assert (ids >= 0).all() and (labels[ids] == L[:, None]).all()


def test_handle_reports_the_path(ops):
    """GGNN.bf_query_labeled_in / _range / _mask: path 1 under the hook, path 0 without it at this
    small shape, the same results either way"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    labels, _, _ = _column()
    base, q, _ = _data(64)
    eng = ggnn.GGNN()
    eng.set_base(base.astype(np.float32))
    eng.set_labels(labels)
    qf = q.astype(np.float32)
    for family, method, kw in (("sets", eng.bf_query_labeled_in, "label_sets"),
                               ("ranges", eng.bf_query_labeled_range, "label_ranges"),
                               ("masks", eng.bf_query_labeled_mask, "label_masks")):
        spec = _spec(family)
        with _lib.hooks(BF_LABEL_TILES=2):
            ids, d = method(qf, 10, **{kw: spec})
            assert eng.last_bf_query_matrix_path() == 1, family
        s_ids, s_d = method(qf, 10, **{kw: spec})
        assert eng.last_bf_query_matrix_path() == 0 and eng.last_bf_query_rescanned() == 0
        assert torch.equal(ids, s_ids) and torch.equal(d, s_d), family
        r_ids, _ = _l2_reference(64, _admitted(family, spec, labels), 10)
        assert np.array_equal(ids.numpy(), r_ids), family
