"""Exact range search (bf_range.hip) on the GPU, bit for bit.

The expected values never come from the code under test: the distance of every (query, row) pair
comes from the CPU oracle's bf_query in the kernels' summation order (orc.wave_order, k = all rows)
or -- integer-valued data under squared L2, where every float sum is exact -- from numpy in int64;
filters and labels are applied in numpy; the expected segment is {i : allowed[i] and d[i] <= r} in
ascending id.  Comparisons: array_equal on lims and ids, tobytes() on dists.

N = 485 rows (64 * 7 + 37) ends mid-batch on every row layout; hook BF_RANGE_SLICES = 1, 3, 4 cuts it
into 1, 3 (192 / 192 / 101) and 4 (128 / 128 / 128 / 101) slices."""
import numpy as np
import pytest

from test_gpu_layout_matrix import F32_DIMS, U8_DIMS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 485
SLICES = (1, 3, 4)
CUTS = (128, 192)           # first slice cut under 4 and under 3 slices
MATRIX = ([("u8", D, m) for D in U8_DIMS for m in (0, 1)] +
          [("f32", D, m) for D in F32_DIMS for m in (0, 1)])
IDS = [f"{t}-D{D}-{'cos' if m else 'l2'}" for t, D, m in MATRIX]
# ids that hold one and the same row: both sides of a batch boundary of every layout (batches are 1
# to 32 rows: 127 | 128, 191 | 192) and of the slice cuts at 128 and 192
TIED = (100, 127, 128, 130, 191, 192, 400)
TWINS = (50, 300)           # two more equal rows; query 1 is that row
NP_DTYPE = {"u8": np.uint8, "f32": np.float32, "i8": np.int8, "f16": np.float16}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def data(dtype, n, D, seed, hi=256):
    a = np.random.default_rng(seed).integers(0, hi, (n, D))
    return a.astype(NP_DTYPE[dtype])


def l2_exact(base, q):
    """squared L2 of integer-valued rows whose sums stay below 2^24: exact in every order"""
    b, x = base.astype(np.int64), q.astype(np.int64)
    d = ((x[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    assert d.max() < 2 ** 24
    return d.astype(np.float32)


def oracle_distances(orc, base, q, measure):
    """[Nq, N] float32: the distance of every pair in the kernels' order, from the oracle's bf_query
    on chunks of at most 6000 rows with k = the chunk's rows"""
    out = np.empty((q.shape[0], base.shape[0]), np.float32)
    with orc.wave_order():
        for c0 in range(0, base.shape[0], 6000):
            chunk = base[c0:c0 + 6000]
            ids, d = orc.bf_query(chunk, q, chunk.shape[0], measure)
            assert (np.sort(ids, axis=1) == np.arange(chunk.shape[0])).all()
            np.put_along_axis(out[:, c0:c0 + chunk.shape[0]], ids.astype(np.int64), d, 1)
    return out


def expected(dist, radii, allowed=None):
    """(lims int64 [Nq + 1], ids int32, dists float32) from the pair distances alone"""
    segs = []
    with np.errstate(invalid="ignore"):
        for n in range(dist.shape[0]):
            hit = dist[n] <= radii[n]
            if allowed is not None:
                hit &= allowed[n]
            segs.append(np.nonzero(hit)[0])
    lims = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    ids = np.concatenate(segs).astype(np.int32) if segs else np.empty(0, np.int32)
    d = (np.concatenate([dist[n][s] for n, s in enumerate(segs)]).astype(np.float32)
         if segs else np.empty(0, np.float32))
    return lims, ids, d


def assert_same(got, want, what):
    lims, ids, d = (x.cpu().numpy() for x in got)
    assert np.array_equal(lims, want[0]), f"{what}: lims"
    assert np.array_equal(ids, want[1]), f"{what}: ids"
    assert d.tobytes() == want[2].tobytes(), f"{what}: distance bits"


def run_slices(ops, b, q, radii, measure, want, what, slices=SLICES, **filt):
    from ggnn_amd import _lib
    r = dev(radii)
    for s in slices:
        with _lib.hooks(BF_RANGE_SLICES=s):
            got = ops.bf_range_query(b, q, r, measure, **filt)
        assert_same(got, want, f"{what}, {s} slices")


def pack_bits(mask, offset=0):
    """bool [N] -> int32 words, row i at bit i + offset"""
    full = np.zeros((offset + mask.size + 31) // 32 * 32, np.uint8)
    full[offset:offset + mask.size] = mask
    return np.packbits(full, bitorder="little").view(np.int32)


# ---- 1. every row layout, both measures, 1 / 3 / 4 slices -------------------------------------
def matrix_case(dtype, D, seed):
    base = data(dtype, N, D, seed)
    q = data(dtype, 8, D, seed + 1)
    for i in TIED[1:]:
        base[i] = base[TIED[0]]
    for i in TWINS:
        base[i] = q[1]
    q[3] = q[2]             # the tie's radius, and the float just below it, for one and the same query
    # query 7 is row 222 with one element moved by one: that row is its one nearest
    q[7] = base[222]
    q[7, 0] += 1 if q[7, 0] < 255 else -1
    return base, q


def matrix_radii(dist):
    r = np.empty(8, np.float32)
    r[0] = -1.0
    r[1] = 0.0
    r[2] = dist[2, TIED[0]]
    r[3] = np.nextafter(r[2], np.float32(0))
    r[4] = np.median(dist[4])
    r[5] = np.inf
    r[6] = np.nan
    r[7] = dist[7].min()
    return r


@pytest.mark.parametrize("dtype,D,measure", MATRIX, ids=IDS)
def test_layout_matrix(orc, ops, dtype, D, measure):
    base, q = matrix_case(dtype, D, 7000 + D)
    dist = oracle_distances(orc, base, q, measure)
    radii = matrix_radii(dist)
    want = expected(dist, radii)
    lims, ids, _ = want
    seg = lambda n: ids[lims[n]:lims[n + 1]]
    # what the cases are there for, from the expected values alone
    assert len(seg(0)) == 0 and len(seg(6)) == 0
    if measure == 0:
        assert list(seg(1)) == list(TWINS)
    tied = np.nonzero(dist[2] == radii[2])[0]
    assert len(tied) >= len(TIED) and set(TIED) <= set(tied.tolist())
    for cut in CUTS:
        assert (tied < cut).any() and (tied >= cut).any()
    assert set(tied.tolist()) <= set(seg(2).tolist()) and not set(tied.tolist()) & set(seg(3).tolist())
    assert len(seg(2)) - len(seg(3)) == len(tied)
    assert len(seg(5)) == N and 0 < len(seg(4)) < N
    assert len(seg(7)) == (dist[7] == dist[7].min()).sum() == 1
    run_slices(ops, dev(base), dev(q), radii, measure, want, f"{dtype} D={D} m={measure}")


# ---- 2. filters ---------------------------------------------------------------------------------
FILTER_CASES = [("f32", 32, 0), ("f32", 32, 1), ("u8", 128, 0), ("u8", 128, 1), ("f16", 128, 0)]


def filter_case(orc, dtype, D, measure):
    hi = 16 if dtype == "f16" else 256
    base = data(dtype, N, D, 8100 + D, hi)
    q = data(dtype, 8, D, 8101 + D, hi)
    if dtype == "f16":
        dist = l2_exact(base, q)
    else:
        dist = oracle_distances(orc, base, q, measure)
    radii = np.sort(dist, axis=1)[:, N // 3].astype(np.float32)
    radii[3] = np.inf
    return base, q, dist, radii


@pytest.mark.parametrize("dtype,D,measure", FILTER_CASES,
                         ids=[f"{t}-D{D}-{'cos' if m else 'l2'}" for t, D, m in FILTER_CASES])
def test_filters(orc, ops, dtype, D, measure):
    base, q, dist, radii = filter_case(orc, dtype, D, measure)
    b, qd = dev(base), dev(q)
    rng = np.random.default_rng(91)
    # a per-call bitset at bit offsets 0 and 37
    mask = rng.random(N) < 0.4
    want = expected(dist, radii, np.broadcast_to(mask, (8, N)))
    assert 0 < want[0][-1] < expected(dist, radii)[0][-1]
    for off in (0, 37):
        run_slices(ops, b, qd, radii, measure, want, f"bitset at offset {off}",
                   filter_bits=dev(pack_bits(mask, off)), filter_bit_offset=off)
    # a filter table of four rows, one of them empty; ids -1 (every row) and 9 (names no row)
    masks = rng.random((4, N)) < 0.5
    masks[2] = False
    table = np.stack([pack_bits(m) for m in masks])
    fids = np.array([0, 1, 2, 3, -1, 9, 2, 0], np.int32)
    allowed = np.stack([masks[f] if 0 <= f < 4 else np.full(N, f == -1) for f in fids])
    want = expected(dist, radii, allowed)
    assert want[0][3] == want[0][2] and want[0][6] == want[0][5] and want[0][5] > want[0][4]
    run_slices(ops, b, qd, radii, measure, want, "filter table",
               filter_table=dev(table), filter_ids=dev(fids))
    # a label column; query labels with -1 (every row) and a label no row carries
    labels = rng.integers(0, 5, N).astype(np.int32)
    qlab = np.array([0, 1, -1, 3, 77, 4, 2, -1], np.int32)
    allowed = np.stack([np.full(N, True) if L == -1 else labels == L for L in qlab])
    want = expected(dist, radii, allowed)
    assert want[0][5] == want[0][4] and want[0][3] - want[0][2] == (dist[2] <= radii[2]).sum()
    run_slices(ops, b, qd, radii, measure, want, "labels", labels=dev(labels),
               query_labels=dev(qlab))
    # the column at an offset: local row i carries labels[i + 5]
    shifted = np.concatenate([np.full(5, 3, np.int32), labels])
    run_slices(ops, b, qd, radii, measure, want, "labels at offset 5", slices=(3,),
               labels=dev(shifted), query_labels=dev(qlab), filter_bit_offset=5)


# ---- 3. capacity ----------------------------------------------------------------------------------
def test_capacity(orc, ops):
    base, q, dist, radii = filter_case(orc, "f32", 32, 0)
    b, qd, r = dev(base), dev(q), dev(radii)
    want = expected(dist, radii)
    total = int(want[0][-1])
    assert total > 8

    def sentinel(n):
        return (torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                torch.full((n,), -7.0, dtype=torch.float32, device="cuda"))

    # one entry short: lims right, outputs untouched
    ids, d = sentinel(total)
    lims, _, _ = ops.bf_range_query(b, qd, r, capacity=total - 1, out=(ids, d))
    assert np.array_equal(lims.cpu().numpy(), want[0])
    assert (ids.cpu().numpy() == -7).all() and (d.cpu().numpy() == -7.0).all()
    # exactly enough, in a larger buffer: filled, nothing behind the total is written
    ids, d = sentinel(total + 3)
    lims, _, _ = ops.bf_range_query(b, qd, r, capacity=total, out=(ids, d))
    assert_same((lims, ids[:total], d[:total]), want, "capacity == total")
    assert (ids[total:].cpu().numpy() == -7).all() and (d[total:].cpu().numpy() == -7.0).all()
    # count only: null outputs
    lims, ids, d = ops.bf_range_query(b, qd, r, capacity=0)
    assert np.array_equal(lims.cpu().numpy(), want[0]) and ids.numel() == 0 and d.numel() == 0
    # the two-call form
    assert_same(ops.bf_range_query(b, qd, r), want, "capacity=None")
    # no queries
    lims, ids, d = ops.bf_range_query(b, qd[:0], r[:0])
    assert lims.cpu().tolist() == [0] and ids.numel() == 0
    # every radius negative
    lims, ids, d = ops.bf_range_query(b, qd, -1.0)
    assert lims.cpu().tolist() == [0] * 9 and ids.numel() == 0


# ---- 4. agreement with bf_query ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,measure", [("f32", 96, 0), ("f32", 96, 1), ("u8", 144, 1)])
def test_agrees_with_bf_query(ops, dtype, D, measure):
    base, q = data(dtype, N, D, 8300), data(dtype, 8, D, 8301)
    base[17] = base[333]                                   # a tie inside the lists
    b, qd = dev(base), dev(q)
    k_ids, k_d = ops.bf_query(b, qd, 10, measure)
    lims, ids, d = ops.bf_range_query(b, qd, k_d[:, 9].contiguous(), measure)
    ids, d = ops.sort_segments(lims, ids, d)
    lims = lims.cpu().numpy()
    assert (np.diff(lims) >= 10).all()
    for n in range(8):
        assert np.array_equal(ids[lims[n]:lims[n] + 10].cpu().numpy(), k_ids[n].cpu().numpy())
        assert d[lims[n]:lims[n] + 10].cpu().numpy().tobytes() == k_d[n].cpu().numpy().tobytes()


# ---- 5. int8 rows: the uint8 rows x ^ 0x80 under squared L2 ---------------------------------------
@pytest.mark.parametrize("D", (128, 144, 1024))
def test_int8_is_shifted_uint8(ops, D):
    rng = np.random.default_rng(8400 + D)
    base = rng.integers(-128, 128, (N, D)).astype(np.int8)
    q = rng.integers(-128, 128, (8, D)).astype(np.int8)
    ub, uq = (base.view(np.uint8) ^ 0x80), (q.view(np.uint8) ^ 0x80)
    dist = l2_exact(base, q) if D <= 256 else None
    if dist is None:
        d64 = ((q.astype(np.int64)[:, None] - base.astype(np.int64)[None]) ** 2).sum(-1)
        radii = np.median(d64, axis=1).astype(np.float32)
    else:
        radii = np.median(dist, axis=1).astype(np.float32)
    from ggnn_amd import _lib
    for s in SLICES:
        with _lib.hooks(BF_RANGE_SLICES=s):
            got = ops.bf_range_query(dev(base), dev(q), dev(radii))
            ref = ops.bf_range_query(dev(ub), dev(uq), dev(radii))
        assert_same(got, tuple(x.cpu().numpy() for x in ref), f"int8 against uint8, {s} slices")
        if dist is not None:
            assert_same(got, expected(dist, radii), f"int8 against numpy, {s} slices")


# ---- 6. limits ------------------------------------------------------------------------------------
# (D = 4096 is part of the layout matrix above, for both element types)
def test_automatic_slices(ops):
    """Nq = 1 over 3 * 4096 + 5 rows, no hook: the automatic choice takes three slices"""
    n = 3 * 4096 + 5
    base, q = data("f32", n, 32, 8500), data("f32", 1, 32, 8501)
    dist = l2_exact(base, q)
    radii = np.array([np.sort(dist[0])[1000]], np.float32)
    want = expected(dist, radii)
    assert want[0][-1] >= 1001
    got = ops.bf_range_query(dev(base), dev(q), dev(radii))
    assert_same(got, want, "automatic slices")
    for r in (np.inf, -1.0):
        rr = np.array([r], np.float32)
        assert_same(ops.bf_range_query(dev(base), dev(q), dev(rr)), expected(dist, rr), f"r={r}")


# ---- through the handle -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle_case():
    n, D = 1500, 32
    base, q = data("f32", n, D, 8600), data("f32", 12, D, 8601)
    dist = l2_exact(base, q)
    radii = np.sort(dist, axis=1)[:, 40].astype(np.float32)
    return base, q, dist, radii


def sorted_expected(want):
    lims, ids, d = want
    seg = np.repeat(np.arange(len(lims) - 1), np.diff(lims))
    o = np.lexsort((ids, d, seg))
    return lims, ids[o], d[o]


def test_handle(handle_case):
    import ggnn_amd as ggnn
    base, q, dist, radii = handle_case
    want = expected(dist, radii)
    want_sorted = sorted_expected(want)
    total = int(want[0][-1])
    scalar = float(radii[3])
    want_scalar = expected(dist, np.full(12, scalar, np.float32))
    eng = ggnn.GGNN()
    eng.set_base(base)
    for state in ("before build", "after build"):
        # host queries, host outputs; a tensor of radii; the counting form and an exact max_results
        got = eng.bf_range_query(q, radii, sort=False)
        assert not got[1].is_cuda and got[0].dtype == torch.int64
        assert_same(got, want, f"{state}: host, sort=False")
        assert_same(eng.bf_range_query(q, radii, max_results=total, sort=False), want,
                    f"{state}: max_results == total")
        assert_same(eng.bf_range_query(q, torch.from_numpy(radii)), want_sorted,
                    f"{state}: sort=True")
        assert_same(eng.bf_range_query(q, scalar, sort=False), want_scalar, f"{state}: scalar")
        # device queries
        assert_same(eng.bf_range_query(dev(q), radii, sort=False), want, f"{state}: device query")
        with pytest.raises(RuntimeError, match=str(total)):
            eng.bf_range_query(q, radii, max_results=total - 1)
        # device outputs
        eng.set_return_results_on_gpu(True)
        got = eng.bf_range_query(dev(q), radii, sort=False)
        assert got[1].is_cuda and got[2].is_cuda
        assert_same(got, want, f"{state}: device outputs")
        assert_same(eng.bf_range_query(q, radii, max_results=total + 5), want_sorted,
                    f"{state}: device outputs, sort=True")
        eng.set_return_results_on_gpu(False)
        if state == "before build":
            eng.build(24, 0.5, 1)
    # sort=True is ascending in (distance, id), sort=False ascending in id
    lims, ids, d = (x.numpy() for x in eng.bf_range_query(q, radii))
    _, ids_u, _ = (x.numpy() for x in eng.bf_range_query(q, radii, sort=False))
    for n in range(12):
        s = slice(lims[n], lims[n + 1])
        assert (np.diff(ids_u[s]) > 0).all()
        dd, ii = d[s], ids[s]
        assert ((np.diff(dd) > 0) | ((np.diff(dd) == 0) & (np.diff(ii) > 0))).all()
    # the approximate counterpart: query() cut by numpy at the radius
    k = 64
    g_ids, g_d = (x.numpy() for x in eng.query(q, k, 0.6, 200))
    lims, ids, d = (x.numpy() for x in eng.range_query(q, radii, k, 0.6, 200))
    for n in range(12):
        keep = 0
        while keep < k and g_d[n, keep] <= radii[n] and g_ids[n, keep] >= 0:
            keep += 1
        assert lims[n + 1] - lims[n] == keep
        assert np.array_equal(ids[lims[n]:lims[n + 1]], g_ids[n, :keep])
        assert d[lims[n]:lims[n + 1]].tobytes() == g_d[n, :keep].tobytes()
    assert lims[-1] > 0


def test_handle_filters(handle_case):
    import ggnn_amd as ggnn
    base, q, dist, radii = handle_case
    n = base.shape[0]
    rng = np.random.default_rng(8700)
    mask = rng.random(n) < 0.5
    masks = rng.random((3, n)) < 0.5
    fids = np.array([0, 1, 2, -1] * 3, np.int32)
    labels = rng.integers(0, 4, n).astype(np.int32)
    qlab = np.array([0, -1, 3, 77] * 3, np.int32)
    eng = ggnn.GGNN()
    eng.set_base(base)
    eng.set_filters(masks)
    eng.set_labels(labels)
    assert_same(eng.bf_range_query_filtered(q, radii, sort=False, filter=mask),
                expected(dist, radii, np.broadcast_to(mask, (12, n))), "bitset")
    allowed = np.stack([masks[f] if f >= 0 else np.full(n, True) for f in fids])
    assert_same(eng.bf_range_query_filtered_by(q, radii, sort=False, filter_ids=fids),
                expected(dist, radii, allowed), "filter ids")
    allowed = np.stack([np.full(n, True) if L == -1 else labels == L for L in qlab])
    assert_same(eng.bf_range_query_labeled(q, radii, sort=False, labels=qlab),
                expected(dist, radii, allowed), "labels")
