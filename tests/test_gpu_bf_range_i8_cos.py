"""Range search of uint8 / int8 rows under cosine on the integer tile kernels (bf_range_i8_cos.hip), bit
for bit.

Expected values from numpy: int64 sums, then finish_cos in float32 operation by operation
(|1 - dot / sqrt(qn * bn)|, 1 where qn * bn == 0), a hit iff value <= r, ids ascending, lims exact; every
case also equals the scan kernels' answer to the same call (BF_RANGE_I8_COS = 1).  BF_RANGE_I8_COS = 2
sends these small shapes to the tiles.  N = 485 = 15 tiles + 5 rows and N = 97 = 3 tiles + 1; Nq = 130 =
two 64-query waves and a partial 32-query set; BF_RANGE_SLICES = 1, 3 cuts inside the base."""
import numpy as np
import pytest

from test_gpu_bf_range import assert_same, dev, expected, ops, pack_bits  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NQ, TWIN, ZROW, ZQ, TQ, KINDS = 130, 200 % 97, 3, 5, 2, 9
NP = {"u8": np.uint8, "i8": np.int8}
_cases = {}


def values(base, q):
    """float32 [Nq, N] the scan's value of every pair, and the largest integer sum"""
    b, x = base.astype(np.int64), q.astype(np.int64)
    dot, bn, qn = x @ b.T, (b * b).sum(1), (x * x).sum(1)
    ns = qn.astype(np.float32)[:, None] * bn.astype(np.float32)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.abs(np.float32(1) - dot.astype(np.float32) / np.sqrt(ns))
    v = np.where(ns > 0, v, np.float32(1)).astype(np.float32)
    return v, int(max(np.abs(dot).max(), bn.max(), qn.max()))


def case(t, D, N):
    """(base, q, v): once per cell, never changed.  Full value range; row ZROW and query ZQ are zero,
    query TQ is row TWIN"""
    if (t, D, N) not in _cases:
        rng = np.random.default_rng(9000 + D + N + (t == "i8"))
        info = np.iinfo(NP[t])
        base = rng.integers(info.min, info.max + 1, (N, D)).astype(NP[t])
        q = rng.integers(info.min, info.max + 1, (NQ, D)).astype(NP[t])
        base[ZROW], q[ZQ], q[TQ] = 0, 0, base[TWIN]
        v, top = values(base, q)
        assert top < 2 ** 24
        _cases[(t, D, N)] = (base, q, v)
    return _cases[(t, D, N)]


def cycle_radii(v):
    """query i gets kind i % 9: negative, NaN, a pair's own value (query TQ: its twin's), the float below
    one, a value between two pairs', 1.0, the float below 1.0, 2.0, +inf"""
    srt = np.sort(v, axis=1)
    k = srt.shape[1] // 4
    r = np.empty(v.shape[0], np.float32)
    r[0::9], r[1::9], r[2::9] = -1.0, np.nan, srt[2::9, k]
    r[TQ] = v[TQ, TWIN]
    r[3::9] = np.nextafter(srt[3::9, k], np.float32(-np.inf))
    r[4::9] = (srt[4::9, k].astype(np.float64) + srt[4::9, k + 1]) / 2
    r[5::9], r[6::9], r[7::9], r[8::9] = 1.0, np.nextafter(np.float32(1), np.float32(0)), 2.0, np.inf
    return r


def run(ops, b, q, radii, slices=(1, 3), fell=0, **kw):
    """the tiles' answers (asserted equal to the scan's, and routed to the integer kernels)"""
    from ggnn_amd import _lib
    r = dev(radii)
    with _lib.hooks(BF_RANGE_I8_COS=1):
        scan = ops.bf_range_query(b, q, r, 1, routed=True, **kw)
    assert scan[3:] == (0, 0)
    for s in slices:
        with _lib.hooks(BF_RANGE_I8_COS=2, BF_RANGE_SLICES=s):
            got = ops.bf_range_query(b, q, r, 1, routed=True, **kw)
        assert got[3:] == (2, fell), (s, got[3:])
        assert_same(got[:3], tuple(x.cpu().numpy() for x in scan[:3]), f"against the scan, {s} parts")
        yield s, got[:3]


@pytest.mark.parametrize("N", [485, 97])
@pytest.mark.parametrize("D", [16, 128, 144, 528])
@pytest.mark.parametrize("t", ["u8", "i8"])
def test_parity(ops, t, D, N):
    base, q, v = case(t, D, N)
    radii = cycle_radii(v)
    want = expected(v, radii)
    lims, ids = want[0], want[1]
    per_q = np.diff(lims)
    assert lims[-1] > 0 and (per_q == 0).any() and (per_q == N).any()
    assert TWIN in ids[lims[TQ]:lims[TQ + 1]]                          # the tie is a hit
    assert ZROW in ids[lims[14]:lims[15]] and ZROW not in ids[lims[15]:lims[16]]   # radius 1.0 / below
    assert per_q[ZQ] == N                                              # zero query at radius 1.0
    assert t == "u8" or want[2].max() > 1
    for s, got in run(ops, dev(base), dev(q), radii):
        assert_same(got, want, f"{t} D={D} N={N}, {s} parts")


@pytest.mark.parametrize("t,D,N,who", [("u8", 272, 485, "row"), ("u8", 272, 485, "query"),
                                       ("i8", 1024, 97, "row")])
def test_norms_from_two_to_the_24_fall_back(ops, t, D, N, who):
    rng = np.random.default_rng(D + N)
    lo = -20 if t == "i8" else 0
    base = rng.integers(lo, lo + 40, (N, D)).astype(NP[t])
    q = rng.integers(lo, lo + 40, (NQ, D)).astype(NP[t])
    if who == "row":
        base[7] = np.iinfo(NP[t]).max if t == "u8" else -128
    else:
        q[11] = 255                                                       # (a query with a radius >= 0)
    radii = np.sort(values(base, q)[0], axis=1)[:, N // 3].astype(np.float32)
    radii[0::9], radii[1::9] = -1.0, np.nan
    b, x = base.astype(np.int64), q.astype(np.int64)
    assert max((b * b).sum(1).max(), (x * x).sum(1).max()) >= 2 ** 24
    got = [g for _, g in run(ops, dev(base), dev(q), radii, fell=1)]      # equal to the scan's
    assert int(got[0][0][-1]) > 0


@pytest.mark.parametrize("D", [128, 144])
def test_filters(ops, D):
    N = 485
    base, q, v = case("u8", D, N)
    radii = np.sort(v, axis=1)[:, N // 3].astype(np.float32)
    rng = np.random.default_rng(71)
    mask = rng.random(N) < 0.4
    cases = [(np.broadcast_to(mask, (NQ, N)),
              dict(filter_bits=dev(pack_bits(mask, 64)), filter_bit_offset=64))]
    masks = rng.random((2, N)) < 0.5
    fids = rng.choice(np.array([0, 1, -1, 9], np.int32), NQ)
    allowed = np.stack([masks[f] if 0 <= f < 2 else np.full(N, f == -1) for f in fids])
    cases.append((allowed, dict(filter_table=dev(np.stack([pack_bits(m) for m in masks])),
                                filter_ids=dev(fids))))
    labels = rng.integers(0, 5, N).astype(np.int32)
    qlab = rng.choice(np.array([0, 1, 4, -1, 77], np.int32), NQ)
    allowed = np.stack([np.full(N, True) if L == -1 else labels == L for L in qlab])
    cases.append((allowed, dict(labels=dev(labels), query_labels=dev(qlab))))
    for i, (allowed, kw) in enumerate(cases):
        want = expected(v, radii, allowed)
        for s, got in run(ops, dev(base), dev(q), radii, **kw):
            assert_same(got, want, f"filter case {i}, {s} parts")


def test_capacity(ops):
    base, q, v = case("u8", 128, 485)
    radii = cycle_radii(v)
    want = expected(v, radii)
    total = int(want[0][-1])
    b, qd = dev(base), dev(q)
    ids = torch.full((total,), -7, dtype=torch.int32, device="cuda")
    dd = torch.full((total,), -7.0, dtype=torch.float32, device="cuda")
    for s, got in run(ops, b, qd, radii, capacity=total - 1, out=(ids, dd)):
        assert np.array_equal(got[0].cpu().numpy(), want[0])
        assert (ids.cpu().numpy() == -7).all() and (dd.cpu().numpy() == -7.0).all()
    for s, got in run(ops, b, qd, radii, capacity=0):
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and got[1].numel() == 0
    for s, got in run(ops, b, qd, radii, capacity=total, out=(ids, dd)):
        assert_same(got, want, f"capacity = total, {s} parts")


def test_handle(ops):
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    base, q, v = case("i8", 128, 485)
    radii = np.sort(v, axis=1)[:, 20].astype(np.float32)
    eng = ggnn.GGNN()
    eng.set_base(base)
    with _lib.hooks(BF_RANGE_I8_COS=2):
        got = eng.bf_range_query(q, radii, ggnn.DistanceMeasure.Cosine, sort=False)
        assert eng.last_bf_range_matrix_path() == 2
    assert_same(got, expected(v, radii), "handle")
