"""Range search of uint8 / int8 rows on the integer tile kernels (bf_range_i8.hip), bit for bit.

Expected values from numpy in int64: d = ((b - q) ** 2).sum(), a hit iff float32(d) <= r, the value
float32(d), ids ascending, lims exact; every case also equals the scan kernels' answer to the same
call (BF_RANGE_I8 = 1).  BF_RANGE_I8 = 2 sends these small shapes to the tiles.
N = 485 = 15 tiles + 5 rows and N = 97 = 3 tiles + 1; Nq = 130 = two 64-query waves and a partial
32-query set; BF_RANGE_SLICES = 1, 3 cuts inside the base (at 192 and 384 / at 64)."""
import numpy as np
import pytest

from test_gpu_bf_range import assert_same, dev, expected, ops, pack_bits  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NQ, TWIN, BIG_ROW, BIG_Q = 130, 200 % 97, 7, 5
NP = {"u8": np.uint8, "i8": np.int8}
_cases = {}


def case(t, D, N):
    """(base, q, d int64 [NQ, N]): once per cell, never changed.  Full value range; query 1 is row
    TWIN; row BIG_ROW is the type's maximum and query BIG_Q its minimum: d = D * 255^2"""
    if (t, D, N) not in _cases:
        rng = np.random.default_rng(7000 + D + N + len(t) * (t == "i8"))
        info = np.iinfo(NP[t])
        base = rng.integers(info.min, info.max + 1, (N, D)).astype(NP[t])
        q = rng.integers(info.min, info.max + 1, (NQ, D)).astype(NP[t])
        q[1], base[BIG_ROW], q[BIG_Q] = base[TWIN], info.max, info.min
        d = ((q.astype(np.int64)[:, None] - base.astype(np.int64)[None]) ** 2).sum(-1)
        _cases[(t, D, N)] = (base, q, d)
    return _cases[(t, D, N)]


def cycle_radii(d, D):
    """per query, from the pair distances: negative, 0 (query 1: its twin), a distance itself, half
    below it, half above it, a non-integer, the extreme pair's bound, +inf (D <= 128: every row)"""
    srt = np.sort(d, axis=1).astype(np.float64)
    r = srt[:, 20] + 0.25
    r[0::8], r[1::8], r[2::8] = -1.0, 0.0, srt[2::8, 20]
    r[3::8], r[4::8] = srt[3::8, 20] - 0.5, srt[4::8, 20] + 0.5
    r[BIG_Q::8] = min(2.0 ** 24 - 1, D * 255.0 ** 2 - 1)     # below d of (BIG_Q, BIG_ROW)
    if D <= 128:
        r[7::8] = np.inf
    return r.astype(np.float32)


def run(ops, b, q, radii, slices=(1, 3), fell=0, **kw):
    """the tiles' answers (asserted equal to the scan's, and routed to the integer kernels)"""
    from ggnn_amd import _lib
    r = dev(radii)
    with _lib.hooks(BF_RANGE_I8=1):
        scan = ops.bf_range_query(b, q, r, routed=True, **kw)
    assert scan[3:] == (0, 0)
    for s in slices:
        with _lib.hooks(BF_RANGE_I8=2, BF_RANGE_SLICES=s):
            got = ops.bf_range_query(b, q, r, routed=True, **kw)
        assert got[3:] == (2, fell), (s, got[3:])
        assert_same(got[:3], tuple(x.cpu().numpy() for x in scan[:3]), f"against the scan, {s} parts")
        yield s, got[:3]


@pytest.mark.parametrize("N", [485, 97])
@pytest.mark.parametrize("D", [16, 128, 144, 272])
@pytest.mark.parametrize("t", ["u8", "i8"])
def test_parity(ops, t, D, N):
    base, q, d = case(t, D, N)
    radii = cycle_radii(d, D)
    want = expected(d.astype(np.float32), radii)
    assert want[0][2] - want[0][1] >= 1 and want[0][1] == 0           # the twin at radius 0; -1: none
    assert d[BIG_Q, BIG_ROW] == D * 255 ** 2 and (D < 272 or d[BIG_Q, BIG_ROW] >= 2 ** 24)
    for s, got in run(ops, dev(base), dev(q), radii):
        assert_same(got, want, f"{t} D={D} N={N}, {s} parts")
        lims, ids = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert BIG_ROW not in ids[lims[BIG_Q]:lims[BIG_Q + 1]]


def test_int8_is_shifted_uint8(ops):
    base, q, d = case("i8", 144, 485)
    radii = cycle_radii(d, 144)
    ub, uq = base.view(np.uint8) ^ 0x80, q.view(np.uint8) ^ 0x80
    for (s, got), (_, ref) in zip(run(ops, dev(base), dev(q), radii), run(ops, dev(ub), dev(uq), radii)):
        assert_same(got, tuple(x.cpu().numpy() for x in ref), f"int8 against uint8, {s} parts")


@pytest.mark.parametrize("t", ["u8", "i8"])
def test_radius_from_two_to_the_24_falls_back_at_d_272(ops, t):
    base, q, d = case(t, 272, 485)
    radii = cycle_radii(d, 272)
    radii[3], radii[4] = 2.0 ** 24, np.inf
    got = [g for _, g in run(ops, dev(base), dev(q), radii, fell=1)]      # equal to the scan's
    lims = got[0][0].cpu().numpy()
    assert lims[5] - lims[4] == 485 and lims[4] - lims[3] >= 484


@pytest.mark.parametrize("D", [128, 144])
def test_filters(ops, D):
    N = 485
    base, q, d = case("u8", D, N)
    radii = np.sort(d, axis=1)[:, N // 3].astype(np.float32)
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
        want = expected(d.astype(np.float32), radii, allowed)
        for s, got in run(ops, dev(base), dev(q), radii, **kw):
            assert_same(got, want, f"filter case {i}, {s} parts")


def test_capacity(ops):
    base, q, d = case("u8", 128, 485)
    radii = cycle_radii(d, 128)
    want = expected(d.astype(np.float32), radii)
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
    base, q, d = case("u8", 128, 485)
    radii = np.sort(d, axis=1)[:, 20].astype(np.float32)
    eng = ggnn.GGNN()
    eng.set_base(base)
    with _lib.hooks(BF_RANGE_I8=2):
        got = eng.bf_range_query(q, radii, sort=False)
        assert eng.last_bf_range_matrix_path() == 2
    assert_same(got, expected(d.astype(np.float32), radii), "handle")
