"""Range search on the tile kernels (bf_range_mfma.hip) against the scan's expected values, bit for bit.

Expected values as in test_gpu_bf_range.py: the CPU oracle in the kernels' order (float32 rows), or
numpy where every sum is exact -- 16-bit rows have no oracle layout, so their data keeps the direct
form exact.  Squared L2: even columns 960 + 4k, odd ones 100 + k/2 (exact in bfloat16): the norms
round, the differences stay exact.  Cosine: small integers (its two forms share their sums).
N = 1061 rows = 33 tiles + 5; Nq = 150 = a query block and a partial one with a partial wave;
BF_RANGE_SLICES = 1, 3, 4 cuts at multiples of 384 and 288; BF_RANGE_PATH = 2 sends these shapes to the
tiles; BF_RANGE_CAND = Nq * N keeps every candidate, except where the test is about the budget."""
import numpy as np
import pytest

from test_gpu_bf_range import (assert_same, data, dev, expected, l2_exact, oracle_distances,  # noqa: F401
                               ops, pack_bits, sorted_expected)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, NQ, SLICES = 1061, 150, (1, 3, 4)
TIED = (100, 287, 288, 383, 384, 767, 768, 1060)   # one row on both sides of tile and part cuts
HALF = {"f16": torch.float16, "bf16": torch.bfloat16}


to_dev = lambda a, t: dev(a) if t == "f32" else dev(a).to(HALF[t])  # noqa: E731
_cases = {}


def case(orc, t, D, measure, kind="plain"):
    # (base, q, dist): computed once per cell, shared by the tests, never changed
    key = (t, D, measure, kind)
    if key not in _cases:
        rng = np.random.default_rng(9000 + D + 7 * measure + len(kind))
        if t == "f32":
            off = 100.0 if kind == "offset" else 0.0
            base = (off + rng.standard_normal((N, D))).astype(np.float32)
            q = (off + rng.standard_normal((NQ, D))).astype(np.float32)
        elif measure == 0:
            col = np.arange(D) % 2
            mixed = lambda n: np.where(col, 100 + rng.integers(0, 32, (n, D)) / 2,
                                       960 + 4 * rng.integers(0, 16, (n, D))).astype(np.float32)
            base, q = mixed(N), mixed(NQ)
        else:
            base = rng.integers(0, 16, (N, D)).astype(np.float32)
            q = rng.integers(0, 16, (NQ, D)).astype(np.float32)
        for i in TIED[1:]:
            base[i] = base[TIED[0]]
        q[1] = base[500]                                   # radius 0 has a hit
        if t == "f32" or measure == 1:
            dist = oracle_distances(orc, base, q, measure)
        else:
            d64 = ((q.astype(np.float64)[:, None] - base.astype(np.float64)[None]) ** 2).sum(-1)
            dist = d64.astype(np.float32)
            assert (dist == d64).all() and d64.max() * 4 < 2 ** 24
            assert (base.astype(np.float64) ** 2).sum(1).max() * 4 > 2 ** 24 or D < 128
        _cases[key] = (base, q, dist)
    return _cases[key]


def cycle_radii(dist, seed=5):  # -1, 0, NaN, row minimum, the tie's distance, median, quantiles
    rng = np.random.default_rng(seed)
    srt = np.sort(dist, axis=1)
    r = srt[np.arange(NQ), rng.integers(0, 40, NQ)].astype(np.float32)
    r[0::8], r[1::8], r[2::8] = -1.0, 0.0, np.nan
    r[3::8] = srt[3::8, 0]
    r[4::8] = dist[4::8, TIED[0]]
    r[5::8] = srt[5::8, N // 2]
    return r


def run(ops, b, q, radii, measure, slices=SLICES, fell=0, path=1, hooks=None, **kw):
    from ggnn_amd import _lib
    for s in slices:
        with _lib.hooks(BF_RANGE_PATH=2, BF_RANGE_SLICES=s, **{"BF_RANGE_CAND": NQ * N, **(hooks or {})}):
            got = ops.bf_range_query(b, q, dev(radii), measure, routed=True, **kw)
        assert got[3] == path and (got[4] >= 1) == bool(fell), (s, got[3:])
        yield s, got[:3]


PARITY = ([("f32", D, m, "plain") for D in (4, 64, 100, 128, 144, 260) for m in (0, 1)] +
          [(t, D, m, "plain") for t in HALF for D in (8, 128, 136) for m in (0, 1)] +
          [("f32", 100, 0, "offset"), ("f32", 100, 0, "offset-nocenter")])


@pytest.mark.parametrize("t,D,measure,kind", PARITY, ids=["-".join(map(str, c)) for c in PARITY])
def test_parity(orc, ops, t, D, measure, kind):
    base, q, dist = case(orc, t, D, measure, kind.split("-")[0])
    radii = cycle_radii(dist)
    want = expected(dist, radii)
    tied = set(np.nonzero(dist[4] == radii[4])[0].tolist())
    assert set(TIED) <= tied and want[0][1] == 0 and (measure or want[0][2] - want[0][1] >= 1)
    hooks = {"BF_NO_CENTER": int(kind.endswith("nocenter"))}
    b, qd = to_dev(base, t), to_dev(q, t)
    for s, got in run(ops, b, qd, radii, measure, hooks=hooks):
        assert_same(got, want, f"{t} D={D} m={measure} {kind}, {s} parts")
    # +inf radii, a batch of their own
    radii = np.full(NQ, np.inf, np.float32)
    for s, got in run(ops, b, qd, radii, measure, slices=(3,), hooks=hooks):
        assert_same(got, expected(dist, radii), f"{t} D={D} m={measure} {kind}, +inf")


@pytest.mark.parametrize("kind,measure", [("plain", 0), ("plain", 1), ("offset-nocenter", 0)])
def test_sharp_threshold(orc, ops, kind, measure):
    """r = the distance of one chosen pair per query, then the float below it: it appears, then not"""
    base, q, dist = case(orc, "f32", 100, measure, kind.split("-")[0])
    pick = (np.arange(NQ) * 7 + 3) % N
    hooks = {"BF_NO_CENTER": int(kind.endswith("nocenter"))}
    for step in (0, 1):
        radii = dist[np.arange(NQ), pick].copy()
        if step:
            radii = np.nextafter(radii, np.float32(0))
        want = expected(dist, radii)
        for s, got in run(ops, dev(base), dev(q), radii, measure, slices=(3,), hooks=hooks):
            assert_same(got, want, f"{kind} step {step}")
            lims, ids = got[0].cpu().numpy(), got[1].cpu().numpy()
            inside = [pick[n] in ids[lims[n]:lims[n + 1]] for n in range(NQ)]
            assert all(inside) if step == 0 else not any(inside)


def test_fallback_and_capacity(orc, ops):
    base, q, dist = case(orc, "f32", 64, 0)
    b, qd = dev(base), dev(q)
    radii = np.median(dist, axis=1).astype(np.float32)
    want = expected(dist, radii)
    total = int(want[0][-1])
    for s, got in run(ops, b, qd, radii, 0, fell=1, hooks={"BF_RANGE_CAND": 64}):
        assert_same(got, want, f"budget 64, {s} parts")
    # a capacity below the total: lims right, outputs as pre-filled; count only: lims
    ids = torch.full((total,), -7, dtype=torch.int32, device="cuda")
    d = torch.full((total,), -7.0, dtype=torch.float32, device="cuda")
    for s, got in run(ops, b, qd, radii, 0, capacity=total - 1, out=(ids, d)):
        assert np.array_equal(got[0].cpu().numpy(), want[0])
        assert (ids.cpu().numpy() == -7).all() and (d.cpu().numpy() == -7.0).all()
    for s, got in run(ops, b, qd, radii, 0, capacity=0):
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and got[1].numel() == 0
    radii = np.full(NQ, np.inf, np.float32)  # count only, default budget (32 Nq + 1/8): the scan
    for s, got in run(ops, b, qd, radii, 0, fell=1, hooks={"BF_RANGE_CAND": 0}, capacity=0):
        assert np.array_equal(got[0].cpu().numpy(), np.arange(NQ + 1) * N), s


@pytest.mark.parametrize("t,D,measure", [("f32", 64, 0), ("f32", 144, 1), ("f16", 136, 0)])
def test_filters(orc, ops, t, D, measure):
    base, q, dist = case(orc, t, D, measure)
    b, qd = to_dev(base, t), to_dev(q, t)
    radii = np.sort(dist, axis=1)[:, N // 3].astype(np.float32)
    rng = np.random.default_rng(93)
    mask = rng.random(N) < 0.4
    cases = []
    for off in (0, 64, 5):                                 # (5: no word per tile -- the scan)
        cases.append((np.broadcast_to(mask, (NQ, N)), int(off != 5),
                      dict(filter_bits=dev(pack_bits(mask, off)), filter_bit_offset=off)))
    cases.append((np.zeros((NQ, N), bool), 1, dict(filter_bits=dev(pack_bits(np.zeros(N, bool))))))
    masks = rng.random((3, N)) < 0.5
    masks[2] = False
    fids = rng.choice(np.array([0, 1, 2, -1, 9], np.int32), NQ)
    allowed = np.stack([masks[f] if 0 <= f < 3 else np.full(N, f == -1) for f in fids])
    cases.append((allowed, 1, dict(filter_table=dev(np.stack([pack_bits(m) for m in masks])),
                                   filter_ids=dev(fids))))
    labels = rng.integers(0, 5, N).astype(np.int32)
    qlab = rng.choice(np.array([0, 1, 4, -1, 77], np.int32), NQ)
    allowed = np.stack([np.full(N, True) if L == -1 else labels == L for L in qlab])
    cases.append((allowed, 1, dict(labels=dev(labels), query_labels=dev(qlab))))
    for i, (allowed, path, kw) in enumerate(cases):
        want = expected(dist, radii, allowed)
        for s, got in run(ops, b, qd, radii, measure, path=path, **kw):
            assert_same(got, want, f"filter case {i}, {s} parts")


def test_automatic_routing_and_handle(ops):  # the default minima, no hook; exact integer rows
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    base, q = data("f32", 4096, 32, 9100), data("f32", 256, 32, 9101)
    dist = l2_exact(base, q)
    radii = np.sort(dist, axis=1)[:, 20].astype(np.float32)
    want = expected(dist, radii)
    got = ops.bf_range_query(dev(base), dev(q), dev(radii), routed=True)
    assert got[3:] == (1, 0)
    assert_same(got[:3], want, "automatic")
    eng = ggnn.GGNN()
    eng.set_base(base)
    assert eng.last_bf_range_matrix_path() == 0
    assert_same(eng.bf_range_query(q, radii, sort=False), want, "handle, sort=False")
    assert eng.last_bf_range_matrix_path() == 1
    assert_same(eng.bf_range_query(q, radii), sorted_expected(want), "handle, sort=True")
    with _lib.hooks(BF_RANGE_PATH=1):
        scan = eng.bf_range_query(q, radii, sort=False)
        assert eng.last_bf_range_matrix_path() == 0
    assert_same(scan, want, "handle, scan")
