"""Range search of float16 / bfloat16 rows on the 16-bit tile kernels (bf_range_f16.hip), bit for bit.

Expected values from numpy in float64 on the exact-sum data of test_gpu_bf_range_mfma.case (the norms
round, the differences stay exact; ties on both sides of tile and part cuts), or -- random data, whose
roundings no plain reference gives -- the scan's answer to the same call (BF_RANGE_PATH = 1).
N = 1061 rows = 33 tiles + 5; Nq = 150 = two full waves and one with a partial first set (a workgroup
takes 256 queries); the random-row cases run Nq = 300, a full workgroup and a partial second one;
BF_RANGE_SLICES = 1, 3, 4; BF_RANGE_F16 = 2 sends these shapes to the 16-bit tiles; BF_RANGE_CAND = Nq * N
keeps every candidate, except where the test is about the budget."""
import numpy as np
import pytest

from test_gpu_bf_range import assert_same, dev, expected, ops, pack_bits  # noqa: F401
from test_gpu_bf_range_mfma import HALF, N, NQ, SLICES, case, cycle_radii, to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def run(ops, b, q, radii, slices=SLICES, fell=0, path=3, hooks=None, **kw):
    from ggnn_amd import _lib
    for s in slices:
        with _lib.hooks(BF_RANGE_F16=2, BF_RANGE_SLICES=s,
                        **{"BF_RANGE_CAND": len(radii) * N, **(hooks or {})}):
            got = ops.bf_range_query(b, q, dev(radii), 0, routed=True, **kw)
        assert (got[3] == 3) == (path == 3) and got[4] == fell, (s, got[3:])
        yield s, got[:3]


@pytest.mark.parametrize("D", [8, 32, 64, 128, 136, 264])
@pytest.mark.parametrize("t", list(HALF))
def test_parity(ops, t, D):
    base, q, dist = case(None, t, D, 0)
    radii = cycle_radii(dist)
    want = expected(dist, radii)
    assert want[0][1] == 0 and want[0][2] - want[0][1] >= 1        # -1: none; 0: the twin
    b, qd = to_dev(base, t), to_dev(q, t)
    for s, got in run(ops, b, qd, radii):
        assert_same(got, want, f"{t} D={D}, {s} parts")
    radii = np.full(NQ, np.inf, np.float32)                        # +inf radii, a batch of their own
    for s, got in run(ops, b, qd, radii, slices=(3,)):
        assert_same(got, expected(dist, radii), f"{t} D={D}, +inf")


@pytest.mark.parametrize("bits", [False, True], ids=["plain", "bitset"])
@pytest.mark.parametrize("t,D", [("bf16", 128), ("f16", 200)])
def test_random_rows_two_query_blocks_equal_the_scan(ops, t, D, bits):
    """Nq = 300: a full workgroup of 256 queries, and a second one with one partial wave (queries 256
    .. 299: a full set and 12 of 32) and three absent waves"""
    from ggnn_amd import _lib
    nq = 300
    rng = np.random.default_rng(40 + D)
    base, q = (rng.standard_normal((n, D)).astype(np.float32) for n in (N, nq))
    if t == "f16":                                                 # no float16 subnormals
        base[np.abs(base) < 2.0 ** -14], q[np.abs(q) < 2.0 ** -14] = 0, 0
    b, qd = to_dev(base, t), to_dev(q, t)
    d = ((qd.double()[:, None] - b.double()[None]) ** 2).sum(-1).cpu().numpy()
    radii = np.sort(d, axis=1)[np.arange(nq), np.arange(nq) % 60].astype(np.float32)
    kw = dict(filter_bits=dev(pack_bits(rng.random(N) < 0.5, 32)), filter_bit_offset=32) if bits else {}
    with _lib.hooks(BF_RANGE_PATH=1):
        scan = ops.bf_range_query(b, qd, dev(radii), 0, routed=True, **kw)
    lims = scan[0].cpu().numpy()
    assert scan[3:] == (0, 0) and (np.diff(lims)[256:] > 0).any()  # the second block has rows to return
    for s, got in run(ops, b, qd, radii, **kw):
        assert_same(got, tuple(x.cpu().numpy() for x in scan[:3]), f"{t} against the scan, {s} parts")


@pytest.mark.parametrize("t,D", [("bf16", 64), ("f16", 136)])
def test_filters(ops, t, D):
    base, q, dist = case(None, t, D, 0)
    b, qd = to_dev(base, t), to_dev(q, t)
    radii = np.sort(dist, axis=1)[:, N // 3].astype(np.float32)
    rng = np.random.default_rng(93)
    mask = rng.random(N) < 0.4
    cases = []
    for off in (0, 64, 5):                                 # (5: no word per tile -- not these tiles)
        cases.append((np.broadcast_to(mask, (NQ, N)), 3 if off != 5 else 0,
                      dict(filter_bits=dev(pack_bits(mask, off)), filter_bit_offset=off)))
    cases.append((np.zeros((NQ, N), bool), 3, dict(filter_bits=dev(pack_bits(np.zeros(N, bool))))))
    masks = rng.random((3, N)) < 0.5
    masks[2] = False
    fids = rng.choice(np.array([0, 1, 2, -1, 9], np.int32), NQ)
    allowed = np.stack([masks[f] if 0 <= f < 3 else np.full(N, f == -1) for f in fids])
    cases.append((allowed, 3, dict(filter_table=dev(np.stack([pack_bits(m) for m in masks])),
                                   filter_ids=dev(fids))))
    labels = rng.integers(0, 5, N).astype(np.int32)
    qlab = rng.choice(np.array([0, 1, 4, -1, 77], np.int32), NQ)
    allowed = np.stack([np.full(N, True) if L == -1 else labels == L for L in qlab])
    cases.append((allowed, 3, dict(labels=dev(labels), query_labels=dev(qlab))))
    for i, (allowed, path, kw) in enumerate(cases):
        want = expected(dist, radii, allowed)
        for s, got in run(ops, b, qd, radii, path=path, **kw):
            assert_same(got, want, f"filter case {i}, {s} parts")


def test_fallbacks_and_capacity(ops):
    base, q, dist = case(None, "f16", 64, 0)
    b, qd = to_dev(base, "f16"), to_dev(q, "f16")
    radii = np.median(dist, axis=1).astype(np.float32)
    want = expected(dist, radii)
    total = int(want[0][-1])
    for s, got in run(ops, b, qd, radii, fell=1, hooks={"BF_RANGE_CAND": 64}):
        assert_same(got, want, f"budget 64, {s} parts")
    # one float16 subnormal element (2^-24; its square is below every distance's last bit): the flag
    sub = b.clone()
    sub[700, 3] = 2.0 ** -24
    d_sub = dist.copy()
    d_sub[:, 700] = ((q.astype(np.float64) - sub[700].double().cpu().numpy()) ** 2).sum(-1)
    for s, got in run(ops, sub, qd, radii, fell=1):
        assert_same(got, expected(d_sub, radii), f"subnormal element, {s} parts")
    # a capacity below the total: lims right, outputs as pre-filled; count only: lims
    ids = torch.full((total,), -7, dtype=torch.int32, device="cuda")
    d = torch.full((total,), -7.0, dtype=torch.float32, device="cuda")
    for s, got in run(ops, b, qd, radii, capacity=total - 1, out=(ids, d)):
        assert np.array_equal(got[0].cpu().numpy(), want[0])
        assert (ids.cpu().numpy() == -7).all() and (d.cpu().numpy() == -7.0).all()
    for s, got in run(ops, b, qd, radii, capacity=0):
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and got[1].numel() == 0


def test_routing_and_handle(ops):
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    base, q, dist = case(None, "bf16", 128, 0)
    radii = np.sort(dist, axis=1)[:, 20].astype(np.float32)
    want = expected(dist, radii)
    eng = ggnn.GGNN()
    eng.set_base_reference(to_dev(base, "bf16"))
    eng.set_return_results_on_gpu(True)
    with _lib.hooks(BF_RANGE_F16=2):
        got = eng.bf_range_query(to_dev(q, "bf16"), radii, sort=False)
        assert eng.last_bf_range_matrix_path() == 3
    assert_same(got, want, "handle, 16-bit tiles")
    with _lib.hooks(BF_RANGE_F16=1, BF_RANGE_PATH=2):
        got = eng.bf_range_query(to_dev(q, "bf16"), radii, sort=False)
        assert eng.last_bf_range_matrix_path() == 1
    assert_same(got, want, "handle, float32-staged tiles")
