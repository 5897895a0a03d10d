"""bf_query of float16 / bfloat16 rows on the 16-bit tile kernels (bf_f16.hip), bit for bit.

BF_F16 = 2 sends these small shapes to the tiles; every case asserts that the handle reports path 2.
Exact-sum data (integers in [-32, 32]: every sum is below 2^24, exact in any order) against numpy in
float64, ordered by (distance, id).  D: 8 below one instruction step, 24 padded to 32, 128 a full single
chunk, 136 chunked with a short last chunk, 264 three chunks.  N = 100 is less than one stage, N = 1000
ends in a ragged tile; Nq = 130 is a ragged query block and a ragged 32-query set.  Rows are duplicated
across the part boundaries that BF_SLICES = 3 and the automatic split cut at (512; 384 and 768).
Fractional data against the scan kernels (BF_SCAN = 1)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
NQ = 130
_cases = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggnn_amd import ops as o
    return o


def tiles(ops, b, q, K, slices=0):
    """the 16-bit tiles' answer: (ids, dist bits as uint32, rescanned), path 2 asserted on a handle"""
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    with _lib.hooks(BF_F16=2, BF_SLICES=slices):
        ids, d, resc = ops.bf_query(b, q, K, 0, rescanned=True)
        eng = ggnn.GGNN()
        eng.set_base_reference(b)
        eng.set_return_results_on_gpu(True)
        h_ids, h_d = eng.bf_query(q, K, ggnn.DistanceMeasure.Euclidean)
        assert eng.last_bf_query_matrix_path() == 2
    assert torch.equal(h_ids, ids) and torch.equal(h_d.view(torch.int32), d.view(torch.int32))
    return ids.cpu().numpy(), d.cpu().numpy().view(np.uint32), resc


def int_case(D, N):
    """(base, q as float32 numpy, ids [NQ, N] in (distance, id) order, d float32): once, never changed"""
    if (D, N) not in _cases:
        rng = np.random.default_rng(100 * D + N)
        base = rng.integers(-32, 33, (N, D)).astype(np.float32)
        q = rng.integers(-32, 33, (NQ, D)).astype(np.float32)
        if N == 1000:
            base[500:560], base[760:800] = base[440:500], base[730:770]   # twins across 512 and 768
            base[384:394] = base[374:384]                                  # ... and across 384
            q[5:65], q[70:80] = base[440:500], base[374:384]               # distance 0, two ids each
        else:
            base[60:70], q[5:15] = base[20:30], base[20:30]
        d = ((q.astype(np.float64)[:, None] - base.astype(np.float64)[None]) ** 2).sum(-1)
        order = np.argsort(d, axis=1, kind="stable")
        _cases[(D, N)] = (base, q, order, np.take_along_axis(d, order, 1).astype(np.float32))
    return _cases[(D, N)]


@pytest.mark.parametrize("N", [100, 1000])
@pytest.mark.parametrize("D", [8, 24, 128, 136, 264])
@pytest.mark.parametrize("t", list(DT))
def test_exact_sums_against_float64(ops, t, D, N):
    base, q, order, dist = int_case(D, N)
    b, dq = torch.from_numpy(base).cuda().to(DT[t]), torch.from_numpy(q).cuda().to(DT[t])
    for K in (1, 10, 100):
        for slices in (0, 3):
            ids, bits, resc = tiles(ops, b, dq, K, slices)
            assert np.array_equal(ids, order[:, :K]), (K, slices)
            assert np.array_equal(bits, dist[:, :K].view(np.uint32)), (K, slices)


def frac_case(kind, t):
    """N(0,1) rounded to the type (D = 128, N = 4096, Nq = 256); `offset`: + 1000 in every column
    (cancellation); `decades`: rows scaled over three decades.  No value is subnormal in its type."""
    rng = np.random.default_rng(31)
    base, q = rng.normal(size=(4096, 128)).astype(np.float32), rng.normal(size=(256, 128)).astype(np.float32)
    if kind == "offset":
        base, q = base + 1000, q + 1000
    if kind == "decades":
        base, q = base * 10.0 ** rng.uniform(-1.5, 1.5, (4096, 1)), q * 10.0 ** rng.uniform(-1.5, 1.5, (256, 1))
    base[np.abs(base) < 1e-4], q[np.abs(q) < 1e-4] = 0, 0
    return (torch.from_numpy(base.astype(np.float32)).cuda().to(DT[t]),
            torch.from_numpy(q.astype(np.float32)).cuda().to(DT[t]))


def scan(ops, b, q, K):
    from ggnn_amd import _lib
    with _lib.hooks(BF_SCAN=1):
        ids, d = ops.bf_query(b, q, K, 0)
    return ids.cpu().numpy(), d.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", ["normal", "offset", "decades"])
@pytest.mark.parametrize("t", list(DT))
def test_fractional_data_equals_the_scan(ops, t, kind):
    b, q = frac_case(kind, t)
    s_ids, s_bits = scan(ops, b, q, 10)
    ids, bits, resc = tiles(ops, b, q, 10)
    assert np.array_equal(ids, s_ids) and np.array_equal(bits, s_bits)
    if kind == "normal":   # otherwise equality with the scan shows nothing about the tiles
        assert resc <= 256 // 10, resc


@pytest.mark.parametrize("what", ["subnormal-in-base", "inf-in-query"])
@pytest.mark.parametrize("t", list(DT))
def test_ineligible_input_is_answered_by_the_scan(ops, t, what):
    b, q = frac_case("normal", t)
    if what == "subnormal-in-base":
        b.view(torch.int16)[7, 3] = 1        # the smallest subnormal of either type
    else:
        q[5, 2] = float("inf")
    s_ids, s_bits = scan(ops, b, q, 10)
    ids, bits, resc = tiles(ops, b, q, 10)
    assert resc == 256
    assert np.array_equal(ids, s_ids) and np.array_equal(bits, s_bits)
