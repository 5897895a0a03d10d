"""CPU: float16 / bfloat16 base and query rows (GGNN_F16 = 2, GGNN_BF16 = 3) at the boundary.

The row layout table of 16-bit rows (8 elements per 16-byte chunk), the GPU matrix of
tests/test_gpu_half_parity.py covering every cell of it, what set_base accepts (CPU tensors, numpy
float16, D not a multiple of 8), that a query of another element type is refused, and the C-ABI's
dtype codes.  No compute calls."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HALF = (torch.float16, torch.bfloat16)
# chunks = ceil(D / 8) -> (lanes per row, chunks per lane), traversal.hpp pick_dist_config
TABLE = ((64, (8, 1)), (128, (8, 2)), (192, (8, 3)), (256, (16, 2)), (512, (16, 4)),
         (2048, (64, 4)), (4096, (64, 16)))


def expected_layout(D):
    for d_max, layout in TABLE:
        if D <= d_max:
            return layout
    raise AssertionError(D)


@pytest.mark.parametrize("dtype", HALF)
def test_dist_layout_of_16bit_rows(dtype):
    from ggnn_amd import ops
    for D in range(1, 4097):
        assert ops.dist_layout(D, dtype) == expected_layout(D), (dtype, D)


def test_gpu_matrix_covers_every_16bit_cell():
    from ggnn_amd import ops
    from test_gpu_half_parity import MATRIX
    cells = {expected_layout(D) for D in range(1, 4097)}
    assert len(cells) == 7
    for name, dtype in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        covered = {(ops.dist_layout(D, dtype), m) for t, D, m in MATRIX if t == name}
        missing = sorted((c, m) for c in cells for m in (0, 1) if (c, m) not in covered)
        assert not missing, (name, missing)


def _rows(kind, N, D):
    a = np.random.default_rng(5).random((N, D)).astype(np.float32)
    if kind == "np-f16":
        return a.astype(np.float16)
    return torch.from_numpy(a).to(torch.float16 if kind == "f16" else torch.bfloat16)


@pytest.mark.parametrize("kind", ["f16", "bf16", "np-f16"])
@pytest.mark.parametrize("D", [64, 100])      # 100: rows padded to 104 elements
def test_set_base_accepts_16bit_rows(kind, D):
    import ggnn_amd as ggnn
    eng = ggnn.GGNN()
    eng.set_base(_rows(kind, 300, D))
    eng2 = ggnn.GGNN()
    eng2.set_base_reference(_rows(kind, 300, D))


QUERY_TYPES = {
    "f32": lambda a: torch.from_numpy(a),
    "u8": lambda a: torch.from_numpy((a * 255).astype(np.uint8)),
    "f16": lambda a: torch.from_numpy(a).to(torch.float16),
    "bf16": lambda a: torch.from_numpy(a).to(torch.bfloat16),
}


@pytest.mark.parametrize("base_t,query_t",
                         [(b, q) for b in QUERY_TYPES for q in QUERY_TYPES if b != q])
def test_query_of_another_dtype_is_refused(base_t, query_t):
    import ggnn_amd as ggnn
    a = np.random.default_rng(7).random((200, 64)).astype(np.float32)
    eng = ggnn.GGNN()
    eng.set_base(QUERY_TYPES[base_t](a))
    with pytest.raises(RuntimeError, match="query data type does not match"):
        eng.bf_query(QUERY_TYPES[query_t](a[:5]), 10)


def test_float64_is_still_refused():
    import ggnn_amd as ggnn
    from ggnn_amd import ops
    eng = ggnn.GGNN()
    with pytest.raises(TypeError, match="float32, uint8, float16 and bfloat16"):
        eng.set_base(np.zeros((10, 16), np.float64))
    with pytest.raises(TypeError, match="float32, uint8, float16 or bfloat16"):
        ops._dtype_code(torch.zeros(2, 2, dtype=torch.float64))


def test_c_abi_dtype_codes():
    from ggnn_amd import _lib
    lib = _lib.lib()
    assert (_lib.F16, _lib.BF16) == (2, 3)
    data = np.zeros((16, 8), np.uint16)
    for code, want in ((_lib.F16, _lib.OK), (_lib.BF16, _lib.OK), (4, _lib.INVALID_ARGUMENT)):
        h = C.c_void_p()
        assert lib.ggnn_create(C.byref(h)) == _lib.OK
        try:
            st = lib.ggnn_set_base(h, data.ctypes.data, 16, 8, code, _lib.CPU, 0, 1)
            assert st == want, (code, st, lib.ggnn_last_error(h))
        finally:
            lib.ggnn_destroy(h)
    lpr, nch = C.c_uint32(), C.c_uint32()
    assert lib.ggnn_op_dist_layout(128, 4, C.byref(lpr), C.byref(nch)) == _lib.INVALID_ARGUMENT


@pytest.mark.parametrize("dtype", HALF)
def test_evaluator_widens_16bit_rows(dtype):
    """Evaluator on 16-bit rows (numpy has no bfloat16) equals Evaluator on the widened copy"""
    import ggnn_amd as ggnn
    r = np.random.default_rng(9)
    base = torch.from_numpy(r.integers(0, 256, (500, 32)).astype(np.float32))
    q = torch.from_numpy(r.integers(0, 256, (20, 32)).astype(np.float32))
    d = ((q[:, None, :] - base[None]) ** 2).sum(-1)
    gt = torch.argsort(d, dim=1, stable=True)[:, :10].to(torch.int32).contiguous()
    res = torch.flip(gt, [1]).contiguous()
    a = ggnn.Evaluator(base.to(dtype), q.to(dtype), gt, 10).evaluate_results(res)
    b = ggnn.Evaluator(base, q, gt, 10).evaluate_results(res)
    assert repr(a) == repr(b) and a.c1 == b.c1 and a.r_k_query == b.r_k_query
