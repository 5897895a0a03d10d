"""The range tile path without a GPU: routing, hooks, C surface, registers and LDS of its kernels."""
import ctypes as C
import os

import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture: the library's kernel metadata)

# (dtype, D, Nq, N, capacity, filter 0 none / 1 bits / 2 labels, bit offset, BF_RANGE_PATH) -> tiles?
ROUTES = [(("F32", 128, 256, 4096, 1, 0, 0, 0), 1), (("F32", 128, 255, 4096, 1, 0, 0, 0), 0),
          (("F32", 128, 256, 4095, 1, 0, 0, 0), 0), (("F32", 128, 255, 4095, 1, 0, 0, 2), 1),
          (("F32", 128, 256, 4096, 0, 0, 0, 0), 0), (("F32", 128, 1024, 65536, 0, 0, 0, 0), 1),
          (("F32", 128, 1023, 65536, 0, 0, 0, 0), 0), (("F32", 128, 1024, 65535, 0, 0, 0, 0), 0),
          (("F32", 128, 8, 64, 0, 0, 0, 2), 1), (("F32", 128, 10000, 1000000, 1, 0, 0, 1), 0),
          (("U8", 128, 10000, 100000, 1, 0, 0, 2), 0), (("I8", 128, 10000, 100000, 1, 0, 0, 2), 0),
          (("F16", 4096, 256, 4096, 1, 0, 0, 0), 1), (("BF16", 136, 256, 4096, 1, 2, 0, 0), 1),
          (("F32", 4100, 256, 4096, 1, 0, 0, 2), 0), (("F32", 130, 256, 4096, 1, 0, 0, 2), 0),
          (("F16", 132, 256, 4096, 1, 0, 0, 2), 0), (("F32", 64, 256, 4096, 1, 1, 64, 0), 1),
          (("F32", 64, 256, 4096, 1, 1, 5, 2), 0), (("F32", 64, 256, 4096, 1, 2, 5, 0), 1)]


@pytest.mark.parametrize("shape,tiles", ROUTES, ids=[str(r[0]) for r in ROUTES])
def test_routing_predicate(shape, tiles):
    from ggnn_amd import _lib
    with _lib.hooks(BF_RANGE_PATH=shape[7]):
        got = _lib.lib().ggnn_debug_bf_range_route(getattr(_lib, shape[0]), *shape[1:7], None)
    assert got == tiles


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hooks_and_c_surface():
    from ggnn_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ggnn_c.h")).read()
    for name in ("BF_RANGE_PATH", "BF_RANGE_CAND"):
        assert f" *   {name} " in header and _lib.get_hook(name) == 0
        with _lib.hooks(**{name: 2}):
            assert _lib.get_hook(name) == 2
        assert _lib.get_hook(name) == 0
    for fn in ("ggnn_op_bf_range_query_routed", "ggnn_last_bf_range_matrix_path"):
        assert f"ggnn_status {fn}(" in header and hasattr(lib, fn)
    assert "always scan kernels (hook BF_RANGE_SLICES" not in header
    out = C.c_int(7)
    assert lib.ggnn_last_bf_range_matrix_path(None, C.byref(out)) == _lib.INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib.ggnn_create(C.byref(h)) == _lib.OK
    assert lib.ggnn_last_bf_range_matrix_path(h, C.byref(out)) == _lib.OK and out.value == 0
    lib.ggnn_destroy(h)


def test_tile_kernels_hold_three_waves_per_simd_without_scratch(kernels):  # noqa: F811
    tile = {n: v for n, v in kernels.items() if n.startswith("bf_range_tile_kernel<")}
    # 3 element types x 2 measures x 3 filter modes x count / fill x (D <= 64, D <= 128, chunked)
    assert len(tile) == 3 * 2 * 3 * 2 * 3, len(tile)
    rest = {n: v for n, v in kernels.items()
            if n.startswith(("bf_range_exact_kernel<", "bf_range_compact_kernel", "bf_range_thr_kernel<",
                             "bf_range_budget_kernel", "bf_range_take_lims_kernel"))}
    assert len(rest) == 3 * 7 * 2 + 1 + 2 + 1 + 1, len(rest)
    bad = {n: v for n, v in {**tile, **rest}.items()
           if v.get("private_segment_fixed_size") != 0 or v.get("vgpr_spill_count", 0) != 0}
    assert not bad, bad
    assert max(v["vgpr_count"] for v in tile.values()) <= 168
    # LDS, 160 KB per CU: three single-chunk workgroups, two chunked ones up to D = 4096; each < 64 KB
    from ggnn_amd import _lib
    lds = C.c_uint64()
    for filt, (D, groups) in ((f, c) for f in (0, 1, 2)
                              for c in ((4, 3), (64, 3), (68, 3), (128, 3), (132, 2), (4096, 2))):
        _lib.lib().ggnn_debug_bf_range_route(_lib.F32, D, 256, 4096, 1, filt, 0, C.byref(lds))
        assert lds.value * groups <= 160 * 1024 and lds.value <= 64 * 1024, (D, lds.value)
