"""The integer range tile path (bf_range_i8.hip) without a GPU: routing, hook, C surface, registers and
LDS of its kernels, and its arithmetic contract in numpy."""
import ctypes as C
import os

import numpy as np
import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture: the library's kernel metadata)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (dtype, measure, D, Nq, N, capacity, filter 0 none / 1 bits / 2 labels, bit offset), BF_RANGE_PATH,
# BF_RANGE_I8 -> integer tiles?
ROUTES = [(("U8", 0, 128, 256, 65536, 1, 0, 0), 0, 0, 1), (("I8", 0, 128, 256, 65536, 0, 0, 0), 0, 0, 1),
          (("U8", 0, 128, 255, 65536, 1, 0, 0), 0, 0, 0), (("I8", 0, 128, 256, 65535, 1, 0, 0), 0, 0, 0),
          (("U8", 1, 128, 256, 65536, 1, 0, 0), 0, 2, 0), (("U8", 0, 24, 256, 65536, 1, 0, 0), 0, 2, 0),
          (("U8", 0, 4112, 256, 65536, 1, 0, 0), 0, 2, 0), (("U8", 0, 4096, 256, 65536, 1, 0, 0), 0, 0, 1),
          (("U8", 0, 64, 256, 65536, 1, 1, 5), 0, 2, 0), (("U8", 0, 64, 256, 65536, 1, 1, 64), 0, 0, 1),
          (("I8", 0, 64, 256, 65536, 1, 2, 5), 0, 0, 1), (("U8", 0, 128, 256, 65536, 1, 0, 0), 1, 2, 0),
          (("U8", 0, 128, 256, 65536, 1, 0, 0), 2, 1, 0), (("F32", 0, 128, 256, 65536, 1, 0, 0), 0, 2, 0),
          (("U8", 0, 16, 8, 64, 0, 0, 0), 0, 2, 1), (("U8", 0, 16, 8, 64, 0, 0, 0), 2, 0, 0)]


@pytest.mark.parametrize("shape,path,i8,tiles", ROUTES, ids=[f"{r[0]}-{r[1]}-{r[2]}" for r in ROUTES])
def test_routing_predicate(shape, path, i8, tiles):
    from ggnn_amd import _lib
    with _lib.hooks(BF_RANGE_PATH=path, BF_RANGE_I8=i8):
        lib = _lib.lib()
        assert lib.ggnn_debug_bf_range_i8_route(getattr(_lib, shape[0]), *shape[1:], None) == tiles
        # the float predicate keeps saying no to byte rows
        assert shape[0] == "F32" or lib.ggnn_debug_bf_range_route(
            getattr(_lib, shape[0]), *shape[2:], None) == 0


def test_hook_and_c_surface():
    from ggnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "ggnn_c.h")).read()
    assert " *   BF_RANGE_I8 " in header and _lib.get_hook("BF_RANGE_I8") == 0
    with _lib.hooks(BF_RANGE_I8=2):
        assert _lib.get_hook("BF_RANGE_I8") == 2
    assert _lib.get_hook("BF_RANGE_I8") == 0
    assert "int ggnn_debug_bf_range_i8_route(" in header
    assert hasattr(_lib.lib(), "ggnn_debug_bf_range_i8_route")


def test_kernels_hold_two_waves_per_simd_without_scratch(kernels):  # noqa: F811
    tile = {n: v for n, v in kernels.items() if n.startswith("bf_range_i8_kernel<")}
    # signed / unsigned x 3 filter modes x count / fill x (D <= 128, chunked)
    assert len(tile) == 2 * 3 * 2 * 2, len(tile)
    rest = {n: v for n, v in kernels.items()
            if n.startswith(("bf_range_i8_norms_kernel<", "bf_range_i8_prep_kernel<",
                             "bf_range_i8_take_lims_kernel"))}
    assert len(rest) == 2 + 2 + 1, len(rest)
    bad = {n: v for n, v in {**tile, **rest}.items()
           if v.get("private_segment_fixed_size") != 0 or v.get("vgpr_spill_count", 0) != 0}
    assert not bad, bad
    assert max(v["vgpr_count"] for v in tile.values()) <= 256       # two waves per SIMD
    assert max(v["vgpr_count"] for n, v in tile.items() if ", false, " in n) <= 192   # count passes
    from ggnn_amd import _lib
    lds = C.c_uint64()
    for filt in (0, 1, 2):
        for D in (16, 128, 144, 4096):      # two workgroups per CU within 160 KB, each < 64 KB
            _lib.lib().ggnn_debug_bf_range_i8_route(_lib.U8, 0, D, 256, 65536, 1, filt, 0, C.byref(lds))
            assert 2 * lds.value <= 160 * 1024 and lds.value <= 64 * 1024, (D, filt, lds.value)


@pytest.mark.parametrize("D,lanes", [(256, 8), (272, 16), (1024, 8), (4096, 16), (4096, 64)])
def test_contract_float_tree_of_integer_partials(D, lanes):
    """The scan's value: exact integer partials per lane (<= 256 elements), a float32 tree over the
    lanes.  (float)d below 2^24, at least 2^24 otherwise -- what the integer path relies on."""
    rng = np.random.default_rng(D + lanes)
    for hi in (256, 40, 255):
        b = rng.integers(hi - 1 if hi == 255 else 0, hi + 1 if hi == 255 else hi, (64, D))
        q = rng.integers(0, 2 if hi == 255 else hi, (64, D))
        part = ((b - q) ** 2).reshape(64, lanes, -1).sum(-1)
        assert part.max() < 2 ** 24
        d, s = part.sum(1), part.astype(np.float32)
        while s.shape[1] > 1:                  # xor-butterfly order: s[i] + s[i ^ half]
            half = s.shape[1] // 2
            s = s[:, :half] + s[:, half:]
        s = s[:, 0]
        small = d < 2 ** 24
        assert s.dtype == np.float32 and (s[small] == d[small]).all() and (s[~small] >= 2 ** 24).all()
        assert D <= 258 or hi != 255 or (~small).any()
