"""The 16-bit range tile path (bf_range_f16.hip) without a GPU: routing, hook, C surface, registers and
LDS of its kernels, and its threshold restated in numpy with the model constant c_m as a parameter."""
import ctypes as C
import os

import numpy as np
import pytest

from test_bf_f16 import PAIRS, _round16
from test_kernel_resources import kernels  # noqa: F401  (fixture: the library's kernel metadata)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = ("BF16", 0, 128, 10000, 1000000, 1, 0, 0)
# (dtype, measure, D, Nq, N, capacity, filter 0 none / 1 bits / 2 labels, bit offset), BF_RANGE_PATH,
# BF_RANGE_F16 -> 16-bit tiles?
ROUTES = [(BIG, 0, 0, 1), (BIG, 0, 1, 0), (BIG, 1, 0, 0), (BIG, 1, 2, 0), (BIG, 2, 0, 1),
          (("BF16", 0, 128, 9999, 1000000, 1, 0, 0), 0, 0, 0), (("BF16", 0, 128, 10000, 999999, 1, 0, 0), 0, 0, 0),
          (("BF16", 0, 128, 10000, 1000000, 0, 2, 5), 0, 0, 1), (("F16", 0, 128, 10000, 1000000, 1, 0, 0), 0, 0, 0),
          (("F16", 0, 128, 10000, 1000000, 1, 0, 0), 0, 2, 1), (("BF16", 1, 128, 10000, 1000000, 1, 0, 0), 0, 2, 0),
          (("F16", 0, 8, 8, 64, 0, 0, 0), 0, 2, 1), (("F16", 0, 132, 150, 1061, 1, 0, 0), 0, 2, 0),
          (("F16", 0, 4096, 150, 1061, 1, 1, 64), 0, 2, 1), (("F16", 0, 4104, 150, 1061, 1, 0, 0), 0, 2, 0),
          (("BF16", 0, 64, 150, 1061, 1, 1, 5), 0, 2, 0), (("BF16", 0, 64, 150, 1061, 1, 2, 5), 0, 2, 1),
          (("F16", 0, 128, 150, 1061, 1, 0, 0), 2, 0, 0), (("BF16", 0, 128, 150, 1061, 1, 0, 0), 2, 0, 0),
          (("F32", 0, 128, 150, 1061, 1, 0, 0), 0, 2, 0), (("U8", 0, 128, 150, 1061, 1, 0, 0), 0, 2, 0)]


@pytest.mark.parametrize("shape,path,f16,tiles", ROUTES, ids=[f"{r[0]}-{r[1]}-{r[2]}" for r in ROUTES])
def test_routing_predicate(shape, path, f16, tiles):
    from ggnn_amd import _lib
    with _lib.hooks(BF_RANGE_PATH=path, BF_RANGE_F16=f16):
        assert _lib.lib().ggnn_debug_bf_range_f16_route(getattr(_lib, shape[0]), *shape[1:], None) == tiles


def test_hook_and_c_surface():
    from ggnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "ggnn_c.h")).read()
    assert " *   BF_RANGE_F16 " in header and _lib.get_hook("BF_RANGE_F16") == 0
    with _lib.hooks(BF_RANGE_F16=2):
        assert _lib.get_hook("BF_RANGE_F16") == 2
    assert _lib.get_hook("BF_RANGE_F16") == 0
    assert "int ggnn_debug_bf_range_f16_route(" in header


def test_kernels_hold_two_waves_per_simd_without_scratch(kernels):  # noqa: F811
    tile = {n: v for n, v in kernels.items() if n.startswith("bf_range_f16_kernel<")}
    # 2 types x 3 filter modes x count / fill x (NM 2 / 4 / 8, chunked)
    assert len(tile) == 2 * 3 * 2 * 4, len(tile)
    rest = {n: v for n, v in kernels.items()
            if n.startswith(("bf_range_f16_exact_kernel<", "bf_range_f16_thr_kernel",
                             "bf_range_f16_budget_kernel", "bf_range_f16_guard_kernel"))}
    assert len(rest) == 2 * 7 + 3, sorted(rest)
    bad = {n: v for n, v in {**tile, **rest}.items()
           if v.get("private_segment_fixed_size") != 0 or v.get("vgpr_spill_count", 0) != 0}
    assert not bad, bad
    # 256 threads = one wave per SIMD and workgroup; two workgroups per CU = two waves per SIMD, each
    # with at most half of the SIMD's 512 registers (three would need <= 168)
    assert max(v["vgpr_count"] for v in tile.values()) <= 256
    from ggnn_amd import _lib
    lds = C.c_uint64()
    for filt in (0, 1, 2):
        for D in (8, 32, 64, 128, 136, 4096):   # two workgroups per CU within 160 KB, each < 64 KB
            _lib.lib().ggnn_debug_bf_range_f16_route(_lib.F16, 0, D, 256, 65536, 1, filt, 0, C.byref(lds))
            assert 2 * lds.value <= 160 * 1024 and lds.value <= 64 * 1024, (D, filt, lds.value)


f32, U = np.float32, np.float32(2.0 ** -24)


def thresholds(r, qn, D, c_m):
    """bf_range_f16_thr_kernel and the host's c restated: their constants, change together"""
    Df = f32(D)
    c = f32(1.03) * f32(c_m) * (f32(2.0625) * Df + f32(24)) * U
    t = r / (f32(1) - f32(1.02) * (Df + f32(3)) * U)
    t = (c.astype(np.float64) * qn + t).astype(f32)          # fmaf
    t = t + (f32(2) * Df + f32(8)) * f32(2.3509887e-38)
    return (t + f32(16) * U * t).astype(f32), c


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(PAIRS))
@pytest.mark.parametrize("D", [8, 136, 960])
@pytest.mark.parametrize("c_m", [1.0, 8.0])
def test_threshold_keeps_every_hit_under_the_instruction_model(kind, name, D, c_m):
    """r = d_dir, the smallest radius that admits the pair; d_e at the far end of the model's bound
    B(q, x) (test_bf_f16.py shows B holds under the model), rounded upward: still a candidate"""
    rng = np.random.default_rng(D + int(c_m))
    q, x = (_round16(v, kind) for v in PAIRS[name](rng, 64, D))
    true = ((q - x) ** 2).sum(1)
    qn = np.add.accumulate((q * q).astype(f32), axis=1, dtype=f32)[:, -1]
    bn = (x * x).astype(f32).sum(1, dtype=f32)
    d_dir = np.add.accumulate((x - q).astype(f32) ** 2, axis=1, dtype=f32)[:, -1]
    B = 1.02 * c_m * (2.0625 * D + 24) * 2.0 ** -24 * (qn.astype(np.float64) + bn) + (2 * D + 8) * 2.0 ** -125
    d_e = np.nextafter((true + B).astype(f32), f32(np.inf))
    t, c = thresholds(d_dir, qn, D, c_m)
    lhs = (d_e.astype(np.float64) - c.astype(np.float64) * bn).astype(f32)   # fmaf(-c, bn, d_e)
    assert not (lhs > t).any(), np.nonzero(lhs > t)[0][:5]
