"""The integer cosine range tile path (bf_range_i8_cos.hip) without a GPU: routing, hook, C surface,
registers and LDS of its kernels, and its pre-test in numpy."""
import ctypes as C
import os

import numpy as np
import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture: the library's kernel metadata)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1024, 65536, 1)
# (dtype, measure, D, Nq, N, capacity, filter 0 none / 1 bits / 2 labels, bit offset), BF_RANGE_PATH,
# BF_RANGE_I8_COS -> integer cosine tiles?
ROUTES = [(("U8", 1, 128, *BIG, 0, 0), 0, 2, 1), (("I8", 1, 128, *BIG, 0, 0), 0, 2, 1),
          (("U8", 0, 128, *BIG, 0, 0), 0, 2, 0), (("I8", 0, 128, *BIG, 0, 0), 0, 2, 0),
          (("U8", 1, 16, *BIG, 0, 0), 0, 2, 1), (("U8", 1, 24, *BIG, 0, 0), 0, 2, 0),
          (("I8", 1, 4096, *BIG, 0, 0), 0, 2, 1), (("I8", 1, 4112, *BIG, 0, 0), 0, 2, 0),
          (("U8", 1, 64, *BIG, 1, 5), 0, 2, 0), (("U8", 1, 64, *BIG, 1, 64), 0, 2, 1),
          (("I8", 1, 64, *BIG, 2, 5), 0, 2, 1), (("U8", 1, 128, *BIG, 0, 0), 1, 2, 0),
          (("U8", 1, 128, *BIG, 0, 0), 2, 1, 0), (("F32", 1, 128, *BIG, 0, 0), 0, 2, 0),
          (("U8", 1, 16, 8, 64, 0, 0, 0), 0, 2, 1), (("U8", 1, 16, 8, 64, 0, 0, 0), 2, 0, 0),
          # auto: the shape classes of DESIGN.md 4.6, unfiltered
          (("U8", 1, 128, 1024, 65536, 1, 0, 0), 0, 0, 1), (("I8", 1, 768, 10000, 1000000, 0, 0, 0), 0, 0, 1),
          (("U8", 1, 128, 1023, 65536, 1, 0, 0), 0, 0, 0), (("U8", 1, 128, 1024, 65535, 1, 0, 0), 0, 0, 0),
          (("U8", 1, 128, 256, 4096, 1, 0, 0), 0, 0, 0), (("I8", 1, 128, 10000, 1000000, 1, 2, 0), 0, 0, 0)]


@pytest.mark.parametrize("shape,path,mode,tiles", ROUTES, ids=[f"{r[0]}-{r[1]}-{r[2]}" for r in ROUTES])
def test_routing_predicate(shape, path, mode, tiles):
    from ggnn_amd import _lib
    with _lib.hooks(BF_RANGE_PATH=path, BF_RANGE_I8_COS=mode):
        lib = _lib.lib()
        assert lib.ggnn_debug_bf_range_i8_cos_route(getattr(_lib, shape[0]), *shape[1:], None) == tiles
        # the squared-L2 predicate keeps refusing cosine
        assert shape[1] == 0 or lib.ggnn_debug_bf_range_i8_route(
            getattr(_lib, shape[0]), *shape[1:], None) == 0


def test_hook_and_c_surface():
    from ggnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "ggnn_c.h")).read()
    assert " *   BF_RANGE_I8_COS " in header and _lib.get_hook("BF_RANGE_I8_COS") == 0
    with _lib.hooks(BF_RANGE_I8_COS=2):
        assert _lib.get_hook("BF_RANGE_I8_COS") == 2
    assert _lib.get_hook("BF_RANGE_I8_COS") == 0
    assert "int ggnn_debug_bf_range_i8_cos_route(" in header


def test_kernels_hold_two_waves_per_simd_without_scratch(kernels):  # noqa: F811
    tile = {n: v for n, v in kernels.items() if n.startswith("bf_range_i8cos_kernel<")}
    # signed / unsigned x 3 filter modes x count / fill x (D <= 128, chunked)
    assert len(tile) == 2 * 3 * 2 * 2, len(tile)
    prep = {n: v for n, v in kernels.items() if n.startswith("bf_range_i8cos_prep_kernel")}
    assert len(prep) == 1
    bad = {n: v for n, v in {**tile, **prep}.items()
           if v.get("private_segment_fixed_size") != 0 or v.get("vgpr_spill_count", 0) != 0}
    assert not bad, bad
    assert max(v["vgpr_count"] for v in tile.values()) <= 256       # two waves per SIMD
    from ggnn_amd import _lib
    lds = C.c_uint64()
    for filt in (0, 1, 2):
        for D in (16, 128, 144, 4096):      # two workgroups per CU within 160 KB, each < 64 KB
            _lib.lib().ggnn_debug_bf_range_i8_cos_route(_lib.U8, 1, D, 256, 65536, 1, filt, 0, C.byref(lds))
            assert 2 * lds.value <= 160 * 1024 and 0 < lds.value <= 64 * 1024, (D, filt, lds.value)


def test_pretest_never_drops_a_hit():
    """fmaf((float)dot, rinv, -c) >= 0 for every pair with value <= r, c = ((1 - r) - 2^-20) * sqrtf(qn):
    float32 operation by operation; the fused product in float64 (three float32 operands: the real sign)"""
    f = np.float32
    rng = np.random.default_rng(24)
    n = 200000
    qn = rng.integers(1, 2 ** 24, n)
    bn = np.where(rng.random(n) < 0.3, qn, rng.integers(1, 2 ** 24, n))       # equal norms: quotients at 1
    lim = np.floor(np.sqrt(qn.astype(np.float64) * bn)).astype(np.int64)
    lim -= (lim * lim > qn * bn)                                              # |dot| <= sqrt(qn bn)
    lim = np.minimum(lim, 2 ** 24 - 1)
    dot = np.where(rng.random(n) < 0.6, lim - rng.integers(0, 4, n), rng.integers(-lim, lim + 1))
    dot = np.where(rng.random(n) < 0.15, -dot, np.maximum(dot, -lim))
    # zero rows and zero queries (dot = 0), and small norms
    qn[:500], dot[:500] = 0, 0
    bn[400:900], dot[400:900] = 0, 0
    small = slice(900, 3000)
    qn[small], bn[small] = rng.integers(1, 40, 2100), rng.integers(1, 40, 2100)
    dot[small] = np.floor(np.sqrt(qn[small] * bn[small])).astype(np.int64) * rng.choice([-1, 0, 1], 2100)
    qf, bf, df = qn.astype(f), bn.astype(f), dot.astype(f)
    ns = qf * bf
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(ns > 0, np.abs(f(1) - df / np.sqrt(ns)), f(1)).astype(f)
        rinv = np.where(bn > 0, f(1) / np.sqrt(bf), f(0)).astype(f)
    one = f(1)
    radii = [f(0), f(2.0 ** -24), np.nextafter(one, f(0)), one, np.nextafter(one, f(2)), f(2), f(2.5), v,
             np.nextafter(v, f(3)), f(0.25), f(1e-30)]
    checked = 0
    for r in radii:
        r = np.broadcast_to(f(r), v.shape)
        c = (((one - r).astype(f) - f(2.0 ** -20)).astype(f) * np.sqrt(qf)).astype(f)
        fused = df.astype(np.float64) * rinv.astype(np.float64) - c.astype(np.float64)
        hit = v <= r
        checked += int(hit.sum())
        assert (fused[hit] >= 0).all(), (r[hit][fused[hit] < 0][:3], v[hit][fused[hit] < 0][:3])
    assert checked > n
