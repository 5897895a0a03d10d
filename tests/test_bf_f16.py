"""The 16-bit tile path of bf_query (bf_f16.hip) without a GPU: routing, hook, C surface, the private
segment of its kernels, and its certificate bound re-derived in float64 under the stated model of one
matrix instruction, with the model constant c_m as a parameter."""
import numpy as np
import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture: the library's kernel metadata)

U = 2.0 ** -24
# (dtype, measure, D, Nq, N, k, filtered), BF_F16, BF_SCAN -> 16-bit tiles?
# (auto routes the measured wins only: bfloat16 from 10k x 1M on, on the two-set kernels of D > 64, which
# hold k <= 13; float16 is hook only -- DESIGN.md 4.6.  At D <= 32 the lists of k = 111 / 112 do not fit
# the LDS beside the stages: the float32-staged tiles keep those calls under every hook value)
ROUTES = [(("BF16", 0, 128, 10000, 1000000, 10, 0), 0, 0, 1), (("BF16", 0, 960, 10000, 1000000, 13, 0), 0, 0, 1),
          (("BF16", 0, 960, 10000, 1000000, 14, 0), 0, 0, 0), (("BF16", 0, 960, 10000, 1000000, 112, 0), 2, 0, 1),
          (("BF16", 0, 64, 10000, 1000000, 10, 0), 0, 0, 0), (("BF16", 0, 72, 10000, 1000000, 10, 0), 0, 0, 1),
          (("BF16", 0, 32, 10000, 1000000, 112, 0), 0, 0, 0), (("BF16", 0, 32, 10000, 1000000, 112, 0), 2, 0, 0),
          (("F16", 0, 32, 256, 4096, 111, 0), 2, 0, 0), (("F16", 0, 32, 256, 4096, 110, 0), 2, 0, 1),
          (("F16", 0, 40, 256, 4096, 112, 0), 2, 0, 1),
          (("BF16", 0, 128, 9999, 1000000, 10, 0), 0, 0, 0), (("BF16", 0, 128, 10000, 999999, 10, 0), 0, 0, 0),
          (("F16", 0, 128, 10000, 1000000, 10, 0), 0, 0, 0), (("F16", 0, 128, 10000, 1000000, 10, 0), 2, 0, 1),
          (("BF16", 0, 128, 10000, 1000000, 10, 0), 1, 0, 0), (("BF16", 0, 128, 10000, 1000000, 10, 0), 0, 1, 0),
          (("BF16", 0, 128, 10000, 1000000, 10, 1), 0, 0, 0), (("BF16", 1, 128, 10000, 1000000, 10, 0), 0, 0, 0),
          (("F16", 0, 128, 255, 4095, 10, 0), 2, 0, 1), (("F16", 0, 8, 1, 1, 1, 0), 2, 0, 1),
          (("F16", 0, 128, 256, 4096, 10, 0), 1, 0, 0), (("F16", 0, 128, 256, 4096, 10, 0), 2, 1, 0),
          (("F16", 1, 128, 256, 4096, 10, 0), 2, 0, 0), (("BF16", 0, 128, 256, 4096, 10, 1), 2, 0, 0),
          (("F16", 0, 4096, 256, 4096, 10, 0), 2, 0, 1), (("F16", 0, 4104, 256, 4096, 10, 0), 2, 0, 0),
          (("F16", 0, 132, 256, 4096, 10, 0), 2, 0, 0), (("F16", 0, 128, 256, 4096, 113, 0), 2, 0, 0),
          (("F32", 0, 128, 256, 4096, 10, 0), 2, 0, 0), (("U8", 0, 128, 256, 4096, 10, 0), 2, 0, 0)]


@pytest.mark.parametrize("shape,f16,scan,tiles", ROUTES, ids=[f"{r[0]}-{r[1]}-{r[2]}" for r in ROUTES])
def test_routing_predicate(shape, f16, scan, tiles):
    from ggnn_amd import _lib
    with _lib.hooks(BF_F16=f16, BF_SCAN=scan):
        assert _lib.lib().ggnn_debug_bf_f16_route(getattr(_lib, shape[0]), *shape[1:]) == tiles


def test_hook_and_c_surface():
    from ggnn_amd import _lib
    assert _lib.get_hook("BF_F16") == 0
    with _lib.hooks(BF_F16=2):
        assert _lib.get_hook("BF_F16") == 2
    assert _lib.get_hook("BF_F16") == 0
    assert hasattr(_lib.lib(), "ggnn_debug_bf_f16_route")


def test_kernels_hold_two_waves_per_simd_without_scratch(kernels):  # noqa: F811
    tile = {n: v for n, v in kernels.items() if n.startswith("bf_f16_kernel<")}
    assert len(tile) == 2 * 4 * 2, sorted(tile)   # types x (NM 2 / 4 / 8, chunked) x sets per wave
    rest = {n: v for n, v in kernels.items()
            if n.startswith(("bf_f16_rerank_kernel<", "bf_f16_flag_kernel<", "bf_f16_pack_kernel<"))}
    assert len(rest) == 2 * 7 + 2 + 2, sorted(rest)
    bad = {n: v for n, v in {**tile, **rest}.items()
           if v.get("private_segment_fixed_size") != 0 or v.get("vgpr_spill_count", 0) != 0}
    assert not bad, bad
    assert max(v["vgpr_count"] for v in tile.values()) <= 256   # two waves per SIMD


def _round16(x, kind):
    if kind == "f16":
        return x.astype(np.float16).astype(np.float64)
    b = x.astype(np.float32).view(np.uint32)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000        # round to nearest even, 8 significant bits
    return b.view(np.float32).astype(np.float64)


PAIRS = {
    "normal": lambda r, n, D: (r.normal(size=(n, D)), r.normal(size=(n, D))),
    "offset": lambda r, n, D: (r.normal(size=(n, D)) + 1000, r.normal(size=(n, D)) + 1000),
    "near": lambda r, n, D: (lambda x: (x, x * (1 + 2.0 ** -9 * r.integers(-1, 2, (n, D)))))(r.normal(size=(n, D)) * 40),
    "decades": lambda r, n, D: (r.normal(size=(n, D)) * 10.0 ** r.uniform(-2, 2, (n, 1)),
                                r.normal(size=(n, D)) * 10.0 ** r.uniform(-2, 2, (n, 1))),
    "alternating": lambda r, n, D: (np.tile([300.0, -300.0], (n, D // 2)) + r.normal(size=(n, D)),
                                    np.tile([300.0, 300.0], (n, D // 2)) + r.normal(size=(n, D))),
}


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(PAIRS))
@pytest.mark.parametrize("D", [8, 136, 960])
@pytest.mark.parametrize("c_m", [1.0, 8.0])
def test_certificate_bound_under_the_instruction_model(kind, name, D, c_m):
    """bf_f16.hip: one instruction returns C + sum_k a_k b_k with error at most c_m 17 u (|C| + sum |a_k b_k|).
    The chain is driven to the model's extremes (every instruction off by the full amount, upward, downward
    and with random signs); float32 norm chains in three orders; d_e must stay within
    B = 1.02 c_m (2.0625 D + 24) u (|q|^2 + |x|^2) of the true squared distance, the bound the re-rank uses."""
    rng = np.random.default_rng(D + int(c_m))
    q, x = (_round16(v, kind) for v in PAIRS[name](rng, 64, D))
    true = ((q - x) ** 2).sum(1)
    pad = (-D) % 16
    prod = np.pad(q * x, ((0, 0), (0, pad))).reshape(64, -1, 16)      # exact in float64 (and in float32)
    f32 = lambda v: v.astype(np.float32)  # noqa: E731
    for sign in (1.0, -1.0, None):
        C = np.zeros(64)
        for i in range(prod.shape[1]):
            s = rng.choice([-1.0, 1.0], 64) if sign is None else sign
            C = C + prod[:, i].sum(1) + s * c_m * 17 * U * (np.abs(C) + np.abs(prod[:, i]).sum(1))
        for order in (slice(None), slice(None, None, -1)):
            qn = np.add.accumulate(f32(q * q)[:, order], axis=1, dtype=np.float32)[:, -1]
            bn = f32((x * x)[:, order]).sum(1, dtype=np.float32)                    # pairwise
            d_e = f32(f32(qn + bn).astype(np.float64) - 2.0 * f32(C).astype(np.float64))
            B = 1.02 * c_m * (2.0625 * D + 24) * U * (qn.astype(np.float64) + bn) + (2 * D + 8) * 2.0 ** -125
            assert (np.abs(d_e.astype(np.float64) - true) <= B).all(), (sign, np.abs(d_e - true).max() / B.min())
            # the guard's two-sided form against the direct form (sequential float32 chain)
            d_dir = np.add.accumulate(f32(f32(x - q) ** 2), axis=1, dtype=np.float32)[:, -1].astype(np.float64)
            assert (d_dir >= true * (1 - 1.01 * (D + 3) * U)).all()
            assert (np.abs(d_e - d_dir) <= B + 1.01 * (D + 3) * U * d_dir).all()
