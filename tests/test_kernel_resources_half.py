"""Guard on the built code objects of the float16 / bfloat16 query kernels (CPU; see
tests/test_kernel_resources.py for why scratch in the traversal kernels is a regression).

The default 16-bit query kernels -- D = 64 (layout {8, 1}: early rows and the hashed visited set)
and D = 96 / 128 (layout {8, 2}) -- for both measures keep a private segment of zero bytes, no
spills, and at most 72 VGPRs (7 waves per SIMD, the float kernels' budget)."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (module fixture)
from test_kernel_resources import pytestmark  # noqa: F401  (needs the library and llvm tools)

HALF_KERNELS = [
    f"query_kernel<{t}, {layout}, 1, {mode}, NoPrescreen, {variant}>"
    for t in ("f16_t", "bf16_t")
    for mode in (0, 1)
    for layout, variant in (("8, 1", "1, true, true"), ("8, 1", "2, true, true"),
                            ("8, 1", "1, true, false"), ("8, 1", "2, true, false"),
                            ("8, 2", "0, false, false"))
]


@pytest.mark.parametrize("name", HALF_KERNELS)
def test_default_16bit_query_kernels_have_no_scratch(kernels, name):  # noqa: F811
    assert name in kernels, f"{name} is not in the library (renamed template parameters?)"
    k = kernels[name]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= 72, k
