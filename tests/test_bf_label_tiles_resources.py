"""The predicate tile kernels of bf_query (bf_mfma_pred.hip, FM = kBfPredicate = 3) without a GPU: hook
BF_LABEL_TILES, and the register budget of every instantiation, read from the built code objects
(tests/test_kernel_resources.py).  The variants in the library are exactly the launcher's set, and each
keeps the budget of tests/test_bf_filtered_resources.py: private segment 0, no spilled register, and 3 /
2 / 1 waves per SIMD for T = 1 / T <= 3 / T = 4."""
import os
import re

from test_kernel_resources import ROOT, kernels, pytestmark  # noqa: F401  (fixture and skip condition)

NAME = re.compile(r"bf_mfma_kernel<(.+), (\d), (\d), (\d+), (\d+), 3>")


def test_hook_exists_defaults_to_auto_and_is_documented():
    from ggnn_amd import _lib
    assert _lib.get_hook("BF_LABEL_TILES") == 0
    with _lib.hooks(BF_LABEL_TILES=2):
        assert _lib.get_hook("BF_LABEL_TILES") == 2
    assert _lib.get_hook("BF_LABEL_TILES") == 0
    with open(os.path.join(ROOT, "include", "ggnn_c.h")) as f:
        assert re.search(r"^ \*   BF_LABEL_TILES +0 ", f.read(), re.M)


def test_the_predicate_variants_are_the_launchers_and_keep_the_budget(kernels):
    found = {}
    for name, k in kernels.items():
        m = NAME.match(name)
        if m:
            found[(m.group(1),) + tuple(int(x) for x in m.groups()[1:])] = k
    assert len({key[0] for key in found}) == 4, sorted(found)   # four element types
    shapes = {(T, 16, 0) for T in (2, 3, 4)} | {(1, NU, 18) for NU in (8, 12, 16)}
    assert {key[2:] for key in found} == shapes
    assert len(found) == 4 * 2 * len(shapes), len(found)        # x two measures
    for key, k in found.items():
        T = key[2]
        assert k["private_segment_fixed_size"] == 0, (key, k)
        assert k["vgpr_spill_count"] == 0, (key, k)
        waves = min(8, 512 // ((k["vgpr_count"] + 7) // 8 * 8))
        assert waves >= (3 if T == 1 else 2 if T <= 3 else 1), (key, k, waves)
