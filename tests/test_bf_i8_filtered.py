"""The filtered integer kernels of bf_query (bf_i8_filtered.hip) without a GPU: hook BF_I8_FILTERED, and the
register budget of every instantiation, read from the built code objects (tests/test_kernel_resources.py)."""
import os
import re

from test_kernel_resources import ROOT, kernels, pytestmark  # noqa: F401  (fixture and skip condition)

NAME = re.compile(r"bf_i8fw?_kernel<")


def test_hook_exists_defaults_to_auto_and_is_documented():
    from ggnn_amd import _lib
    assert _lib.get_hook("BF_I8_FILTERED") == 0
    with _lib.hooks(BF_I8_FILTERED=2):
        assert _lib.get_hook("BF_I8_FILTERED") == 2
    assert _lib.get_hook("BF_I8_FILTERED") == 0
    with open(os.path.join(ROOT, "include", "ggnn_c.h")) as f:
        assert re.search(r"^ \*   BF_I8_FILTERED +0 ", f.read(), re.M)


def test_every_instantiation_holds_two_waves_without_a_private_segment(kernels):
    found = {n: k for n, k in kernels.items() if NAME.match(n)}
    # two resident widths x three list lengths x three filter modes, and the streamed regime's nine
    assert len(found) == 27, sorted(found)
    for name, k in found.items():
        assert not name.startswith("bf_mfma_kernel<"), name
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] <= 256, (name, k)
