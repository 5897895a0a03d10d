"""Register budget of the filtered tile kernels of bf_query (bf_mfma_bits.hip, bf_mfma_labels.hip),
read from the built code objects the way tests/test_kernel_resources.py reads them (no GPU needed).

A filtered `bf_mfma_kernel<..., FM>` keeps the budget of its unfiltered sibling: private segment 0
and no fewer waves per SIMD -- 3 for the single-chunk kernels (T == 1), 2 for T <= 3, 1 for T == 4
(512 registers per SIMD lane, allocated in blocks of 8).  The single-chunk kernels hold it with the
list length as the constant 18 only (bf_common.hpp: longer lists run the chunked kernels): the list
below is what the launcher can select, and the test also checks that no other filtered variant --
none with a run-time list length at T == 1 -- is in the library."""
import re

import pytest

from test_kernel_resources import kernels, pytestmark  # noqa: F401  (fixture and skip condition)

TYPES = ["float", "f16_t", "bf16_t", "unsigned char"]
NAME = re.compile(r"bf_mfma_kernel<(.+), (\d), (\d), (\d+), (\d+), ([12])>$")


def _expected():
    out = []
    for fm in (1, 2):
        for t in TYPES:
            for mode in (0, 1):
                for T in (2, 3, 4):
                    out.append((t, mode, T, 16, 0, fm))
                for NU in (8, 12, 16):
                    out.append((t, mode, 1, NU, 18, fm))   # kBfFilteredSingleChunkKP
    return out


def _filtered(kernels):
    found = {}
    for name, k in kernels.items():
        m = NAME.match(name)
        if m:
            t = {"_Float16": "f16_t", "__hip_bfloat16": "bf16_t"}.get(m.group(1), m.group(1))
            found[(t,) + tuple(int(x) for x in m.groups()[1:])] = k
    return found


def test_the_filtered_variants_are_the_budgeted_ones(kernels):
    found = _filtered(kernels)
    types = {k[0] for k in found}
    assert len(types) == 4, types   # four element types, whatever their spelling in the symbol
    want = _expected()
    assert len(found) == len(want), (len(found), len(want))
    by_rest = {}
    for k in found:
        by_rest.setdefault(k[1:], set()).add(k[0])
    for t, *rest in want:
        assert tuple(rest) in by_rest, rest


def test_filtered_kernels_keep_their_siblings_budget(kernels):
    found = _filtered(kernels)
    assert found, "no filtered bf_mfma_kernel in the library"
    for key, k in found.items():
        T = key[2]
        assert k["private_segment_fixed_size"] == 0, (key, k)
        assert k["vgpr_spill_count"] == 0, (key, k)
        waves = min(8, 512 // ((k["vgpr_count"] + 7) // 8 * 8))
        assert waves >= (3 if T == 1 else 2 if T <= 3 else 1), (key, k, waves)
