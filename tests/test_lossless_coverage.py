"""CPU: tests/test_gpu_lossless_matrix.py launches every kernel of PrescreenExact in the library.

The query kernels that take exact distances from lossless pre-screen codes are instantiated per
float layout <LPR, NCH>, filter class and visited set, and only the engine handle reaches them.
The kernels are listed from the built library's code objects (the fixture of
tests/test_kernel_resources.py); each must be the `exact_variant` of at least one cell of
test_gpu_lossless_matrix.CASES on a D of its layout, or stand in UNREACHABLE with the reason why no
engine launches it.  A new variant, or a D moved to another layout, fails here until the GPU matrix
follows."""
import re

import pytest

from test_kernel_resources import kernels, pytestmark  # noqa: F401  (the same skip condition)

torch = pytest.importorskip("torch")

EXACT_NAME = re.compile(r"(query_kernel|query_filtered_kernel|query_labeled_kernel)<float, (\d+), "
                        r"(\d+), 1, 0, PrescreenExact<8, 1, 0>, (-?\d+), true(, true)?>$")

# rows of at most 8 chunks are at most 32 float32 dimensions, and the engine makes no pre-screen copy
# of rows of fewer than 64 padded dimensions (ensure_prescreen, engine_residency.cpp): launch_query_cfg
# instantiates the variants for the layout all the same
SHORT_ROWS = "layout {8,1} is D <= 32; no pre-screen copy below 64 padded dimensions"
UNREACHABLE = [((family, 8, 1, hb), SHORT_ROWS)
               for family, hbs in (("query_kernel", (1, 2, -8, -9)),
                                   ("query_filtered_kernel", (1, 2)),
                                   ("query_labeled_kernel", (1, 2)))
               for hb in hbs]


def exact_kernels(kernels):
    """{(family, LPR, NCH, HB): name} of the PrescreenExact kernels in the library"""
    out = {}
    for name in kernels:
        if "PrescreenExact" not in name:
            continue
        m = EXACT_NAME.match(name)
        assert m, f"{name}: a PrescreenExact kernel of a form this test does not know"
        family, lpr, nch, hb, gr = m.groups()
        assert (gr is not None) == (family == "query_kernel"), name
        out[(family, int(lpr), int(nch), int(hb))] = name
    return out


def cells_by_variant():
    """{(family, LPR, NCH, HB): [cell, ...]} over CASES"""
    from ggnn_amd import ops
    from test_gpu_lossless_matrix import CASES, exact_variant
    out = {}
    for cell in CASES:
        how, D, kb, K, tau, iters, hooks = cell
        v = exact_variant(how, D, kb, K, iters, dict(hooks))
        if v:
            layout = ops.dist_layout((D + 3) // 4 * 4, torch.float32)
            out.setdefault((v[0], *layout, v[1]), []).append(cell)
    return out


def test_every_exact_kernel_has_a_cell_in_the_gpu_matrix(kernels):
    lib = exact_kernels(kernels)
    covered = cells_by_variant()
    listed = dict(UNREACHABLE)
    missing = sorted(name for key, name in lib.items() if key not in covered and key not in listed)
    assert not missing, \
        f"PrescreenExact kernels without a cell in test_gpu_lossless_matrix.CASES: {missing}"
    gone = sorted(key for key in listed if key not in lib)
    assert not gone, f"UNREACHABLE lists variants that are not in the library: {gone}"
    both = sorted(key for key in listed if key in covered)
    assert not both, f"UNREACHABLE variants that a cell of CASES launches: {both}"
    unknown = sorted(key for key in covered if key not in lib)
    assert not unknown, f"cells of CASES whose exact variant is not in the library: {unknown}"
    reachable = [key for key in lib if key not in listed]
    print(f"{len(reachable)} PrescreenExact kernels reachable through the engine, "
          f"{len(listed)} unreachable")
    # unfiltered 4 sets x 3 layouts, filtered 2 x 3, labelled 2 x 3
    assert len(reachable) >= 24


def test_the_unreachable_layouts_have_no_exact_variant():
    """the reason in UNREACHABLE, checked against the layout table and the restated launchers"""
    from ggnn_amd import ops
    from test_gpu_lossless_matrix import exact_variant
    layouts = {key[1:3] for key, _ in UNREACHABLE}
    dims = [D for D in range(1, 4097) if ops.dist_layout(D, torch.float32) in layouts]
    assert dims and max(dims) < 61          # 61..64 are padded to 64
    for D in dims:
        for how, iters in (("plain", 175), ("plain", 600), ("bitset", 175), ("labels", 400)):
            assert exact_variant(how, D, 24, 10, iters) is None, (how, D, iters)


def test_the_oracle_cells_are_exact_cells_of_the_matrix():
    """one cell of every family at D = 128, the tag set on the other layouts"""
    from test_gpu_lossless_matrix import CASES, ORACLE_CELLS, exact_variant
    seen = set()
    for cell in ORACLE_CELLS:
        assert cell in CASES
        how, D, kb, K, tau, iters, hooks = cell
        seen.add((D, exact_variant(how, D, kb, K, iters, dict(hooks))))
    assert {v for d, v in seen if d == 128} == \
        {("query_kernel", hb) for hb in (1, 2, -8, -9)} | \
        {(f, hb) for f in ("query_filtered_kernel", "query_labeled_kernel") for hb in (1, 2)}
    assert {(96, ("query_kernel", -8)), (100, ("query_kernel", -8)),
            (64, ("query_kernel", -8))} <= seen


def test_the_boundary_cells_lie_on_both_sides():
    """the restated launchers at the cells meant as boundaries: what the GPU matrix then asserts of
    the rows read is the intended side"""
    from test_gpu_lossless_matrix import exact_variant as ev
    assert ev("plain", 128, 24, 10, 992) == ("query_kernel", -8)
    assert ev("plain", 128, 24, 10, 993) is None and ev("plain", 128, 24, 10, 1000) is None
    assert ev("plain", 128, 24, 47, 700) == ("query_kernel", -8)
    assert ev("plain", 128, 24, 48, 700) is None and ev("bitset", 128, 24, 48, 256) is None
    assert ev("plain", 128, 24, 1, 600) == ("query_kernel", -8)
    assert ev("plain", 128, 24, 10, 1500) == ("query_kernel", -9)
    assert ev("plain", 128, 20, 10, 175) == ("query_kernel", 1)
    assert ev("plain", 128, 40, 10, 175) is None and ev("labels", 128, 40, 10, 400) is None
    assert ev("plain", 132, 24, 10, 175) is None and ev("labels", 132, 24, 10, 400) is None
    assert ev("plain", 128, 24, 10, 175, {"QUERY_GLOBAL_RING": 0}) is None
    assert ev("bitset", 128, 24, 10, 400, {"QUERY_GLOBAL_RING": 0}) == ("query_filtered_kernel", 2)
    assert ev("bitset", 128, 24, 10, 400, {"QUERY_EARLY": 0}) is None
    assert ev("bitset", 128, 24, 10, 256) == ("query_filtered_kernel", 1)      # 192-key ring wraps
    assert ev("labels", 96, 24, 10, 512) == ("query_labeled_kernel", 2)        # 480-key ring wraps
    assert ev("table", 128, 24, 10, 600) is None
    assert ev("labels", 70, 24, 10, 175) == ("query_labeled_kernel", 1)
