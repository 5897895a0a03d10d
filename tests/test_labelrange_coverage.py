"""CPU: tests/test_gpu_labelrange_layout_matrix.py launches every label-range kernel in the library.

query_labelrange_kernel* are instantiated per row layout <LPR, NCH>, element type, measure, list
size, pre-screen and visited set, bf_query_labelrange_kernel* per layout, element type, measure and
list size: the instantiations of the label-set kernels (tests/test_labelset_coverage.py), name for
name.  The kernels are listed from the built library's code objects (the fixture of
tests/test_kernel_resources.py); each traversal kernel must be the `labelrange_kernel` of at least
one case of LADDER_CASES, or stand in UNREACHABLE with the reason why no launch reaches it, and each
scan kernel the `bf_labelrange_kernel` of a cell of SCAN_MATRIX at one of the test's K.  A new
variant, or a D moved to another layout, fails here until the GPU matrix follows.

The masks of the GPU matrix are checked here as well, without a GPU: its interval lists, on the plain
column and on the edge column, select what the label sets of tests/test_gpu_labelset_layout_matrix.py
select, which is what lets the two modules share their references."""
import re

import pytest

from test_kernel_resources import kernels, pytestmark  # noqa: F401  (the same skip condition)

torch = pytest.importorskip("torch")

from test_gpu_labelset_layout_matrix import prescreen_layout  # noqa: E402

LDS_NAME = re.compile(r"query_labelrange_kernel_lds<float, (\d+), (\d+), ([01]), "
                      r"Prescreen<(\d+), (\d+), ([01])> >$")
FLOAT_LAYOUTS = ((8, 1), (8, 2), (8, 3), (16, 2), (16, 4), (64, 4), (64, 16))
# launch_query_cfg (query_wave.hpp) takes the pre-screened kernels for a sorted part of at most 512,
# and launch_query_ladder gives such a part a register list: FilteredLadder instantiates the LDS list
# under the pre-screen all the same
NO_LDS_LIST = "the pre-screen is taken for a sorted part of at most 512: a register list"
# GGNN_DISPATCH_DIST_32_8 (traversal.hpp) instantiates every layout for both element types, and rows
# of 16 elements per chunk reach {64, 16} above 4096 elements only, which the entry points refuse
# (the layout table: here; the refusal: test_labelrange_refuses_byte_rows_above_4096 of the GPU
# matrix)
WIDE_BYTE_ROWS = "uint8 rows of at most 4096 elements stop at layout {64,4}"
LISTS = (1, 2, 4, 8, 16, 32)


# [(kernel, reason)] of the traversal kernels and of the scan kernels
UNREACHABLE = [("query_labelrange_kernel_lds<float, %d, %d, %d, Prescreen<%d, %d, %d> >"
                % (lpr, nch, m, *prescreen_layout(lpr, nch), m), NO_LDS_LIST)
               for lpr, nch in FLOAT_LAYOUTS for m in (0, 1)] + \
    [(f"query_labelrange_kernel<unsigned char, 64, 16, {R}, {m}, NoPrescreen, 0, false>", WIDE_BYTE_ROWS)
     for R in LISTS for m in (0, 1)] + \
    [(f"query_labelrange_kernel_lds<unsigned char, 64, 16, {m}, NoPrescreen>", WIDE_BYTE_ROWS)
     for m in (0, 1)]
UNREACHABLE_SCAN = [(f"bf_query_labelrange_kernel<unsigned char, 64, 16, {R}, {m}>", WIDE_BYTE_ROWS)
                    for R in (1, 2, 4) for m in (0, 1)] + \
    [(f"bf_query_labelrange_lds_kernel<unsigned char, 64, 16, {m}>", WIDE_BYTE_ROWS) for m in (0, 1)]


def labelrange_kernels(kernels):
    out = [n for n in kernels if n.startswith("query_labelrange_kernel")]
    assert out, "the library holds no query_labelrange_kernel*"
    return out


def scan_kernels(kernels):
    out = [n for n in kernels if n.startswith("bf_query_labelrange_")]
    assert out, "the library holds no bf_query_labelrange_* kernels"
    return out


def cases_by_kernel():
    from test_gpu_labelrange_layout_matrix import LADDER_CASES, labelrange_kernel
    out = {}
    for case in LADDER_CASES:
        kind, D, m, K, tau, iters, hooks = case
        out.setdefault(labelrange_kernel(kind, D, m, K, iters, hooks), []).append(case)
    return out


def test_every_labelrange_traversal_kernel_has_a_case(kernels):
    lib = labelrange_kernels(kernels)
    covered = cases_by_kernel()
    listed = dict(UNREACHABLE)
    missing = sorted(n for n in lib if n not in covered and n not in listed)
    assert not missing, \
        f"label-range kernels without a case in test_gpu_labelrange_layout_matrix.LADDER_CASES: {missing}"
    gone = sorted(n for n in listed if n not in lib)
    assert not gone, f"UNREACHABLE lists kernels that are not in the library: {gone}"
    both = sorted(n for n in listed if n in covered)
    assert not both, f"UNREACHABLE kernels that a case of LADDER_CASES launches: {both}"
    unknown = sorted(n for n in covered if n not in lib)
    assert not unknown, f"cases of LADDER_CASES whose kernel is not in the library: {unknown}"
    reachable = [n for n in lib if n not in listed]
    print(f"{len(reachable)} label-range traversal kernels reachable, {len(listed)} unreachable")
    assert len(reachable) >= REACHABLE and len(lib) >= REACHABLE + len(listed)


# read from the library that introduced this test: 494 kernels (290 of float32 / uint8 rows, 204 of
# 16-bit rows), the instantiations of the label-set kernels.  Rows read directly: 7 lists (R = 1 ..
# 32, LDS) x 2 measures on 7 float32 + 6 uint8 + 7 + 7 16-bit layouts = 378, and HB 1 / 2 with early
# rows on the four {8,1} layouts = 16; pre-screened float32: 4 lists x 2 x 7 layouts = 56, and HB 1 /
# 2 on the four layouts behind Prescreen<8, 1> = 16.  Unreachable: 14 pre-screened LDS lists and the
# 14 kernels of uint8 {64,16}
REACHABLE = 466


def test_the_unreachable_kernels_are_never_chosen(kernels):
    """the reasons in UNREACHABLE, checked against the layout table and the restated launcher"""
    from ggnn_amd import ops
    from test_gpu_labelrange_layout_matrix import labelrange_kernel
    listed = dict(UNREACHABLE)
    lib = labelrange_kernels(kernels)
    # 1. a pre-screened launch never takes the LDS list: every float32 layout at its ends, every
    # list size; and the names are all the pre-screened LDS kernels the library holds
    no_lds = {n for n, reason in listed.items() if reason == NO_LDS_LIST}
    assert no_lds == {n for n in lib if "_lds<" in n and "Prescreen<" in n}
    for n in no_lds:
        lpr, nch, m, plpr, pnch, pm = map(int, LDS_NAME.match(n).groups())
        assert (plpr, pnch) == prescreen_layout(lpr, nch) and pm == m
    layouts = {}
    for D in range(4, 4097, 4):
        layouts.setdefault(ops.dist_layout(D, torch.float32), []).append(D)
    assert set(layouts) == set(FLOAT_LAYOUTS)
    for dims in layouts.values():
        for D in (dims[0], dims[-1]):
            for K in (1, 10, 47, 48, 100, 200, 400, 495, 496, 900, 2000, 2100, 6000):
                for iters in (64, 600):
                    for m in (0, 1):
                        name = labelrange_kernel("f32_ps", D, m, K, iters)
                        assert name not in listed, (D, K, iters)
                        assert ("_lds<" in name) <= ("NoPrescreen" in name), (D, K, iters, name)
                        assert ops.query_sizing(D, K, iters)[1] <= 512 or "NoPrescreen" in name
    # 2. no uint8 row of a D the entry points take has layout {64, 16}; and the names are all the
    # kernels of that layout and type the library holds
    wide = {n for n, reason in listed.items() if reason == WIDE_BYTE_ROWS}
    assert no_lds | wide == set(listed)
    scan = dict(UNREACHABLE_SCAN)
    assert set(scan.values()) == {WIDE_BYTE_ROWS}
    held = {n for n in kernels if "labelrange" in n and "<unsigned char, 64, 16, " in n}
    assert held == wide | set(scan)
    byte_layouts = {ops.dist_layout(D, torch.uint8) for D in range(1, 4097)}
    assert (64, 16) not in byte_layouts and (64, 4) in byte_layouts and len(byte_layouts) == 6
    assert ops.dist_layout(4096, torch.uint8) == (64, 4) and ops.dist_layout(4097, torch.uint8) == (64, 16)


def test_every_labelrange_scan_kernel_has_a_cell(kernels):
    from test_gpu_labelrange_layout_matrix import SCAN_KS, SCAN_MATRIX, bf_labelrange_kernel
    lib = scan_kernels(kernels)
    covered = {bf_labelrange_kernel(kind, D, m, K) for kind, D, m in SCAN_MATRIX for K in SCAN_KS}
    listed = dict(UNREACHABLE_SCAN)
    missing = sorted(n for n in lib if n not in covered and n not in listed)
    assert not missing, f"label-range scan kernels without a cell and K in the GPU matrix: {missing}"
    gone = sorted(n for n in listed if n not in lib)
    assert not gone, f"unreachable scan kernels that are not in the library: {gone}"
    both = sorted(n for n in listed if n in covered)
    assert not both, f"unreachable scan kernels that a cell of SCAN_MATRIX launches: {both}"
    unknown = sorted(n for n in covered if n not in lib)
    assert not unknown, f"cells of SCAN_MATRIX whose kernel is not in the library: {unknown}"
    reachable = [n for n in lib if n not in listed]
    print(f"{len(reachable)} label-range scan kernels reachable, {len(listed)} unreachable")
    # 224 kernels: 27 layouts (7 float32, 6 uint8, 7 + 7 16-bit) x 2 measures x (R = 1, 2, 4 and the
    # LDS list) = 216, and the 8 of uint8 {64,16}
    assert len(reachable) >= 216 and len(lib) >= 224


def test_no_labelrange_kernel_for_int8_rows_or_exact_codes(kernels):
    """label ranges are not built for int8 rows (GGNN_UNSUPPORTED), and a lossless base takes the
    ordinary pre-screened kernels: no PrescreenExact variant under either name"""
    for n in labelrange_kernels(kernels) + scan_kernels(kernels):
        assert "signed char" not in n.replace("unsigned char", ""), n
        assert "PrescreenExact" not in n, n


def test_the_cases_lie_on_every_rung(kernels):
    """the points of LADDER_CASES are meant to take one kernel each: per cell the long lists give
    list registers 2, 4, 8, 16, 32 and the LDS list, the early-rows cells both bucket counts and
    the R = 1 kernel without early rows; the scan's K the list registers 1, 2, 4 and the LDS list"""
    from test_gpu_labelrange_layout_matrix import (BASE_POINT, LADDER_CASES, LONG_POINTS, MATRIX,
                                                   SCAN_KS, SCAN_MATRIX, bf_labelrange_kernel,
                                                   labelrange_kernel)
    from test_gpu_labelset_layout_matrix import EARLY_DIMS, NO_EARLY, VIS_HOOKS
    for kind, D, m in MATRIX:
        names = [labelrange_kernel(kind, D, m, K, iters) for K, tau, iters in LONG_POINTS]
        regs = [re.search(r", (\d+), [01], (No)?Prescreen", n) for n in names[:-1]]
        assert [int(r.group(1)) for r in regs] == [2, 4, 8, 16, 32], (kind, D, m, names)
        assert names[-1].startswith("query_labelrange_kernel_lds<"), names[-1]
        assert [("NoPrescreen" not in n) for n in names] == [kind == "f32_ps"] * 3 + [False] * 3
        base = labelrange_kernel(kind, D, m, BASE_POINT[0], BASE_POINT[2])
        cell = [c[3:] for c in LADDER_CASES if c[:3] == (kind, D, m)]
        assert all((*p, ()) in cell for p in [BASE_POINT] + LONG_POINTS), (kind, D, m)
        if D in EARLY_DIMS[kind]:
            assert base.endswith(", 1, true>"), base
            assert labelrange_kernel(kind, D, m, 10, 400).endswith(", 2, true>")
            plain = labelrange_kernel(kind, D, m, 10, 600)
            assert plain.endswith(", 0, false>") and f", 1, {m}, " in plain
            for iters in (BASE_POINT[2], 400):
                assert labelrange_kernel(kind, D, m, 10, iters, NO_EARLY) == plain
                assert (10, 0.6, iters, NO_EARLY) in cell
            assert (10, 0.6, 400, ()) in cell and (10, 0.6, 600, ()) in cell
            hooked = [c for c in cell if c[3] in VIS_HOOKS]
            assert len(hooked) == (8 if kind in ("f32", "f32_ps") else 0), (kind, D, m)
        else:
            assert base.endswith(", 0, false>"), base
            assert len(cell) == 7, (kind, D, m)
        assert base in kernels
    for kind, D, m in SCAN_MATRIX:
        names = [bf_labelrange_kernel(kind, D, m, K) for K in SCAN_KS]
        regs = [re.search(r", (\d+), [01]>$", n) for n in names[:-1]]
        assert [int(r.group(1)) for r in regs] == [1, 2, 4], names
        assert names[-1].startswith("bf_query_labelrange_lds_kernel<"), names[-1]


def test_the_range_lists_select_the_masks_of_the_label_sets():
    """RANGES on the plain column and EDGE_RANGES on the edge column, as lists and as the int32
    arrays the device takes (width 4; width 3 on the long lists), against `composed` of the label-set
    module for every (D, measure), with filter ids and without"""
    from test_gpu_labelrange_layout_matrix import MATRIX, check_masks
    cells = sorted({(D, m) for kind, D, m in MATRIX})
    assert len(cells) >= 20
    for D, m in cells:
        check_masks(D, m)
