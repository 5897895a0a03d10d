"""CPU: the filtered layout matrix covers every layout cell.

query_filtered_kernel*, query_labeled_kernel* and the FILT / LAB forms of the scan kernels are
instantiated per row layout <LPR, NCH> of pick_dist_config (ggnn_amd/csrc/traversal.hpp), element
type and measure.  A cell without a case in tests/test_gpu_filtered_layout_matrix.py is a filtered
kernel that no reference has ever met under a filter that denies a row: a new layout, or a D moved
to another one, fails here until the filtered matrix follows."""
import pytest

torch = pytest.importorskip("torch")

TYPES = {"f32": torch.float32, "u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def layouts():
    from ggnn_amd import ops
    return {(name, D): ops.dist_layout(D, tdt) for name, tdt in TYPES.items()
            for D in range(1, 4097)}


def test_filtered_matrix_covers_every_cell_and_measure(layouts):
    from test_gpu_filtered_layout_matrix import MATRIX
    cells = {(name, lpr, nch) for (name, D), (lpr, nch) in layouts.items()}
    # float32 and the 16-bit types reach all seven layouts, uint8 (16 elements per chunk) six
    assert {t: len([c for c in cells if c[0] == t]) for t in TYPES} == \
        {"f32": 7, "u8": 6, "f16": 7, "bf16": 7}
    covered = {(name, *layouts[(name, D)], m) for name, D, m in MATRIX if name in TYPES}
    missing = sorted((name, lpr, nch, m) for name, lpr, nch in cells for m in (0, 1)
                     if (name, lpr, nch, m) not in covered)
    assert not missing, \
        f"layout cells without a case in test_gpu_filtered_layout_matrix.MATRIX: {missing}"


def test_prescreened_float32_runs_wherever_float32_does():
    """the pre-screened traversal is a kernel family of its own per float32 layout"""
    from test_gpu_filtered_layout_matrix import MATRIX
    plain = {(D, m) for name, D, m in MATRIX if name == "f32"}
    screened = {(D, m) for name, D, m in MATRIX if name == "f32_ps"}
    assert plain == screened and plain
