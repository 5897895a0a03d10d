"""CPU: the oracle's wave-order layout table equals the engine's, and the GPU layout matrix covers
every layout cell.

The oracle restates the kernels' summation order (orc.wave_order) from its own copy of the row
layout table (wave_layout in oracle/ggnn_oracle.cpp).  If that copy and pick_dist_config
(ggnn_amd/csrc/traversal.hpp) drift apart, every D the GPU tests do not happen to use gets a
wave-order oracle that sums in the wrong order.  And a layout cell without a GPU case is a kernel
instantiation that ships untested: a change to the table fails here until
tests/test_gpu_layout_matrix.py covers the new cell."""
import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def layouts(orc):
    from ggnn_amd import ops
    out = {}
    for name, tdt in (("f32", torch.float32), ("u8", torch.uint8)):
        code = getattr(orc, "F32" if name == "f32" else "U8")
        for D in range(1, 4097):
            eng = ops.dist_layout(D, tdt)
            assert eng == orc.wave_layout(D, code), (name, D, eng, orc.wave_layout(D, code))
            out[(name, D)] = eng
    return out


def test_engine_layout_equals_oracle_layout_for_every_d(layouts):
    assert len(layouts) == 2 * 4096
    # the table itself: 16-byte chunks per row = lanes per row x chunks per lane, at least
    epc = {"f32": 4, "u8": 16}
    for (name, D), (lpr, nch) in layouts.items():
        assert lpr * nch * epc[name] >= D, (name, D, lpr, nch)
        assert lpr in (8, 16, 64), (name, D, lpr)


def test_layout_matrix_covers_every_cell_and_measure(layouts):
    from test_gpu_layout_matrix import MATRIX
    cells = {(name, lpr, nch) for (name, D), (lpr, nch) in layouts.items()}
    # float32 reaches all seven layouts, uint8 (16 elements per chunk, D <= 4096) six of them
    assert len([c for c in cells if c[0] == "f32"]) == 7
    assert len([c for c in cells if c[0] == "u8"]) == 6
    covered = {(name, *layouts[(name, D)], m) for name, D, m in MATRIX}
    missing = sorted((name, lpr, nch, m) for name, lpr, nch in cells for m in (0, 1)
                     if (name, lpr, nch, m) not in covered)
    assert not missing, f"layout cells without a case in test_gpu_layout_matrix.MATRIX: {missing}"
