"""CPU: int8 (signed 8-bit) base and query rows, GGNN_I8 = 5, at the boundary.

The dtype codes of the C-ABI (5 is int8, 4 stays reserved and refused), the row layout table (that
of uint8 rows: 16 elements per 16-byte chunk, six cells), what set_base accepts, that a query of
another element type is refused, CharDataset, the Evaluator on signed rows (a guard: it widens
through astype(float32) already), Dataset<int8_t> through the C++ facade, the resources of the int8
counterparts of the uint8 kernels that tests/test_kernel_resources.py guards, and a GPU case for
every int8 query kernel in the library.  No compute calls."""
import ctypes as C

import numpy as np
import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture: the built library's code objects)
from test_kernel_resources import pytestmark as needs_built_library

torch = pytest.importorskip("torch")

# chunks = ceil(D / 16) -> (lanes per row, chunks per lane), traversal.hpp pick_dist_config
CELLS = {(8, 1), (8, 2), (8, 3), (16, 2), (16, 4), (64, 4)}


def int8_rows(N, D, seed):
    """full-range signed bytes, -128 and 127 included"""
    a = np.random.default_rng(seed).integers(-128, 128, (N, D)).astype(np.int8)
    a[0, 0], a[0, 1] = -128, 127
    return a


# ---- dtype codes -------------------------------------------------------------------------------
def test_c_abi_int8_code():
    from ggnn_amd import _lib
    lib = _lib.lib()
    assert _lib.I8 == 5
    data = int8_rows(16, 16, 1)
    for code, want in ((_lib.I8, _lib.OK), (4, _lib.INVALID_ARGUMENT), (6, _lib.INVALID_ARGUMENT)):
        h = C.c_void_p()
        assert lib.ggnn_create(C.byref(h)) == _lib.OK
        try:
            st = lib.ggnn_set_base(h, data.ctypes.data, 16, 16, code, _lib.CPU, 0, 1)
            assert st == want, (code, st, lib.ggnn_last_error(h))
        finally:
            lib.ggnn_destroy(h)
    lpr, nch = C.c_uint32(), C.c_uint32()
    assert lib.ggnn_op_dist_layout(128, 5, C.byref(lpr), C.byref(nch)) == _lib.OK
    assert (lpr.value, nch.value) == (8, 1)
    for code in (4, 6):
        assert lib.ggnn_op_dist_layout(128, code, C.byref(lpr), C.byref(nch)) == _lib.INVALID_ARGUMENT


# ---- layouts -----------------------------------------------------------------------------------
def test_dist_layout_of_int8_rows_is_that_of_uint8_rows():
    from ggnn_amd import ops
    seen = set()
    for D in range(1, 4097):
        cell = ops.dist_layout(D, torch.int8)
        assert cell == ops.dist_layout(D, torch.uint8), D
        seen.add(cell)
    assert seen == CELLS


def test_gpu_matrix_covers_every_int8_cell():
    from ggnn_amd import ops
    from test_gpu_int8_parity import MATRIX
    covered = {(ops.dist_layout(D, torch.int8), m) for D, m in MATRIX}
    assert covered == {(c, m) for c in CELLS for m in (0, 1)}
    # D = 48: three chunks in the {8, 1} layout, chunk_valid is false on five lanes
    assert (48, 0) in MATRIX and (48, 1) in MATRIX


# ---- boundary ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["torch", "numpy"])
@pytest.mark.parametrize("D", [64, 100])      # 100: rows padded to 112 elements
def test_set_base_accepts_int8_rows(kind, D):
    import ggnn_amd as ggnn
    a = int8_rows(300, D, 5)
    rows = a if kind == "numpy" else torch.from_numpy(a)
    eng = ggnn.GGNN()
    eng.set_base(rows)
    eng2 = ggnn.GGNN()
    eng2.set_base_reference(rows)


OTHER_TYPES = {
    "f32": lambda a: torch.from_numpy(a.astype(np.float32)),
    "u8": lambda a: torch.from_numpy(a.view(np.uint8) ^ 0x80),
    "f16": lambda a: torch.from_numpy(a.astype(np.float32)).to(torch.float16),
    "bf16": lambda a: torch.from_numpy(a.astype(np.float32)).to(torch.bfloat16),
}


@pytest.mark.parametrize("other", list(OTHER_TYPES))
def test_query_of_another_dtype_is_refused(other):
    import ggnn_amd as ggnn
    a = int8_rows(200, 64, 7)
    eng = ggnn.GGNN()
    eng.set_base(torch.from_numpy(a))
    with pytest.raises(RuntimeError, match="query data type does not match"):
        eng.bf_query(OTHER_TYPES[other](a[:5]), 10)
    eng = ggnn.GGNN()
    eng.set_base(OTHER_TYPES[other](a))
    with pytest.raises(RuntimeError, match="query data type does not match"):
        eng.bf_query(torch.from_numpy(a[:5].copy()), 10)


def test_float64_is_still_refused_and_the_messages_name_int8():
    import ggnn_amd as ggnn
    from ggnn_amd import ops
    eng = ggnn.GGNN()
    with pytest.raises(TypeError) as e:
        eng.set_base(np.zeros((10, 16), np.float64))
    assert "int8, float32, uint8, float16 and bfloat16 are supported" in str(e.value)
    assert "float32, uint8, float16 and bfloat16" in str(e.value)
    with pytest.raises(TypeError) as e:
        ops._dtype_code(torch.zeros(2, 2, dtype=torch.float64))
    assert "int8, float32, uint8, float16 or bfloat16" in str(e.value)
    assert "float32, uint8, float16 or bfloat16" in str(e.value)


# ---- CharDataset -------------------------------------------------------------------------------
def test_char_dataset_round_trip(tmp_path):
    import ggnn_amd as ggnn
    assert "CharDataset" in ggnn.__all__
    a = int8_rows(37, 24, 11)
    assert (a < 0).any()
    f = str(tmp_path / "x.bvecs")
    ggnn.CharDataset(a).store(f)
    back = ggnn.CharDataset.load(f)
    assert back.view.dtype == torch.int8 and (back.N, back.D) == (37, 24)
    assert np.array_equal(back.view.numpy(), a)
    part = ggnn.CharDataset.load(f, from_=5, num=9)
    assert np.array_equal(part.view.numpy(), a[5:14])
    assert ggnn.CharDataset.load(f, from_=30, num=100).N == 7
    # the record layout of UCharDataset: the same file read as unsigned bytes
    assert np.array_equal(ggnn.UCharDataset.load(f).view.numpy(), a.view(np.uint8))
    with pytest.raises(TypeError):
        ggnn.CharDataset(a.view(np.uint8))


# ---- Evaluator ---------------------------------------------------------------------------------
def test_evaluator_widens_int8_rows():
    """the case of test_half_dtypes.test_evaluator_widens_16bit_rows, with values below zero"""
    import ggnn_amd as ggnn
    r = np.random.default_rng(9)
    base8 = torch.from_numpy(r.integers(-128, 128, (500, 32)).astype(np.int8))
    q8 = torch.from_numpy(r.integers(-128, 128, (20, 32)).astype(np.int8))
    base, q = base8.float(), q8.float()
    d = ((q[:, None, :] - base[None]) ** 2).sum(-1)
    gt = torch.argsort(d, dim=1, stable=True)[:, :10].to(torch.int32).contiguous()
    res = torch.flip(gt, [1]).contiguous()
    a = ggnn.Evaluator(base8, q8, gt, 10).evaluate_results(res)
    b = ggnn.Evaluator(base, q, gt, 10).evaluate_results(res)
    assert repr(a) == repr(b) and a.c1 == b.c1 and a.r_k_query == b.r_k_query


# ---- kernel resources --------------------------------------------------------------------------
# the `signed char` counterparts of the uint8 entries of test_kernel_resources.DEFAULT_KERNELS and of
# its production merge entry, inside the budgets that file states for uint8 rows: the int8 kernels
# do the same work with another dot instruction
INT8_KERNELS = [
    ("query_kernel<signed char, 8, 1, 1, 0, NoPrescreen, 1, true, true>", 64),
    ("query_kernel<signed char, 8, 1, 1, 0, NoPrescreen, 2, true, true>", 64),
    ("merge_kernel<signed char, 8, 1, 1, 0, NoPrescreen, 1, true, true>", 72),
    ("merge_kernel<signed char, 8, 1, 1, 0, NoPrescreen, 1, true, false>", 72),
    ("sym_kernel<signed char, 8, 1, 1, 0, NoPrescreen>", 72),
]


@needs_built_library
@pytest.mark.parametrize("name,vgprs", INT8_KERNELS)
def test_int8_kernels_have_no_scratch(kernels, name, vgprs):  # noqa: F811
    assert name in kernels, f"{name} is not in the library"
    k = kernels[name]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= vgprs, k


@needs_built_library
def test_int8_kernels_exist_on_six_layouts_only(kernels):  # noqa: F811
    """rows of at most 4096 bytes never reach {64, 16}: no kernel of it ships for the type"""
    import re
    # the kernels templated on <BaseT, LPR, NCH, ...> (DistEngine users)
    families = ("query_kernel", "query_kernel_lds", "query_filtered_kernel", "query_filtered_kernel_lds",
                "query_labeled_kernel", "query_labeled_kernel_lds", "merge_kernel", "sym_kernel",
                "top_kernel", "bf_query_kernel", "bf_query_lds_kernel", "bf_rerank_kernel")
    cells = {f: set() for f in families}
    for name in kernels:
        m = re.match(r"(\w+)<signed char, (\d+), (\d+), ", name)
        if m and m.group(1) in cells:
            cells[m.group(1)].add((int(m.group(2)), int(m.group(3))))
    for f in families:
        assert cells[f] == CELLS, (f, cells[f])


# ---- kernel coverage ---------------------------------------------------------------------------
# Every `signed char` query kernel in the library -- query, query_filtered, query_labeled and their
# LDS-list forms -- is the kernel of at least one case of test_gpu_int8_parity.LADDER_CASES (by the
# launchers' ladder restated there, int8_kernel), or stands in UNREACHABLE with the reason why no
# launch reaches it.  The idea of tests/test_lossless_coverage.py, applied to the new type: a new
# variant, or a D moved to another layout, fails here until the GPU cases follow.
#
# UNREACHABLE: the hashed set (HB 1, 2) and the tag set (HB -8, -9) are taken for one chunk per lane
# only (`fits = PSC::enabled || NCH == 1`, QueryLadder::launch), and every int8 layout but {8, 1}
# has two chunks or more; QueryLadder instantiates the four variants for those layouts all the same,
# as it does for uint8 rows.
MULTI_CHUNK = "hashed / tag sets need NCH == 1 without pre-screen; instantiated by QueryLadder anyway"
UNREACHABLE = {f"query_kernel<signed char, {lpr}, {nch}, 1, {m}, NoPrescreen, {hb}, false, false>":
               MULTI_CHUNK
               for lpr, nch in sorted(CELLS - {(8, 1)}) for m in (0, 1) for hb in (1, 2, -8, -9)}


@needs_built_library
def test_every_int8_query_kernel_has_a_gpu_case(kernels):  # noqa: F811
    from test_gpu_int8_parity import LADDER_CASES, int8_kernel
    lib = {n for n in kernels if n.startswith("query_") and "<signed char, " in n}
    covered = {}
    for how, D, m, K, tau, iters, hooks in LADDER_CASES:
        covered.setdefault(int8_kernel(how, D, m, K, iters, hooks), []).append((how, D, m, K, iters))
    missing = sorted(lib - set(covered) - set(UNREACHABLE))
    assert not missing, f"int8 query kernels without a case in LADDER_CASES: {missing}"
    unknown = sorted(set(covered) - lib)
    assert not unknown, f"cases whose restated kernel is not in the library: {unknown}"
    gone = sorted(set(UNREACHABLE) - lib)
    assert not gone, f"UNREACHABLE lists kernels that are not in the library: {gone}"
    both = sorted(set(UNREACHABLE) & set(covered))
    assert not both, f"UNREACHABLE kernels that a case launches: {both}"
    print(f"{len(lib)} int8 query kernels: {len(covered)} launched, {len(UNREACHABLE)} unreachable")
    assert len(lib) == len(covered) + len(UNREACHABLE)


def test_the_unreachable_int8_kernels_are_never_chosen():
    """the reason in UNREACHABLE against the restated ladder: at no D of a multi-chunk layout does
    any iteration count, with or without early rows, pick a hashed or tag set"""
    from ggnn_amd import ops
    from test_gpu_int8_parity import int8_kernel
    dims = {}
    for D in range(16, 4097, 16):
        dims.setdefault(ops.dist_layout(D, torch.int8), D)
    for cell, D in dims.items():
        if cell == (8, 1):
            continue
        for iters in (100, 175, 200, 400, 500, 600, 1000, 1500, 2040, 4000):
            for hooks in ((), (("QUERY_EARLY", 0),)):
                for kb in (24, 40):
                    name = int8_kernel("plain", D, 0, 10, iters, hooks, kbuild=kb)
                    assert name.endswith("NoPrescreen, 0, false, false>"), (D, iters, hooks, name)


# ---- C++ facade --------------------------------------------------------------------------------
FACADE_PROGRAM = r'''
#include <ggnn/base/ggnn.cuh>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
using namespace ggnn;
int main()
{
  static_assert(detail::TypeTag<int8_t>::value == DataType::INT8);
  std::vector<int8_t> rows(300 * 32);
  for (size_t i = 0; i < rows.size(); ++i)
    rows[i] = static_cast<int8_t>(static_cast<int>(i * 37 % 256) - 128);
  Dataset<int8_t> base = Dataset<int8_t>::copy(rows, 32);
  if (base.N != 300 || base.D != 32 || base[0] != -128 || base.type != DataType::INT8)
    return 2;
  ggnn::GGNN<int32_t, float> engine;
  engine.setBaseReference(base);          // GGNN_I8 through dtype_of: accepted
  ggnn::GGNN<int32_t, float> other;
  Dataset<int32_t> ints = Dataset<int32_t>::empty(10, 32);
  try {
    other.setBaseReference(ints);
    return 3;
  }
  catch (const std::runtime_error& e) {
    if (std::string(e.what()).find("int8_t") == std::string::npos)
      return 4;
  }
  std::printf("int8 facade ok\n");
  return 0;
}
'''


def test_cpp_facade_takes_int8_datasets(tmp_path):
    """Dataset<int8_t> maps to GGNN_I8 in include/ggnn/base/ggnn.cuh (set on the host: no GPU);
    another integer type is still refused, by the extended message"""
    import subprocess
    from test_cpp_facade import FLAGS, LINK
    from ggnn_amd import _lib
    _lib.lib()
    src, exe = tmp_path / "facade_int8.cpp", tmp_path / "facade_int8"
    src.write_text(FACADE_PROGRAM)
    subprocess.check_call(["g++", *FLAGS, str(src), *LINK, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "int8 facade ok" in out.stdout, out.stdout + out.stderr
