"""CPU tests of the label-range filters (include/ggnn_c.h, ggnn_*_labeled_range): the new C-ABI
symbols, the status codes that need no device, the padding and validation of `label_ranges` in
Python, `ordered_int32`, and the built kernels of the new family read from the library's code
objects."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_kernel_resources import FILTERED_KERNELS, kernels  # noqa: F401  (the module fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN, MAX = -2 ** 31, 2 ** 31 - 1

NEW_SYMBOLS = {
    # name -> number of parameters of the prototype in include/ggnn_c.h: those of *_labeled_in
    "ggnn_query_labeled_range": 21,        # ggnn_query (14) + ranges, n, location, gpu + ids, location, gpu
    "ggnn_bf_query_labeled_range": 19,     # ggnn_bf_query (12) + 7
    "ggnn_query_async_labeled_range": 16,  # ggnn_query_async (13) + ranges, n, ids
    "ggnn_op_query_labeled_range": 34,     # ggnn_op_query_labeled_in, ranges for sets
    "ggnn_op_bf_query_labeled_range": 20,  # ggnn_op_bf_query_labeled_in, likewise
}


def test_new_symbols_match_the_header():
    from ggnn_amd import _lib
    lib = _lib.lib()
    src = open(os.path.join(ROOT, "include", "ggnn_c.h")).read()
    assert re.search(r"#define\s+GGNN_MAX_LABEL_RANGES\s+4\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_params in NEW_SYMBOLS.items():
        m = re.search(r"ggnn_status\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in ggnn_c.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == n_params, (name, len(params))
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == n_params, name
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is C.c_void_p, (name, p)
            elif p.startswith("uint64_t"):
                assert t is C.c_uint64, (name, p)
            elif p.startswith("uint32_t"):
                assert t is C.c_uint32, (name, p)
            elif p.startswith("float"):
                assert t is C.c_float, (name, p)
            else:                                  # enums and int
                assert t is C.c_int, (name, p)
        # the argument list of the label-set call, with ranges for sets
        assert argtypes == _lib.SIGNATURES[name.replace("_range", "_in")][1], name
        assert "query_label_ranges" in m.group(1) and "n_ranges" in m.group(1), name
    # existing entry points keep their signatures
    assert len(_lib.SIGNATURES["ggnn_query_labeled_in"][1]) == 21
    assert len(_lib.SIGNATURES["ggnn_op_query_labeled_in"][1]) == 34


def test_status_codes_without_a_device():
    from ggnn_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.ggnn_create(C.byref(h)) == _lib.OK
    try:
        N, D = 100, 16
        base = np.zeros((N, D), np.float32)
        q = np.zeros((2, D), np.float32)
        ids = np.zeros((2, 5), np.int32)
        dists = np.zeros((2, 5), np.float32)
        labels = (np.arange(N) % 7).astype(np.int32)
        ranges = np.array([[[3, 4], [1, 0], [MIN, MAX]], [[-1, -1], [0, 0], [MAX, MIN]]], np.int32)
        fids = np.array([0, -1], np.int32)
        table = np.full((2, (N + 31) // 32), -1, np.int32)

        def query_range(ranges_ptr, n, ids_ptr, qq=q, dtype=_lib.F32):
            return lib.ggnn_query_labeled_range(h, qq.ctypes.data, 2, D, dtype, _lib.CPU, 0, 5, 0.5,
                                                100, 0, ids.ctypes.data, dists.ctypes.data,
                                                _lib.CPU, ranges_ptr, n, _lib.CPU, 0, ids_ptr,
                                                _lib.CPU, 0)

        def bf_range(ranges_ptr, n, ids_ptr, qq=q, dtype=_lib.F32):
            return lib.ggnn_bf_query_labeled_range(h, qq.ctypes.data, 2, D, dtype, _lib.CPU, 0, 5,
                                                   0, ids.ctypes.data, dists.ctypes.data, _lib.CPU,
                                                   ranges_ptr, n, _lib.CPU, 0, ids_ptr, _lib.CPU, 0)

        def async_range(ranges_ptr, n, ids_ptr, qq=q, dtype=_lib.F32):
            return lib.ggnn_query_async_labeled_range(h, qq.ctypes.data, 2, D, dtype, -1, 5, 0.5,
                                                      100, 0, ids.ctypes.data, dists.ctypes.data,
                                                      0, ranges_ptr, n, ids_ptr)

        calls = (query_range, bf_range, async_range)
        assert lib.ggnn_set_base(h, base.ctypes.data, N, D, _lib.F32, _lib.CPU, 0, 1) == _lib.OK
        # no labels yet
        for call in calls:
            assert call(ranges.ctypes.data, 3, None) == _lib.INVALID_STATE, call.__name__
            assert b"labels" in lib.ggnn_last_error(h)
        assert lib.ggnn_set_labels(h, labels.ctypes.data, N, _lib.CPU, 0) == _lib.OK
        for call in calls:
            # the number of ranges and the range array
            for n in (0, 5, 2 ** 31):
                assert call(ranges.ctypes.data, n, None) == _lib.INVALID_ARGUMENT, call.__name__
                assert b"n_ranges" in lib.ggnn_last_error(h)
            assert call(None, 3, None) == _lib.INVALID_ARGUMENT, call.__name__
            # filter ids without a filter table
            assert call(ranges.ctypes.data, 3, fids.ctypes.data) == _lib.INVALID_STATE, call.__name__
            assert b"filter table" in lib.ggnn_last_error(h)
        assert lib.ggnn_set_filters(h, table.ctypes.data, 2, N, _lib.CPU, 0) == _lib.OK
        # host-resident ids outside [-1, num_filters): the blocking calls read them
        for bad in (np.array([0, 2], np.int32), np.array([-2, 1], np.int32)):
            assert query_range(ranges.ctypes.data, 3, bad.ctypes.data) == _lib.INVALID_ARGUMENT
            assert b"outside [-1, 2)" in lib.ggnn_last_error(h)
            assert bf_range(ranges.ctypes.data, 3, bad.ctypes.data) == _lib.INVALID_ARGUMENT
        # well-formed arguments (no range value is invalid), no graph: the state error of ggnn_query
        for n in (1, 3):
            for ids_ptr in (None, fids.ctypes.data):
                assert query_range(ranges.ctypes.data, n, ids_ptr) == _lib.INVALID_STATE
                assert b"graph" in lib.ggnn_last_error(h)
                assert async_range(ranges.ctypes.data, n, ids_ptr) == _lib.INVALID_STATE
        # an int8 base (a handle of its own: the first set_base fixes the type): not built for it
        base8 = np.zeros((N, D), np.int8)
        q8 = np.zeros((2, D), np.int8)
        lib.ggnn_destroy(h)
        assert lib.ggnn_create(C.byref(h)) == _lib.OK
        assert lib.ggnn_set_base(h, base8.ctypes.data, N, D, _lib.I8, _lib.CPU, 0, 1) == _lib.OK
        assert lib.ggnn_set_labels(h, labels.ctypes.data, N, _lib.CPU, 0) == _lib.OK
        for call in calls:
            assert call(ranges.ctypes.data, 3, None, q8, _lib.I8) == _lib.UNSUPPORTED, call.__name__
            assert b"int8" in lib.ggnn_last_error(h)
    finally:
        lib.ggnn_destroy(h)
    # the operator seam checks its label-range arguments before it touches anything
    one = np.zeros(2, np.int32)
    p = one.ctypes.data

    def op(labels_ptr, ranges_ptr, n, table_ptr=None, F=0):
        return lib.ggnn_op_query_labeled_range(None, 0, 0, 0, None, None, None, 0, None, 0, None, 0,
                                               None, 1, 0.5, 1, 0, 1, 0, None, None, None, None,
                                               None, labels_ptr, 1, ranges_ptr, n, table_ptr, F, 32,
                                               None, 0, None)

    def bf_op(labels_ptr, ranges_ptr, n):
        return lib.ggnn_op_bf_query_labeled_range(None, 0, 0, 0, None, 0, 1, 0, None, None,
                                                  labels_ptr, 1, ranges_ptr, n, None, 0, 0, None, 0,
                                                  None)

    for f in (op, bf_op):
        assert f(None, p, 1) == _lib.INVALID_ARGUMENT
        assert f(p, None, 1) == _lib.INVALID_ARGUMENT
        assert f(p, p, 0) == _lib.INVALID_ARGUMENT
        assert f(p, p, 5) == _lib.INVALID_ARGUMENT
    assert op(p, p, 1, p, 0) == _lib.INVALID_ARGUMENT      # a table of no rows
    assert op(p, p, 1, None, 2) == _lib.INVALID_ARGUMENT   # rows of no table


def test_python_surface_and_label_range_arguments():
    import torch

    import ggnn_amd
    from ggnn_amd import ops
    from ggnn_amd.api import MAX_LABEL_RANGES, QueryTicket, _label_ranges
    assert MAX_LABEL_RANGES == ops.MAX_LABEL_RANGES == 4
    for name, want in (
            ("query_labeled_range", ["query", "k_query", "tau_query", "max_iterations", "measure",
                                     "label_ranges", "filter_ids"]),
            ("bf_query_labeled_range", ["query", "k_gt", "measure", "label_ranges", "filter_ids"]),
            ("query_async_labeled_range", ["query", "k_query", "tau_query", "max_iterations",
                                           "measure", "slot", "label_ranges", "filter_ids"])):
        sig = inspect.signature(getattr(ggnn_amd.GGNN, name))
        assert list(sig.parameters)[1:] == want, name
        assert sig.parameters["label_ranges"].default is None
        assert sig.parameters["filter_ids"].default is None
    assert inspect.signature(ggnn_amd.GGNN.query_labeled_range).parameters["max_iterations"].default == 400
    assert inspect.signature(ggnn_amd.GGNN.bf_query_labeled_range).parameters["k_gt"].default == 100
    assert inspect.signature(ggnn_amd.GGNN.query_async_labeled_range).parameters["slot"].default == 0
    # the existing methods keep their signatures
    assert list(inspect.signature(ggnn_amd.GGNN.query_labeled_in).parameters)[1:] == [
        "query", "k_query", "tau_query", "max_iterations", "measure", "label_sets", "filter_ids"]
    assert list(inspect.signature(ggnn_amd.GGNN.query_async_labeled_in).parameters)[-3:] == [
        "slot", "label_sets", "filter_ids"]
    for name in ("query_labeled_range", "bf_query_labeled_range", "_need_label_ranges"):
        assert callable(getattr(ops, name)), name
    assert "label_ranges" in QueryTicket.__slots__ and "label_sets" in QueryTicket.__slots__

    # ragged rows are padded to the longest with an EMPTY interval (lo > hi)
    lr = _label_ranges([[(1, 5)], [(2, 3), (-7, -7), (MIN, MAX)], ((0, 0), [9, 8])], 3)
    assert lr.dtype == torch.int32 and lr.is_contiguous() and tuple(lr.shape) == (3, 3, 2)
    assert lr.tolist() == [[[1, 5], [1, 0], [1, 0]], [[2, 3], [-7, -7], [MIN, MAX]],
                           [[0, 0], [9, 8], [1, 0]]]
    assert _label_ranges([[(4, 4)]], 1).tolist() == [[[4, 4]]]
    assert _label_ranges([[np.array([5, 6])], [torch.tensor([7, 8]), (1, 2)]], 2).tolist() == [
        [[5, 6], [1, 0]], [[7, 8], [1, 2]]]
    four = [(i, i + 1) for i in range(4)]
    assert _label_ranges([four, [(MAX, MIN)]], 2).tolist() == [
        [list(p) for p in four], [[MAX, MIN]] + [[1, 0]] * 3]
    # 3-D arrays and tensors are taken as they are; int64 is converted
    a = np.array([[[1, 2], [3, -1]], [[MIN, MAX], [0, 0]]], np.int32)
    assert _label_ranges(a, 2).tolist() == a.tolist()
    t = _label_ranges(torch.from_numpy(a.astype(np.int64)), 2)
    assert t.dtype == torch.int32 and t.tolist() == a.tolist()
    f = np.asfortranarray(np.arange(12, dtype=np.int32).reshape(2, 3, 2))
    assert _label_ranges(f, 2).is_contiguous() and _label_ranges(f, 2).tolist() == f.tolist()
    # no interval, five of them, a 3-D array of 0 or 5 intervals, a wrong number of rows
    for bad in ([[(1, 2)], []], [[(1, 2)], [(i, i) for i in range(5)]],
                np.zeros((2, 5, 2), np.int32), np.zeros((2, 0, 2), np.int32),
                np.zeros((3, 2, 2), np.int32), [[(1, 2)]], [[(1, 2)], [(1, 2, 3)]]):
        with pytest.raises(ValueError):
            _label_ranges(bad, 2)
    with pytest.raises(ValueError):
        _label_ranges(np.array([[[0, 2 ** 31]]], np.int64), 1)
    with pytest.raises(ValueError):
        _label_ranges(np.array([[[-2 ** 31 - 1, 0]]], np.int64), 1)
    with pytest.raises(ValueError):
        _label_ranges([[(0, 2 ** 31)]], 1)
    with pytest.raises(TypeError):
        _label_ranges(np.zeros((2, 2), np.int32), 2)       # 2-D: that is `label_sets`
    with pytest.raises(TypeError):
        _label_ranges(np.zeros((2, 2, 3), np.int32), 2)    # not pairs
    with pytest.raises(TypeError):
        _label_ranges(np.zeros((2, 2, 2), np.float32), 2)


def test_ordered_int32():
    import torch

    import ggnn_amd
    from ggnn_amd import ordered_int32
    assert "ordered_int32" in ggnn_amd.__all__
    tiny = np.float32(1e-45)                               # the smallest subnormal
    x = np.array([-np.inf, -3.0e38, -1.5, -1.0, -1e-38, -tiny, 0.0, tiny, 1e-40, 1e-38, 0.5, 1.0,
                  1.0 + 2.0 ** -23, 7.25, 3.0e38, np.inf], np.float32)
    assert np.all(np.diff(x) > 0) and x[5] < 0 < x[7] and abs(x[5]) < np.finfo(np.float32).tiny
    o = ordered_int32(x)
    assert o.dtype == np.int32 and o.shape == x.shape
    assert np.all(np.diff(o.astype(np.int64)) > 0), o      # strictly order-preserving
    # -0.0 and +0.0 are equal values: one image, between the subnormals of either sign
    z = ordered_int32(np.array([-0.0, 0.0], np.float32))
    assert z[0] == z[1] == 0 and o[5] < 0 < o[7]
    # the formula, on the bits; non-negative floats keep their bits
    b = x.view(np.int32)
    assert np.array_equal(o, b ^ ((b >> 31) & 0x7fffffff))
    assert np.array_equal(o[6:], b[6:])
    assert o[0] == ordered_int32(np.float32(-np.inf)) == -0x7f800001 and o[-1] == 0x7f800000
    # tensors: the same values, int32 on the tensor's device; scalars: an int
    t = ordered_int32(torch.from_numpy(x))
    assert t.dtype == torch.int32 and np.array_equal(t.numpy(), o)
    assert ordered_int32(torch.tensor([-0.0, 0.0])).tolist() == [0, 0]
    assert isinstance(ordered_int32(1.5), int) and ordered_int32(1.5) == 0x3fc00000
    assert ordered_int32(-2.0) < ordered_int32(-1.0) < ordered_int32(0.0) < ordered_int32(0.25)
    # random values against a sort
    r = np.random.default_rng(5).standard_normal(4096).astype(np.float32) * np.float32(1e3)
    assert np.array_equal(np.argsort(r, kind="stable"), np.argsort(ordered_int32(r), kind="stable"))
    for bad in (np.array([1.0, np.nan], np.float32), torch.tensor([float("nan")]), float("nan")):
        with pytest.raises(ValueError):
            ordered_int32(bad)
    with pytest.raises(TypeError):
        ordered_int32(np.zeros(3, np.float64))
    with pytest.raises(TypeError):
        ordered_int32(torch.zeros(3, dtype=torch.float64))


def _labelrange(kernels):
    found = {n: k for n, k in kernels.items() if n.startswith("query_labelrange_")}
    assert found, "the library holds no query_labelrange_* kernels"
    return found


def test_early_rows_l2_kernels_have_no_scratch(kernels):  # noqa: F811
    """the early-rows squared-L2 kernels of float32 / uint8 rows (R = 1, HB 1 and 2): no private
    segment at the occupancy the family is built for"""
    pat = re.compile(r"query_labelrange_kernel<(float|unsigned char), \d+, \d+, 1, 0, .*, [12], true>$")
    hit = {n: k for n, k in _labelrange(kernels).items() if pat.match(n)}
    layouts = {re.match(r"query_labelrange_kernel<([^,]+, \d+, \d+)", n).group(1) for n in hit}
    print(sorted((n, k["vgpr_count"]) for n, k in hit.items()))
    # every float32 layout with a pre-screen in front of it, and the 8 x 1 layouts read directly
    assert {"float, 8, 1", "float, 8, 2", "float, 8, 3", "float, 16, 2", "unsigned char, 8, 1"} <= layouts
    assert any("NoPrescreen" in n for n in hit) and any("Prescreen<8, 1, 0>" in n for n in hit)
    for n, k in hit.items():
        assert k["private_segment_fixed_size"] == 0, (n, k)
        assert k["vgpr_spill_count"] == 0, (n, k)
        assert k["vgpr_count"] <= 80, (n, k)


def test_no_int8_and_no_exact_code_kernels(kernels):  # noqa: F811
    names = list(_labelrange(kernels))
    assert any(n.startswith("query_labelrange_kernel_lds<") for n in names)
    for want in ("float", "unsigned char", "f16_t", "bf16_t"):
        assert any(re.match(r"query_labelrange_kernel<" + want + ",", n) for n in names), want
        assert any(re.match(r"query_labelrange_kernel_lds<" + want + ",", n) for n in names), want
    bf = [n for n in kernels if n.startswith("bf_query_labelrange_")]
    assert any(n.startswith("bf_query_labelrange_kernel<") for n in bf)
    assert any(n.startswith("bf_query_labelrange_lds_kernel<") for n in bf)
    for n in names + bf:
        assert "signed char" not in n.replace("unsigned char", ""), n
        assert "PrescreenExact" not in n, n
    # the names the label-set tests select their kernels by stay theirs
    for n in kernels:
        if "labelrange" in n:
            assert "labelset" not in n, n


# The headline and shard kernels under label ranges: DESIGN.md 4.9 quotes these counts.  The bound is
# what the build that introduced the family gave, read with this fixture -- VGPRS below, private
# segment 0 in all four -- so that any growth shows up here.
VGPRS = (75, 77, 75, 77)


@pytest.mark.parametrize("name,vgprs", [
    (n % "query_labelrange_kernel", v) for n, v in zip(FILTERED_KERNELS, VGPRS)])
def test_headline_kernels_keep_their_registers(kernels, name, vgprs):  # noqa: F811
    assert name in kernels, f"{name} is not in the library (renamed template parameters?)"
    k = kernels[name]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= vgprs, k
