"""CPU tests of the label-set filters (include/ggnn_c.h, ggnn_*_labeled_in): the new C-ABI symbols,
the status codes that need no device, the padding and validation of `label_sets` in Python, and the
built kernels of the new family read from the library's code objects."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {
    # name -> number of parameters of the prototype in include/ggnn_c.h
    "ggnn_query_labeled_in": 21,        # ggnn_query (14) + sets, width, location, gpu + ids, location, gpu
    "ggnn_bf_query_labeled_in": 19,     # ggnn_bf_query (12) + 7
    "ggnn_query_async_labeled_in": 16,  # ggnn_query_async (13) + sets, width, ids
    "ggnn_op_query_labeled_in": 34,     # ggnn_op_query_labeled (29) + width, table, F, n_bits, ids
    "ggnn_op_bf_query_labeled_in": 20,  # ggnn_op_bf_query_labeled (15) + 5
}


def test_new_symbols_match_the_header():
    from ggnn_amd import _lib
    lib = _lib.lib()
    src = open(os.path.join(ROOT, "include", "ggnn_c.h")).read()
    assert re.search(r"#define\s+GGNN_MAX_LABEL_SET\s+8\b", src)
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
    # up to out_location the handle calls are the *_labeled prototypes
    for old, new, head in (("ggnn_query_labeled", "ggnn_query_labeled_in", 14),
                           ("ggnn_bf_query_labeled", "ggnn_bf_query_labeled_in", 12),
                           ("ggnn_query_async_labeled", "ggnn_query_async_labeled_in", 13)):
        assert _lib.SIGNATURES[old][1][:head] == _lib.SIGNATURES[new][1][:head], new
    # existing entry points keep their signatures
    assert len(_lib.SIGNATURES["ggnn_query_labeled"][1]) == 17
    assert len(_lib.SIGNATURES["ggnn_op_query_labeled"][1]) == 29


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
        sets = np.array([[3, 4, 3], [-1, 0, 0]], np.int32)
        fids = np.array([0, -1], np.int32)
        table = np.full((2, (N + 31) // 32), -1, np.int32)

        def query_in(sets_ptr, width, ids_ptr, qq=q, dtype=_lib.F32):
            return lib.ggnn_query_labeled_in(h, qq.ctypes.data, 2, D, dtype, _lib.CPU, 0, 5, 0.5,
                                             100, 0, ids.ctypes.data, dists.ctypes.data, _lib.CPU,
                                             sets_ptr, width, _lib.CPU, 0, ids_ptr, _lib.CPU, 0)

        def bf_in(sets_ptr, width, ids_ptr, qq=q, dtype=_lib.F32):
            return lib.ggnn_bf_query_labeled_in(h, qq.ctypes.data, 2, D, dtype, _lib.CPU, 0, 5, 0,
                                                ids.ctypes.data, dists.ctypes.data, _lib.CPU,
                                                sets_ptr, width, _lib.CPU, 0, ids_ptr, _lib.CPU, 0)

        def async_in(sets_ptr, width, ids_ptr, qq=q, dtype=_lib.F32):
            return lib.ggnn_query_async_labeled_in(h, qq.ctypes.data, 2, D, dtype, -1, 5, 0.5, 100, 0,
                                                   ids.ctypes.data, dists.ctypes.data, 0, sets_ptr,
                                                   width, ids_ptr)

        calls = (query_in, bf_in, async_in)
        assert lib.ggnn_set_base(h, base.ctypes.data, N, D, _lib.F32, _lib.CPU, 0, 1) == _lib.OK
        # no labels yet
        for call in calls:
            assert call(sets.ctypes.data, 3, None) == _lib.INVALID_STATE, call.__name__
            assert b"labels" in lib.ggnn_last_error(h)
        assert lib.ggnn_set_labels(h, labels.ctypes.data, N, _lib.CPU, 0) == _lib.OK
        for call in calls:
            # the width and the set array
            for width in (0, 9, 2 ** 31):
                assert call(sets.ctypes.data, width, None) == _lib.INVALID_ARGUMENT, call.__name__
                assert b"set_width" in lib.ggnn_last_error(h)
            assert call(None, 3, None) == _lib.INVALID_ARGUMENT, call.__name__
            # filter ids without a filter table
            assert call(sets.ctypes.data, 3, fids.ctypes.data) == _lib.INVALID_STATE, call.__name__
            assert b"filter table" in lib.ggnn_last_error(h)
        assert lib.ggnn_set_filters(h, table.ctypes.data, 2, N, _lib.CPU, 0) == _lib.OK
        # host-resident ids outside [-1, num_filters): the blocking calls read them
        for bad in (np.array([0, 2], np.int32), np.array([-2, 1], np.int32)):
            assert query_in(sets.ctypes.data, 3, bad.ctypes.data) == _lib.INVALID_ARGUMENT
            assert b"outside [-1, 2)" in lib.ggnn_last_error(h)
            assert bf_in(sets.ctypes.data, 3, bad.ctypes.data) == _lib.INVALID_ARGUMENT
        # well-formed arguments of every width, no graph: the state error of ggnn_query
        for width in (1, 3):
            for ids_ptr in (None, fids.ctypes.data):
                assert query_in(sets.ctypes.data, width, ids_ptr) == _lib.INVALID_STATE
                assert b"graph" in lib.ggnn_last_error(h)
                assert async_in(sets.ctypes.data, width, ids_ptr) == _lib.INVALID_STATE
        # an int8 base (a handle of its own: the first set_base fixes the type): not built for it
        base8 = np.zeros((N, D), np.int8)
        q8 = np.zeros((2, D), np.int8)
        lib.ggnn_destroy(h)
        assert lib.ggnn_create(C.byref(h)) == _lib.OK
        assert lib.ggnn_set_base(h, base8.ctypes.data, N, D, _lib.I8, _lib.CPU, 0, 1) == _lib.OK
        assert lib.ggnn_set_labels(h, labels.ctypes.data, N, _lib.CPU, 0) == _lib.OK
        for call in calls:
            assert call(sets.ctypes.data, 3, None, q8, _lib.I8) == _lib.UNSUPPORTED, call.__name__
            assert b"int8" in lib.ggnn_last_error(h)
    finally:
        lib.ggnn_destroy(h)
    # the operator seam checks its label-set arguments before it touches anything
    one = np.zeros(1, np.int32)
    p = one.ctypes.data

    def op(labels_ptr, sets_ptr, width, table_ptr=None, F=0):
        return lib.ggnn_op_query_labeled_in(None, 0, 0, 0, None, None, None, 0, None, 0, None, 0,
                                            None, 1, 0.5, 1, 0, 1, 0, None, None, None, None, None,
                                            labels_ptr, 1, sets_ptr, width, table_ptr, F, 32, None, 0,
                                            None)

    def bf_op(labels_ptr, sets_ptr, width):
        return lib.ggnn_op_bf_query_labeled_in(None, 0, 0, 0, None, 0, 1, 0, None, None, labels_ptr,
                                               1, sets_ptr, width, None, 0, 0, None, 0, None)

    for f in (op, bf_op):
        assert f(None, p, 1) == _lib.INVALID_ARGUMENT
        assert f(p, None, 1) == _lib.INVALID_ARGUMENT
        assert f(p, p, 0) == _lib.INVALID_ARGUMENT
        assert f(p, p, 9) == _lib.INVALID_ARGUMENT
    assert op(p, p, 1, p, 0) == _lib.INVALID_ARGUMENT      # a table of no rows
    assert op(p, p, 1, None, 2) == _lib.INVALID_ARGUMENT   # rows of no table


def test_python_surface_and_label_set_arguments():
    import torch

    import ggnn_amd
    from ggnn_amd import ops
    from ggnn_amd.api import MAX_LABEL_SET, _label_sets
    assert MAX_LABEL_SET == ops.MAX_LABEL_SET == 8
    for name, want in (
            ("query_labeled_in", ["query", "k_query", "tau_query", "max_iterations", "measure",
                                  "label_sets", "filter_ids"]),
            ("bf_query_labeled_in", ["query", "k_gt", "measure", "label_sets", "filter_ids"]),
            ("query_async_labeled_in", ["query", "k_query", "tau_query", "max_iterations", "measure",
                                        "slot", "label_sets", "filter_ids"])):
        sig = inspect.signature(getattr(ggnn_amd.GGNN, name))
        assert list(sig.parameters)[1:] == want, name
        assert sig.parameters["label_sets"].default is None
        assert sig.parameters["filter_ids"].default is None
    assert inspect.signature(ggnn_amd.GGNN.query_labeled_in).parameters["max_iterations"].default == 400
    assert inspect.signature(ggnn_amd.GGNN.bf_query_labeled_in).parameters["k_gt"].default == 100
    assert inspect.signature(ggnn_amd.GGNN.query_async_labeled_in).parameters["slot"].default == 0
    # the existing methods keep their signatures
    assert list(inspect.signature(ggnn_amd.GGNN.query_labeled).parameters)[1:] == [
        "query", "k_query", "tau_query", "max_iterations", "measure", "labels"]
    assert list(inspect.signature(ggnn_amd.GGNN.query_async).parameters)[-2:] == ["slot", "filter_ids"]
    for name in ("query_labeled_in", "bf_query_labeled_in"):
        assert callable(getattr(ops, name)), name

    # ragged rows are padded to the longest by repeating their first entry
    ls = _label_sets([[1], [2, 3, -7], (0, -1)], 3)
    assert ls.dtype == torch.int32 and ls.is_contiguous()
    assert ls.tolist() == [[1, 1, 1], [2, 3, -7], [0, -1, 0]]
    assert _label_sets([[4]], 1).tolist() == [[4]]
    assert _label_sets([np.array([5, 6]), torch.tensor([7])], 2).tolist() == [[5, 6], [7, 7]]
    eight = list(range(10, 18))
    assert _label_sets([eight, [-2 ** 31, 2 ** 31 - 1]], 2).tolist() == [
        eight, [-2 ** 31, 2 ** 31 - 1] + [-2 ** 31] * 6]
    # 2-D arrays and tensors are taken as they are; int64 is converted
    a = np.array([[1, 2], [3, -1]], np.int32)
    assert _label_sets(a, 2).tolist() == a.tolist()
    t = _label_sets(torch.from_numpy(a.astype(np.int64)), 2)
    assert t.dtype == torch.int32 and t.tolist() == a.tolist()
    assert _label_sets(np.asfortranarray(np.arange(6, dtype=np.int32).reshape(2, 3)), 2).is_contiguous()
    # an empty row, a row of nine, a 2-D array of width 0 or 9, a wrong number of rows
    for bad in ([[1], []], [[1], list(range(9))], np.zeros((2, 9), np.int32), np.zeros((2, 0), np.int32),
                np.zeros((3, 2), np.int32), [[1]]):
        with pytest.raises(ValueError):
            _label_sets(bad, 2)
    with pytest.raises(ValueError):
        _label_sets(np.array([[2 ** 31]], np.int64), 1)
    with pytest.raises(ValueError):
        _label_sets([[2 ** 31]], 1)
    with pytest.raises(TypeError):
        _label_sets(np.zeros(2, np.int32), 2)              # 1-D: that is `labels` of query_labeled
    with pytest.raises(TypeError):
        _label_sets(np.zeros((2, 2), np.float32), 2)


def _labelset(kernels):
    found = {n: k for n, k in kernels.items() if n.startswith("query_labelset_")}
    assert found, "the library holds no query_labelset_* kernels"
    return found


def test_early_rows_l2_kernels_have_no_scratch(kernels):
    """the early-rows squared-L2 kernels of float32 / uint8 rows (R = 1, HB 1 and 2): no private
    segment at the occupancy the family is built for"""
    pat = re.compile(r"query_labelset_kernel<(float|unsigned char), \d+, \d+, 1, 0, .*, [12], true>$")
    hit = {n: k for n, k in _labelset(kernels).items() if pat.match(n)}
    layouts = {re.match(r"query_labelset_kernel<([^,]+, \d+, \d+)", n).group(1) for n in hit}
    print(sorted(hit))
    # every float32 layout with a pre-screen in front of it, and the 8 x 1 layouts read directly
    assert {"float, 8, 1", "float, 8, 2", "float, 8, 3", "float, 16, 2", "unsigned char, 8, 1"} <= layouts
    assert any("NoPrescreen" in n for n in hit) and any("Prescreen<8, 1, 0>" in n for n in hit)
    for n, k in hit.items():
        assert k["private_segment_fixed_size"] == 0, (n, k)
        assert k["vgpr_spill_count"] == 0, (n, k)
        assert k["vgpr_count"] <= 80, (n, k)


def test_no_int8_and_no_exact_code_kernels(kernels):
    names = list(_labelset(kernels))
    assert any(n.startswith("query_labelset_kernel_lds<") for n in names)
    for want in ("float", "unsigned char", "f16_t", "bf16_t"):
        assert any(re.match(r"query_labelset_kernel(_lds)?<" + want + ",", n) for n in names), want
    for n in names:
        assert "signed char" not in n.replace("unsigned char", ""), n
        assert "PrescreenExact" not in n, n
    bf = [n for n in kernels if n.startswith("bf_query_labelset_")]
    assert bf and not any("signed char" in n.replace("unsigned char", "") for n in bf)
