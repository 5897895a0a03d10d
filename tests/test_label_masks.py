"""CPU tests of the label-mask filters (include/ggnn_c.h, ggnn_*_labeled_mask): the new C-ABI
symbols, the status codes that need no device, the padding, wrapping and validation of `label_masks`
in Python, `label_mask`, and the built kernels of the new family read from the library's code
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
B31 = -2 ** 31                                             # bit 31 as an int32

NEW_SYMBOLS = {
    # name -> number of parameters of the prototype in include/ggnn_c.h: those of *_labeled_range
    "ggnn_query_labeled_mask": 21,        # ggnn_query (14) + masks, n, location, gpu + ids, location, gpu
    "ggnn_bf_query_labeled_mask": 19,     # ggnn_bf_query (12) + 7
    "ggnn_query_async_labeled_mask": 16,  # ggnn_query_async (13) + masks, n, ids
    "ggnn_op_query_labeled_mask": 34,     # ggnn_op_query_labeled_range, masks for ranges
    "ggnn_op_bf_query_labeled_mask": 20,  # ggnn_op_bf_query_labeled_range, likewise
}


def test_new_symbols_match_the_header():
    from ggnn_amd import _lib
    lib = _lib.lib()
    src = open(os.path.join(ROOT, "include", "ggnn_c.h")).read()
    assert re.search(r"#define\s+GGNN_MAX_LABEL_MASKS\s+2\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)

    def params_of(name):
        m = re.search(r"ggnn_status\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in ggnn_c.h"
        return [" ".join(p.split()) for p in m.group(1).split(",")]

    for name, n_params in NEW_SYMBOLS.items():
        params = params_of(name)
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
        # the argument list of the label-range call, with masks for ranges: types and names
        twin = name.replace("_mask", "_range")
        assert argtypes == _lib.SIGNATURES[twin][1], name
        renamed = [p.replace("query_label_ranges", "query_label_masks").replace("n_ranges", "n_masks")
                   .replace("ranges_location", "masks_location").replace("ranges_gpu_id", "masks_gpu_id")
                   for p in params_of(twin)]
        assert params == renamed, name
        assert any(p == "const int32_t* query_label_masks" for p in params), name
        assert any(p == "uint32_t n_masks" for p in params), name
    # existing entry points keep their signatures
    assert len(_lib.SIGNATURES["ggnn_query_labeled_range"][1]) == 21
    assert len(_lib.SIGNATURES["ggnn_op_query_labeled_range"][1]) == 34


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
        # clauses of any value, unsatisfiable ones included: (1, 3, 0) has a value bit outside its
        # mask, (B31, 0, -1) uses bit 31 and every any-bit
        masks = np.array([[[3, 1, 4], [1, 3, 0]], [[0, 0, 0], [B31, 0, -1]]], np.int32)
        fids = np.array([0, -1], np.int32)
        table = np.full((2, (N + 31) // 32), -1, np.int32)

        def query_mask(masks_ptr, n, ids_ptr, qq=q, dtype=_lib.F32):
            return lib.ggnn_query_labeled_mask(h, qq.ctypes.data, 2, D, dtype, _lib.CPU, 0, 5, 0.5,
                                               100, 0, ids.ctypes.data, dists.ctypes.data,
                                               _lib.CPU, masks_ptr, n, _lib.CPU, 0, ids_ptr,
                                               _lib.CPU, 0)

        def bf_mask(masks_ptr, n, ids_ptr, qq=q, dtype=_lib.F32):
            return lib.ggnn_bf_query_labeled_mask(h, qq.ctypes.data, 2, D, dtype, _lib.CPU, 0, 5,
                                                  0, ids.ctypes.data, dists.ctypes.data, _lib.CPU,
                                                  masks_ptr, n, _lib.CPU, 0, ids_ptr, _lib.CPU, 0)

        def async_mask(masks_ptr, n, ids_ptr, qq=q, dtype=_lib.F32):
            return lib.ggnn_query_async_labeled_mask(h, qq.ctypes.data, 2, D, dtype, -1, 5, 0.5,
                                                     100, 0, ids.ctypes.data, dists.ctypes.data,
                                                     0, masks_ptr, n, ids_ptr)

        calls = (query_mask, bf_mask, async_mask)
        assert lib.ggnn_set_base(h, base.ctypes.data, N, D, _lib.F32, _lib.CPU, 0, 1) == _lib.OK
        # no labels yet
        for call in calls:
            assert call(masks.ctypes.data, 2, None) == _lib.INVALID_STATE, call.__name__
            assert b"labels" in lib.ggnn_last_error(h)
        assert lib.ggnn_set_labels(h, labels.ctypes.data, N, _lib.CPU, 0) == _lib.OK
        for call in calls:
            # the number of clauses and the clause array
            for n in (0, 3, 2 ** 31):
                assert call(masks.ctypes.data, n, None) == _lib.INVALID_ARGUMENT, call.__name__
                assert b"n_masks" in lib.ggnn_last_error(h)
            assert call(None, 2, None) == _lib.INVALID_ARGUMENT, call.__name__
            # filter ids without a filter table
            assert call(masks.ctypes.data, 2, fids.ctypes.data) == _lib.INVALID_STATE, call.__name__
            assert b"filter table" in lib.ggnn_last_error(h)
        assert lib.ggnn_set_filters(h, table.ctypes.data, 2, N, _lib.CPU, 0) == _lib.OK
        # host-resident ids outside [-1, num_filters): the blocking calls read them
        for bad in (np.array([0, 2], np.int32), np.array([-2, 1], np.int32)):
            assert query_mask(masks.ctypes.data, 2, bad.ctypes.data) == _lib.INVALID_ARGUMENT
            assert b"outside [-1, 2)" in lib.ggnn_last_error(h)
            assert bf_mask(masks.ctypes.data, 2, bad.ctypes.data) == _lib.INVALID_ARGUMENT
        # well-formed arguments (no clause value is invalid), no graph: the state error of ggnn_query
        for n in (1, 2):
            for ids_ptr in (None, fids.ctypes.data):
                assert query_mask(masks.ctypes.data, n, ids_ptr) == _lib.INVALID_STATE
                assert b"graph" in lib.ggnn_last_error(h)
                assert async_mask(masks.ctypes.data, n, ids_ptr) == _lib.INVALID_STATE
        # an int8 base (a handle of its own: the first set_base fixes the type): not built for it
        base8 = np.zeros((N, D), np.int8)
        q8 = np.zeros((2, D), np.int8)
        lib.ggnn_destroy(h)
        assert lib.ggnn_create(C.byref(h)) == _lib.OK
        assert lib.ggnn_set_base(h, base8.ctypes.data, N, D, _lib.I8, _lib.CPU, 0, 1) == _lib.OK
        assert lib.ggnn_set_labels(h, labels.ctypes.data, N, _lib.CPU, 0) == _lib.OK
        for call in calls:
            assert call(masks.ctypes.data, 2, None, q8, _lib.I8) == _lib.UNSUPPORTED, call.__name__
            assert b"int8" in lib.ggnn_last_error(h)
    finally:
        lib.ggnn_destroy(h)
    # the operator seam checks its label-mask arguments before it touches anything
    one = np.zeros(3, np.int32)
    p = one.ctypes.data

    def op(labels_ptr, masks_ptr, n, table_ptr=None, F=0):
        return lib.ggnn_op_query_labeled_mask(None, 0, 0, 0, None, None, None, 0, None, 0, None, 0,
                                              None, 1, 0.5, 1, 0, 1, 0, None, None, None, None,
                                              None, labels_ptr, 1, masks_ptr, n, table_ptr, F, 32,
                                              None, 0, None)

    def bf_op(labels_ptr, masks_ptr, n):
        return lib.ggnn_op_bf_query_labeled_mask(None, 0, 0, 0, None, 0, 1, 0, None, None,
                                                 labels_ptr, 1, masks_ptr, n, None, 0, 0, None, 0,
                                                 None)

    for f in (op, bf_op):
        assert f(None, p, 1) == _lib.INVALID_ARGUMENT
        assert f(p, None, 1) == _lib.INVALID_ARGUMENT
        assert f(p, p, 0) == _lib.INVALID_ARGUMENT
        assert b"n_masks" in lib.ggnn_last_error(None)
        assert f(p, p, 3) == _lib.INVALID_ARGUMENT
    assert op(p, p, 1, p, 0) == _lib.INVALID_ARGUMENT      # a table of no rows
    assert op(p, p, 1, None, 2) == _lib.INVALID_ARGUMENT   # rows of no table


def test_python_surface_and_label_mask_arguments():
    import torch

    import ggnn_amd
    from ggnn_amd import ops
    from ggnn_amd.api import MAX_LABEL_MASKS, QueryTicket, _label_masks
    assert MAX_LABEL_MASKS == ops.MAX_LABEL_MASKS == 2
    for name, want in (
            ("query_labeled_mask", ["query", "k_query", "tau_query", "max_iterations", "measure",
                                    "label_masks", "filter_ids"]),
            ("bf_query_labeled_mask", ["query", "k_gt", "measure", "label_masks", "filter_ids"]),
            ("query_async_labeled_mask", ["query", "k_query", "tau_query", "max_iterations",
                                          "measure", "slot", "label_masks", "filter_ids"])):
        sig = inspect.signature(getattr(ggnn_amd.GGNN, name))
        assert list(sig.parameters)[1:] == want, name
        assert sig.parameters["label_masks"].default is None
        assert sig.parameters["filter_ids"].default is None
    assert inspect.signature(ggnn_amd.GGNN.query_labeled_mask).parameters["max_iterations"].default == 400
    assert inspect.signature(ggnn_amd.GGNN.bf_query_labeled_mask).parameters["k_gt"].default == 100
    assert inspect.signature(ggnn_amd.GGNN.query_async_labeled_mask).parameters["slot"].default == 0
    # the existing methods keep their signatures
    assert list(inspect.signature(ggnn_amd.GGNN.query_labeled_range).parameters)[1:] == [
        "query", "k_query", "tau_query", "max_iterations", "measure", "label_ranges", "filter_ids"]
    assert list(inspect.signature(ggnn_amd.GGNN.query_async_labeled_range).parameters)[-3:] == [
        "slot", "label_ranges", "filter_ids"]
    for name in ("query_labeled_mask", "bf_query_labeled_mask", "_need_label_masks"):
        assert callable(getattr(ops, name)), name
    for name in ("query_labeled_mask", "bf_query_labeled_mask"):
        p = inspect.signature(getattr(ops, name)).parameters
        assert "bit_offset" in p and "label_masks" in p, name
    p = inspect.signature(ops.query_labeled_mask).parameters
    assert "counters" in p and "prescreen" in p
    assert {"label_masks", "label_ranges", "label_sets"} <= set(QueryTicket.__slots__)

    # ragged rows are padded to the longest by repeating the row's FIRST triple
    lm = _label_masks([[(1, 1, 0)], [(6, 2, 0), (0, 0, 8)], ((3, 3, 4), [9, 8, 7])], 3)
    assert lm.dtype == torch.int32 and lm.is_contiguous() and tuple(lm.shape) == (3, 2, 3)
    assert lm.tolist() == [[[1, 1, 0], [1, 1, 0]], [[6, 2, 0], [0, 0, 8]], [[3, 3, 4], [9, 8, 7]]]
    assert _label_masks([[(4, 4, 0)]], 1).tolist() == [[[4, 4, 0]]]
    assert _label_masks([[np.array([5, 4, 0])], [torch.tensor([7, 0, 8]), (1, 1, 2)]], 2).tolist() == [
        [[5, 4, 0], [5, 4, 0]], [[7, 0, 8], [1, 1, 2]]]
    # 3-D arrays and tensors are taken as they are; int64 is converted; [Nq, 3] is one clause each
    a = np.array([[[1, 1, 0], [3, -1, 5]], [[MIN, MAX, 0], [0, 0, 0]]], np.int32)
    assert _label_masks(a, 2).tolist() == a.tolist()
    t = _label_masks(torch.from_numpy(a.astype(np.int64)), 2)
    assert t.dtype == torch.int32 and t.tolist() == a.tolist()
    f = np.asfortranarray(np.arange(12, dtype=np.int32).reshape(2, 2, 3))
    assert _label_masks(f, 2).is_contiguous() and _label_masks(f, 2).tolist() == f.tolist()
    two = np.array([[1, 1, 0], [6, 4, 8]], np.int32)
    for form in (two, two.astype(np.int64), torch.from_numpy(two)):
        got = _label_masks(form, 2)
        assert tuple(got.shape) == (2, 1, 3) and got.dtype == torch.int32
        assert got.tolist() == [[[1, 1, 0]], [[6, 4, 8]]]
    # values in [-2**31, 2**32) wrap to int32: 0x80000000 is bit 31, 0xffffffff is -1
    for form in ([[(0x80000000, 0x80000000, 0xffffffff)], [(MIN, -1, 2 ** 32 - 1)]],
                 np.array([[[0x80000000, 0x80000000, 0xffffffff]], [[MIN, -1, 2 ** 32 - 1]]], np.int64),
                 torch.tensor([[0x80000000, 0x80000000, 0xffffffff], [MIN, -1, 2 ** 32 - 1]])):
        w = _label_masks(form, 2)
        assert w.dtype == torch.int32 and w.tolist() == [[[MIN, MIN, -1]], [[MIN, -1, -1]]]
    # ... and one past either end is refused, in lists and in int64 arrays
    for v in (2 ** 32, -2 ** 31 - 1):
        with pytest.raises(ValueError):
            _label_masks([[(v, 0, 0)]], 1)
        with pytest.raises(ValueError):
            _label_masks(np.array([[[0, v, 0]]], np.int64), 1)
        with pytest.raises(ValueError):
            _label_masks(np.array([[0, 0, v]], np.int64), 1)
    # no clause, three of them, a 3-D array of 0 or 3 clauses, a wrong number of rows, no triple
    for bad in ([[(1, 1, 0)], []], [[(1, 1, 0)], [(i, i, 0) for i in range(3)]],
                np.zeros((2, 3, 3), np.int32), np.zeros((2, 0, 3), np.int32),
                np.zeros((3, 2, 3), np.int32), [[(1, 1, 0)]], [[(1, 1, 0)], [(1, 2)]],
                np.zeros((3, 3), np.int32)):
        with pytest.raises(ValueError):
            _label_masks(bad, 2)
    with pytest.raises(TypeError):
        _label_masks(np.zeros((2, 2), np.int32), 2)        # 2-D but not triples
    with pytest.raises(TypeError):
        _label_masks(np.zeros((2, 2, 2), np.int32), 2)     # pairs: that is `label_ranges`
    with pytest.raises(TypeError):
        _label_masks(np.zeros((2, 2, 3), np.float32), 2)
    with pytest.raises(TypeError):
        _label_masks(np.zeros((2, 1, 3), np.uint32), 2)


def test_label_mask():
    import ggnn_amd
    from ggnn_amd import label_mask
    assert "label_mask" in ggnn_amd.__all__
    assert label_mask() == (0, 0, 0)                                      # every row
    assert label_mask(all_of=0b0101) == (0b0101, 0b0101, 0)
    assert label_mask(none_of=0b1000) == (0b1000, 0, 0)
    assert label_mask(any_of=0b0110) == (0, 0, 0b0110)
    assert label_mask(all_of=1, none_of=6, any_of=0x18) == (7, 1, 0x18)   # all of A, none of B, any of C
    assert label_mask(field_mask=0xff00, field_value=0x2a00) == (0xff00, 0x2a00, 0)
    assert label_mask(field_mask=0xff00) == (0xff00, 0, 0)                # the field equals 0
    assert label_mask(all_of=1, none_of=2, any_of=0xc, field_mask=0xff00, field_value=0x0100) == (
        0xff03, 0x0101, 0xc)
    assert label_mask(any_of=3, none_of=1) == (1, 0, 3)                   # any may overlap: no error
    # bit 31 is a bit like any other, written as it reads or as an int32
    assert label_mask(all_of=0x80000000) == (B31, B31, 0)
    assert label_mask(all_of=B31) == (B31, B31, 0)
    assert label_mask(none_of=0x80000000, any_of=0xffffffff) == (B31, 0, -1)
    assert label_mask(field_mask=0xf0000000, field_value=0x90000000) == (-0x10000000, -0x70000000, 0)
    assert label_mask(all_of=0x7fffffff, none_of=0x80000000) == (-1, MAX, 0)
    assert all(isinstance(v, int) and MIN <= v <= MAX for v in label_mask(0xffffffff, 0, 0xffffffff))
    # the three ways to build a clause that means something else
    with pytest.raises(ValueError, match="all_of"):
        label_mask(all_of=0b0110, none_of=0b0100)
    with pytest.raises(ValueError, match="field_value"):
        label_mask(field_mask=0xff00, field_value=0x2a01)
    with pytest.raises(ValueError, match="field_mask"):
        label_mask(all_of=0x0100, field_mask=0xff00, field_value=0x0200)
    with pytest.raises(ValueError, match="field_mask"):
        label_mask(none_of=0x8000, field_mask=0xff00)
    with pytest.raises(ValueError):
        label_mask(all_of=0x80000000, none_of=B31)                        # the same bit, two spellings
    for bad in (2 ** 32, -2 ** 31 - 1):
        with pytest.raises(ValueError):
            label_mask(any_of=bad)
    # the triple means what it says, under the definition of the predicate
    lab = np.random.default_rng(1).integers(0, 2 ** 32, 4096).astype(np.int64)
    m, v, a = (x & 0xffffffff for x in label_mask(all_of=0x80000001, none_of=6, any_of=0x18,
                                                  field_mask=0xf00, field_value=0x300))
    got = ((lab & m) == v) & ((lab & a) != 0)
    want = ((lab & 0x80000001) == 0x80000001) & ((lab & 6) == 0) & ((lab & 0x18) != 0) & \
        (((lab >> 8) & 0xf) == 3)
    assert np.array_equal(got, want) and 0 < want.sum() < len(lab)


def _labelmask(kernels):
    found = {n: k for n, k in kernels.items() if n.startswith("query_labelmask_")}
    assert found, "the library holds no query_labelmask_* kernels"
    return found


def _twin(name):
    return name.replace("labelmask", "labelrange")


def test_kernels_of_the_family(kernels):  # noqa: F811
    """query_labelmask_kernel* and bf_query_labelmask_* exist for float, unsigned char and both
    16-bit types on the layouts the range family has -- the same template arguments, name for name --
    and none for signed char or PrescreenExact"""
    names = list(_labelmask(kernels))
    assert any(n.startswith("query_labelmask_kernel_lds<") for n in names)
    for want in ("float", "unsigned char", "f16_t", "bf16_t"):
        assert any(re.match(r"query_labelmask_kernel<" + want + ",", n) for n in names), want
        assert any(re.match(r"query_labelmask_kernel_lds<" + want + ",", n) for n in names), want
    bf = [n for n in kernels if n.startswith("bf_query_labelmask_")]
    assert any(n.startswith("bf_query_labelmask_kernel<") for n in bf)
    assert any(n.startswith("bf_query_labelmask_lds_kernel<") for n in bf)
    for want in ("float", "unsigned char", "f16_t", "bf16_t"):
        assert any(re.match(r"bf_query_labelmask_kernel<" + want + ",", n) for n in bf), want
        assert any(re.match(r"bf_query_labelmask_lds_kernel<" + want + ",", n) for n in bf), want
    for n in names + bf:
        assert "signed char" not in n.replace("unsigned char", ""), n
        assert "PrescreenExact" not in n, n
    # the layouts the range family has: every range kernel has its mask twin and the other way round
    ranges = {n for n in kernels if n.startswith(("query_labelrange_", "bf_query_labelrange_"))}
    assert ranges and {_twin(n) for n in names + bf} == ranges
    # the names the other label tests select their kernels by stay theirs
    for n in kernels:
        if "labelmask" in n:
            assert "labelset" not in n and "labelrange" not in n, n


def test_early_rows_l2_kernels_have_no_scratch(kernels):  # noqa: F811
    """the early-rows squared-L2 kernels of float32 / uint8 rows (R = 1, HB 1 and 2): no private
    segment at the occupancy the family is built for"""
    pat = re.compile(r"query_labelmask_kernel<(float|unsigned char), \d+, \d+, 1, 0, .*, [12], true>$")
    hit = {n: k for n, k in _labelmask(kernels).items() if pat.match(n)}
    layouts = {re.match(r"query_labelmask_kernel<([^,]+, \d+, \d+)", n).group(1) for n in hit}
    print(sorted((n, k["vgpr_count"]) for n, k in hit.items()))
    assert {"float, 8, 1", "float, 8, 2", "float, 8, 3", "float, 16, 2", "unsigned char, 8, 1"} <= layouts
    assert any("NoPrescreen" in n for n in hit) and any("Prescreen<8, 1, 0>" in n for n in hit)
    for n, k in hit.items():
        assert k["private_segment_fixed_size"] == 0, (n, k)
        assert k["vgpr_spill_count"] == 0, (n, k)
        assert k["vgpr_count"] <= 80, (n, k)


@pytest.mark.parametrize("pattern", FILTERED_KERNELS)
def test_headline_kernels_against_their_range_siblings(kernels, pattern):  # noqa: F811
    """the headline and shard kernels under label masks: private segment 0, and no more VGPRs than
    query_labelrange_kernel of the same template arguments IN THE SAME LIBRARY (DESIGN.md 4.9 quotes
    the counts)"""
    name, sibling = pattern % "query_labelmask_kernel", pattern % "query_labelrange_kernel"
    assert name in kernels, f"{name} is not in the library (renamed template parameters?)"
    assert sibling in kernels, sibling
    k, s = kernels[name], kernels[sibling]
    print(name, k, "sibling:", s["vgpr_count"])
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= s["vgpr_count"], (k, s)
