"""CPU tests of the label filters (include/ggnn_c.h, ggnn_set_labels / *_labeled): the new C-ABI
symbols, the status codes that need no device, the Python argument checks, and the parametric
predicate of the filter read restated in numpy -- one formula, three parameter sets (bitset,
label L, label -1) -- against plain masks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from filtered_reference import pack_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {
    # name -> number of parameters of the prototype in include/ggnn_c.h
    "ggnn_set_labels": 5,
    "ggnn_update_labels": 6,
    "ggnn_get_num_labels": 2,
    "ggnn_query_labeled": 17,        # ggnn_query (14) + query_labels, location, gpu
    "ggnn_bf_query_labeled": 15,     # ggnn_bf_query (12) + 3
    "ggnn_query_async_labeled": 14,  # ggnn_query_async (13) + query_labels
    "ggnn_op_query_labeled": 29,     # ggnn_op_query_filtered_by (30) - table, F, n_bits + labels, n
    "ggnn_op_bf_query_labeled": 15,
}


def test_new_symbols_match_the_header():
    from ggnn_amd import _lib
    lib = _lib.lib()
    src = open(os.path.join(ROOT, "include", "ggnn_c.h")).read()
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
                assert t in (C.c_void_p, C.POINTER(C.c_uint64)), (name, p)
            elif p.startswith("uint64_t"):
                assert t is C.c_uint64, (name, p)
            elif p.startswith("uint32_t"):
                assert t is C.c_uint32, (name, p)
            elif p.startswith("float"):
                assert t is C.c_float, (name, p)
            else:                                  # enums and int
                assert t is C.c_int, (name, p)
    # the handle calls are the *_filtered_by prototypes: query labels in place of filter ids
    for by, labeled in (("ggnn_query_filtered_by", "ggnn_query_labeled"),
                        ("ggnn_bf_query_filtered_by", "ggnn_bf_query_labeled"),
                        ("ggnn_query_async_filtered_by", "ggnn_query_async_labeled")):
        assert _lib.SIGNATURES[by] == _lib.SIGNATURES[labeled], labeled
    # existing entry points keep their signatures
    assert len(_lib.SIGNATURES["ggnn_query_filtered_by"][1]) == 17
    assert len(_lib.SIGNATURES["ggnn_op_query_filtered_by"][1]) == 30
    assert len(_lib.SIGNATURES["ggnn_op_bf_query_filtered_by"][1]) == 16


def test_status_codes_without_a_device():
    from ggnn_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.ggnn_create(C.byref(h)) == _lib.OK
    try:
        N, D = 100, 8
        base = np.zeros((N, D), np.float32)
        q = np.zeros((2, D), np.float32)
        ids = np.zeros((2, 5), np.int32)
        dists = np.zeros((2, 5), np.float32)
        labels = (np.arange(N) % 7).astype(np.int32)
        qlab = np.array([3, -1], np.int32)
        n = C.c_uint64(77)

        def set_labels(ptr, count):
            return lib.ggnn_set_labels(h, ptr, count, _lib.CPU, 0)

        def update(id_list, values):
            i = np.asarray(id_list, np.int64)
            v = np.asarray(values, np.int32)
            return lib.ggnn_update_labels(h, i.ctypes.data, v.ctypes.data, len(i), _lib.CPU, 0)

        def query_l(ptr):
            return lib.ggnn_query_labeled(h, q.ctypes.data, 2, D, _lib.F32, _lib.CPU, 0, 5, 0.5, 100,
                                          0, ids.ctypes.data, dists.ctypes.data, _lib.CPU, ptr,
                                          _lib.CPU, 0)

        def bf_l(ptr):
            return lib.ggnn_bf_query_labeled(h, q.ctypes.data, 2, D, _lib.F32, _lib.CPU, 0, 5, 0,
                                             ids.ctypes.data, dists.ctypes.data, _lib.CPU, ptr,
                                             _lib.CPU, 0)

        def async_l(ptr):
            return lib.ggnn_query_async_labeled(h, q.ctypes.data, 2, D, _lib.F32, -1, 5, 0.5, 100, 0,
                                                ids.ctypes.data, dists.ctypes.data, 0, ptr)

        # labels need the base they are over
        assert set_labels(labels.ctypes.data, N) == _lib.INVALID_STATE
        assert lib.ggnn_get_num_labels(h, C.byref(n)) == _lib.OK and n.value == 0
        assert lib.ggnn_set_base(h, base.ctypes.data, N, D, _lib.F32, _lib.CPU, 0, 1) == _lib.OK
        # no labels yet: the *_labeled calls and update_labels have nothing to refer to
        for call in (query_l, bf_l, async_l):
            assert call(qlab.ctypes.data) == _lib.INVALID_STATE, call.__name__
            assert b"labels" in lib.ggnn_last_error(h)
        assert update([0], [1]) == _lib.INVALID_STATE
        # wrong n
        assert set_labels(labels.ctypes.data, N - 1) == _lib.INVALID_ARGUMENT
        assert set_labels(labels.ctypes.data, N + 1) == _lib.INVALID_ARGUMENT
        assert b"must equal N" in lib.ggnn_last_error(h)
        assert lib.ggnn_get_num_labels(h, C.byref(n)) == _lib.OK and n.value == 0
        # a well-formed column is kept on the host until there is a GPU to place it on
        assert set_labels(labels.ctypes.data, N) == _lib.OK
        assert lib.ggnn_get_num_labels(h, C.byref(n)) == _lib.OK and n.value == N
        # update_labels validates every id before it changes anything
        # (what a refused update left unchanged is read back on the GPU: tests/test_gpu_labels.py)
        assert update([0, N], [50, 51]) == _lib.OUT_OF_RANGE
        assert update([1, -1], [50, 51]) == _lib.OUT_OF_RANGE
        assert update([2, 2 ** 40], [50, 51]) == _lib.OUT_OF_RANGE
        assert b"outside [0, 100)" in lib.ggnn_last_error(h)
        assert lib.ggnn_update_labels(h, None, None, 3, _lib.CPU, 0) == _lib.INVALID_ARGUMENT
        assert update([], []) == _lib.OK
        assert update([5, 6, 5], [9, 9, -7]) == _lib.OK
        assert lib.ggnn_get_num_labels(h, C.byref(n)) == _lib.OK and n.value == N
        # no label value is invalid; a null array is
        assert query_l(None) == _lib.INVALID_ARGUMENT
        # well-formed query labels of any value, no graph: the state error of ggnn_query
        for wild in (qlab, np.array([-2 ** 31, 2 ** 31 - 1], np.int32)):
            assert query_l(wild.ctypes.data) == _lib.INVALID_STATE
            assert b"graph" in lib.ggnn_last_error(h)
            assert async_l(wild.ctypes.data) == _lib.INVALID_STATE
        # a null pointer drops the labels, and so does ggnn_set_base
        assert set_labels(None, 0) == _lib.OK
        assert lib.ggnn_get_num_labels(h, C.byref(n)) == _lib.OK and n.value == 0
        assert update([0], [1]) == _lib.INVALID_STATE
        assert set_labels(labels.ctypes.data, N) == _lib.OK
        assert lib.ggnn_set_base(h, base.ctypes.data, N, D, _lib.F32, _lib.CPU, 0, 1) == _lib.OK
        assert lib.ggnn_get_num_labels(h, C.byref(n)) == _lib.OK and n.value == 0
        assert lib.ggnn_set_labels(None, labels.ctypes.data, N, _lib.CPU, 0) == _lib.INVALID_ARGUMENT
        assert lib.ggnn_get_num_labels(h, None) == _lib.INVALID_ARGUMENT
    finally:
        lib.ggnn_destroy(h)
    # the operator seam refuses a null label column / null query labels before it touches anything
    assert lib.ggnn_op_query_labeled(None, 0, 0, 0, None, None, None, 0, None, 0, None, 0, None, 1,
                                     0.5, 1, 0, 1, 0, None, None, None, None, None, None, 0, None,
                                     0, None) == _lib.INVALID_ARGUMENT
    assert lib.ggnn_op_bf_query_labeled(None, 0, 0, 0, None, 0, 1, 0, None, None, None, 0, None, 0,
                                        None) == _lib.INVALID_ARGUMENT


def test_python_surface_and_argument_checks():
    import inspect

    import torch

    import ggnn_amd
    from ggnn_amd import _lib, ops
    from ggnn_amd.api import _labels
    for name, want in (("query_labeled", ["query", "k_query", "tau_query", "max_iterations",
                                          "measure", "labels"]),
                       ("bf_query_labeled", ["query", "k_gt", "measure", "labels"]),
                       ("set_labels", ["labels"]), ("update_labels", ["ids", "labels"])):
        sig = inspect.signature(getattr(ggnn_amd.GGNN, name))
        assert list(sig.parameters)[1:] == want, name
    sig = inspect.signature(ggnn_amd.GGNN.query_labeled)
    assert sig.parameters["max_iterations"].default == 400 and sig.parameters["labels"].default is None
    assert inspect.signature(ggnn_amd.GGNN.bf_query_labeled).parameters["k_gt"].default == 100
    # query_async keeps its signature (tests/test_filter_table.py pins it): the labels are the
    # keyword of a method of its own, which takes no filter ids
    sig = inspect.signature(ggnn_amd.GGNN.query_async)
    assert list(sig.parameters)[-2:] == ["slot", "filter_ids"]
    sig = inspect.signature(ggnn_amd.GGNN.query_async_labeled)
    assert list(sig.parameters)[1:] == ["query", "k_query", "tau_query", "max_iterations",
                                        "measure", "slot", "labels"]
    assert sig.parameters["labels"].default is None and sig.parameters["slot"].default == 0
    # the reference-shaped methods keep their signatures
    assert list(inspect.signature(ggnn_amd.GGNN.query).parameters)[1:] == [
        "query", "k_query", "tau_query", "max_iterations", "measure"]
    assert list(inspect.signature(ggnn_amd.GGNN.bf_query).parameters)[1:] == [
        "query", "k_gt", "measure"]
    assert isinstance(ggnn_amd.GGNN.num_labels, property)
    for name in ("query_labeled", "bf_query_labeled"):
        assert callable(getattr(ops, name)), name

    # dtype and shape
    lab = _labels(np.array([0, -1, 3], np.int64), 3)             # int64 is accepted and converted
    assert lab.dtype == torch.int32 and lab.tolist() == [0, -1, 3]
    lab = _labels(torch.tensor([-2 ** 31, 2 ** 31 - 1], dtype=torch.int64), 2)
    assert lab.tolist() == [-2 ** 31, 2 ** 31 - 1]
    with pytest.raises(ValueError):
        _labels(np.zeros(4, np.int32), 3)
    with pytest.raises(TypeError):
        _labels(np.zeros((3, 1), np.int32), 3)
    with pytest.raises(TypeError):
        _labels(np.zeros(3, np.float32), 3)
    with pytest.raises(TypeError):
        _labels(np.zeros(3, np.int16), 3)
    with pytest.raises(TypeError):
        _labels([0, 1, 2], 3)
    # int64 values must fit int32
    for bad in (2 ** 31, -2 ** 31 - 1):
        with pytest.raises(ValueError, match="int32"):
            _labels(np.array([0, bad], np.int64), 2)

    eng = ggnn_amd.GGNN()
    N = 64
    eng.set_base(np.zeros((N, 8), np.float32))
    assert eng.num_labels == 0
    q = np.zeros((3, 8), np.float32)
    with pytest.raises(RuntimeError, match="labels"):          # no labels set
        eng.query_labeled(q, 5, 0.5, labels=np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        eng.set_labels(np.zeros(N + 1, np.int32))
    with pytest.raises(TypeError):
        eng.set_labels(np.zeros((N, 1), np.int32))
    with pytest.raises(TypeError):
        eng.set_labels(np.zeros(N, np.float32))
    with pytest.raises(ValueError, match="int32"):
        eng.set_labels(np.full(N, 2 ** 31, np.int64))
    assert eng.num_labels == 0
    eng.set_labels(np.arange(N, dtype=np.int64) % 5)
    assert eng.num_labels == N
    eng.set_labels(torch.arange(N, dtype=torch.int32) % 3)
    assert eng.num_labels == N
    eng.update_labels(np.array([1, 2, 1]), np.array([7, 8, 9]))
    eng.update_labels(torch.tensor([3], dtype=torch.int32), torch.tensor([4], dtype=torch.int32))
    with pytest.raises(IndexError):
        eng.update_labels(np.array([0, N]), np.array([1, 1]))
    with pytest.raises(IndexError):
        eng.update_labels(np.array([-1]), np.array([1]))
    with pytest.raises(ValueError):
        eng.update_labels(np.array([0, 1]), np.array([1]))
    with pytest.raises(ValueError, match="int32"):
        eng.update_labels(np.array([0]), np.array([2 ** 31], np.int64))
    with pytest.raises(TypeError):
        eng.update_labels(np.array([0.0]), np.array([1]))
    # one label per query
    with pytest.raises(ValueError):
        eng.query_labeled(q, 5, 0.5, labels=np.zeros(4, np.int32))
    with pytest.raises(TypeError):
        eng.bf_query_labeled(q, 5, labels=np.zeros(3, np.float32))
    # labels together with filter_ids: no asynchronous call takes both
    with pytest.raises(TypeError, match="labels"):
        eng.query_async(q, 5, 0.5, filter_ids=np.zeros(3, np.int32), labels=np.zeros(3, np.int32))
    with pytest.raises(TypeError, match="filter_ids"):
        eng.query_async_labeled(q, 5, 0.5, filter_ids=np.zeros(3, np.int32),
                                labels=np.zeros(3, np.int32))
    with pytest.raises(ValueError):                             # one label per query
        eng.query_async_labeled(q, 5, 0.5, labels=np.zeros(4, np.int32))
    # well-formed labels, no graph: the state error of query
    with pytest.raises(_lib.GGNNError) as e:
        eng.query_labeled(q, 5, 0.5, labels=np.array([0, -1, 2 ** 31 - 1], np.int64))
    assert e.value.status == _lib.INVALID_STATE
    eng.set_labels(None)
    assert eng.num_labels == 0
    with pytest.raises(RuntimeError, match="labels"):
        eng.update_labels(np.array([0]), np.array([1]))


# ---- the parametric predicate, restated --------------------------------------------------------
#   word   = words[(cand + offset) >> shift]
#   denied = ((word >> ((cand + offset) & smask)) & vmask) != want
def params_bitset():
    return dict(shift=5, smask=31, vmask=1, want=1)


def params_label(L):
    if L == -1:
        return dict(shift=0, smask=0, vmask=0, want=0)
    return dict(shift=0, smask=0, vmask=0xffffffff, want=int(np.uint32(np.int32(L))))


def denied(words, cand, offset, shift, smask, vmask, want):
    b = (np.asarray(cand, np.uint32) + np.uint32(offset)).astype(np.uint32)
    word = np.asarray(words).view(np.uint32)[b >> np.uint32(shift)]
    return ((word >> (b & np.uint32(smask))) & np.uint32(vmask)) != np.uint32(want)


@pytest.mark.parametrize("offset", [0, 1, 31, 33, 1000, 2999])
def test_parametric_predicate_against_plain_masks(offset):
    rs = np.random.default_rng(offset)
    N = 3000
    total = offset + N                                   # the shard's ids are the last N
    cand = rs.integers(0, N, 500)
    # bitset mode == the pack_bits lookup
    mask = rs.random(total) < 0.3
    words = pack_bits(mask)
    got = denied(words, cand, offset, **params_bitset())
    assert np.array_equal(got, ~mask[cand + offset])
    b = cand + offset
    assert np.array_equal(got, ((words[b >> 5] >> (b & 31).astype(np.uint32)) & 1) == 0)
    # label mode == (labels == L)
    labels = rs.choice(np.array([0, 1, 2, 9, -7, -2 ** 31, 2 ** 31 - 1], np.int64), total)
    labels = labels.astype(np.int32)
    for L in (0, 1, 2, 9, -7, -2 ** 31, 2 ** 31 - 1, 5, -2):
        got = denied(labels, cand, offset, **params_label(L))
        assert np.array_equal(got, labels[cand + offset] != L), L
        if L in (5, -2):                                 # a label no row carries: all denied
            assert got.all()
    # the -1 set denies nothing, whatever the labels are -- rows labelled -1 included
    labels[rs.integers(0, total, 50)] = -1
    assert not denied(labels, cand, offset, **params_label(-1)).any()
    # ... and every read is in bounds: the word index is the global id itself
    assert ((cand + offset) >> params_label(-1)["shift"]).max() < total
