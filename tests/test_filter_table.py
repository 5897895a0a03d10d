"""CPU tests of the per-query filters (include/ggnn_c.h, ggnn_set_filters / *_filtered_by): the
table packing, the new C-ABI symbols, the argument errors that need no device, and the semantic
model restated on the CPU -- query n with filter id f is the per-call filtered search of that
query with row f of the table, id -1 is the unfiltered search, any other id an empty result."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from filtered_reference import pack_bits, py_query_filtered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 3000])
def test_pack_filters_is_row_wise_pack_filter(N, F):
    import torch

    import ggnn_amd
    from ggnn_amd.api import _filter_table
    masks = np.random.default_rng(N * 10 + F).random((F, N)) < 0.4
    masks[0, N - 1] = True                      # the last real bit is set: the padding is what is left
    words = (N + 31) // 32
    for m in (masks, torch.from_numpy(masks)):
        got = ggnn_amd.pack_filters(m)
        assert got.dtype == torch.int32 and not got.is_cuda and tuple(got.shape) == (F, words)
        for f in range(F):
            row = ggnn_amd.pack_filter(masks[f]).numpy()
            assert np.array_equal(got[f].numpy(), row), (N, f)
            assert np.array_equal(got[f].numpy().view(np.uint32), pack_bits(masks[f])), (N, f)
    # padding bits (at and above N) are zero
    w = got.numpy().view(np.uint32)
    if N % 32:
        assert not (w[:, -1] >> np.uint32(N % 32)).any()
    # boolean masks and packed words end up as the same table
    assert np.array_equal(_filter_table(masks, N).numpy(), got.numpy())
    assert np.array_equal(_filter_table(w, N).numpy(), got.numpy())
    assert np.array_equal(_filter_table(got, N).numpy(), got.numpy())


def test_pack_filters_argument_errors():
    import ggnn_amd
    from ggnn_amd.api import _filter_ids, _filter_table
    with pytest.raises(TypeError):
        ggnn_amd.pack_filters(np.ones(10, bool))                 # 1-D: that is pack_filter
    with pytest.raises(TypeError):
        ggnn_amd.pack_filters(np.ones((2, 10), np.int32))
    with pytest.raises(ValueError):
        _filter_table(np.ones((2, 10), bool), 11)
    with pytest.raises(ValueError):
        _filter_table(np.zeros((2, 2), np.uint32), 100)
    with pytest.raises(TypeError):
        _filter_table(np.zeros((2, 4), np.float32), 100)
    import torch
    ids = _filter_ids(np.array([0, -1, 3], np.int64), 3)         # int64 is accepted and converted
    assert ids.dtype == torch.int32 and ids.tolist() == [0, -1, 3]
    with pytest.raises(ValueError):
        _filter_ids(np.zeros(4, np.int32), 3)
    with pytest.raises(TypeError):
        _filter_ids(np.zeros((3, 1), np.int32), 3)
    with pytest.raises(TypeError):
        _filter_ids(np.zeros(3, np.float32), 3)


NEW_SYMBOLS = {
    # name -> number of parameters of the prototype in include/ggnn_c.h
    "ggnn_set_filters": 6,
    "ggnn_update_filter": 6,
    "ggnn_get_num_filters": 2,
    "ggnn_query_filtered_by": 17,        # ggnn_query (14) + filter_ids, location, gpu
    "ggnn_bf_query_filtered_by": 15,     # ggnn_bf_query (12) + 3
    "ggnn_query_async_filtered_by": 14,  # ggnn_query_async (13) + filter_ids
    "ggnn_op_query_filtered_by": 30,     # ggnn_op_query_filtered (27) - bits + table, F, n_bits, ids
    "ggnn_op_bf_query_filtered_by": 16,
    "ggnn_op_pack_filters": 5,
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
                assert t in (C.c_void_p, C.POINTER(C.c_uint32)), (name, p)
            elif p.startswith("uint64_t"):
                assert t is C.c_uint64, (name, p)
            elif p.startswith("uint32_t"):
                assert t is C.c_uint32, (name, p)
            elif p.startswith("float"):
                assert t is C.c_float, (name, p)
            else:                                  # enums and int
                assert t is C.c_int, (name, p)
    # the handle calls are the unfiltered prototypes plus the id array (and where it lives)
    for plain, by, extra in (("ggnn_query", "ggnn_query_filtered_by", [C.c_void_p, C.c_int, C.c_int]),
                             ("ggnn_bf_query", "ggnn_bf_query_filtered_by",
                              [C.c_void_p, C.c_int, C.c_int]),
                             ("ggnn_query_async", "ggnn_query_async_filtered_by", [C.c_void_p])):
        a, b = _lib.SIGNATURES[plain][1], _lib.SIGNATURES[by][1]
        assert b[:len(a)] == a and b[len(a):] == extra, by
    # existing entry points keep their signatures
    assert len(_lib.SIGNATURES["ggnn_query_filtered"][1]) == 18
    assert len(_lib.SIGNATURES["ggnn_op_query_filtered"][1]) == 27


def test_argument_errors_without_a_device():
    from ggnn_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.ggnn_create(C.byref(h)) == _lib.OK
    try:
        N, D, F = 100, 8, 3
        words = (N + 31) // 32
        base = np.zeros((N, D), np.float32)
        q = np.zeros((2, D), np.float32)
        ids = np.zeros((2, 5), np.int32)
        dists = np.zeros((2, 5), np.float32)
        table = np.full((F, words), 0xffffffff, np.uint32)
        fids = np.array([0, -1], np.int32)
        nf = C.c_uint32(77)

        def set_filters(ptr, f, n_bits):
            return lib.ggnn_set_filters(h, ptr, f, n_bits, _lib.CPU, 0)

        def query_by(ptr):
            return lib.ggnn_query_filtered_by(h, q.ctypes.data, 2, D, _lib.F32, _lib.CPU, 0, 5, 0.5,
                                              100, 0, ids.ctypes.data, dists.ctypes.data, _lib.CPU,
                                              ptr, _lib.CPU, 0)

        def bf_by(ptr):
            return lib.ggnn_bf_query_filtered_by(h, q.ctypes.data, 2, D, _lib.F32, _lib.CPU, 0, 5, 0,
                                                 ids.ctypes.data, dists.ctypes.data, _lib.CPU, ptr,
                                                 _lib.CPU, 0)

        def async_by(ptr):
            return lib.ggnn_query_async_filtered_by(h, q.ctypes.data, 2, D, _lib.F32, -1, 5, 0.5,
                                                    100, 0, ids.ctypes.data, dists.ctypes.data, 0,
                                                    ptr)

        # a table needs the base it is over
        assert set_filters(table.ctypes.data, F, N) == _lib.INVALID_STATE
        assert lib.ggnn_get_num_filters(h, C.byref(nf)) == _lib.OK and nf.value == 0
        assert lib.ggnn_set_base(h, base.ctypes.data, N, D, _lib.F32, _lib.CPU, 0, 1) == _lib.OK
        # no table yet: the *_filtered_by calls and update_filter have nothing to refer to
        for call in (query_by, bf_by, async_by):
            assert call(fids.ctypes.data) == _lib.INVALID_STATE, call.__name__
            assert b"filter table" in lib.ggnn_last_error(h)
        assert lib.ggnn_update_filter(h, 0, table.ctypes.data, N, _lib.CPU, 0) == _lib.INVALID_STATE
        # wrong n_bits, null table with F > 0
        assert set_filters(table.ctypes.data, F, N - 1) == _lib.INVALID_ARGUMENT
        assert set_filters(table.ctypes.data, F, N + 1) == _lib.INVALID_ARGUMENT
        assert b"n_bits" in lib.ggnn_last_error(h)
        assert set_filters(None, F, N) == _lib.INVALID_ARGUMENT
        assert b"null" in lib.ggnn_last_error(h)
        assert lib.ggnn_get_num_filters(h, C.byref(nf)) == _lib.OK and nf.value == 0
        # a well-formed table is kept on the host until there is a GPU to place it on
        assert set_filters(table.ctypes.data, F, N) == _lib.OK
        assert lib.ggnn_get_num_filters(h, C.byref(nf)) == _lib.OK and nf.value == F
        # update_filter: index, n_bits, null
        assert lib.ggnn_update_filter(h, F, table.ctypes.data, N, _lib.CPU, 0) == _lib.OUT_OF_RANGE
        assert lib.ggnn_update_filter(h, F + 7, table.ctypes.data, N, _lib.CPU, 0) == _lib.OUT_OF_RANGE
        assert lib.ggnn_update_filter(h, 0, table.ctypes.data, N + 1, _lib.CPU, 0) == _lib.INVALID_ARGUMENT
        assert lib.ggnn_update_filter(h, 0, None, N, _lib.CPU, 0) == _lib.INVALID_ARGUMENT
        assert lib.ggnn_update_filter(h, F - 1, table.ctypes.data, N, _lib.CPU, 0) == _lib.OK
        # host-side ids are validated on the host: anything outside [-1, F)
        for bad in (F, -2, 2 ** 31 - 1, -2 ** 31):
            assert query_by(np.array([0, bad], np.int32).ctypes.data) == _lib.INVALID_ARGUMENT, bad
            assert b"filter id" in lib.ggnn_last_error(h)
            assert bf_by(np.array([bad, -1], np.int32).ctypes.data) == _lib.INVALID_ARGUMENT, bad
        assert query_by(None) == _lib.INVALID_ARGUMENT
        # well-formed ids, no graph: the state error of ggnn_query
        assert query_by(fids.ctypes.data) == _lib.INVALID_STATE
        assert async_by(fids.ctypes.data) == _lib.INVALID_STATE
        # num_filters == 0 drops the table, and so does ggnn_set_base
        assert set_filters(None, 0, 0) == _lib.OK
        assert lib.ggnn_get_num_filters(h, C.byref(nf)) == _lib.OK and nf.value == 0
        assert set_filters(table.ctypes.data, F, N) == _lib.OK
        assert lib.ggnn_set_base(h, base.ctypes.data, N, D, _lib.F32, _lib.CPU, 0, 1) == _lib.OK
        assert lib.ggnn_get_num_filters(h, C.byref(nf)) == _lib.OK and nf.value == 0
        assert lib.ggnn_set_filters(None, table.ctypes.data, F, N, _lib.CPU, 0) == _lib.INVALID_ARGUMENT
    finally:
        lib.ggnn_destroy(h)
    # the operator seam refuses a null table / null ids before it touches anything
    assert lib.ggnn_op_query_filtered_by(None, 0, 0, 0, None, None, None, 0, None, 0, None, 0, None,
                                         1, 0.5, 1, 0, 1, 0, None, None, None, None, None, None, 0,
                                         0, None, 0, None) == _lib.INVALID_ARGUMENT
    assert lib.ggnn_op_bf_query_filtered_by(None, 0, 0, 0, None, 0, 1, 0, None, None, None, 0, 0,
                                            None, 0, None) == _lib.INVALID_ARGUMENT


def test_python_surface():
    import inspect

    import ggnn_amd
    # the per-call methods keep their signatures (tests/test_filtered_reference.py pins them); the
    # filter ids are the keyword of methods of their own and a trailing keyword of query_async
    for name, want in (("query_filtered", ["query", "k_query", "tau_query", "max_iterations",
                                           "measure", "filter"]),
                       ("bf_query_filtered", ["query", "k_gt", "measure", "filter"]),
                       ("query_filtered_by", ["query", "k_query", "tau_query", "max_iterations",
                                              "measure", "filter_ids", "filter"]),
                       ("bf_query_filtered_by", ["query", "k_gt", "measure", "filter_ids", "filter"]),
                       ("query_async", ["query", "k_query", "tau_query", "max_iterations",
                                        "measure", "slot", "filter_ids"])):
        sig = inspect.signature(getattr(ggnn_amd.GGNN, name))
        assert list(sig.parameters)[1:] == want, name
        for kw in ("filter_ids", "filter"):
            assert kw not in sig.parameters or sig.parameters[kw].default is None, (name, kw)
    for name in ("set_filters", "update_filter", "num_filters"):
        assert hasattr(ggnn_amd.GGNN, name), name
    assert "pack_filters" in ggnn_amd.__all__ and "pack_filter" in ggnn_amd.__all__
    from ggnn_amd import ops
    for name in ("query_filtered_by", "bf_query_filtered_by", "pack_filters"):
        assert callable(getattr(ops, name)), name
    assert "filter_ids" in ggnn_amd.api.QueryTicket.__slots__

    eng = ggnn_amd.GGNN()
    eng.set_base(np.zeros((64, 8), np.float32))
    assert eng.num_filters == 0
    q = np.zeros((3, 8), np.float32)
    both = dict(filter=np.ones(64, bool), filter_ids=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="filter_ids"):
        eng.query_filtered_by(q, 5, 0.5, **both)
    with pytest.raises(ValueError, match="filter_ids"):
        eng.bf_query_filtered_by(q, 5, **both)
    eng.set_filters(np.ones((2, 64), bool))
    assert eng.num_filters == 2
    eng.update_filter(1, np.zeros(64, bool))
    with pytest.raises(IndexError):
        eng.update_filter(2, np.zeros(64, bool))
    from ggnn_amd import _lib
    with pytest.raises(_lib.GGNNError) as e:
        eng.query_filtered_by(q, 5, 0.5, filter_ids=np.array([0, 1, 2], np.int32))   # id 2 of 2 rows
    assert e.value.status == _lib.INVALID_ARGUMENT
    eng.set_filters(None)
    assert eng.num_filters == 0


# ---- the semantic model, restated on the CPU -----------------------------------------------------
@pytest.fixture(scope="module")
def toy(orc):
    """the 3000 x 16 base of test_filtered_reference.py, its graph, and a table of four filters"""
    N, D, KB = 3000, 16, 24
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (N, D)).astype(np.float32)
    cfg, graph, tr, sel, stats = orc.build(base, KB, 0.5, 1, rng=orc.make_rng(N, 5))
    start = tr[cfg.STs_offsets[3]:cfg.STs_offsets[3] + cfg.Ns[3]]
    q = rng.integers(0, 256, (10, D)).astype(np.float32)
    table = np.stack([np.random.default_rng(40 + f).random(N) < share
                      for f, share in enumerate((1.0, 0.5, 0.1, 0.01))])
    return dict(N=N, base=base, graph=graph[:N], start=start, stats=stats, q=q, table=table)


def model_query_filtered_by(t, table, filter_ids, K, tau, iters):
    """the whole contract: row table[f] for f in [0, F), all ones for -1, all zeros otherwise"""
    F, N = table.shape
    out = []
    for n, f in enumerate(filter_ids):
        allowed = table[f] if 0 <= f < F else np.full(N, f == -1)
        out.append(py_query_filtered(t["base"], t["q"][n], t["graph"], t["start"], t["stats"], K,
                                     tau, iters, allowed))
    return out


def test_semantic_model_on_the_cpu(orc, toy):
    t = toy
    K, tau, iters = 10, 0.6, 200
    F = len(t["table"])
    filter_ids = np.array([0, 1, 2, 3, -1, F, -1, 1, -7, 2 ** 31 - 1], np.int64)
    res = model_query_filtered_by(t, t["table"], filter_ids, K, tau, iters)
    o_ids, o_d, o_nd, o_pop = orc.query(t["base"], t["q"], t["graph"], t["start"], t["stats"], K,
                                        tau, iters, counters=True)
    for n, f in enumerate(filter_ids):
        ids, dists, n_dist, n_pop = res[n]
        if 0 <= f < F:
            # the per-call filtered search of that query with row f (same function: the identity
            # the kernels are held to), and never a denied id
            want = py_query_filtered(t["base"], t["q"][n], t["graph"], t["start"], t["stats"], K,
                                     tau, iters, t["table"][f])
            assert np.array_equal(ids, want[0]) and dists.tobytes() == want[1].tobytes(), n
            assert (n_dist, n_pop) == (want[2], want[3]), n
            fin = np.isfinite(dists)
            assert t["table"][f][ids[fin]].all(), n
        elif f == -1:
            # unfiltered: bit for bit the oracle's query, counters included
            assert np.array_equal(ids, o_ids[n]), n
            assert dists.tobytes() == o_d[n].tobytes(), n
            assert (n_dist, n_pop) == (int(o_nd[n]), int(o_pop[n])), n
        else:
            # an id that names no row: an empty result, every slot (-1, +inf)
            assert (ids == -1).all() and np.isinf(dists).all() and (dists > 0).all(), n
            assert n_pop <= iters
    # row 0 is all ones: the same as -1
    assert np.array_equal(res[0][0], o_ids[0]) and res[0][1].tobytes() == o_d[0].tobytes()
