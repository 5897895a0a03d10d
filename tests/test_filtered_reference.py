"""CPU tests of the filtered search: the Python reference of the filtered traversal
(tests/filtered_reference.py) is tied to the C++ oracle through the all-ones filter and checked
for the invariants every filtered result must have; the bit packing, the new C-ABI symbols and
the argument errors that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from filtered_reference import (bf_filtered_reference, check_filtered_invariants, l2_exact,
                                pack_bits, py_query_filtered)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _start_points(g):
    cfg = g["cfg"]
    return g["tr"][cfg.STs_offsets[3]:cfg.STs_offsets[3] + cfg.Ns[3]]


@pytest.mark.parametrize("K,tau,iters", [(10, 0.5, 400), (10, 0.9, 200), (40, 0.7, 64),
                                         (1, 0.3, 20), (100, 0.6, 300)])
def test_all_ones_filter_equals_oracle(orc, small_graph, K, tau, iters):
    g = small_graph
    base, N = g["base"], g["N"]
    q = np.random.default_rng(K * 1000 + iters).integers(0, 256, (12, g["D"])).astype(np.float32)
    start = _start_points(g)
    ids, dists, nd, npop = orc.query(base, q, g["graph"][:N], start, g["stats"], K, tau, iters,
                                     counters=True)
    ones = np.ones(N, bool)
    for i in range(q.shape[0]):
        p_ids, p_d, p_nd, p_pop = py_query_filtered(base, q[i], g["graph"][:N], start, g["stats"],
                                                    K, tau, iters, ones)
        assert np.array_equal(ids[i], p_ids), i
        assert dists[i].tobytes() == p_d.tobytes(), i
        assert (int(nd[i]), int(npop[i])) == (p_nd, p_pop), i


def test_all_ones_filter_equals_oracle_on_tied_data(orc):
    N, D, KB = 1500, 16, 24
    base = np.random.default_rng(1).integers(0, 3, (N, D)).astype(np.float32)
    cfg, graph, tr, sel, stats = orc.build(base, KB, 0.5, 1, rng=orc.make_rng(N, 5))
    start = tr[cfg.STs_offsets[3]:cfg.STs_offsets[3] + cfg.Ns[3]]
    q = np.random.default_rng(2).integers(0, 3, (10, D)).astype(np.float32)
    ones = np.ones(N, bool)
    for K, tau, iters in ((10, 0.9, 200), (20, 1.5, 100)):
        ids, dists, nd, npop = orc.query(base, q, graph[:N], start, stats, K, tau, iters,
                                         counters=True)
        for i in range(q.shape[0]):
            p = py_query_filtered(base, q[i], graph[:N], start, stats, K, tau, iters, ones)
            assert np.array_equal(ids[i], p[0]) and dists[i].tobytes() == p[1].tobytes(), (K, i)
            assert (int(nd[i]), int(npop[i])) == (p[2], p[3]), (K, i)


@pytest.mark.parametrize("share", [0.5, 0.1, 0.01, 0.0])
def test_random_filters_keep_the_invariants(orc, share):
    N, D, KB, K, tau, iters = 3000, 16, 24, 10, 0.6, 200
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (N, D)).astype(np.float32)
    cfg, graph, tr, sel, stats = orc.build(base, KB, 0.5, 1, rng=orc.make_rng(N, 5))
    start = tr[cfg.STs_offsets[3]:cfg.STs_offsets[3] + cfg.Ns[3]]
    q = rng.integers(0, 256, (8, D)).astype(np.float32)
    allowed = np.random.default_rng(int(share * 100) + 7).random(N) < share
    ids = np.empty((len(q), K), np.int32)
    dists = np.empty((len(q), K), np.float32)
    for i in range(len(q)):
        ids[i], dists[i], n_dist, n_pop = py_query_filtered(base, q[i], graph[:N], start, stats, K,
                                                            tau, iters, allowed)
        assert n_pop <= iters and n_dist > 0
    check_filtered_invariants(orc, base, q, ids, dists, allowed, l2_exact(base), K)
    if share == 0.0:
        assert np.isinf(dists).all() and (ids == -1).all()
    if share == 0.5:
        assert np.isfinite(dists).all()


def test_pack_filter_round_trip():
    import torch

    import ggnn_amd
    from ggnn_amd.api import _filter_words
    for N in (1, 31, 32, 33, 77, 1000, 2048):
        mask = np.random.default_rng(N).random(N) < 0.4
        want = pack_bits(mask)
        assert want.size == (N + 31) // 32
        for m in (mask, torch.from_numpy(mask)):
            got = ggnn_amd.pack_filter(m)
            assert got.dtype == torch.int32 and not got.is_cuda
            assert np.array_equal(got.numpy().view(np.uint32), want), N
        w = got.numpy().view(np.uint32)
        back = np.array([(int(w[i >> 5]) >> (i & 31)) & 1 for i in range(N)], bool)
        assert np.array_equal(back, mask)
        # boolean and packed inputs end up as the same words
        assert np.array_equal(_filter_words(mask, N).numpy().view(np.uint32), want)
        assert np.array_equal(_filter_words(want, N).numpy().view(np.uint32), want)
        assert np.array_equal(_filter_words(got, N).numpy().view(np.uint32), want)
    with pytest.raises(ValueError):
        _filter_words(np.ones(10, bool), 11)
    with pytest.raises(ValueError):
        _filter_words(np.zeros(2, np.uint32), 100)
    with pytest.raises(TypeError):
        _filter_words(np.zeros(4, np.float32), 100)
    with pytest.raises(TypeError):
        ggnn_amd.pack_filter(np.zeros(4, np.int32))


NEW_SYMBOLS = {
    # name -> number of parameters of the prototype in include/ggnn_c.h
    "ggnn_query_filtered": 18,        # ggnn_query (14) + bits, n_bits, location, gpu
    "ggnn_bf_query_filtered": 16,     # ggnn_bf_query (12) + 4
    "ggnn_op_query_filtered": 27,
    "ggnn_op_bf_query_filtered": 13,  # ggnn_op_bf_query (11) + bits, offset
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
                assert t is C.c_void_p, (name, p)
            elif p.startswith("uint64_t"):
                assert t is C.c_uint64, (name, p)
            elif p.startswith("uint32_t"):
                assert t is C.c_uint32, (name, p)
            elif p.startswith("float"):
                assert t is C.c_float, (name, p)
            else:                                  # enums and int
                assert t is C.c_int, (name, p)
    # the filtered handle calls are the unfiltered prototypes plus the four filter arguments
    for plain, filt in (("ggnn_query", "ggnn_query_filtered"),
                        ("ggnn_bf_query", "ggnn_bf_query_filtered")):
        a, b = _lib.SIGNATURES[plain][1], _lib.SIGNATURES[filt][1]
        assert b[:len(a)] == a and b[len(a):] == [C.c_void_p, C.c_uint64, C.c_int, C.c_int]


def test_argument_errors_without_a_device():
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
        bits = np.full((N + 31) // 32, 0xffffffff, np.uint32)
        assert lib.ggnn_set_base(h, base.ctypes.data, N, D, _lib.F32, _lib.CPU, 0, 1) == _lib.OK

        def query(ptr, n_bits):
            return lib.ggnn_query_filtered(h, q.ctypes.data, 2, D, _lib.F32, _lib.CPU, 0, 5, 0.5,
                                           100, 0, ids.ctypes.data, dists.ctypes.data, _lib.CPU,
                                           ptr, n_bits, _lib.CPU, 0)

        def bf(ptr, n_bits):
            return lib.ggnn_bf_query_filtered(h, q.ctypes.data, 2, D, _lib.F32, _lib.CPU, 0, 5, 0,
                                              ids.ctypes.data, dists.ctypes.data, _lib.CPU, ptr,
                                              n_bits, _lib.CPU, 0)

        for call in (query, bf):
            assert call(None, N) == _lib.INVALID_ARGUMENT
            assert b"null" in lib.ggnn_last_error(h)
            assert call(bits.ctypes.data, N - 1) == _lib.INVALID_ARGUMENT
            assert call(bits.ctypes.data, N + 1) == _lib.INVALID_ARGUMENT
            assert b"n_bits" in lib.ggnn_last_error(h)
        # well-formed filter, no graph: the state error of ggnn_query
        assert query(bits.ctypes.data, N) == _lib.INVALID_STATE
        assert lib.ggnn_query_filtered(None, q.ctypes.data, 2, D, _lib.F32, _lib.CPU, 0, 5, 0.5,
                                       100, 0, ids.ctypes.data, dists.ctypes.data, _lib.CPU,
                                       bits.ctypes.data, N, _lib.CPU, 0) == _lib.INVALID_ARGUMENT
    finally:
        lib.ggnn_destroy(h)
    # the operator seam refuses a null bitset before it touches anything
    assert lib.ggnn_op_query_filtered(None, 0, 0, 0, None, None, None, 0, None, 0, None, 0, None, 1,
                                      0.5, 1, 0, 1, 0, None, None, None, None, None, None, 0,
                                      None) == _lib.INVALID_ARGUMENT
    assert lib.ggnn_op_bf_query_filtered(None, 0, 0, 0, None, 0, 1, 0, None, None, None, 0,
                                         None) == _lib.INVALID_ARGUMENT


def test_python_surface():
    import inspect

    import ggnn_amd
    sig = inspect.signature(ggnn_amd.GGNN.query_filtered)
    assert list(sig.parameters)[1:] == ["query", "k_query", "tau_query", "max_iterations", "measure",
                                        "filter"]
    assert sig.parameters["filter"].default is None
    sig = inspect.signature(ggnn_amd.GGNN.bf_query_filtered)
    assert list(sig.parameters)[1:] == ["query", "k_gt", "measure", "filter"]
    assert "pack_filter" in ggnn_amd.__all__
    from ggnn_amd import ops
    assert callable(ops.query_filtered) and callable(ops.bf_query_filtered)


def test_bf_reference_helper(orc):
    """the helper the GPU tests compare with: ids mapped back, ties by lower id, (-1, +inf) tail"""
    rng = np.random.default_rng(5)
    base = rng.integers(0, 4, (200, 8)).astype(np.float32)
    base[100:150] = base[:50]                                  # duplicates across the boundary
    q = rng.integers(0, 4, (6, 8)).astype(np.float32)
    allowed = np.zeros(200, bool)
    allowed[::3] = True
    ids, d = bf_filtered_reference(orc, base, q, 80, allowed)
    assert ids.shape == (6, 80) and (ids[:, 67:] == -1).all() and np.isinf(d[:, 67:]).all()
    assert allowed[ids[:, :67]].all()
    for i in range(6):
        order = sorted(np.nonzero(allowed)[0], key=lambda k: (((base[k] - q[i]) ** 2).sum(), k))
        assert ids[i, :67].tolist() == order
