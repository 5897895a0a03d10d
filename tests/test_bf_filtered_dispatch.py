"""CPU tests of the filtered brute force on the matrix cores: the new C-ABI entry points, the
status code that needs no device, and the verdicts the filtered tile kernels stage (bf_mfma.hip,
FilterStage) restated in numpy against plain masks, in the style of tests/test_labels.py: the word
of a tile, bit j of it, the three-way row select for filter ids, and the label compare."""
import ctypes as C
import os
import re

import numpy as np

from filtered_reference import pack_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {
    # name -> number of parameters of the prototype in include/ggnn_c.h
    "ggnn_last_bf_query_matrix_path": 2,
    "ggnn_op_bf_query_filtered_certified": 15,      # ggnn_op_bf_query_filtered (13) + 2
    "ggnn_op_bf_query_filtered_by_certified": 18,   # ggnn_op_bf_query_filtered_by (16) + 2
    "ggnn_op_bf_query_labeled_certified": 17,       # ggnn_op_bf_query_labeled (15) + 2
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
    # the certified calls are the existing prototypes + (n_rescanned, matrix_path) before the stream
    for plain in ("ggnn_op_bf_query_filtered", "ggnn_op_bf_query_filtered_by",
                  "ggnn_op_bf_query_labeled"):
        a, b = _lib.SIGNATURES[plain][1], _lib.SIGNATURES[plain + "_certified"][1]
        assert list(b[:len(a) - 1]) == list(a[:-1]) and b[-1] is a[-1], plain
        assert b[-3] is C.c_void_p and b[-2] is C.POINTER(C.c_int), plain
    # existing entry points keep their signatures
    assert len(_lib.SIGNATURES["ggnn_op_bf_query_filtered"][1]) == 13
    assert len(_lib.SIGNATURES["ggnn_op_bf_query_filtered_by"][1]) == 16
    assert len(_lib.SIGNATURES["ggnn_op_bf_query_labeled"][1]) == 15


def test_matrix_path_getter_rejects_null():
    from ggnn_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.ggnn_create(C.byref(h)) == 0
    try:
        out = C.c_int(-7)
        assert lib.ggnn_last_bf_query_matrix_path(h, C.byref(out)) == 0
        assert out.value == 0                       # no bf_query yet
        assert lib.ggnn_last_bf_query_matrix_path(h, None) == _lib.INVALID_ARGUMENT
        assert lib.ggnn_last_bf_query_matrix_path(None, C.byref(out)) != 0
    finally:
        lib.ggnn_destroy(h)


# ---- the staged verdicts, restated ---------------------------------------------------------------
def tile_word(row_words, row0, end, offset):
    """FilterStage<kBfBits>::load: the one word of a query's bitset that holds the verdicts of the
    tile starting at row0 (a multiple of 32; offset a multiple of 32; a padding tile of a group,
    row0 >= end, re-reads the word of the last row)"""
    return row_words[(min(row0, end - 1) + offset) >> 5]


def select_row(table, consts, words, num_filters, f):
    """FilterStage<kBfBits>::open: table row / all-ones row / all-zero row, by an unsigned compare"""
    if np.uint32(np.int32(f)) < np.uint32(num_filters):
        return table[int(f) * words:(int(f) + 1) * words]
    return consts[:words] if f == -1 else consts[words:2 * words]


def test_staged_bit_verdicts_equal_plain_masks():
    rs = np.random.default_rng(5)
    for N, F in ((4500, 5), (9100, 3), (4096, 1)):
        for _ in range(4):
            offset = 32 * int(rs.integers(0, 200))
            n_bits = offset + N + int(rs.integers(0, 70))
            masks = rs.random((F, n_bits)) < rs.random((F, 1))
            words = (n_bits + 31) // 32
            table = np.concatenate([pack_bits(m) for m in masks])
            consts = np.concatenate([np.full(words, 0xffffffff, np.uint32), np.zeros(words, np.uint32)])
            T = int(rs.integers(1, 5))
            ntiles = (N + 31) // 32
            ntiles_padded = (ntiles + T - 1) // T * T     # a group always runs its T tiles
            for f in list(range(-1, F)) + [F, 7, -5, 2**31 - 1, -2**31]:
                row = select_row(table, consts, words, F, f)
                want = (masks[f, offset:offset + N] if 0 <= f < F
                        else np.ones(N, bool) if f == -1 else np.zeros(N, bool))
                got = np.zeros(N, bool)
                for t in range(ntiles_padded):
                    w = tile_word(row, 32 * t, N, offset)     # never outside the row
                    for j in range(32):
                        if 32 * t + j < N:                    # rows past the end: padding norm
                            got[32 * t + j] = (int(w) >> j) & 1
                assert np.array_equal(got, want), (N, F, offset, f)


def test_staged_label_verdicts_equal_plain_masks():
    rs = np.random.default_rng(6)
    N = 4500
    for offset in (0, 32 * 141, 64):
        column = rs.integers(-1, 6, offset + N + 10).astype(np.int32)
        for ql in (-1, 0, 3, 5, 8, -2):
            # FilterStage<kBfLabels>::load + bf_label_denied
            rows = np.minimum(np.arange(N), N - 1)
            row_label = column[offset + rows]
            denied = (ql != -1) & (row_label != ql)
            want = np.ones(N, bool) if ql == -1 else column[offset:offset + N] == ql
            assert np.array_equal(~denied, want), (offset, ql)
            # the LabelFilter predicate (traversal.hpp) with vmask / want fixed per query
            vmask = np.uint32(0) if ql == -1 else np.uint32(0xffffffff)
            w = np.uint32(np.int32(ql)) & vmask
            assert np.array_equal((row_label.view(np.uint32) & vmask) == w, want), (offset, ql)
