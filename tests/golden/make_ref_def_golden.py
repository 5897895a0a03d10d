"""Writes tests/golden/ref_def_h.npz: the reference's own sizing helpers (include/ggnn/base/def.h,
bit_ceil / next_multiple<32> / align8, and the DistanceMeasure codes) evaluated on every value the
sizing rules can see (query_kernels.cu:55-110: KQuery <= 6000, max_iterations <= 8192, D <= 4096).

Source of the values: oracle/_ref/libggnn_ref_def.so, i.e. def.h compiled unchanged with g++
(oracle/ref_def_harness.cpp, `make -C oracle ref`, only where the reference tree is available).
The fixture holds outputs only, so tests/test_oracle.py needs no reference tree.  Regenerate
deliberately with:  python tests/golden/make_ref_def_golden.py"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_def_h.npz")


def uint32_values():
    return np.array(list(range(0, 8300)) + [2 ** k + o for k in range(13, 32) for o in (-1, 0, 1)
                                           if 0 <= 2 ** k + o < 2 ** 31 + 1], dtype=np.uint64)


def size_t_values():
    return np.array(list(range(0, 100)) + [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1,
                                           125_793_824 * 24 * 4 + 13], dtype=np.uint64)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle import oracle as orc
    if not os.path.exists(orc.REF_DEF_SO):
        raise SystemExit("oracle/_ref/libggnn_ref_def.so missing: build it with `make -C oracle ref`")
    ref = C.CDLL(orc.REF_DEF_SO)
    ref.ref_bit_ceil.restype = C.c_uint32
    ref.ref_next_multiple32.restype = C.c_uint32
    ref.ref_align8.restype = C.c_size_t
    ref.ref_align8.argtypes = [C.c_size_t]
    u, s = uint32_values(), size_t_values()
    np.savez_compressed(
        OUT, uint32_values=u, size_t_values=s,
        bit_ceil=np.array([ref.ref_bit_ceil(C.c_uint32(int(v))) for v in u], dtype=np.uint64),
        next_multiple32=np.array([ref.ref_next_multiple32(C.c_uint32(int(v))) for v in u],
                                 dtype=np.uint64),
        align8=np.array([ref.ref_align8(int(v)) for v in s], dtype=np.uint64),
        measure=np.array([ref.ref_measure_euclidean(), ref.ref_measure_cosine()], dtype=np.int64))
    print("wrote", OUT)
