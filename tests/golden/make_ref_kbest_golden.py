"""Writes tests/golden/ref_kbest.npz: what the reference's own KBestList
(include/ggnn/cuda_utils/k_best_list.cuh) keeps of seeded (distance, id) streams, executed on an
MI355X.

Source of the values: oracle/_ref/libggnn_ref_kbest.so, i.e. k_best_list.cuh compiled unchanged
for gfx950 (oracle/ref_kbest_harness.hip, `make -C oracle ref`, only where the reference tree is
available).  The inputs are regenerated from their seeds by tests/test_gpu_ref_kbest.py (the
functions below); the fixture holds the reference's outputs only, so the tests need no reference
tree.  Regenerate deliberately, on a GPU, with:
    python tests/golden/make_ref_kbest_golden.py [out.npz]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_kbest.npz")

BLOCKS = (32, 64, 128, 256)
BESTS = (1, 2, 10, 24, 33, 100, 300)
ENGINE_K = 17


def streams(block, best):
    """(n, dists, ids) of the three streams of one (block, best) case: many exact ties"""
    r = np.random.default_rng(block * 1000 + best)
    for n, hi in ((5, 4), (200, 20), (1500, 1000)):
        dists = r.integers(0, hi, n).astype(np.float32)
        ids = r.integers(0, 10**6, n).astype(np.int32)
        yield n, dists, ids


def key(block, best, check_worst, n):
    return f"b{block}_k{best}_w{int(check_worst)}_n{n}"


def engine_case():
    """base, queries and the exact distances of each query in base order (tiny value range ->
    many ties)"""
    r = np.random.default_rng(5)
    base = r.integers(0, 6, (4000, 8)).astype(np.float32)
    q = r.integers(0, 6, (3, 8)).astype(np.float32)
    dists = [((base - q[n]) ** 2).sum(1).astype(np.float32) for n in range(q.shape[0])]
    return base, q, dists


def main(out):
    import torch
    sys.path.insert(0, ROOT)
    from oracle import oracle as orc
    if not os.path.exists(orc.REF_KBEST_SO):
        raise SystemExit("oracle/_ref/libggnn_ref_kbest.so missing: build it with `make -C oracle ref`")
    lib = C.CDLL(orc.REF_KBEST_SO)
    lib.ref_kbest_script.restype = C.c_int
    lib.ref_kbest_script.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_int, C.c_void_p, C.c_void_p]

    def run_ref(block, best, dists, ids, check_worst):
        d_d = torch.from_numpy(dists).cuda()
        d_i = torch.from_numpy(ids).cuda()
        o_d = torch.empty(best, dtype=torch.float32, device="cuda")
        o_i = torch.empty(best, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = lib.ref_kbest_script(block, best, d_d.data_ptr(), d_i.data_ptr(), dists.size,
                                  int(check_worst), o_d.data_ptr(), o_i.data_ptr())
        assert rc == 0, rc
        return o_d.cpu().numpy(), o_i.cpu().numpy()

    res = {}
    for block in BLOCKS:
        for best in BESTS:
            for check_worst in (True, False):
                for n, dists, ids in streams(block, best):
                    rd, ri = run_ref(block, best, dists, ids, check_worst)
                    res[key(block, best, check_worst, n) + "_d"] = rd
                    res[key(block, best, check_worst, n) + "_i"] = ri
    _, _, dists = engine_case()
    rows = [run_ref(32, ENGINE_K, d, np.arange(d.size, dtype=np.int32), True) for d in dists]
    res["engine_d"] = np.stack([r[0] for r in rows])
    res["engine_i"] = np.stack([r[1] for r in rows])
    # provenance: which library produced the vectors, and on which device
    import hashlib
    with open(orc.REF_KBEST_SO, "rb") as fh:
        res["source_library_sha256"] = np.array(hashlib.sha256(fh.read()).hexdigest())
    res["source"] = np.array("oracle/_ref/libggnn_ref_kbest.so: the reference's "
                             "include/ggnn/cuda_utils/k_best_list.cuh compiled unchanged for gfx950 "
                             "(oracle/ref_kbest_harness.hip), run on " +
                             torch.cuda.get_device_name(0))
    np.savez_compressed(out, **res)
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
