"""Times the exact range search beside the K-best scan of the same shape, on one GPU:

    python scripts/bf_range_bench.py [--reps 5] [--out FILE.json] [--dtype uint8|int8] [--measure l2|cosine]

Shapes: 10k x 1M x 128 float32 and uint8, 100 x 1M x 128 float32, 10k x 1M x 960 float32 cosine, and a
sweep around the routing minima of the tile path (Nq 256 / 1024, N 4096 / 65536).  Per shape, with the radius of every
query at its 10th and at (about) its 1000th neighbour's distance: the count-only call (one distance pass) and
the full call into an exactly sized buffer (two passes), in alternating runs with `bf_query` of the
same shape under hook BF_SCAN = 1, k = 10 (the scan kernels: one pass that also keeps a list) and on
the tile kernels (`mfma_k10`).  The range calls run under BF_RANGE_PATH = 1 (the scan: `count_r*`,
`full_r*`) and = 2 (tile pre-selection, exact hits: `tile_count_r*`, `tile_full_r*`).  Prints
Byte rows alternate hook BF_RANGE_I8 = 1 (the scan) and = 2 (the integer tile kernels, exact verdicts)
instead.  --dtype uint8|int8 runs the byte-row sweep: 10k x 1M x 128 and the four shapes around the
routing minima, integer data over the full value range; the radii are pair distances, so integers.
--dtype uint8|int8 --measure cosine runs the same sweep under cosine, with 10k x 1M x 768 behind it, hook
BF_RANGE_I8_COS = 1 (the scan) against = 2 (the integer cosine tile kernels, bf_range_i8_cos.hip).
--dtype f16|bf16 runs the 16-bit sweep on N(0,1) rows: 10k x 1M x 128 and x 960 and the four small shapes,
hook BF_RANGE_F16 = 1 (the float32-staged tiles where BF_RANGE_PATH's minima admit the shape, else the
scan) against = 2 (the 16-bit tile kernels); `path_fell_back` records (matrix_path, fell_back) of each.
--no-kbest leaves the two `bf_query` columns out (they are not what the 16-bit sweep is about).
Prints one JSON line per shape: median and min / max milliseconds over the repetitions, and results per query.
No figure here is asserted anywhere: it is the measurement behind DESIGN.md 4.6."""
import argparse
import json
import statistics

import numpy as np
import torch

from ggnn_amd import _lib, ops

SHAPES = [("f32", 10_000, 1_000_000, 128, 0), ("u8", 10_000, 1_000_000, 128, 0),
          ("f32", 100, 1_000_000, 128, 0), ("f32", 10_000, 1_000_000, 960, 1)] + \
         [("f32", Nq, N, 128, 0) for Nq in (256, 1024) for N in (4096, 65536)]
BYTE = {"uint8": "u8", "int8": "i8"}
HALF = {"f16": torch.float16, "bf16": torch.bfloat16}


def byte_shapes(t, measure=0):
    return [(t, 10_000, 1_000_000, 128, measure)] + \
           [(t, Nq, N, 128, measure) for Nq in (256, 1024) for N in (4096, 65536)] + \
           ([(t, 10_000, 1_000_000, 768, 1)] if measure else [])


def half_shapes(t):
    return [(t, 10_000, 1_000_000, D, 0) for D in (128, 960)] + [(t, Nq, N, 128, 0) for Nq in (256, 1024)
                                                                  for N in (4096, 65536)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--shapes", type=int, nargs="*")
    ap.add_argument("--dtype", choices=sorted(BYTE) + sorted(HALF))
    ap.add_argument("--measure", choices=["l2", "cosine"], default="l2", help="byte-row sweep only")
    ap.add_argument("--no-kbest", action="store_true", help="skip the bf_query columns")
    args = ap.parse_args()
    shapes = (half_shapes(args.dtype) if args.dtype in HALF
              else byte_shapes(BYTE[args.dtype], int(args.measure == "cosine")) if args.dtype else SHAPES)
    lines = []
    for si in (args.shapes if args.shapes is not None else range(len(shapes))):
        dtype, Nq, N, D, measure = shapes[si]
        g = torch.Generator(device="cuda").manual_seed(si)
        if dtype in ("u8", "i8"):
            lo, tt = (0, torch.uint8) if dtype == "u8" else (-128, torch.int8)
            base = torch.randint(lo, lo + 256, (N, D), dtype=tt, device="cuda", generator=g)
            query = torch.randint(lo, lo + 256, (Nq, D), dtype=tt, device="cuda", generator=g)
        elif dtype in HALF:
            # N(0,1) rows; float16: values below the smallest normal flushed to zero (else the
            # eligibility flag sends every call to the scan and the figure is that of both paths)
            base = torch.randn((N, D), device="cuda", generator=g).to(HALF[dtype])
            query = torch.randn((Nq, D), device="cuda", generator=g).to(HALF[dtype])
            if dtype == "f16":
                base[base.abs() < 2.0 ** -14], query[query.abs() < 2.0 ** -14] = 0, 0
        else:
            base = torch.rand((N, D), device="cuda", generator=g)
            query = torch.rand((Nq, D), device="cuda", generator=g)
        # the radii: the exact 10th neighbour's distance, and the 10th neighbour's distance within the
        # first 1 % of the base -- on i.i.d. rows about the 1000th neighbour's of the whole base
        # (results_per_query below says what the radii really admit)
        d10 = ops.bf_query(base, query, 10, measure)[1]
        d1000 = ops.bf_query(base[:N // 100], query, 10, measure)[1]
        radii = {10: d10[:, 9].contiguous(), 1000: d1000[:, 9].contiguous()}
        totals = {k: int(ops.bf_range_query(base, query, r, measure, capacity=0)[0][-1])
                  for k, r in radii.items()}
        bufs = {k: (torch.empty(t, dtype=torch.int32, device="cuda"),
                    torch.empty(t, dtype=torch.float32, device="cuda")) for k, t in totals.items()}
        ms = {"scan_k10": [], "mfma_k10": []}
        hook = ("BF_RANGE_I8" if dtype in ("u8", "i8") and measure == 0
                else "BF_RANGE_I8_COS" if dtype in ("u8", "i8")
                else "BF_RANGE_F16" if dtype in HALF else "BF_RANGE_PATH")
        paths = {"": 1, "tile_": 2}
        fell = {}
        for k in radii:
            for pre in paths:
                ms[f"{pre}count_r{k}"], ms[f"{pre}full_r{k}"] = [], []
        for rep in range(-1, args.reps):                                         # -1: warm-up
            got = {}
            if not args.no_kbest:
                with _lib.hooks(BF_SCAN=1):
                    got["scan_k10"] = timed(lambda: ops.bf_query(base, query, 10, measure))[0]
                got["mfma_k10"] = timed(lambda: ops.bf_query(base, query, 10, measure))[0]
            for pre, path in paths.items():                                      # alternating runs
                # 16-bit rows: the float32-staged tiles (or, below their minima, the scan) against the
                # 16-bit tiles, BF_RANGE_PATH as it is by default
                with _lib.hooks(**{hook: path}):
                    for k, r in radii.items():
                        if rep < 0 and (dtype in HALF or hook == "BF_RANGE_I8_COS"):   # which path ran, and whether the scan answered
                            fell[f"{pre}r{k}"] = ops.bf_range_query(base, query, r, measure, out=bufs[k],
                                                                    routed=True)[3:]
                        got[f"{pre}count_r{k}"] = timed(
                            lambda: ops.bf_range_query(base, query, r, measure, capacity=0))[0]
                        got[f"{pre}full_r{k}"] = timed(
                            lambda: ops.bf_range_query(base, query, r, measure, out=bufs[k]))[0]
            if rep >= 0:
                for k, v in got.items():
                    ms[k].append(v)
        line = {"dtype": dtype, "Nq": Nq, "N": N, "D": D, "measure": measure, "reps": args.reps,
                "results_per_query": {f"r{k}": round(t / Nq, 2) for k, t in totals.items()},
                **({"path_fell_back": fell} if fell else {}),
                **{k: stats(v) for k, v in ms.items() if v}}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del base, query, d10, d1000, bufs
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
