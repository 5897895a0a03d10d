"""Times the exact range search beside the K-best scan of the same shape, on one GPU:

    python scripts/bf_range_bench.py [--reps 5] [--out FILE.json]

Shapes: 10k x 1M x 128 float32 and uint8, 100 x 1M x 128 float32.  Per shape, with the radius of every
query at its 10th and at (about) its 1000th neighbour's distance: the count-only call (one distance pass) and
the full call into an exactly sized buffer (two passes), in alternating runs with `bf_query` of the
same shape under hook BF_SCAN = 1, k = 10 (the scan kernels: one pass that also keeps a list).  Prints
one JSON line per shape: median and min / max milliseconds over the repetitions, and results per query.
No figure here is asserted anywhere: it is the measurement behind DESIGN.md 4.6."""
import argparse
import json
import statistics

import numpy as np
import torch

from ggnn_amd import _lib, ops

SHAPES = [("f32", 10_000, 1_000_000, 128), ("u8", 10_000, 1_000_000, 128),
          ("f32", 100, 1_000_000, 128)]


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
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))))
    args = ap.parse_args()
    lines = []
    for si in args.shapes:
        dtype, Nq, N, D = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(si)
        if dtype == "u8":
            base = torch.randint(0, 256, (N, D), dtype=torch.uint8, device="cuda", generator=g)
            query = torch.randint(0, 256, (Nq, D), dtype=torch.uint8, device="cuda", generator=g)
        else:
            base = torch.rand((N, D), device="cuda", generator=g)
            query = torch.rand((Nq, D), device="cuda", generator=g)
        # the radii: the exact 10th neighbour's distance, and the 10th neighbour's distance within the
        # first 1 % of the base -- on i.i.d. rows about the 1000th neighbour's of the whole base
        # (results_per_query below says what the radii really admit)
        d10 = ops.bf_query(base, query, 10)[1]
        d1000 = ops.bf_query(base[:N // 100], query, 10)[1]
        radii = {10: d10[:, 9].contiguous(), 1000: d1000[:, 9].contiguous()}
        totals = {k: int(ops.bf_range_query(base, query, r, capacity=0)[0][-1]) for k, r in radii.items()}
        bufs = {k: (torch.empty(t, dtype=torch.int32, device="cuda"),
                    torch.empty(t, dtype=torch.float32, device="cuda")) for k, t in totals.items()}
        ms = {"scan_k10": []}
        for k in radii:
            ms[f"count_r{k}"], ms[f"full_r{k}"] = [], []
        with _lib.hooks(BF_SCAN=1):
            ops.bf_query(base, query, 10)                                        # warm-up
            for _ in range(args.reps):                                           # alternating runs
                ms["scan_k10"].append(timed(lambda: ops.bf_query(base, query, 10))[0])
                for k, r in radii.items():
                    ms[f"count_r{k}"].append(
                        timed(lambda: ops.bf_range_query(base, query, r, capacity=0))[0])
                    ms[f"full_r{k}"].append(
                        timed(lambda: ops.bf_range_query(base, query, r, out=bufs[k]))[0])
        line = {"dtype": dtype, "Nq": Nq, "N": N, "D": D, "reps": args.reps,
                "results_per_query": {f"r{k}": round(t / Nq, 2) for k, t in totals.items()},
                **{k: stats(v) for k, v in ms.items()}}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del base, query, d10, d1000, bufs
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
