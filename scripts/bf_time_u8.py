"""bf_query timing for uint8 / int8 rows on one GPU:

    python scripts/bf_time_u8.py [n=1M] [k=10] [D=128] [--nq 10000] [--dtype u8|i8] [--hook NAME=V ...]
    python scripts/bf_time_u8.py --wide-table [--reps 7] [--once] [--out FILE.json]
    python scripts/bf_time_u8.py --cos-table [--reps 7] [--once] [--out FILE.json]

First form: one shape under the given hooks (e.g. --hook BF_I8_V1=1 times the LDS-list kernel), mean of
5 calls.  --wide-table: the wide-row integer kernel (bf_i8_wide.hip, hook BF_I8_WIDE = 2) against the
float32-staged tiles (BF_I8_WIDE = 1) at 10k x 1M x {256 u8, 768 i8, 960 u8} and {1024 x 65536, 256 x
4096} x 256 u8, k = 10: the two paths alternate within one process; per shape and path one JSON line with
median / minimum / maximum milliseconds of the whole call (device events), n_rescanned and whether ids
and distance bits of the two paths agree.  --cos-table: the same for the integer cosine kernel
(bf_i8_cos.hip, hook BF_I8_COS = 2 against = 1) under cosine, at D = 128 in place of 256 for the first shape;
uint8 rows wider than 258 bytes are halved so that every norm stays below 2^24 (otherwise the table would
time the re-scan).  --once: every path once after a warm-up, the run to put under
`rocprofv3 --kernel-trace --stats`.  Nothing here is asserted: it is the measurement behind DESIGN.md 4.6."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ggnn_amd import _lib, ops
from bench import synthetic

WIDE = [("u8", 10_000, 1_000_000, 256), ("i8", 10_000, 1_000_000, 768), ("u8", 10_000, 1_000_000, 960),
        ("u8", 1024, 65536, 256), ("u8", 256, 4096, 256)]
COS = [("u8", 10_000, 1_000_000, 128)] + WIDE[1:]


def rows(n, D, seed, dtype):
    x = synthetic("lowrank16", n, D, seed, torch.device("cuda", 0)).to(torch.uint8)
    return x if dtype == "u8" else (x.to(torch.int16) - 128).to(torch.int8)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def table(args, shapes, hook, measure, new_path):
    PATHS = {"f32_staged": 1, new_path: 2}
    lines = []
    for dtype, Nq, N, D in shapes:
        base, query = rows(N, D, 1234, dtype), rows(Nq, D, 4321, dtype)
        if measure == 1 and dtype == "u8" and D > 258:
            base, query = base >> 1, query >> 1
        ms, out = {p: [] for p in PATHS}, {}
        for rep in range(-1, 1 if args.once else args.reps):                     # -1: warm-up
            for p, v in PATHS.items():                                           # alternating runs
                with _lib.hooks(**{hook: v}):
                    took, out[p] = timed(lambda: ops.bf_query(base, query, 10, measure, rescanned=True))
                if rep >= 0:
                    ms[p].append(took)
        same = bool(torch.equal(out["f32_staged"][0], out[new_path][0]) and
                    torch.equal(out["f32_staged"][1].view(torch.int32), out[new_path][1].view(torch.int32)))
        for p in PATHS:
            line = {"dtype": dtype, "Nq": Nq, "N": N, "D": D, "path": p, "reps": len(ms[p]),
                    "median_ms": round(statistics.median(ms[p]), 3), "min_ms": round(min(ms[p]), 3),
                    "max_ms": round(max(ms[p]), 3), "n_rescanned": out[p][2], "same_bits": same}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del base, query, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=1_000_000)
    ap.add_argument("k", type=int, nargs="?", default=10)
    ap.add_argument("D", type=int, nargs="?", default=128)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--dtype", choices=("u8", "i8"), default="u8")
    ap.add_argument("--hook", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--wide-table", action="store_true")
    ap.add_argument("--cos-table", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.wide_table:
        return table(args, WIDE, "BF_I8_WIDE", 0, "i8_wide")
    if args.cos_table:
        return table(args, COS, "BF_I8_COS", 1, "i8_cos")
    hooks = {h.split("=")[0]: int(h.split("=")[1]) for h in args.hook}
    base, query = rows(args.n, args.D, 1234, args.dtype), rows(args.nq, args.D, 4321, args.dtype)
    with _lib.hooks(**hooks):
        for _ in range(2):
            ids, d = ops.bf_query(base, query, args.k)
        torch.cuda.synchronize()
        ms, (ids, d) = timed(lambda: [ops.bf_query(base, query, args.k) for _ in range(5)][-1])
    ms /= 5
    print(f"bf_query {args.dtype} {args.nq}x{args.n}x{args.D} k={args.k} {hooks}: {ms:.2f} ms  "
          f"{2 * args.nq * args.n * args.D / ms / 1e9:.1f} Top/s checksum {int(ids.sum())} {float(d.sum())}")


if __name__ == "__main__":
    main()
