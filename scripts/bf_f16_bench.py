"""Times bf_query of float16 / bfloat16 rows on the 16-bit tile kernels (bf_f16.hip, hook BF_F16 = 2)
against the float32-staged tile kernels (BF_F16 = 1), on one GPU:

    python scripts/bf_f16_bench.py [--reps 7] [--out FILE.json] [--shapes I ...] [--once] [--flush-tiny]

Shapes (both types, squared L2, k = 10, N(0,1) rows): 10k x 1M x 128, 10k x 1M x 960 and the sweep around
the routing minima {256, 1024} x {4096, 65536} x 128.  The two paths alternate within one process; per
shape and path one JSON line with the median, minimum and maximum milliseconds of the whole call over
the repetitions (device events around the call), n_rescanned, and whether ids and distance bits of the
two paths agree.  --once runs every path once after a warm-up and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats`, which gives the kernels' own times (bf_f16_kernel / bf_mfma_kernel
and the passes around them) -- profiled and end-to-end figures come from separate runs.
No figure here is asserted anywhere: it is the measurement behind DESIGN.md 4.6."""
import argparse
import json
import statistics

import torch

from ggnn_amd import _lib, ops

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
SHAPES = [(t, Nq, N, D) for t in DT for (Nq, N, D) in
          [(10_000, 1_000_000, 128), (10_000, 1_000_000, 960)] +
          [(Nq, N, 128) for Nq in (256, 1024) for N in (4096, 65536)]]
PATHS = {"f32_staged": 1, "tiles_16bit": 2}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--shapes", type=int, nargs="*")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--flush-tiny", action="store_true",
                    help="zero every |value| < 1e-4: no float16 subnormals, so float16 runs its tiles")
    args = ap.parse_args()
    lines = []
    for si in (args.shapes if args.shapes is not None else range(len(SHAPES))):
        t, Nq, N, D = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(si)
        base = torch.randn((N, D), device="cuda", generator=g).to(DT[t])
        query = torch.randn((Nq, D), device="cuda", generator=g).to(DT[t])
        if args.flush_tiny:
            base[base.abs() < 1e-4], query[query.abs() < 1e-4] = 0, 0
        ms, out = {p: [] for p in PATHS}, {}
        for rep in range(-1, 1 if args.once else args.reps):                  # -1: warm-up
            for p, v in PATHS.items():                                           # alternating runs
                with _lib.hooks(BF_F16=v):
                    took, out[p] = timed(lambda: ops.bf_query(base, query, 10, 0, rescanned=True))
                if rep >= 0:
                    ms[p].append(took)
        same = bool(torch.equal(out["f32_staged"][0], out["tiles_16bit"][0]) and
                    torch.equal(out["f32_staged"][1].view(torch.int32),
                                out["tiles_16bit"][1].view(torch.int32)))
        for p in PATHS:
            line = {"dtype": t, "Nq": Nq, "N": N, "D": D, "path": p, "reps": len(ms[p]),
                    "median_ms": round(statistics.median(ms[p]), 3), "min_ms": round(min(ms[p]), 3),
                    "max_ms": round(max(ms[p]), 3), "n_rescanned": out[p][2], "same_bits": same}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del base, query, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
