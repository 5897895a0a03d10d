"""float32 / float16 / bfloat16 / uint8 / int8 bases of the same data: speed, bytes and recall
(1M x 128).
    python scripts/dtype_probe.py [kinds] [n] [variants]
    python scripts/dtype_probe.py lowrank16,lowrankf16 1000000
    python scripts/dtype_probe.py lowrank16 1000000 uint8,int8,uint8,int8   (alternating A/B)

Every base is built from the same float32 rows (bench.synthetic) converted to each type; float32
runs with the pre-screen on (default) and off.  lowrank16 holds integers in [0, 255], exact in all
three types (speed alone differs); lowrankf16 is fractional, so the 16-bit bases are rounded (the
recall cost of the rounding).  Ground truth: each base's own bf_query.  Per variant, at the bench
operating point and at the cheapest point of POINTS that reaches recall@10 0.99: queries/s and
query-kernel ms on 10k-query batches, rows read per query x row bytes, HBM bytes per base row,
build time and bf_query ms.  One JSON line per (kind, variant, point).
uint8 / int8 (integer kinds only, i.e. lowrank16): the uint8 base holds the integers themselves, the
int8 base the same rows `^ 0x80` (x - 128), so both do identical work; they are not part of the
default variants (name them in the third argument, repeated for alternating runs)."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import ggnn_amd as ggnn  # noqa: E402
from bench import recall_at_k, synthetic  # noqa: E402

ggnn.set_log_level(-1)
kinds = sys.argv[1].split(",") if len(sys.argv) > 1 else ["lowrank16", "lowrankf16"]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D, K, NQ = 128, 10, 10_000
BENCH_POINT = (0.85, 175)
# candidate points in ascending cost: the first that reaches 0.99 is the "cheapest 0.99 point"
POINTS = ((0.85, 150), (0.85, 175), (0.9, 200), (0.95, 225), (1.0, 250), (1.0, 300), (1.1, 400),
          (1.2, 600))
VARIANTS = (("f32", torch.float32, True), ("f32-nops", torch.float32, False),
            ("f16", torch.float16, False), ("bf16", torch.bfloat16, False))
BYTE_VARIANTS = {"uint8": ("uint8", torch.uint8, False), "int8": ("int8", torch.int8, False)}
if len(sys.argv) > 3:
    by_name = {**{v[0]: v for v in VARIANTS}, **BYTE_VARIANTS}
    VARIANTS = tuple(by_name[v] for v in sys.argv[3].split(","))
dev = torch.device("cuda", 0)


def rows_as(x32, dt):
    """the float32 rows in element type dt; int8: the uint8 rows biased by 128"""
    if dt == torch.int8:
        return (x32.to(torch.uint8) ^ 0x80).view(torch.int8).contiguous()
    return x32.to(dt).contiguous()


def timed_point(eng, q, gt, tau, iters, steps=3):
    for _ in range(2):
        eng.query(q, K, tau, iters)
    ms, wall = [], []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, _ = eng.query(q, K, tau, iters)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        ms.append(eng.last_timing_ms()["query_ms"])
    rec = recall_at_k(ids, gt)
    eng.set_collect_counters(True)
    eng.query(q, K, tau, iters)
    rows = eng.last_query_rows_read()
    cnt = eng.last_query_counters()
    eng.set_collect_counters(False)
    return dict(tau=tau, iters=iters, recall=round(rec, 4), kernel_ms=round(min(ms), 4),
                qps=round(NQ / min(wall)), rows=rows, n_dist=cnt["n_dist"])


for kind in kinds:
    base32 = synthetic(kind, n, D, 1234, dev)
    q32 = synthetic(kind, NQ, D, 4321, dev)
    for name, dt, ps in VARIANTS:
        base, q = rows_as(base32, dt), rows_as(q32, dt)
        es = base.element_size()
        eng = ggnn.GGNN()
        eng.set_base_reference(base)
        eng.set_return_results_on_gpu(True)
        eng.set_prescreen(ps)
        t0 = time.perf_counter()
        eng.build(24, 0.5, 2)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        gt, _ = eng.bf_query(q, K)
        eng.bf_query(q, K)
        bf_ms = eng.last_timing_ms()["bf_query_ms"]
        # bytes per base row held in HBM: the row itself + the pre-screen code row (float32, on)
        code_b = 128 if (ps and dt == torch.float32) else 0
        common = dict(kind=kind, variant=name, build_s=round(build_s, 3), bf_ms=round(bf_ms, 3),
                      hbm_bytes_per_row=D * es + code_b)
        chosen = None
        for tau, iters in POINTS:
            r = timed_point(eng, q, gt, tau, iters, steps=1)
            if r["recall"] >= 0.99:
                chosen = (tau, iters)
                break
        for label, pt in (("bench", BENCH_POINT), ("cheapest_0.99", chosen)):
            if pt is None:
                print(json.dumps({**common, "point": label, "reached": False}), flush=True)
                continue
            r = timed_point(eng, q, gt, *pt)
            fr, cr = r["rows"]["float_rows"], r["rows"]["code_rows"]
            bytes_q = (fr * D * es + cr * code_b) / NQ
            print(json.dumps({**common, "point": label, **r, "rows_per_query": round(fr / NQ, 1),
                              "code_rows_per_query": round(cr / NQ, 1),
                              "row_bytes_per_query": round(bytes_q)}), flush=True)
        del eng
        torch.cuda.empty_cache()
