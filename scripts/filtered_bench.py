"""Cost and recall of the filtered search at the headline operating point:
1M x 128 float32, k = 10, 10 000 queries, 100 / 50 / 10 / 1 % of the rows allowed.

    python scripts/filtered_bench.py [--n 1000000] [--queries 10000] [--tau 0.5] [--iters 400]

Per share: kernel ms of the filtered call (best of --reps), n_dist and n_pop per query, recall@10
against bf_query_filtered, and the scan time of that brute force; the first line is the
unfiltered call of the same handle (the 100 % line against it is the cost of the bit read).
One JSON line per row."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggnn_amd as ggnn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rs = np.random.default_rng(1)
    centres = rs.normal(size=(256, a.d)).astype(np.float32) * 2
    base = centres[rs.integers(0, 256, a.n)] + rs.normal(size=(a.n, a.d)).astype(np.float32)
    query = centres[rs.integers(0, 256, a.queries)] + rs.normal(size=(a.queries, a.d)).astype(np.float32)
    g = ggnn.GGNN()
    g.set_base(torch.from_numpy(base).cuda())
    g.build(24, 0.5)
    q = torch.from_numpy(query).cuda()

    def timed(fn):
        best = float("inf")
        for _ in range(a.reps):
            out = fn()
            best = min(best, g.last_timing_ms()["query_ms"])
        return out, best

    def counters(fn):
        g.set_collect_counters(True)
        fn()
        c = g.last_query_counters()
        g.set_collect_counters(False)
        return c["n_dist"] / a.queries, c["n_pop"] / a.queries

    plain = lambda: g.query(q, a.k, a.tau, a.iters)  # noqa: E731
    (ids, _), ms = timed(plain)
    nd, npop = counters(plain)
    gt, _ = g.bf_query(q, a.k)
    rec = np.mean([len(set(x.tolist()) & set(y.tolist())) / a.k for x, y in zip(ids, gt)])
    print(json.dumps({"filter": "none", "query_ms": round(ms, 4), "n_dist": round(nd, 1),
                      "n_pop": round(npop, 1), "recall": round(float(rec), 4),
                      "bf_ms": round(g.last_timing_ms()["bf_query_ms"], 3)}), flush=True)
    for share in (1.0, 0.5, 0.1, 0.01):
        mask = np.random.default_rng(int(share * 1000)).random(a.n) < share
        bits = ggnn.pack_filter(mask).cuda()
        call = lambda: g.query_filtered(q, a.k, a.tau, a.iters, filter=bits)  # noqa: E731
        (ids, _), ms = timed(call)
        nd, npop = counters(call)
        gt, _ = g.bf_query_filtered(q, a.k, filter=bits)
        bf_ms = g.last_timing_ms()["bf_query_ms"]
        rec = np.mean([len(set(x.tolist()) & set(y.tolist())) / a.k for x, y in zip(ids, gt)])
        print(json.dumps({"filter": share, "allowed": int(mask.sum()), "query_ms": round(ms, 4),
                          "n_dist": round(nd, 1), "n_pop": round(npop, 1),
                          "recall": round(float(rec), 4), "bf_filtered_ms": round(bf_ms, 3)}),
              flush=True)


if __name__ == "__main__":
    main()
