"""Label ranges three ways at the headline operating point ("Label index"):
1M x 128 float32, k = 10, 10 000 queries, one window of a timestamp column per query, windows admitting
0.01 / 0.1 / 1 / 10 % of the rows.

    python scripts/label_spans_bench.py [--n 1000000] [--queries 10000] [--tau 0.85] [--iters 175]
                                        [--shares 0.0001 0.001 0.01 0.1] [--reps 3]

Per share, the time of
  * "index":     ops.label_spans_resolve + ops.bf_query_label_spans, the exact search of the window's
                 own rows through the label index;
  * "scan":      ops.bf_query_labeled_range, the exact scan of the whole base;
  * "traversal": query_labeled_range of the handle at (--tau, --iters), with its recall@k against the
                 exact result,
alternating per repeat, every repeat listed.  "index" and "scan" are GPU time between two events on the
stream around the call (results asserted bit-identical first); "traversal" is the handle's own kernel
time (last_timing_ms).  Also printed: the bytes the index path reads by the rule total x (row bytes + 4)
against the scan's N x row bytes, per query.  One JSON line per share."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggnn_amd as ggnn  # noqa: E402
from ggnn_amd import ops  # noqa: E402


def event_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return out, start.elapsed_time(end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--tau", type=float, default=0.85)       # the bench operating point
    ap.add_argument("--iters", type=int, default=175)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shares", type=float, nargs="+", default=[0.0001, 0.001, 0.01, 0.1])
    a = ap.parse_args()
    rs = np.random.default_rng(1)
    centres = rs.normal(size=(256, a.d)).astype(np.float32) * 2
    base = centres[rs.integers(0, 256, a.n)] + rs.normal(size=(a.n, a.d)).astype(np.float32)
    query = centres[rs.integers(0, 256, a.queries)] + rs.normal(size=(a.queries, a.d)).astype(np.float32)
    span = 1_000_000_000                                     # timestamps: uniform over a long period
    stamps = rs.integers(0, span, a.n).astype(np.int32)

    g = ggnn.GGNN()
    d_base = torch.from_numpy(base).cuda()
    g.set_base(d_base)
    g.set_labels(stamps)
    g.build(24, 0.5)
    q = torch.from_numpy(query).cuda()
    d_stamps = torch.from_numpy(stamps).cuda()
    keys, offsets, rows = (t.cuda() for t in ops.label_index_build(stamps))
    row_bytes = a.d * 4

    for share in a.shares:
        width = int(span * share)
        lo = rs.integers(0, span - width, a.queries)
        windows = torch.from_numpy(np.stack([lo, lo + width - 1], 1).astype(np.int32)[:, None, :]).cuda()
        totals = ops.label_spans_resolve(keys, offsets, label_ranges=windows)[1]
        limit = int(totals.max())
        calls = {
            "index": lambda: ops.bf_query_label_index_range(d_base, q, a.k, keys, offsets, rows,
                                                            windows, span_limit=limit),
            "scan": lambda: ops.bf_query_labeled_range(d_base, q, a.k, d_stamps, windows),
            "traversal": lambda: g.query_labeled_range(q, a.k, a.tau, a.iters, label_ranges=windows),
        }
        exact, scan, approx = (fn() for fn in calls.values())
        assert torch.equal(exact[0], scan[0]) and torch.equal(exact[1], scan[1])
        e, t = exact[0].cpu().numpy(), approx[0].cpu().numpy()[:, :a.k]
        recall = float(np.mean([len(set(x[x >= 0].tolist()) & set(y[y >= 0].tolist())) /
                                max(1, int((y >= 0).sum())) for x, y in zip(t, e)]))
        ms = {k: [] for k in calls}
        for _ in range(a.reps):                               # alternating
            for k, fn in calls.items():
                if k == "traversal":
                    fn()
                    ms[k].append(round(g.last_timing_ms()["query_ms"], 3))
                else:
                    ms[k].append(round(event_ms(fn)[1], 3))
        print(json.dumps({"share": share, "rows_per_query": round(float(totals.float().mean()), 1),
                          "max_rows": limit, "ms": ms, "traversal_recall": round(recall, 4),
                          "index_bytes_per_query": int(float(totals.float().mean()) * (row_bytes + 4)),
                          "scan_bytes_per_query": a.n * row_bytes}), flush=True)


if __name__ == "__main__":
    main()
