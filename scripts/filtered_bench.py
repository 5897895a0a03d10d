"""Cost and recall of the filtered search at the headline operating point:
1M x 128 float32, k = 10, 10 000 queries, 100 / 50 / 10 / 1 % of the rows allowed.

    python scripts/filtered_bench.py [--n 1000000] [--queries 10000] [--tau 0.5] [--iters 400]

Per share: kernel ms of the filtered call (best of --reps), n_dist and n_pop per query, recall@10
against bf_query_filtered, and the scan time of that brute force; the first line is the
unfiltered call of the same handle (the 100 % line against it is the cost of the bit read).
One JSON line per row.

    python scripts/filtered_bench.py --mixed [--tenants 16] [--big-table 1024]

Per-query filters (a resident filter table, one filter id per query), every repeat listed:
  * "indirection": the 50 % and 10 % bitsets as a one-row table with every id 0 against the
    per-call query_filtered of the same bitset, alternating: kernel ms;
  * "mixed": --tenants disjoint tenants of N / tenants rows, ids drawn uniformly: one
    query_filtered(filter_ids=...) call, the same batch as two query_async slots, and the only way
    without a table -- one per-call query_filtered per tenant on the queries grouped by tenant,
    host bitsets staged per call: queries/s end to end (host clock around calls that end
    synchronised, queries and ids on the GPU), recall@10 against bf_query_filtered(filter_ids=...),
    bytes staged per batch;
  * "locality": kernel ms of a mixed batch over --tenants and over --big-table random rows of
    equal density (1 / tenants), so that only the table's footprint changes.

    python scripts/filtered_bench.py --labels [--label-tenants 16 1024]

Label filters (one int32 label per base vector, one per query) against the filter table of the
same tenants on the same handle and graph; per tenant count T: T disjoint tenants of N / T rows,
query labels drawn uniformly.  Kernel ms of the mixed batch through `query_labeled` and through a
T-row table (`query_filtered_by`), alternating, every repeat listed; recall@10 of the labelled
call against `bf_query_labeled`; resident bytes per GPU of both forms.

    python scripts/filtered_bench.py --bf [--tenants 16] [--big-table 1024]

The filtered brute force alone (no graph is built): on one handle, alternating per repeat, the
time of each call under hook BF_SCAN = 1 (the scan kernels) and without it (the matrix-core tile
kernels where the dispatch takes them), every repeat listed, with the path and the rescanned
count of the matrix run: the unfiltered call, the per-call bitset at 100 / 50 / 10 / 1 % allowed,
the --tenants-row and --big-table-row filter tables, and the same tenant counts as labels.

    python scripts/filtered_bench.py --label-sets [--tenants 16]

Label sets (`query_labeled_in`) against `query_labeled` on the same handle, graph and predicate:
--tenants disjoint tenants, one label per query, width 1 and no filter ids; kernel ms of both calls,
alternating, every repeat listed.  Then one row for width 8 (eight of the tenants per query) with a
50 % bitset as the one row of the filter table, next to `query_filtered_by` of the bitset alone (a
wider predicate: the figure says what a search under the bitset costs, not what the label read adds).

    python scripts/filtered_bench.py --ranges

Label ranges (`query_labeled_range`) against label sets (`query_labeled_in`) on the same handle,
graph and masks: a label column whose values 0..7 cover 50 % of the rows, 8..15 10 % and 16..17
1 %, every query under the same mask, written once as a set of the values and once as one interval
around them; results asserted equal, then kernel ms and queries/s (host clock around calls that end
synchronised) of both calls, alternating, every repeat listed.

    python scripts/filtered_bench.py --masks

Label masks (`query_labeled_mask`) against label ranges (`query_labeled_range`) in the same way, on
the column of --ranges: the three intervals are aligned blocks of values, so each is also one clause
(mask, value, 0) on the bits above the block -- the same rows, 50 %, 10 % and 1 % of them."""
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
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--tenants", type=int, default=16)
    ap.add_argument("--big-table", type=int, default=1024)
    ap.add_argument("--labels", action="store_true")
    ap.add_argument("--label-tenants", type=int, nargs="+", default=[16, 1024])
    ap.add_argument("--bf", action="store_true")
    ap.add_argument("--label-sets", action="store_true")
    ap.add_argument("--ranges", action="store_true")
    ap.add_argument("--masks", action="store_true")
    a = ap.parse_args()
    rs = np.random.default_rng(1)
    centres = rs.normal(size=(256, a.d)).astype(np.float32) * 2
    base = centres[rs.integers(0, 256, a.n)] + rs.normal(size=(a.n, a.d)).astype(np.float32)
    query = centres[rs.integers(0, 256, a.queries)] + rs.normal(size=(a.queries, a.d)).astype(np.float32)
    g = ggnn.GGNN()
    g.set_base(torch.from_numpy(base).cuda())
    q = torch.from_numpy(query).cuda()
    if a.bf:
        brute_force(a, g, q)
        return
    g.build(24, 0.5)
    if a.mixed:
        mixed(a, g, q)
        return
    if a.labels:
        labeled(a, g, q)
        return
    if a.label_sets:
        label_sets(a, g, q)
        return
    if a.ranges:
        label_ranges(a, g, q)
        return
    if a.masks:
        label_masks(a, g, q)
        return

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


def brute_force(a, g, q):
    """scan against matrix path of the filtered brute force, alternating per repeat"""
    from ggnn_amd import _lib
    rs = np.random.default_rng(3)

    def ab(name, call, **extra):
        scan, matrix = [], []
        for _ in range(a.reps):
            with _lib.hooks(BF_SCAN=1):
                call()
            scan.append(round(g.last_timing_ms()["bf_query_ms"], 3))
            call()
            matrix.append(round(g.last_timing_ms()["bf_query_ms"], 3))
        print(json.dumps({"bf": name, **extra, "scan_ms": scan, "matrix_ms": matrix,
                          "matrix_path": g.last_bf_query_matrix_path(),
                          "rescanned": g.last_bf_query_rescanned()}), flush=True)

    ab("unfiltered", lambda: g.bf_query(q, a.k))
    for share in (1.0, 0.5, 0.1, 0.01):
        mask = np.random.default_rng(int(share * 1000)).random(a.n) < share
        bits = ggnn.pack_filter(mask).cuda()
        ab("bitset", lambda: g.bf_query_filtered(q, a.k, filter=bits), allowed=share)
    for T in (a.tenants, a.big_table):
        tenant = rs.integers(0, T, a.n).astype(np.int32)
        ids = torch.from_numpy(rs.integers(0, T, a.queries).astype(np.int32)).cuda()
        g.set_labels(tenant)
        ab("labels", lambda: g.bf_query_labeled(q, a.k, labels=ids), tenants=T)
        g.set_labels(None)
        # (the table row by row: T x N booleans at once would be a gigabyte at T = 1024)
        words = np.stack([ggnn.pack_filter(tenant == t).numpy() for t in range(T)])
        g.set_filters(torch.from_numpy(words))
        ab("table", lambda: g.bf_query_filtered_by(q, a.k, filter_ids=ids), rows=T)
        g.set_filters(None)


def mixed(a, g, q):
    import time

    def recall(ids, gt):
        ids, gt = ids.cpu().numpy(), gt.cpu().numpy()
        return float(np.mean([len(set(x[x >= 0].tolist()) & set(y[y >= 0].tolist())) /
                              max(1, int((y >= 0).sum())) for x, y in zip(ids, gt)]))

    def kernel_ms(fn):
        fn()
        return g.last_timing_ms()["query_ms"]

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    words = (a.n + 31) // 32
    # ---- cost of the indirection ----------------------------------------------------------------
    for share in (0.5, 0.1):
        mask = np.random.default_rng(int(share * 1000)).random(a.n) < share
        bits = ggnn.pack_filter(mask).cuda()
        g.set_filters(bits[None, :])
        zero = torch.zeros(a.queries, dtype=torch.int32, device="cuda")
        per_call = lambda: g.query_filtered(q, a.k, a.tau, a.iters, filter=bits)  # noqa: E731
        by_id = lambda: g.query_filtered_by(q, a.k, a.tau, a.iters, filter_ids=zero)  # noqa: E731
        x, y = per_call(), by_id()
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        ms = {"per_call": [], "table": []}
        for _ in range(a.reps):                               # alternating
            ms["per_call"].append(round(kernel_ms(per_call), 4))
            ms["table"].append(round(kernel_ms(by_id), 4))
        print(json.dumps({"indirection": share, "kernel_ms": ms}), flush=True)

    # ---- what the feature buys ------------------------------------------------------------------
    F = a.tenants
    rs = np.random.default_rng(7)
    tenant = torch.from_numpy(rs.permutation(a.n) % F).cuda()        # disjoint, N / F rows each
    masks = tenant[None, :] == torch.arange(F, device="cuda")[:, None]
    table = ggnn.pack_filters(masks)
    g.set_filters(table)
    fids_h = rs.integers(0, F, a.queries).astype(np.int32)
    fids = torch.from_numpy(fids_h).cuda()
    host_bits = [table[f].cpu() for f in range(F)]
    groups = [q[torch.from_numpy(np.nonzero(fids_h == f)[0]).cuda()].contiguous() for f in range(F)]
    half = a.queries // 2
    parts = [(q[:half], fids[:half]), (q[half:], fids[half:])]

    def one_call():
        return g.query_filtered_by(q, a.k, a.tau, a.iters, filter_ids=fids)

    def two_slots():
        t = [g.query_async(x, a.k, a.tau, a.iters, slot=i, filter_ids=f)
             for i, (x, f) in enumerate(parts)]
        g.synchronize()
        return t

    def per_tenant():
        return [g.query_filtered(groups[f], a.k, a.tau, a.iters, filter=host_bits[f])
                for f in range(F)]

    gt, _ = g.bf_query_filtered_by(q, a.k, filter_ids=fids)
    ids, _ = one_call()
    grouped = per_tenant()
    ids_grouped = torch.empty_like(ids)
    for f in range(F):
        ids_grouped[torch.from_numpy(np.nonzero(fids_h == f)[0])] = grouped[f][0]
    t = two_slots()
    ids_async = torch.cat([t[0].ids, t[1].ids])[:, :a.k].cpu()
    rows = {"one_call": (one_call, ids, 0),
            "two_async_slots": (two_slots, ids_async, 0),
            "per_tenant_calls": (per_tenant, ids_grouped, F * words * 4)}
    secs = {k: [] for k in rows}
    for _ in range(a.reps):                                   # alternating
        for k, (fn, _, _) in rows.items():
            secs[k].append(wall(fn))
    for k, (fn, r_ids, staged) in rows.items():
        print(json.dumps({"mixed": k, "tenants": F,
                          "queries_per_s": [round(a.queries / s) for s in secs[k]],
                          "recall": round(recall(r_ids, gt), 4),
                          "bytes_staged_per_batch": staged}), flush=True)

    # ---- table locality -------------------------------------------------------------------------
    for rows_f in (F, a.big_table):
        rs = np.random.default_rng(rows_f)
        tab = torch.empty((rows_f, words), dtype=torch.int32, device="cuda")
        for r0 in range(0, rows_f, 64):                       # random rows of density 1 / F
            n_r = min(64, rows_f - r0)
            m = torch.rand((n_r, a.n), device="cuda") < 1.0 / F
            tab[r0:r0 + n_r] = ggnn.pack_filters(m)
        g.set_filters(tab)
        ids_r = torch.from_numpy(rs.integers(0, rows_f, a.queries).astype(np.int32)).cuda()
        call = lambda: g.query_filtered_by(q, a.k, a.tau, a.iters, filter_ids=ids_r)  # noqa: E731
        call()
        print(json.dumps({"locality": rows_f, "table_mb": round(rows_f * words * 4 / 2 ** 20, 2),
                          "kernel_ms": [round(kernel_ms(call), 4) for _ in range(a.reps)]}),
              flush=True)


def labeled(a, g, q):
    words = (a.n + 31) // 32
    for T in a.label_tenants:
        rs = np.random.default_rng(T)
        tenant = torch.from_numpy((rs.permutation(a.n) % T).astype(np.int32)).cuda()
        qlab = torch.from_numpy(rs.integers(0, T, a.queries).astype(np.int32)).cuda()
        g.set_labels(tenant)
        table = torch.empty((T, words), dtype=torch.int32, device="cuda")
        for r0 in range(0, T, 64):                            # [64, N] masks at a time
            rows = torch.arange(r0, min(T, r0 + 64), device="cuda", dtype=torch.int32)
            table[r0:r0 + len(rows)] = ggnn.pack_filters(tenant[None, :] == rows[:, None])
        g.set_filters(table)
        by_label = lambda: g.query_labeled(q, a.k, a.tau, a.iters, labels=qlab)  # noqa: E731
        by_table = lambda: g.query_filtered_by(q, a.k, a.tau, a.iters, filter_ids=qlab)  # noqa: E731
        x, y = by_label(), by_table()
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        ms = {"labels": [], "table": []}
        for _ in range(a.reps):                               # alternating
            by_label()
            ms["labels"].append(round(g.last_timing_ms()["query_ms"], 4))
            by_table()
            ms["table"].append(round(g.last_timing_ms()["query_ms"], 4))
        gt, _ = g.bf_query_labeled(q, a.k, labels=qlab)
        bf_ms = g.last_timing_ms()["bf_query_ms"]
        ids, gt = x[0].cpu().numpy(), gt.cpu().numpy()
        rec = float(np.mean([len(set(u[u >= 0].tolist()) & set(v[v >= 0].tolist())) /
                             max(1, int((v >= 0).sum())) for u, v in zip(ids, gt)]))
        print(json.dumps({"labels": T, "kernel_ms": ms, "recall": round(rec, 4),
                          "bf_labeled_ms": round(bf_ms, 3),
                          "resident_bytes": {"labels": 4 * a.n, "table": (T + 2) * words * 4}}),
              flush=True)
        g.set_filters(None)
        g.set_labels(None)


def label_sets(a, g, q):
    T = a.tenants
    rs = np.random.default_rng(T)
    tenant = torch.from_numpy((rs.permutation(a.n) % T).astype(np.int32)).cuda()
    qlab = torch.from_numpy(rs.integers(0, T, a.queries).astype(np.int32)).cuda()
    g.set_labels(tenant)

    def ab(name, calls, **extra):
        outs = {k: fn() for k, fn in calls.items()}
        ms = {k: [] for k in calls}
        for _ in range(a.reps):                               # alternating
            for k, fn in calls.items():
                fn()
                ms[k].append(round(g.last_timing_ms()["query_ms"], 4))
        print(json.dumps({"label_sets": name, **extra, "kernel_ms": ms}), flush=True)
        return outs

    one = qlab[:, None].contiguous()
    o = ab("width 1, no ids", {
        "query_labeled": lambda: g.query_labeled(q, a.k, a.tau, a.iters, labels=qlab),
        "query_labeled_in": lambda: g.query_labeled_in(q, a.k, a.tau, a.iters, label_sets=one)},
        tenants=T)
    x, y = o["query_labeled"], o["query_labeled_in"]
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    # width 8 with a 50 % bitset: eight distinct tenants per query
    w = min(8, T)
    sets = np.stack([rs.choice(T, w, replace=False) for _ in range(a.queries)]).astype(np.int32)
    sets = torch.from_numpy(sets).cuda()
    bits = ggnn.pack_filter(np.random.default_rng(500).random(a.n) < 0.5).cuda()
    g.set_filters(bits[None, :])
    zero = torch.zeros(a.queries, dtype=torch.int32, device="cuda")
    ab(f"width {w}, 50 % bitset", {
        "query_labeled_in": lambda: g.query_labeled_in(q, a.k, a.tau, a.iters, label_sets=sets,
                                                       filter_ids=zero),
        "query_filtered_by (bitset alone)": lambda: g.query_filtered_by(q, a.k, a.tau, a.iters,
                                                                        filter_ids=zero)},
       tenants=T, allowed_share=round(0.5 * w / T, 4))
    g.set_filters(None)
    g.set_labels(None)


def label_ranges(a, g, q):
    import time
    rs = np.random.default_rng(19)
    # values 0..7: 6.25 % of the rows each, 8..15: 1.25 % each, 16..17: 0.5 % each, 18: the rest
    p = np.array([0.0625] * 8 + [0.0125] * 8 + [0.005] * 2 + [0.39])
    column = rs.choice(len(p), a.n, p=p / p.sum()).astype(np.int32)
    g.set_labels(torch.from_numpy(column).cuda())
    for name, lo, hi in (("50 %", 0, 7), ("10 %", 8, 15), ("1 %", 16, 17)):
        values = list(range(lo, hi + 1))
        sets = torch.tensor([values] * a.queries, dtype=torch.int32).cuda()
        ranges = torch.tensor([[[lo, hi]]] * a.queries, dtype=torch.int32).cuda()
        calls = {"query_labeled_in": lambda: g.query_labeled_in(q, a.k, a.tau, a.iters, label_sets=sets),
                 "query_labeled_range": lambda: g.query_labeled_range(q, a.k, a.tau, a.iters,
                                                                      label_ranges=ranges)}
        x, y = (fn() for fn in calls.values())
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        ms, qps = {k: [] for k in calls}, {k: [] for k in calls}
        for _ in range(a.reps):                               # alternating
            for k, fn in calls.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                qps[k].append(round(a.queries / (time.perf_counter() - t)))
                ms[k].append(round(g.last_timing_ms()["query_ms"], 4))
        print(json.dumps({"ranges": name, "labels": values, "interval": [lo, hi],
                          "allowed": int(((column >= lo) & (column <= hi)).sum()),
                          "kernel_ms": ms, "queries_per_s": qps}), flush=True)
    g.set_labels(None)


def label_masks(a, g, q):
    import time
    rs = np.random.default_rng(19)
    # the column of label_ranges: values 0..7 6.25 % of the rows each, 8..15 1.25 %, 16..17 0.5 %
    p = np.array([0.0625] * 8 + [0.0125] * 8 + [0.005] * 2 + [0.39])
    column = rs.choice(len(p), a.n, p=p / p.sum()).astype(np.int32)
    g.set_labels(torch.from_numpy(column).cuda())
    for name, lo, hi in (("50 %", 0, 7), ("10 %", 8, 15), ("1 %", 16, 17)):
        clause = (~(hi - lo), lo, 0)                          # the bits above an aligned block
        assert lo & (hi - lo) == 0 and (hi - lo) & (hi - lo + 1) == 0
        ranges = torch.tensor([[[lo, hi]]] * a.queries, dtype=torch.int32).cuda()
        masks = torch.tensor([[clause]] * a.queries, dtype=torch.int32).cuda()
        calls = {"query_labeled_range": lambda: g.query_labeled_range(q, a.k, a.tau, a.iters,
                                                                      label_ranges=ranges),
                 "query_labeled_mask": lambda: g.query_labeled_mask(q, a.k, a.tau, a.iters,
                                                                    label_masks=masks)}
        x, y = (fn() for fn in calls.values())
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        ms, qps = {k: [] for k in calls}, {k: [] for k in calls}
        for _ in range(a.reps):                               # alternating
            for k, fn in calls.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                qps[k].append(round(a.queries / (time.perf_counter() - t)))
                ms[k].append(round(g.last_timing_ms()["query_ms"], 4))
        print(json.dumps({"masks": name, "interval": [lo, hi], "clause": list(clause),
                          "allowed": int(((column & clause[0]) == clause[1]).sum()),
                          "kernel_ms": ms, "queries_per_s": qps}), flush=True)
    g.set_labels(None)


if __name__ == "__main__":
    main()
