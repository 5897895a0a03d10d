"""Time windows of very different width: narrow ones exactly through the label index, the rest through
the graph.

    python examples/label_index_range_search.py

The label column (examples/label_range_search.py) is the row's creation time.  A window of a few
minutes admits a handful of rows: the traversal of such a query runs to max_iterations, and the exact
scan reads the whole base for it.  The label index (ops.label_index_build) holds the row ids sorted by
(label, id), so a closed interval of labels is ONE contiguous run of positions in it:
ops.label_spans_resolve turns every query's intervals into such runs and says how many rows they
hold, ops.label_spans_classify splits the batch at a cutoff, ops.bf_query_label_spans answers the
narrow queries exactly from their own rows -- bit for bit what ops.bf_query_labeled_range gives --
and ops.query_labeled_range searches the graph for the wide ones.  Everything here is the operator
seam: the handle only builds the graph.
"""
import numpy as np
import torch

import ggnn_amd as ggnn
from ggnn_amd import ops

N, D, K, NQ = 100_000, 64, 10, 1000
DAY, NOW = 86_400, 1_700_000_000
CUTOFF = 2_000                                   # rows; see DESIGN.md 4.9 for what is measured
rng = np.random.default_rng(0)
base = rng.normal(size=(N, D)).astype(np.float32)
query = rng.normal(size=(NQ, D)).astype(np.float32)
created = (NOW - rng.integers(0, 30 * DAY, N)).astype(np.int32)      # the last 30 days

g = ggnn.GGNN()
g.set_base(base)
g.build(24, 0.5)
graph = g.get_graph(0)
d_graph0 = torch.from_numpy(np.ascontiguousarray(graph.graph[0].view.numpy()).reshape(N, -1)).cuda()
d_start = torch.from_numpy(np.ascontiguousarray(graph.translation[3].view.numpy()).reshape(-1)).cuda()
d_stats = torch.from_numpy(np.ascontiguousarray(graph.nn1_stats.view.numpy()).reshape(-1)).cuda()

d_base, d_query = torch.from_numpy(base).cuda(), torch.from_numpy(query).cuda()
d_created = torch.from_numpy(created).cuda()
keys, offsets, rows = (t.cuda() for t in ops.label_index_build(created))     # 4 N + 8 L + 4 bytes

# every query: one window ending now -- ten minutes, an hour, a day or a week wide
width = rng.choice([600, 3_600, DAY, 7 * DAY], NQ)
windows = np.stack([NOW - width, np.full(NQ, NOW)], 1).astype(np.int32)[:, None, :]     # [Nq, 1, 2]
d_windows = torch.from_numpy(windows).cuda()

spans, totals = ops.label_spans_resolve(keys, offsets, label_ranges=d_windows)
routed, rest = ops.label_spans_classify(totals, CUTOFF)             # both in ascending query order
routed, rest = routed.long(), rest.long()
print(f"{NQ} windows: {routed.numel()} of at most {CUTOFF} rows through the index, "
      f"{rest.numel()} through the graph")

ids = torch.empty((NQ, K), dtype=torch.int32, device="cuda")
dists = torch.empty((NQ, K), dtype=torch.float32, device="cuda")
if routed.numel():
    ids[routed], dists[routed] = ops.bf_query_label_spans(
        d_base, d_query[routed].contiguous(), K, rows, spans[routed].contiguous(), span_limit=CUTOFF)
if rest.numel():
    ids[rest], dists[rest] = ops.query_labeled_range(
        d_base, d_query[rest].contiguous(), d_graph0, d_start, d_stats, K, 0.7, d_created,
        d_windows[rest].contiguous(), max_iterations=800)

# the exact answer of the whole batch: the scan of the label column
gt, gt_d = ops.bf_query_labeled_range(d_base, d_query, K, d_created, d_windows)
assert torch.equal(ids[routed], gt[routed]) and torch.equal(dists[routed], gt_d[routed])
ids_n, gt_n = ids.cpu().numpy(), gt.cpu().numpy()
found = ids_n >= 0
t = created[np.where(found, ids_n, 0)]
assert ((t >= windows[:, 0, :1]) & (t <= windows[:, 0, 1:]))[found].all()
rest_n = rest.cpu().numpy()
recall = np.mean([len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) / max(1, (b >= 0).sum())
                  for a, b in zip(ids_n[rest_n], gt_n[rest_n])]) if len(rest_n) else 1.0
print(f"narrow windows: exact, bit for bit the scan's result; wide windows: recall@{K} = {recall:.3f}")

# label sets go the same way: any of up to eight labels is at most eight runs
some_days = torch.from_numpy(rng.choice(created, (4, 3)).astype(np.int32)).cuda()     # three timestamps
s_ids, s_d = ops.bf_query_label_index_in(d_base, d_query[:4].contiguous(), K, keys, offsets, rows,
                                         some_days)
w_ids, w_d = ops.bf_query_labeled_in(d_base, d_query[:4].contiguous(), K, d_created, some_days)
assert torch.equal(s_ids, w_ids) and torch.equal(s_d, w_d)
print("label sets through the index: same result as the scan")
