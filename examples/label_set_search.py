"""Label sets with a bitset: a tenant's rows in any of three categories, minus the deleted rows.

    python examples/label_set_search.py

The label column (examples/labeled_search.py) holds one int32 per base vector; here it encodes the
tenant and the category of a row.  A query names up to eight labels -- "this tenant, categories 2, 5
or 7" is three of them -- and, independently, a row of the resident filter table
(examples/multi_tenant_search.py): the tombstones.  Both are checked inside one traversal; neither
costs a table row per combination.
"""
import numpy as np
import torch

import ggnn_amd as ggnn

N, D, K, TENANTS, CATEGORIES = 100_000, 64, 10, 40, 8
rng = np.random.default_rng(0)
base = rng.normal(size=(N, D)).astype(np.float32)
query = rng.normal(size=(1000, D)).astype(np.float32)
tenant = rng.integers(0, TENANTS, N)
category = rng.integers(0, CATEGORIES, N)
label_of_row = (tenant * CATEGORIES + category).astype(np.int32)     # the label column
alive = rng.random(N) > 0.1                                          # 10 % of the rows are deleted

g = ggnn.GGNN()
g.set_base(base)
g.set_labels(label_of_row)
g.set_filters(alive[None, :])            # one row: the tombstones, shared by every tenant
g.build(24, 0.5)

# every query: its tenant, three categories (ragged lists work too: see the admin below)
asking = rng.integers(0, TENANTS, len(query))
wanted = np.stack([rng.choice(CATEGORIES, 3, replace=False) for _ in query])
label_sets = (asking[:, None] * CATEGORIES + wanted).astype(np.int32)           # [Nq, 3]
not_deleted = np.zeros(len(query), np.int32)                                    # row 0 of the table

ids, dists = g.query_labeled_in(query, K, 0.7, 800, label_sets=label_sets, filter_ids=not_deleted)
gt, _ = g.bf_query_labeled_in(query, K, label_sets=label_sets, filter_ids=not_deleted)
ids_n, gt_n = ids.numpy(), gt.numpy()
found = ids_n >= 0
rows = np.where(found, ids_n, 0)
ok = (label_of_row[rows][:, :, None] == label_sets[:, None, :]).any(2) & alive[rows]
assert ok[found].all()
recall = np.mean([len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) / max(1, (b >= 0).sum())
                  for a, b in zip(ids_n, gt_n)])
print(f"{len(query)} queries, tenant and 3 of {CATEGORIES} categories, tombstones applied: "
      f"recall@{K} = {recall:.3f}")

# ragged sets in one batch: one category, two categories, and an admin (-1: every label) who still
# does not see deleted rows
mixed = [[int(label_sets[0, 0])], label_sets[1, :2].tolist(), [-1]]
m_ids, _ = g.query_labeled_in(query[:3], K, 0.7, 800, label_sets=mixed, filter_ids=not_deleted[:3])
assert alive[m_ids.numpy()[m_ids.numpy() >= 0]].all()
print("ragged sets:", [len(s) for s in mixed], "entries, padded by repetition")

# the same on two asynchronous slots
q_gpu = torch.from_numpy(query).cuda()
half = len(query) // 2
t0 = g.query_async_labeled_in(q_gpu[:half], K, 0.7, 800, slot=0, label_sets=label_sets[:half],
                              filter_ids=not_deleted[:half])
t1 = g.query_async_labeled_in(q_gpu[half:], K, 0.7, 800, slot=1, label_sets=label_sets[half:],
                              filter_ids=not_deleted[half:])
g.synchronize()
assert torch.equal(torch.cat([t0.ids, t1.ids])[:, :K].cpu(), ids)
print("two asynchronous slots: same result")

# deleting a row rewrites one bitset row; the labels stay as they are
n = int(np.nonzero(found[:, 0])[0][0])
row = int(ids_n[n, 0])
alive[row] = False
g.update_filter(0, alive)
after, _ = g.query_labeled_in(query[n:n + 1], K, 0.7, 800, label_sets=label_sets[n:n + 1],
                              filter_ids=not_deleted[:1])
assert row not in after.numpy()
print(f"row {row} deleted: gone from the results of query {n}")
