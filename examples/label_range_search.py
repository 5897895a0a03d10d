"""Label ranges with a bitset: a tenant's rows of the last seven days, or pinned ones.

    python examples/label_range_search.py

The label column (examples/labeled_search.py) holds one int32 per base vector; here it is the row's
creation time in seconds, and pinned rows carry a time far in the future.  A query names up to four
closed intervals of that column -- "created in the last 7 days, or pinned" is two of them -- and,
independently, a row of the resident filter table (examples/multi_tenant_search.py): its tenant.
Both are checked inside one traversal; a moving bound costs eight int32 per query and no bitset.
"""
import numpy as np
import torch

import ggnn_amd as ggnn

N, D, K, TENANTS = 100_000, 64, 10, 4
DAY, NOW, PINNED = 86_400, 1_700_000_000, 2_000_000_000
rng = np.random.default_rng(0)
base = rng.normal(size=(N, D)).astype(np.float32)
query = rng.normal(size=(1000, D)).astype(np.float32)
created = (NOW - rng.integers(0, 30 * DAY, N)).astype(np.int32)      # the last 30 days
pinned = rng.random(N) < 0.02
created[pinned] = PINNED
tenant = rng.integers(0, TENANTS, N)

g = ggnn.GGNN()
g.set_base(base)
g.set_labels(created)                                                # the timestamp column
g.set_filters(tenant[None, :] == np.arange(TENANTS)[:, None])        # one row per tenant
g.build(24, 0.5)

# every query: its tenant, and two intervals -- the last seven days, or pinned
asking = rng.integers(0, TENANTS, len(query)).astype(np.int32)
recent_or_pinned = np.tile(np.array([[NOW - 7 * DAY, NOW], [PINNED, PINNED]], np.int32),
                           (len(query), 1, 1))                       # [Nq, 2, 2]

ids, dists = g.query_labeled_range(query, K, 0.7, 800, label_ranges=recent_or_pinned,
                                   filter_ids=asking)
gt, _ = g.bf_query_labeled_range(query, K, label_ranges=recent_or_pinned, filter_ids=asking)
ids_n, gt_n = ids.numpy(), gt.numpy()
found = ids_n >= 0
rows = np.where(found, ids_n, 0)
t = created[rows]
ok = (((t >= NOW - 7 * DAY) & (t <= NOW)) | (t == PINNED)) & (tenant[rows] == asking[:, None])
assert ok[found].all()
recall = np.mean([len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) / max(1, (b >= 0).sum())
                  for a, b in zip(ids_n, gt_n)])
print(f"{len(query)} queries, own tenant, last 7 days or pinned: recall@{K} = {recall:.3f}")

# ragged lists in one batch: one interval, two, and an open bound written with the ends of int32;
# a shorter list is padded with an empty interval (lo > hi), which admits nothing
mixed = [[(NOW - DAY, NOW)], [(NOW - 7 * DAY, NOW), (PINNED, PINNED)], [(NOW - 30 * DAY, 2 ** 31 - 1)]]
m_ids, _ = g.query_labeled_range(query[:3], K, 0.7, 800, label_ranges=mixed, filter_ids=asking[:3])
m = m_ids.numpy()
assert (created[m[0][m[0] >= 0]] >= NOW - DAY).all() and (created[m[2][m[2] >= 0]] >= NOW - 30 * DAY).all()
print("ragged lists:", [len(r) for r in mixed], "intervals, padded with an empty one")

# the same on two asynchronous slots
q_gpu = torch.from_numpy(query).cuda()
half = len(query) // 2
t0 = g.query_async_labeled_range(q_gpu[:half], K, 0.7, 800, slot=0,
                                 label_ranges=recent_or_pinned[:half], filter_ids=asking[:half])
t1 = g.query_async_labeled_range(q_gpu[half:], K, 0.7, 800, slot=1,
                                 label_ranges=recent_or_pinned[half:], filter_ids=asking[half:])
g.synchronize()
assert torch.equal(torch.cat([t0.ids, t1.ids])[:, :K].cpu(), ids)
print("two asynchronous slots: same result")

# unpinning a row rewrites one label; no bitset is rebuilt
n, j = np.argwhere(found & (created[rows] == PINNED))[0]
row = int(ids_n[n, j])
g.update_labels(np.array([row]), np.array([NOW - 30 * DAY], np.int32))
after, _ = g.query_labeled_range(query[n:n + 1], K, 0.7, 800, label_ranges=recent_or_pinned[n:n + 1],
                                 filter_ids=asking[n:n + 1])
assert row not in after.numpy()
print(f"row {row} unpinned and a month old: gone from the results of query {n}")

# a float attribute: map it to int32 in the same order first
price = rng.gamma(2.0, 20.0, N).astype(np.float32)
g.set_labels(ggnn.ordered_int32(price))
band = [[(ggnn.ordered_int32(10.0), ggnn.ordered_int32(25.0))]] * 3
p_ids, _ = g.query_labeled_range(query[:3], K, 0.7, 800, label_ranges=band)
p = price[p_ids.numpy()[p_ids.numpy() >= 0]]
assert ((p >= 10.0) & (p <= 25.0)).all()
print(f"price band 10..25: {len(p)} results, all inside")
