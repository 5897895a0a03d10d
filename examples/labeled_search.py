"""Label filters: a tenant column on the base, one tenant per query.

    python examples/labeled_search.py

The engine keeps ONE int32 label per base vector on every GPU it drives (4 * N bytes, however many
tenants there are -- a filter table, examples/multi_tenant_search.py, costs N / 8 bytes per
tenant) and every query carries the label it may see.  A mixed batch is one call, blocking or on
the asynchronous slots; label -1 searches unfiltered; moving a row to another tenant rewrites one
label.
"""
import numpy as np
import torch

import ggnn_amd as ggnn

N, D, K, TENANTS = 100_000, 64, 10, 500
rng = np.random.default_rng(0)
base = rng.normal(size=(N, D)).astype(np.float32)
query = rng.normal(size=(1000, D)).astype(np.float32)
tenant_of_row = rng.integers(0, TENANTS, N).astype(np.int32)               # the label column
tenant_of_query = rng.integers(0, TENANTS, len(query)).astype(np.int32)    # who is asking
tenant_of_query[::50] = -1                                                 # an admin: sees everything

g = ggnn.GGNN()
g.set_base(base)
g.set_labels(tenant_of_row)
g.build(24, 0.5)
print(f"{g.num_labels} labels resident ({4 * N / 2 ** 20:.1f} MiB; a table of {TENANTS} bitsets "
      f"would be {TENANTS * N / 8 / 2 ** 20:.1f} MiB)")

# one mixed batch, blocking
ids, dists = g.query_labeled(query, K, 0.7, 800, labels=tenant_of_query)
gt, _ = g.bf_query_labeled(query, K, labels=tenant_of_query)
found = ids.numpy() >= 0
mine = (tenant_of_row[ids.numpy()] == tenant_of_query[:, None]) | (tenant_of_query[:, None] == -1)
assert mine[found].all()
recall = np.mean([len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) / max(1, (b >= 0).sum())
                  for a, b in zip(ids.numpy(), gt.numpy())])
print(f"mixed batch of {len(query)} queries over {TENANTS} tenants: recall@{K} = {recall:.3f}")

# the same batch as two halves in flight on two slots
q_gpu = torch.from_numpy(query).cuda()
l_gpu = torch.from_numpy(tenant_of_query).cuda()
half = len(query) // 2
t0 = g.query_async_labeled(q_gpu[:half], K, 0.7, 800, slot=0, labels=l_gpu[:half])
t1 = g.query_async_labeled(q_gpu[half:], K, 0.7, 800, slot=1, labels=l_gpu[half:])
g.synchronize()
assert torch.equal(torch.cat([t0.ids, t1.ids])[:, :K].cpu(), ids)
print("two asynchronous slots: same result")

# a row moves from its tenant to tenant 7: one label is rewritten on every GPU
n = int(np.nonzero(tenant_of_query >= 0)[0][0])
row, old = int(ids[n, 0]), int(tenant_of_query[n])
g.update_labels(np.array([row]), np.array([7]))
after, _ = g.query_labeled(query[n:n + 1], K, 0.7, 800, labels=np.array([old], np.int32))
assert old == 7 or row not in after.numpy()
seen, _ = g.query_labeled(query[n:n + 1], K, 0.7, 800, labels=np.array([7], np.int32))
print(f"row {row} moved from tenant {old} to tenant 7: gone from {old}'s results, "
      f"{'in' if row in seen.numpy() else 'not among'} the {K} nearest of tenant 7")
