"""Multi-tenant serving: one batch whose queries belong to different tenants.

    python examples/multi_tenant_search.py

A label column becomes a filter table (one bitset per tenant, packed on the GPU and kept there by
the engine); every query then carries the id of its tenant's row, so a mixed batch is ONE call --
blocking, or enqueued on the asynchronous slots like any other batch.  Id -1 searches unfiltered.
"""
import numpy as np
import torch

import ggnn_amd as ggnn

N, D, K, TENANTS = 100_000, 64, 10, 8
rng = np.random.default_rng(0)
base = rng.normal(size=(N, D)).astype(np.float32)
query = rng.normal(size=(1000, D)).astype(np.float32)
tenant_of_row = torch.from_numpy(rng.integers(0, TENANTS, N)).cuda()      # the label column
tenant_of_query = rng.integers(0, TENANTS, len(query)).astype(np.int32)   # who is asking

g = ggnn.GGNN()
g.set_base(base)
g.build(24, 0.5)

# label column -> [TENANTS, N] masks -> [TENANTS, ceil(N / 32)] words, all on the GPU
masks = tenant_of_row[None, :] == torch.arange(TENANTS, device="cuda")[:, None]
g.set_filters(ggnn.pack_filters(masks))
print(f"{g.num_filters} filters resident")

# one mixed batch, blocking
ids, dists = g.query_filtered_by(query, K, 0.7, 800, filter_ids=tenant_of_query)
gt, _ = g.bf_query_filtered_by(query, K, filter_ids=tenant_of_query)
rows = tenant_of_row.cpu().numpy()
assert (rows[ids.numpy()] == tenant_of_query[:, None])[ids.numpy() >= 0].all()
recall = np.mean([len(set(a.tolist()) & set(b.tolist())) / K for a, b in zip(ids, gt)])
print(f"mixed batch of {len(query)} queries over {TENANTS} tenants: recall@{K} = {recall:.3f}")

# the same batch as two halves in flight on two slots
q_gpu = torch.from_numpy(query).cuda()
f_gpu = torch.from_numpy(tenant_of_query).cuda()
half = len(query) // 2
t0 = g.query_async(q_gpu[:half], K, 0.7, 800, slot=0, filter_ids=f_gpu[:half])
t1 = g.query_async(q_gpu[half:], K, 0.7, 800, slot=1, filter_ids=f_gpu[half:])
g.synchronize()
assert torch.equal(torch.cat([t0.ids, t1.ids])[:, :K].cpu(), ids)
print("two asynchronous slots: same result")

# rows deleted since the build: replace one tenant's row
alive = masks[3].clone()
alive[::2] = False
g.update_filter(3, alive.cpu())
