"""Filtered serving: nearest neighbours among the rows a tenant may see.

    python examples/filtered_search.py

One allowed-id bitset per call, shared by the queries of the batch.  Denied rows still route the
search (the graph stays connected under any filter) but are never returned; slots that could not
be filled hold id -1 and distance +inf.  For very selective filters the exact filtered brute
force is the better call.
"""
import numpy as np
import torch

import ggnn_amd as ggnn

N, D, K = 100_000, 64, 10
rng = np.random.default_rng(0)
base = rng.normal(size=(N, D)).astype(np.float32)
query = rng.normal(size=(1000, D)).astype(np.float32)
tenant = rng.integers(0, 8, N)                      # eight tenants share the index

g = ggnn.GGNN()
g.set_base(base)
g.build(24, 0.5)

mask = tenant == 3                                  # boolean mask over the base ids ...
bits = ggnn.pack_filter(mask).cuda()                # ... or packed once and kept on the GPU
ids, dists = g.query_filtered(query, K, 0.7, 800, filter=bits)
gt, _ = g.bf_query_filtered(query, K, filter=bits)
assert mask[ids[ids >= 0].numpy()].all()
recall = np.mean([len(set(a.tolist()) & set(b.tolist())) / K for a, b in zip(ids, gt)])
print(f"tenant 3: {int(mask.sum())} of {N} rows allowed, recall@{K} = {recall:.3f}")
