"""Exact range search: near-duplicate detection on a small synthetic base.

    python examples/range_search.py

`bf_query` answers "the k nearest"; `bf_range_query` answers "EVERYTHING within this radius", however
many that is -- the call for de-duplication, thresholded retrieval and density passes.  The result is
CSR-shaped: the matches of query n are ids[lims[n]:lims[n + 1]].

Under the Euclidean measure every distance of this engine is a SQUARED L2 distance, and so is the
radius: to find everything within Euclidean distance r, pass r * r.
"""
import numpy as np

import ggnn_amd as ggnn

N, D, DUPES = 50_000, 64, 300
rng = np.random.default_rng(0)
base = rng.normal(size=(N, D)).astype(np.float32)
# plant near-duplicates: row N - DUPES + i is row i plus a little noise
base[N - DUPES:] = base[:DUPES] + 0.01 * rng.normal(size=(DUPES, D)).astype(np.float32)

g = ggnn.GGNN()
g.set_base(base)                       # no graph needed: the exact search scans the base

# every row queries the base; a near-duplicate lies within Euclidean distance 0.2 (random rows of
# this base are about sqrt(2 * D) = 11 apart)
r = 0.2
query = base[:2000]
lims, ids, dists = g.bf_range_query(query, r * r)            # squared units
counts = np.diff(lims.numpy())
# every row matches itself at distance 0 and comes first (sorted by distance, then id)
assert (ids.numpy()[lims.numpy()[:-1]] == np.arange(len(query))).all()
dup_of = {n: ids[lims[n] + 1:lims[n + 1]].tolist() for n in np.nonzero(counts > 1)[0]}
assert set(dup_of) == set(range(DUPES)) and all(v == [N - DUPES + n] for n, v in dup_of.items())
print(f"{len(query)} rows checked: {len(dup_of)} have a near-duplicate within distance {r}, "
      f"{int(lims[-1])} matches in all")

# one radius per query, engine order (ascending id), and a caller-sized buffer: one call, and an
# error that names the needed size if it is too small
radii = np.full(len(query), r * r, np.float32)
radii[::2] = 0.0                                             # exact duplicates only: the row itself
lims, ids, dists = g.bf_range_query(query, radii, max_results=4000, sort=False)
assert (np.diff(lims.numpy())[::2] == 1).all()
try:
    g.bf_range_query(query, 150.0, max_results=10_000)       # half of the base per query: too many
except RuntimeError as e:
    print("too small a buffer:", e)

# count only, at the operator seam: how dense is the neighbourhood of each row?
import torch
from ggnn_amd import ops
b = torch.from_numpy(base).cuda()
lims, _, _ = ops.bf_range_query(b, b[:2000].contiguous(), 100.0, capacity=0)
print("rows within squared distance 100 of a row: median",
      int(torch.diff(lims).median()), "max", int(torch.diff(lims).max()))
