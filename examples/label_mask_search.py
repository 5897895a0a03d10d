"""Label masks: a document visible to several groups, a "deleted" flag, and "mine or public".

    python examples/label_mask_search.py

The label column (examples/labeled_search.py) holds one int32 per base vector; here it is read as 32
tag bits, so a row belongs to as many groups as it has bits.  Bits 0..15 are access groups, bits
16..23 the owner's id, bit 30 says "public" and bit 31 "deleted".  A query carries one or two clauses
(mask, value, any): a row passes a clause iff (label & mask) == value and (any == 0 or
(label & any) != 0), and the query is given the rows that pass one of its clauses.
`ggnn.label_mask` writes a clause from sets of bits.  Granting a group rewrites one label; no bitset
is rebuilt.
"""
import numpy as np
import torch

import ggnn_amd as ggnn

N, D, K, GROUPS = 100_000, 64, 10, 16
OWNER_SHIFT, OWNER_FIELD = 16, 0xff << 16
PUBLIC, DELETED = 1 << 30, 0x80000000
rng = np.random.default_rng(0)
base = rng.normal(size=(N, D)).astype(np.float32)
query = rng.normal(size=(1000, D)).astype(np.float32)
groups = np.zeros(N, np.int64)
for b in range(GROUPS):                                               # each group sees about 15 %
    groups |= (rng.random(N) < 0.15).astype(np.int64) << b
owner = rng.integers(0, 200, N)
label = groups | (owner << OWNER_SHIFT)
label[rng.random(N) < 0.05] |= PUBLIC
label[rng.random(N) < 0.03] |= DELETED
column = label.astype(np.uint32).view(np.int32)                       # bit 31 set: a negative int32

g = ggnn.GGNN()
g.set_base(base)
g.set_labels(column)
g.build(24, 0.5)


def rows_of(ids):
    found = ids >= 0
    return found, label[np.where(found, ids, 0)]


# every query: a user who is in two groups; not deleted, visible to either group
mine = np.array([(1 << a) | (1 << b) for a, b in rng.integers(0, GROUPS, (len(query), 2))])
visible = [[ggnn.label_mask(none_of=DELETED, any_of=int(m))] for m in mine]
ids, dists = g.query_labeled_mask(query, K, 0.7, 800, label_masks=visible)
gt, _ = g.bf_query_labeled_mask(query, K, label_masks=visible)
ids_n, gt_n = ids.numpy(), gt.numpy()
found, lab = rows_of(ids_n)
assert (((lab & DELETED) == 0) & ((lab & mine[:, None]) != 0))[found].all()
recall = np.mean([len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) / max(1, (b >= 0).sum())
                  for a, b in zip(ids_n, gt_n)])
print(f"{len(query)} queries, visible to one of the user's groups, not deleted: recall@{K} = {recall:.3f}")

# "mine or public": two clauses -- the owner field equals the user, or the public bit -- neither deleted
users = rng.integers(0, 200, len(query))
mine_or_public = [[ggnn.label_mask(none_of=DELETED, field_mask=OWNER_FIELD,
                                   field_value=int(u) << OWNER_SHIFT),
                   ggnn.label_mask(all_of=PUBLIC, none_of=DELETED)] for u in users]
m_ids, _ = g.query_labeled_mask(query, K, 0.7, 800, label_masks=mine_or_public)
found, lab = rows_of(m_ids.numpy())
owned = ((lab & OWNER_FIELD) >> OWNER_SHIFT) == users[:, None]
ok = ((lab & DELETED) == 0) & (owned | ((lab & PUBLIC) != 0))
assert ok[found].all()
print("mine or public: two clauses per query, every result owned by the user or public")

# the clauses as an array: [Nq, n_masks, 3] int32 (or int64 with 0x80000000 written as it reads), on
# the GPU next to the queries; the same on two asynchronous slots
clauses = torch.tensor(mine_or_public, dtype=torch.int64).cuda()      # [Nq, 2, 3]
q_gpu = torch.from_numpy(query).cuda()
half = len(query) // 2
t0 = g.query_async_labeled_mask(q_gpu[:half], K, 0.7, 800, slot=0, label_masks=clauses[:half])
t1 = g.query_async_labeled_mask(q_gpu[half:], K, 0.7, 800, slot=1, label_masks=clauses[half:])
g.synchronize()
assert torch.equal(torch.cat([t0.ids, t1.ids])[:, :K].cpu(), m_ids)
print("two asynchronous slots: same result")

# granting a group: rewrite the labels of a few rows the user could not see
n = 0
hidden = np.nonzero(((label & mine[n]) == 0) & ((label & DELETED) == 0))[0]
exact, _ = g.bf_query(query[n:n + 1], 50)
grant = np.array([r for r in exact.numpy()[0] if r in set(hidden.tolist())][:3])
label[grant] |= int(mine[n]) & -int(mine[n])                          # the lower of the user's groups
g.update_labels(grant, label[grant].astype(np.uint32).view(np.int32))
after, _ = g.bf_query_labeled_mask(query[n:n + 1], 50, label_masks=visible[n:n + 1])
assert set(grant.tolist()) <= set(after.numpy()[0].tolist())
print(f"rows {grant.tolist()} granted to a group of user {n}: now among the results")

# deleting is one bit as well
gone = int(after.numpy()[0][0])
label[gone] |= DELETED
g.update_labels(np.array([gone]), label[[gone]].astype(np.uint32).view(np.int32))
again, _ = g.bf_query_labeled_mask(query[n:n + 1], 50, label_masks=visible[n:n + 1])
assert gone not in again.numpy()
print(f"row {gone} flagged deleted: gone from the results")
