"""CPU reference of the FILTERED traversal (include/ggnn_c.h, ggnn_query_filtered): `PyCache` and
`py_query` of tests/test_oracle_traversal_restatement.py extended by the one rule of the filtered
search -- in push(k, d) of a DENIED key, logical positions below BEST are never active -- and an
`allowed` array over the base ids.  Everything else (duplicate test, criteria, quirks Q1 / Q2,
visited ring, pop, xi, start points, counters) is the stock restatement, which
tests/test_filtered_reference.py ties to the C++ oracle through the all-ones filter.

Also the helpers the filtered tests share: bit packing in the format of the C-ABI and the exact
reference of the filtered brute force (orc.bf_query on the compacted base, ids mapped back).
"""
import numpy as np

import test_oracle_traversal_restatement as R

EMPTY_KEY = R.EMPTY_KEY


def make_filtered_cache(allowed):
    class FilteredPyCache(R.PyCache):
        def push(self, key, dist):
            if allowed[key]:
                return super().push(key, dist)
            # the stock push (simple_knn_cache.cuh:126-213 as restated by PyCache.push) with
            # `active = idx < S` replaced by `active = idx < S and logical index >= BEST`
            B, S, BLOCK = self.BEST, self.SORTED, self.BLOCK
            if (self.s_cache[:S] == key).any():
                return
            head = self.r_prioQ_head
            head_in = head - B
            t = np.arange(BLOCK)
            idx = np.zeros(BLOCK, np.int64)
            r_cache = np.zeros(BLOCK, np.int64)
            r_dists = np.zeros(BLOCK, np.float32)
            active = np.zeros(BLOCK, bool)
            block_start = ((S + BLOCK - 1) // BLOCK) * BLOCK
            while True:
                if active.any():
                    for l in np.nonzero(active)[0]:
                        if r_cache[l] != EMPTY_KEY:
                            nxt = B if idx[l] + 1 == S else idx[l] + 1
                            if nxt != B and nxt != head:
                                self.s_cache[nxt] = r_cache[l]
                                self.s_dists[nxt] = r_dists[l]
                    ins = []
                    for l in np.nonzero(active)[0]:
                        has_prev = idx[l] != 0 and idx[l] != head
                        prev = idx[l] - 1 if idx[l] != B else S - 1
                        if not has_prev or self.s_dists[prev] < dist:
                            ins.append(idx[l])
                    for i in ins:
                        self.s_cache[i] = key
                        self.s_dists[i] = dist
                if block_start == 0:
                    break
                block_start -= BLOCK
                logical = block_start + t
                idx = logical
                active = (idx < S) & (logical >= B)          # the one rule
                ring = active & (idx >= B)
                wrapped = np.where(idx + head_in < S, idx + head_in, idx + head_in - S + B)
                idx = np.where(ring, wrapped, idx)
                safe = np.where(active, idx, 0)
                r_cache = self.s_cache[safe]
                r_dists = self.s_dists[np.minimum(safe, S - 1)]
                active = active & (r_dists >= dist)

    return FilteredPyCache


def py_query_filtered(base, q, graph0, start, nn1_stats, KQuery, tau, max_iters, allowed,
                      cosine=False):
    """py_query with the filtered cache: (ids, dists, n_dist, n_pop) of one query.  `allowed`:
    boolean array over the keys of this base (graph)."""
    allowed = np.asarray(allowed, bool)
    stock = R.PyCache
    R.PyCache = make_filtered_cache(allowed)
    try:
        return R.py_query(base, q, graph0, start, nn1_stats, KQuery, tau, max_iters, cosine=cosine)
    finally:
        R.PyCache = stock


def pack_bits(mask):
    """uint32 words, id i allowed iff bit (i & 31) of word (i >> 5) -- written independently of
    ggnn_amd.pack_filter, which the tests compare with it"""
    mask = np.asarray(mask, bool)
    words = np.zeros((mask.size + 31) // 32, np.uint32)
    for i in np.nonzero(mask)[0]:
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words


def bf_filtered_reference(orc, base, query, K, allowed, measure=0):
    """exact K nearest among the allowed rows: orc.bf_query on the compacted sub-base, ids mapped
    back through the ascending list of allowed ids; slots beyond their number are (-1, +inf)"""
    sub = np.nonzero(np.asarray(allowed, bool))[0]
    ids = np.full((query.shape[0], K), -1, np.int32)
    dists = np.full((query.shape[0], K), np.inf, np.float32)
    kk = min(K, len(sub))
    if kk:
        g_ids, g_d = orc.bf_query(np.ascontiguousarray(base[sub]), query, kk, measure)[:2]
        ids[:, :kk] = sub[g_ids].astype(np.int32)
        dists[:, :kk] = g_d
    return ids, dists


def check_filtered_invariants(orc, base, q, ids, dists, allowed, exact_fn, K):
    """what every filtered result must satisfy: no denied id, unfilled slots (-1, +inf) at the end,
    every finite distance is the exact one of its id, ascending rows, no more finite entries than
    allowed ids, and the exact filtered brute force is a lower bound entry by entry"""
    allowed = np.asarray(allowed, bool)
    n_allowed = int(allowed.sum())
    g_ids, g_d = bf_filtered_reference(orc, base, q, K, allowed)
    for i in range(q.shape[0]):
        fin = np.isfinite(dists[i])
        assert allowed[ids[i][fin]].all(), ("denied id reported", i)
        assert (ids[i][~fin] == -1).all(), i
        assert not fin[int(fin.sum()):].any(), ("finite entry behind an unfilled slot", i)
        assert int(fin.sum()) <= n_allowed, i
        assert len(set(ids[i][fin].tolist())) == int(fin.sum()), ("duplicate id", i)
        ex = exact_fn(ids[i][fin], q[i])
        assert ex.tobytes() == dists[i][fin].tobytes(), i
        assert (np.diff(dists[i][fin]) >= 0).all(), i
        assert (g_d[i] <= dists[i]).all(), i


def l2_exact(base):
    def fn(ids, q):
        d = base[ids].astype(np.float64) - q.astype(np.float64)
        return (d * d).sum(1).astype(np.float32)
    return fn
