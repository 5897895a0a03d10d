"""Filtered bf_query on the integer matrix cores (bf_i8_filtered.hip, hook BF_I8_FILTERED = 2) against
int64 numpy: ids and distance bits ordered by (d, id) among the admitted rows, -1 / +inf past them, under a
per-call bitset, a filter table and labels, in both row regimes; the 2^24 rule under a filter; routing."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N, NQ = 5000, 300      # a ragged last tile and stage; one full 256-query block, then a full and a 12-query set
LIMIT = 1 << 24
INF = np.iinfo(np.int64).max


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pack(mask):
    """bool [.., n] -> int32 words [.., ceil(n / 32)], bit i of word i >> 5"""
    pad = (-mask.shape[-1]) % 32
    m = np.concatenate([mask, np.zeros(mask.shape[:-1] + (pad,), bool)], -1)
    return np.packbits(m, axis=-1, bitorder="little").view(np.int32)


def reference(base, q, K, admitted):
    """(ids, float32 distances, int64 K-th distance) by (d, id) over admitted [Nq, N]; -1 / +inf padded"""
    b, x = base.astype(np.float64), q.astype(np.float64)          # integers below 2^53: exact
    d = ((x * x).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (x @ b.T)).astype(np.int64)
    d[~admitted] = INF
    ids = np.argsort(d, axis=1, kind="stable")[:, :K]             # stable: the lower id first
    dk = np.take_along_axis(d, ids, 1)
    out_d = np.where(dk == INF, np.inf, dk).astype(np.float32)
    return np.where(dk == INF, -1, ids).astype(np.int32), out_d, dk[:, -1]


@functools.lru_cache(maxsize=None)
def tie_heavy(D):
    rng = np.random.default_rng(1000 + D)
    hi = 128 if D > 258 else 256                                  # D = 528: every distance below 2^24
    base = rng.integers(0, hi, (N, D)).astype(np.uint8)
    base[N // 2:N // 2 + 400] = base[:400]                        # twins across slices ...
    base[N - 300:] = base[100:400]                                # ... and at the very end of the base
    q = rng.integers(0, hi, (NQ, D)).astype(np.uint8)
    q[5:205] = base[100:300]                                      # three copies each: distance 0 ties
    return base, q


@functools.lru_cache(maxsize=None)
def filters():
    """mode -> (admitted [NQ, N], call(ops, base, q, K, **kw))"""
    rng = np.random.default_rng(7)
    mask = rng.random(N) < 0.3
    rows = np.stack([rng.random(N) < 0.5, rng.random(N) < 0.1, rng.random(N) < 0.9, np.zeros(N, bool)])
    rows[3, rng.choice(N, 6, replace=False)] = True               # a row that admits 6 rows: fewer than K
    fid = rng.integers(0, 4, NQ).astype(np.int32)                 # mixed within every 32 queries
    fid[::7], fid[3::11] = -1, 4                                  # unfiltered; one id past the table
    by_id = np.concatenate([rows, np.zeros((1, N), bool), np.ones((1, N), bool)])   # [4]: none, [-1]: all
    labels = rng.integers(0, 3, N).astype(np.int32)
    labels[rng.choice(N, 6, replace=False)] = 5                   # a class of six rows
    ql = rng.integers(0, 3, NQ).astype(np.int32)
    ql[::7], ql[3::11], ql[5::13] = -1, 5, 7                      # 7: a label no row carries
    return {
        "bitset": (np.broadcast_to(mask, (NQ, N)),
                   lambda ops, b, q, K: ops.bf_query_filtered(b, q, K, dev(pack(mask)), 0, rescanned=True)),
        "table": (by_id[fid],
                  lambda ops, b, q, K: ops.bf_query_filtered_by(b, q, K, dev(pack(rows)), dev(fid), 0,
                                                                rescanned=True)),
        "labels": ((ql[:, None] == -1) | (ql[:, None] == labels[None, :]),
                   lambda ops, b, q, K: ops.bf_query_labeled(b, q, K, dev(labels), dev(ql), 0,
                                                             rescanned=True)),
    }


def run(call, base, q, K, **hooks):
    from ggnn_amd import _lib, ops
    with _lib.hooks(**hooks):
        ids, d, rescanned, path = call(ops, dev(base), dev(q), K)
    return ids.cpu().numpy(), d.cpu().numpy(), rescanned, path


@pytest.mark.parametrize("signed", [False, True], ids=["uint8", "int8"])
@pytest.mark.parametrize("mode", ["bitset", "table", "labels"])
@pytest.mark.parametrize("K", [1, 10, 16])
@pytest.mark.parametrize("D", [32, 128, 144, 528])   # one column block; the resident row; a 16-byte last chunk; a second stage
def test_equals_int64_reference(D, K, mode, signed):
    base, q = tie_heavy(D)
    admitted, call = filters()[mode]
    r_ids, r_d, _ = reference(base, q, K, admitted)
    if signed:                                        # the same distances: squared L2 under a common shift
        base, q = (base ^ 0x80).view(np.int8), (q ^ 0x80).view(np.int8)
    for extra in ({"BF_SLICES": 1}, {"BF_SLICES": 7}, {"BF_SLICES": 7, "BF_I8_SEED": 256}):
        ids, d, rescanned, path = run(call, base, q, K, BF_I8_FILTERED=2, **extra)
        assert (path, rescanned) == (3, 0), extra
        assert np.take_along_axis(admitted, np.maximum(ids, 0), 1)[ids >= 0].all(), extra
        assert np.array_equal(ids, r_ids), extra
        assert d.tobytes() == r_d.tobytes(), extra
    s_ids, s_d, _, s_path = run(call, base, q, K, BF_I8_FILTERED=2, BF_SCAN=1)
    assert s_path == 0 and np.array_equal(s_ids, r_ids) and s_d.tobytes() == r_d.tobytes()


@pytest.mark.parametrize("K", [1, 10, 16])
def test_queries_at_or_above_2_pow_24_go_to_the_filtered_scan(K):
    D = 272
    rng = np.random.default_rng(272)
    base = rng.integers(0, 6, (N, D)).astype(np.uint8)
    q = rng.integers(0, 6, (NQ, D)).astype(np.uint8)
    q[10:30] = 255
    for i in range(40):                                           # K-th distances around 2^24
        q[60 + i] = 251
        q[60 + i, :20 + 2 * i] = 252
    mask = rng.random(N) < 0.5
    rows = np.stack([mask, np.zeros(N, bool)])
    rows[1, :K - 1] = True                                        # fewer than K admitted rows
    fid = np.zeros(NQ, np.int32)
    fid[[12, 70]] = 1                                             # far queries, yet complete by construction
    admitted = rows[fid]
    r_ids, r_d, r_kth = reference(base, q, K, admitted)
    open_ = (r_kth >= LIMIT) & (r_kth < INF)
    assert 0 < open_.sum() < NQ and not open_[[12, 70]].any()

    def call(ops, b, x, K):
        return ops.bf_query_filtered_by(b, x, K, dev(pack(rows)), dev(fid), 0, rescanned=True)
    ids, d, rescanned, path = run(call, base, q, K, BF_I8_FILTERED=2)
    assert path == 3 and rescanned == open_.sum()
    assert np.array_equal(ids[~open_], r_ids[~open_]) and d[~open_].tobytes() == r_d[~open_].tobytes()
    s_ids, s_d, _, _ = run(call, base, q, K, BF_SCAN=1)
    assert np.array_equal(ids, s_ids) and d.tobytes() == s_d.tobytes()


def test_routing():
    rng = np.random.default_rng(3)
    mask = rng.random(N) < 0.3
    bits = pack(mask)
    shifted = pack(np.concatenate([np.zeros(40, bool), mask]))    # the same rows at bit offset 40

    def path(signed, D, offset=0, **hooks):
        b = rng.integers(0, 256, (N, D)).astype(np.uint8)
        x = rng.integers(0, 256, (NQ, D)).astype(np.uint8)
        if signed:
            b, x = b.view(np.int8), x.view(np.int8)

        def call(ops, b, x, K):
            return ops.bf_query_filtered(b, x, K, dev(shifted if offset else bits), 0, offset, rescanned=True)
        ids, _, _, p = run(call, b, x, 10, **hooks)
        assert mask[ids[ids >= 0]].all()
        return p
    assert path(True, 128) == 0 and path(False, 256) == 1        # default hooks: the parent's routing
    assert path(True, 128, BF_I8_FILTERED=1) == 0 and path(False, 256, BF_I8_FILTERED=1) == 1
    assert path(True, 128, BF_I8_FILTERED=2) == 3 and path(False, 256, BF_I8_FILTERED=2) == 3
    assert path(True, 128, BF_I8_FILTERED=2, BF_NO_I8=1) != 3
    assert path(False, 256, BF_I8_FILTERED=2, BF_NO_I8=1) != 3
    assert path(False, 256, 40, BF_I8_FILTERED=2) == 0


def test_handle_on_an_int8_base_in_two_shards():
    import ggnn_amd as ggnn
    from ggnn_amd import _lib
    D, K = 64, 10
    base, q = tie_heavy(D)
    admitted = {m: a for m, (a, _) in filters().items()}
    rng = np.random.default_rng(11)
    rows = np.stack([rng.random(N) < 0.5, rng.random(N) < 0.1])
    fid = rng.integers(-1, 2, NQ).astype(np.int32)                # -1: unfiltered
    labels = rng.integers(0, 3, N).astype(np.int32)
    ql = rng.integers(-1, 4, NQ).astype(np.int32)                 # 3: a label no row carries
    eng = ggnn.GGNN()
    eng.set_base(torch.from_numpy((base ^ 0x80).view(np.int8)))
    eng.set_shard_size(N // 2)
    eng.set_filters(rows)
    eng.set_labels(labels)
    x = torch.from_numpy((q ^ 0x80).view(np.int8))
    before = eng.bf_query(x, K)
    by_id = np.concatenate([rows, np.ones((1, N), bool)])
    cases = [(lambda: eng.bf_query_filtered(x, K, filter=admitted["bitset"][0].copy()), admitted["bitset"]),
             (lambda: eng.bf_query_filtered_by(x, K, filter_ids=fid), by_id[fid]),
             (lambda: eng.bf_query_labeled(x, K, labels=ql),
              (ql[:, None] == -1) | (ql[:, None] == labels[None, :]))]
    with _lib.hooks(BF_I8_FILTERED=2):
        for call, adm in cases:
            ids, d = call()
            r_ids, r_d, _ = reference(base, q, K, adm)
            assert eng.last_bf_query_matrix_path() == 3 and eng.last_bf_query_rescanned() == 0
            assert np.array_equal(ids.numpy(), r_ids) and d.numpy().tobytes() == r_d.tobytes()
    after = eng.bf_query(x, K)
    assert torch.equal(before[0], after[0]) and before[1].numpy().tobytes() == after[1].numpy().tobytes()
