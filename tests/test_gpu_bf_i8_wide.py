"""bf_query on the wide-row integer kernel (bf_i8_wide.hip, hook BF_I8_WIDE = 2) against int64 numpy:
ids and distance bits ordered by (d, id), exact below 2^24, and the 2^24 rule at D = 272."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N, NQ = 5000, 300      # a ragged last tile; one full 256-query block, then a full and a 12-query set
LIMIT = 1 << 24


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def reference(base, q, K):
    """(ids, float32 distances, int64 K-th distance) by (d, id); base / q: uint8"""
    b, x = base.astype(np.float64), q.astype(np.float64)          # integers below 2^53: exact
    d = ((x * x).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (x @ b.T)).astype(np.int64)
    ids = np.argsort(d, axis=1, kind="stable")[:, :K]             # stable: the lower id first
    dk = np.take_along_axis(d, ids, 1)
    return ids.astype(np.int32), dk.astype(np.float32), dk[:, -1], int(d.max())


@functools.lru_cache(maxsize=None)
def tie_heavy(D):
    rng = np.random.default_rng(1000 + D)
    hi = 128 if D > 258 else 256                                  # D = 528: every distance below 2^24
    base = rng.integers(0, hi, (N, D)).astype(np.uint8)
    base[N // 2:N // 2 + 400] = base[:400]                        # twins across slices ...
    base[N - 300:] = base[100:400]                                # ... and at the very end of the base
    q = rng.integers(0, hi, (NQ, D)).astype(np.uint8)
    q[5:205] = base[100:300]                                      # three copies each: distance 0 ties
    return base, q, reference(base, q, 16)


def run(base, q, K, **hooks):
    from ggnn_amd import _lib, ops
    with _lib.hooks(**hooks):
        ids, d, rescanned = ops.bf_query(dev(base), dev(q), K, 0, rescanned=True)
    return ids.cpu().numpy(), d.cpu().numpy(), rescanned


@pytest.mark.parametrize("signed", [False, True], ids=["uint8", "int8"])
@pytest.mark.parametrize("K", [1, 10, 16])
@pytest.mark.parametrize("D", [144, 256, 528])   # a 16-byte last chunk; two chunks; a second stage
def test_equals_int64_reference(D, K, signed):
    from ggnn_amd import _lib
    base, q, (r_ids, r_d, _, d_max) = tie_heavy(D)
    assert d_max < LIMIT
    if signed:
        base, q = (base ^ 0x80).view(np.int8), (q ^ 0x80).view(np.int8)
    shape = (_lib.I8 if signed else _lib.U8, 0, D, NQ, N, K, 0)
    with _lib.hooks(BF_I8_WIDE=2):
        assert _lib.lib().ggnn_debug_bf_i8_wide_route(*shape) == 1
    with _lib.hooks(BF_I8_WIDE=1):
        assert _lib.lib().ggnn_debug_bf_i8_wide_route(*shape) == 0
    for extra in ({}, {"BF_SLICES": 1}, {"BF_SLICES": 7}, {"BF_SLICES": 7, "BF_I8_SEED": 256}):
        ids, d, rescanned = run(base, q, K, BF_I8_WIDE=2, **extra)
        assert rescanned == 0, extra
        assert np.array_equal(ids, r_ids[:, :K]), extra
        assert d.tobytes() == np.ascontiguousarray(r_d[:, :K]).tobytes(), extra


@pytest.mark.parametrize("K", [1, 10, 16])
def test_queries_at_or_above_2_pow_24_go_to_the_scan(K):
    D = 272
    rng = np.random.default_rng(272)
    base = rng.integers(0, 6, (N, D)).astype(np.uint8)
    q = rng.integers(0, 6, (NQ, D)).astype(np.uint8)
    q[10:30] = 255
    for i in range(40):                                           # K-th distances around 2^24
        q[60 + i] = 251
        q[60 + i, :20 + 2 * i] = 252
    r_ids, r_d, r_kth, _ = reference(base, q, K)
    open_ = r_kth >= LIMIT
    assert 20 < open_.sum() < NQ and (~open_[60:100]).any() and open_[60:100].any()
    ids, d, rescanned = run(base, q, K, BF_I8_WIDE=2)
    assert rescanned == open_.sum()
    assert np.array_equal(ids[~open_], r_ids[~open_]) and d[~open_].tobytes() == r_d[~open_].tobytes()
    s_ids, s_d, _ = run(base, q, K, BF_SCAN=1)
    assert np.array_equal(ids, s_ids) and d.tobytes() == s_d.tobytes()
