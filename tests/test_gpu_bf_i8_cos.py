"""bf_query under cosine on the integer cosine kernel (bf_i8_cos.hip, hook BF_I8_COS = 2) against numpy:
exact int64 sums, finish_cos in float32 operation by operation, ids and value bits ordered by (value, id);
and the 2^24 rule on the norms at D = 272."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N, NQ = 5000, 300      # a ragged last tile; one full 256-query block, then a full and a 12-query set
LIMIT = 1 << 24
HOOKS = ({}, {"BF_SLICES": 1}, {"BF_SLICES": 7}, {"BF_SLICES": 7, "BF_I8_SEED": 256})


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def reference(base, q, K):
    """(ids, float32 values, largest |sum|) by (value, id)"""
    b, x = base.astype(np.int64), q.astype(np.int64)
    dot = (x.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)   # integers below 2^53: exact
    bn, qn = (b * b).sum(1), (x * x).sum(1)
    top = int(max(np.abs(dot).max(), bn.max(), qn.max()))
    ns = qn.astype(np.float32)[:, None] * bn.astype(np.float32)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.abs(np.float32(1) - dot.astype(np.float32) / np.sqrt(ns))
    v = np.where(ns > 0, v, np.float32(1)).astype(np.float32)
    ids = np.argsort(v, axis=1, kind="stable")[:, :K]             # stable: the lower id first
    return ids.astype(np.int32), np.take_along_axis(v, ids, 1), top


@functools.lru_cache(maxsize=None)
def adversarial(D, signed):
    rng = np.random.default_rng(2000 + D + signed)
    lo, hi = (-90, 90) if signed else (0, 128)                    # D = 528: every sum below 2^24
    base = rng.integers(lo, hi, (N, D))
    base[200:300] = rng.integers(lo // 2, hi // 2, (100, D)) // 2 * 2   # even, and twice fits
    base[1000:1040] = 0                                           # zero rows: value 1
    q = rng.integers(lo, hi, (NQ, D))
    q[5:105] = base[100:200]                                      # a base row: quotients at 1 +- ulp
    q[105:155] = 2 * base[200:250]                                # twice a base row
    q[155:205] = base[250:300] // 2                               # half a base row
    q[210] = 0                                                    # every value 1: the lowest ids win
    if signed:
        base[2000:2050] = -q[220:270]                             # value 2
    base[N // 2:N // 2 + 400] = base[:400]                        # twins across slices ...
    base[N - 300:] = base[100:400]                                # ... and at the very end of the base
    t = np.int8 if signed else np.uint8
    base, q = base.astype(t), q.astype(t)
    return base, q, reference(base, q, 16)


def run(base, q, K, **hooks):
    from ggnn_amd import _lib, ops
    with _lib.hooks(**hooks):
        ids, d, rescanned = ops.bf_query(dev(base), dev(q), K, 1, rescanned=True)
    return ids.cpu().numpy(), d.cpu().numpy(), rescanned


@pytest.mark.parametrize("signed", [False, True], ids=["uint8", "int8"])
@pytest.mark.parametrize("K", [1, 10, 16])
@pytest.mark.parametrize("D", [16, 128, 144, 528])   # one slot; a full chunk; a 16-byte last chunk; a second stage
def test_equals_exact_reference(D, K, signed):
    from ggnn_amd import _lib
    base, q, (r_ids, r_d, top) = adversarial(D, signed)
    assert top < LIMIT
    shape = (_lib.I8 if signed else _lib.U8, 1, D, NQ, N, K, 0)
    with _lib.hooks(BF_I8_COS=2):
        assert _lib.lib().ggnn_debug_bf_i8_cos_route(*shape) == 1
    with _lib.hooks(BF_I8_COS=1):
        assert _lib.lib().ggnn_debug_bf_i8_cos_route(*shape) == 0
    for extra in HOOKS:
        ids, d, rescanned = run(base, q, K, BF_I8_COS=2, **extra)
        assert rescanned == 0, extra
        assert np.array_equal(ids, r_ids[:, :K]), extra
        assert d.tobytes() == np.ascontiguousarray(r_d[:, :K]).tobytes(), extra


@pytest.mark.parametrize("wide_row", [False, True], ids=["queries", "base_row"])
def test_norms_at_or_above_2_pow_24_go_to_the_scan(wide_row):
    D, K = 272, 10
    rng = np.random.default_rng(272)
    base = rng.integers(0, 6, (N, D)).astype(np.uint8)
    q = rng.integers(0, 6, (NQ, D)).astype(np.uint8)
    if wide_row:
        base[N - 7] = 255                                         # sum o^2 >= 2^24: no query is certified
    else:
        q[10:30] = 255                                            # sum q^2 >= 2^24: exactly these
    ids, d, rescanned = run(base, q, K, BF_I8_COS=2)
    assert rescanned == (NQ if wide_row else 20)
    s_ids, s_d, _ = run(base, q, K, BF_SCAN=1)
    assert np.array_equal(ids, s_ids) and d.tobytes() == s_d.tobytes()
