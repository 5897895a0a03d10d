"""CPU tests of tests/results_reference.py: the numpy references that tests/test_gpu_results.py
holds the result sort, the result merge, the uniform generator and the nn1 statistics to are tied
to what restates the same rule elsewhere -- the oracle's stable sort, the torch stand-in of the
merge, a Python-integer splitmix64 and known answers, the oracle's serial float64 mean -- and the
one place where two of them disagree is written down: inside a tie the reference's heap merge (the
oracle) orders ids as libstdc++'s heap happens to, the project by "lower part first"."""
import numpy as np
import pytest

from results_reference import (FLT_MAX, NN1_SIZES, UNIFORM_KNOWN, UNIFORM_STREAMS, bits, merge_input,
                               merge_ref, nn1_exact_input, nn1_generic_input, nn1_ref,
                               same_up_to_tie_order, sort_rows_input, sort_rows_ref, uniform_python,
                               uniform_ref)


# ---------------------------------------------------------------------------------------------
# sort
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,row_len", [(50, 2), (50, 40), (20, 65), (5, 1000)])
def test_sort_ref_equals_oracle(orc, rows, row_len):
    ids, d = sort_rows_input(rows, row_len, 100 + row_len)
    assert np.isneginf(d).any() and np.isposinf(d).any() and (d == FLT_MAX).any()
    assert (bits(d) == 0x80000000).any() and (bits(d) == 0).any() and (bits(d) == 1).any()
    r_ids, r_d = sort_rows_ref(ids, d)
    o_ids, o_d = orc.sort_shard_results(ids, d)
    assert np.array_equal(r_ids, o_ids) and np.array_equal(bits(r_d), bits(o_d))


def test_sort_ref_is_stable_and_keeps_zero_signs():
    ids = np.arange(6, dtype=np.int32)[None]
    d = np.array([[0.0, -0.0, 1.0, -0.0, 0.0, -1.0]], np.float32)
    r_ids, r_d = sort_rows_ref(ids, d)
    assert r_ids.tolist() == [[5, 0, 1, 3, 4, 2]]
    assert bits(r_d).tolist() == [[0xbf800000, 0, 0x80000000, 0x80000000, 0, 0x3f800000]]


# ---------------------------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------------------------
MERGE_CPU_CASES = [(P, K, spg) for P in (2, 3, 8) for K in (1, 2, 5, 10) for spg in (1, 2)]


@pytest.mark.parametrize("offset", [0, 1000])
@pytest.mark.parametrize("P,K,spg", MERGE_CPU_CASES)
def test_merge_ref_equals_torch_stand_in(P, K, spg, offset):
    torch = pytest.importorskip("torch")
    from ggnn_amd.distributed import merge_gathered
    for zeros in (False, True):
        ids, d = merge_input(P, 200, K * spg, 7 * P + K, signed_zeros=zeros)
        r_ids, r_d = merge_ref(ids, d, K, offset)
        s_ids, s_d = merge_gathered(torch.from_numpy(ids), torch.from_numpy(d), K, offset)
        assert np.array_equal(r_ids, s_ids.numpy())
        assert np.array_equal(bits(r_d), bits(s_d.numpy()))


def _oracle_merge(orc, ids, d, K, spg, offset):
    assert offset % spg == 0
    return orc.merge_results(list(ids), list(d), K, spg, offset // spg)


def test_merge_ref_and_oracle_agree_up_to_tie_order_only(orc):
    """Same distances, same ids per distance value -- and NOT the same ids per position: the
    reference's ResultMerger pops a heap whose comparator is `a.dist >= b.dist`, so what it emits
    first among equal distances is what libstdc++'s heap yields; the project's rule is its own
    (lower part first, then position).  Neither side is to be "fixed" to match the other."""
    differing = rows = 0
    for P, K, spg in MERGE_CPU_CASES:
        for offset in (0, 1000):
            ids, d = merge_input(P, 200, K * spg, 7 * P + K)
            r_ids, r_d = merge_ref(ids, d, K, offset)
            o_ids, o_d = _oracle_merge(orc, ids, d, K, spg, offset)
            assert same_up_to_tie_order(r_ids, r_d, o_ids, o_d), (P, K, spg, offset)
            differing += int((r_ids != o_ids).any(1).sum())
            rows += len(r_ids)
    print(f"merge_ref vs oracle: ids differ in {differing} of {rows} rows")
    assert differing >= 1


def test_merge_ref_rule_by_hand():
    inf = np.inf
    d = np.array([[[1, 1, 2]], [[0, 1, inf]], [[1, 1, 1]]], np.float32)          # [3, 1, 3]
    ids = np.array([[[10, 11, 12]], [[20, 21, -1]], [[30, 31, 32]]], np.int32)
    r_ids, r_d = merge_ref(ids, d, 6, 100)
    assert r_ids.tolist() == [[120, 10, 11, 121, 230, 231]]
    assert r_d.tolist() == [[0, 1, 1, 1, 1, 1]]
    r_ids, r_d = merge_ref(ids, d, 9, 100)                     # takes everything, the tail last
    assert r_ids.tolist() == [[120, 10, 11, 121, 230, 231, 232, 12, 99]]
    assert bits(r_d)[0, -1] == 0x7f800000


def test_same_up_to_tie_order_rejects_what_it_must():
    d = np.array([[1, 1, 2, 2, 3, 3]], np.float32)
    ids = np.array([[5, 6, 7, 8, 9, 10]], np.int32)

    def other(pairs):
        o = ids.copy()
        for pos, v in pairs:
            o[0, pos] = v
        return o

    assert same_up_to_tie_order(ids, d, ids, d)
    assert same_up_to_tie_order(ids, d, other([(0, 6), (1, 5)]), d)          # order inside a tie
    assert same_up_to_tie_order(ids, d, other([(5, 77)]), d)   # the last group may be cut elsewhere
    assert not same_up_to_tie_order(ids, d, other([(1, 7), (2, 6)]), d)      # swapped across groups
    assert not same_up_to_tie_order(ids, d, other([(1, 5)]), d)              # one id twice
    assert not same_up_to_tie_order(ids, d, other([(2, 99)]), d)             # not a candidate
    d2 = d.copy()
    d2[0, 3] = np.nextafter(np.float32(2), np.float32(3))
    assert not same_up_to_tie_order(ids, d, ids, d2)                         # a changed distance
    z, nz = np.array([[0.0, 1.0]], np.float32), np.array([[-0.0, 1.0]], np.float32)
    assert not same_up_to_tie_order(ids[:, :2], z, ids[:, :2], nz)           # the sign of a zero


# ---------------------------------------------------------------------------------------------
# uniform
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,stream", UNIFORM_STREAMS)
def test_uniform_ref_equals_python_integers_and_known_answers(seed, stream):
    u = uniform_ref(1000, seed, stream)
    assert u.dtype == np.float32
    assert np.array_equal(bits(u), bits(uniform_python(1000, seed, stream)))
    assert tuple(int(b) for b in bits(u[:3])) == UNIFORM_KNOWN[(seed, stream)]
    assert u.min() > 0.0 and u.max() <= 1.0
    # a prefix of a longer stream is the shorter stream: the value depends on the index alone
    assert np.array_equal(uniform_ref(257, seed, stream), u[:257])


# ---------------------------------------------------------------------------------------------
# nn1 statistics
# ---------------------------------------------------------------------------------------------
def nn1_inputs():
    for N in NN1_SIZES:
        yield f"exact-{N}", nn1_exact_input(N, N)
    yield "mixed-signs", nn1_exact_input(1000, 1, shift=2.0 ** 16)
    yield "all-negative", nn1_exact_input(1000, 2, shift=2.0 ** 18)
    yield "generic", nn1_generic_input()


def test_nn1_ref_equals_oracle(orc):
    for name, v in nn1_inputs():
        mean, mx = nn1_ref(v)
        o = orc.nn1_stats(v)
        assert bits(mean) == bits(o[0]) and bits(mx) == bits(o[1]), name
    v = nn1_exact_input(1000, 1, shift=2.0 ** 16)
    assert v.min() < 0 < v.max()
    assert nn1_exact_input(1000, 2, shift=2.0 ** 18).max() < 0
