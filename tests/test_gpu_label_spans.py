"""GPU tests of the label spans: label sets and label ranges answered through a label index.  Every
comparison is bit for bit: array_equal on ids, tobytes() on distances.

Data: the bases, queries and label column of tests/test_gpu_label_index.py (segments of 1 .. 130 rows
on both sides of every layout's batch, one large label), copied, plus what that data does not have --
equal rows in two DIFFERENT labels A < B (by key) where the row of A has the HIGHER id, so that the
order of positions in rows[] is the reverse of the id order, and the query placed on them:

  pair 1  last row of label 3 (15 rows) = first row of label 4 (16 rows)
  pair 2  last row of label 9 (17 rows) = first row of label 40 (33 rows): in the set {3, 9, 40} these
          are the virtual positions 31 and 32, on either side of a batch boundary of every layout
  pair 3  last row of label 1000 (64 rows) = first row of label 70000 (65 rows): virtual positions 63
          and 64 of the set {1000, 70000}, on either side of the cut of 3 and of 4 slices

The scan of the whole base reports the lower id first; a K-best list that keeps insertion order among
equal distances reports the higher one first here.  reference() asserts that the expected results
really have those ids leading and ascending."""
import numpy as np
import pytest

from filtered_reference import bf_filtered_reference, pack_bits
from test_gpu_label_index import (CASES, CASE_IDS, LARGE, SEG_LABELS, SEGMENTS, UNUSED, _cast,  # noqa: F401
                                  _i32, assert_same, data, device_index, ops, positions)
from test_label_spans import (HAND_KEYS, HAND_OFFSETS, HAND_RANGES, HAND_SETS, INT32_MAX, INT32_MIN,
                              numpy_resolve)

pytestmark = pytest.mark.gpu

LOW, HIGH = SEG_LABELS[0], SEG_LABELS[-1]           # INT32_MIN + 1 (1 row), INT32_MAX - 1 (130 rows)
PAIRS = ((3, 4), (9, 40), (1000, 70000))            # (A, B) of the three tie pairs; queries 0, 1, 2

# one label set per query (padded to eight entries by repeating the first one)
SET_ROWS = [
    [3, 4],                                         # pair 1
    [40, 3, 9],                                     # pair 2: spans of 15 + 17 + 33 positions
    [70000, 1000],                                  # pair 3: 64 + 65
    [LOW, -5, 3, 9, 40],                            # 1 + 2 + 15 + 17 + 33 rows: spans end mid-batch
    [LARGE],
    [3, -1],                                        # the wildcard: every row
    [UNUSED, INT32_MIN],                            # no key: an empty result
    [HIGH, LOW, 41, 10, -5, 11, 4, UNUSED],         # eight entries, five spans
    [LOW, 3, 9, 11, 41, 1000, HIGH],                # seven spans, none touching
    [-5, LOW],                                      # 3 rows: shorter than four slices
]
# up to four closed intervals per query (padded with the empty interval (1, 0))
RANGE_ROWS = [
    [(3, 4)],                                       # pair 1: two adjacent keys
    [(40, 40), (3, 3), (9, 9)],                     # pair 2
    [(1000, 70000)],                                # pair 3
    [(9, 9)],                                       # one key
    [(3, 11)],                                      # five adjacent keys
    [(LARGE, LARGE)],
    [(INT32_MIN, INT32_MAX)],                       # every row
    [(5, 8), (2, 1)],                               # between two keys, and lo > hi: an empty result
    [(INT32_MIN, -5), (10, 40), (12, 39), (41, 41)],
    [(LOW, LOW)],                                   # 1 row
]
NQ = len(SET_ROWS)
assert len(RANGE_ROWS) == NQ
SETS = np.array([r + [r[0]] * (8 - len(r)) for r in SET_ROWS], np.int32)
RANGES = np.array([r + [(1, 0)] * (4 - len(r)) for r in RANGE_ROWS], np.int32)


def set_allowed(labels, row):
    return np.ones(len(labels), bool) if -1 in row else np.isin(labels, row)


def range_allowed(labels, row):
    ok = np.zeros(len(labels), bool)
    for lo, hi in row:
        ok |= (labels >= lo) & (labels <= hi)
    return ok


ALLOWED = {"sets": lambda labels, i: set_allowed(labels, SET_ROWS[i]),
           "ranges": lambda labels, i: range_allowed(labels, RANGE_ROWS[i])}

_spans_data, _refs = {}, {}


def spans_data(D, measure):
    """(base, queries [NQ, D], labels, pairs): a copy of the label-index data with the three cross-label
    tie pairs written in; pairs[i] = (id in A, id in B), the first the higher"""
    key = (D, measure)
    if key not in _spans_data:
        base0, q0, labels = data(D, measure)
        base, q = base0.copy(), q0[:NQ].copy()
        pairs = []
        for i, (A, B) in enumerate(PAIRS):
            a, b = int(positions(labels, A)[-1]), int(positions(labels, B)[0])
            assert A < B and a > b, (A, B, a, b)     # position order is the reverse of id order
            base[a] = base[b]
            q[i] = base[b]
            pairs.append((a, b))
        _spans_data[key] = base, q, labels, pairs
    return _spans_data[key]


def reference(orc, D, measure, K, kind, mask=None):
    """the exact K nearest under SET_ROWS / RANGE_ROWS (and the per-query masks, if any): the CPU
    oracle on the compacted rows, which reports equal distances in ascending id"""
    key = (D, measure, K, kind, None if mask is None else mask.tobytes())
    if key not in _refs:
        base, q, labels, pairs = spans_data(D, measure)
        ids = np.empty((NQ, K), np.int32)
        d = np.empty((NQ, K), np.float32)
        for i in range(NQ):
            ok = ALLOWED[kind](labels, i)
            if mask is not None:
                ok = ok & mask[i]
            ids[i:i + 1], d[i:i + 1] = bf_filtered_reference(orc, base, q[i:i + 1], K, ok, measure)
        if mask is None and K >= 2:
            # the test that matters: the tie pairs lead their queries, the LOWER id (label B) first
            for i, (a, b) in enumerate(pairs):
                assert ids[i, 0] == b and ids[i, 1] == a and b < a, (kind, i, ids[i, :3])
                assert d[i, 0] == d[i, 1], (kind, i)
            assert (ids[6 if kind == "sets" else 7] == -1).all()
        _refs[key] = ids, d
    return _refs[key]


def _torch():
    import torch
    return torch


def selections(kind):
    return {"label_sets": _i32(SETS)} if kind == "sets" else {"label_ranges": _i32(RANGES)}


def through_index(ops, kind, d_base, d_q, K, index, measure, sel=None, **kw):
    keys, offsets, rows = index
    sel = selections(kind) if sel is None else sel
    if kind == "sets":
        return ops.bf_query_label_index_in(d_base, d_q, K, keys, offsets, rows, sel["label_sets"],
                                           measure=measure, **kw)
    return ops.bf_query_label_index_range(d_base, d_q, K, keys, offsets, rows, sel["label_ranges"],
                                          measure=measure, **kw)


def whole_base_scan(ops, kind, d_base, d_q, K, d_labels, measure, **kw):
    if kind == "sets":
        return ops.bf_query_labeled_in(d_base, d_q, K, d_labels, _i32(SETS), measure=measure, **kw)
    return ops.bf_query_labeled_range(d_base, d_q, K, d_labels, _i32(RANGES), measure=measure, **kw)


# ---- resolve against numpy -------------------------------------------------------------------------
def _resolve_equals_model(ops, keys, offsets, **sel):
    d_keys, d_offsets = _i32(keys), _i32(offsets)
    got = ops.label_spans_resolve(d_keys, d_offsets, **{k: _i32(v) for k, v in sel.items()})
    want = numpy_resolve(keys, offsets, **sel)
    assert np.array_equal(got[0].cpu().numpy(), want[0]), sel
    assert np.array_equal(got[1].cpu().numpy(), want[1]), sel
    return want


@pytest.mark.parametrize("width", range(1, 9))
def test_resolve_sets(ops, width):
    """every width: the hand-written sets that fit (padded with repeats), then random sets over keys,
    non-keys, INT32_MIN / INT32_MAX and the wildcard in the first, a middle and the last place"""
    rows = [r + [r[0]] * (width - len(r)) for r, _ in HAND_SETS if len(r) <= width]
    spans, _ = _resolve_equals_model(ops, HAND_KEYS, HAND_OFFSETS, label_sets=np.array(rows, np.int32))
    hand = [w for r, w in HAND_SETS if len(r) <= width]
    for got, want in zip(spans, hand):                       # (and the model against the hand values)
        assert [tuple(s) for s in got if s[1] > s[0]] == want
    rng = np.random.default_rng(40 + width)
    pool = np.concatenate([HAND_KEYS, [5, 6, -8, 11, INT32_MAX - 1, INT32_MIN + 1]])
    sets = rng.choice(pool, (200, width)).astype(np.int32)
    sets[sets == -1] = 0                                      # (-1 only where it is put below)
    sets[0:20, 0] = -1
    sets[20:40, width // 2] = -1
    sets[40:60, width - 1] = -1
    _resolve_equals_model(ops, HAND_KEYS, HAND_OFFSETS, label_sets=sets)
    # the test column's index, its keys next to the lowest and the highest int32
    labels = data(32, 0)[2]
    keys, offsets, _ = (t.numpy() for t in ops.label_index_build(labels))
    pool = np.concatenate([keys, [UNUSED, INT32_MIN, INT32_MAX, -1]])
    _resolve_equals_model(ops, keys, offsets, label_sets=rng.choice(pool, (200, width)).astype(np.int32))
    if width == 8:
        _resolve_equals_model(ops, keys, offsets, label_sets=SETS)


@pytest.mark.parametrize("n_ranges", range(1, 5))
def test_resolve_ranges(ops, n_ranges):
    """1 .. 4 intervals: the hand-written rows that fit (lo > hi, nested, overlapping, touching, between
    two keys, [INT32_MIN, INT32_MAX], single keys), then random intervals"""
    rows = [r + [(1, 0)] * (n_ranges - len(r)) for r, _ in HAND_RANGES if len(r) <= n_ranges]
    spans, _ = _resolve_equals_model(ops, HAND_KEYS, HAND_OFFSETS,
                                     label_ranges=np.array(rows, np.int32))
    hand = [w for r, w in HAND_RANGES if len(r) <= n_ranges]
    for got, want in zip(spans, hand):
        assert [tuple(s) for s in got if s[1] > s[0]] == want
    rng = np.random.default_rng(50 + n_ranges)
    pool = np.concatenate([HAND_KEYS, HAND_KEYS[1:] - 1, HAND_KEYS[:-1] + 1, [5, 8]]).astype(np.int32)
    _resolve_equals_model(ops, HAND_KEYS, HAND_OFFSETS,
                          label_ranges=rng.choice(pool, (300, n_ranges, 2)))
    labels = data(32, 0)[2]
    keys, offsets, _ = (t.numpy() for t in ops.label_index_build(labels))
    pool = np.concatenate([keys, keys[1:] - 1, keys[:-1] + 1, [INT32_MIN, INT32_MAX]]).astype(np.int32)
    _resolve_equals_model(ops, keys, offsets, label_ranges=rng.choice(pool, (300, n_ranges, 2)))
    if n_ranges == 4:
        _resolve_equals_model(ops, keys, offsets, label_ranges=RANGES)


# ---- the seam on every layout ------------------------------------------------------------------------
@pytest.mark.parametrize("kind,D,measure", CASES, ids=CASE_IDS)
def test_seam_every_layout(ops, orc, kind, D, measure):
    """k = 10 in every cell, k = 100 (the R = 2 register list) at D = 96 / 128 / 1024: label sets and
    label ranges through the index equal the CPU reference and -- for every type but int8, which those
    ops refuse -- ops.bf_query_labeled_in / ops.bf_query_labeled_range on the same column"""
    base, q, labels, _ = spans_data(D, measure)
    d_base, d_q, d_labels = _cast(base, kind), _cast(q, kind), _i32(labels)
    index = device_index(ops, labels)
    for K in (10, 100) if D in (96, 128, 1024) else (10,):
        for sel in ("sets", "ranges"):
            got = through_index(ops, sel, d_base, d_q, K, index, measure)
            assert_same(got, reference(orc, D, measure, K, sel), (kind, D, measure, K, sel, "reference"))
            if kind != "i8":
                assert_same(got, whole_base_scan(ops, sel, d_base, d_q, K, d_labels, measure),
                            (kind, D, measure, K, sel, "whole-base scan"))


def test_int8_is_refused_by_the_whole_base_scan(ops):
    """why int8 is held to the CPU reference alone"""
    from ggnn_amd._lib import GGNNError
    base, q, labels, _ = spans_data(64, 0)
    for sel in ("sets", "ranges"):
        with pytest.raises(GGNNError):
            whole_base_scan(ops, sel, _cast(base, "i8"), _cast(q, "i8"), 10, _i32(labels), 0)


# ---- filter table -----------------------------------------------------------------------------------
FILTER_IDS = np.array([0, 2, 0, 0, 1, -1, 0, 3, -7, 2], np.int32)   # 3 >= F; -7: negative, not -1


@pytest.mark.parametrize("D", [32, 128])                   # layouts {8, 1} and {16, 2} of float32
def test_filter_table(ops, orc, D):
    """three table rows (random half, all zero, all ones); ids -1, >= F and negative: equal to the
    whole-base scans called with the same table, and to the CPU reference"""
    torch = _torch()
    measure, K = 0, 10
    base, q, labels, _ = spans_data(D, measure)
    N = len(base)
    rng = np.random.default_rng(77 + D)
    masks = np.stack([rng.random(N) < 0.5, np.zeros(N, bool), np.ones(N, bool)])
    table = torch.from_numpy(np.stack([pack_bits(m) for m in masks]).view(np.int32)).cuda()
    per_query = np.stack([masks[f] if 0 <= f < 3 else np.full(N, f == -1) for f in FILTER_IDS])
    assert len(FILTER_IDS) == NQ
    d_base, d_q, d_labels, fids = _cast(base, "f32"), _cast(q, "f32"), _i32(labels), _i32(FILTER_IDS)
    index = device_index(ops, labels)
    for sel in ("sets", "ranges"):
        got = through_index(ops, sel, d_base, d_q, K, index, measure, filter_table=table,
                            filter_ids=fids)
        assert_same(got, reference(orc, D, measure, K, sel, per_query), (D, sel, "reference"))
        assert_same(got, whole_base_scan(ops, sel, d_base, d_q, K, d_labels, measure,
                                         filter_table=table, filter_ids=fids), (D, sel, "scan"))
        # a table without ids is not read: spans only
        assert_same(through_index(ops, sel, d_base, d_q, K, index, measure, filter_table=table),
                    reference(orc, D, measure, K, sel), (D, sel, "table without ids"))
        # ids without a table: -1 or nothing
        no_table = np.stack([np.full(N, f == -1) for f in FILTER_IDS])
        assert_same(through_index(ops, sel, d_base, d_q, K, index, measure, filter_ids=fids),
                    reference(orc, D, measure, K, sel, no_table), (D, sel, "ids without a table"))


# ---- LDS list and slices, layout {8, 1} ----------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 300, 2100])
def test_lds_list_and_slices(ops, orc, K):
    """float32 D = 32: k = 300 and k = 2100 run label_spans_scan_lds_kernel and, under slices, the LDS
    merge; LABEL_INDEX_SLICES = 1, 3 and 4 cut the 129 positions of pair 3's set at 64 and 128 -- the
    higher id in the earlier slice -- and find spans of 1 and 3 positions shorter than the slice
    count; then a cosine sub-batch"""
    from ggnn_amd import _lib
    D = 32
    for measure, picks in ((0, None), (1, np.array([2, 9, 0, 7, 6]))):
        base, q, labels, _ = spans_data(D, measure)
        d_base, d_labels = _cast(base, "f32"), _i32(labels)
        index = device_index(ops, labels)
        for sel in ("sets", "ranges"):
            ref = reference(orc, D, measure, K, sel)
            if picks is None:
                d_q, chosen = _cast(q, "f32"), None
                assert_same(whole_base_scan(ops, sel, d_base, d_q, K, d_labels, measure), ref,
                            (K, sel, "whole-base scan"))
                assert_same(through_index(ops, sel, d_base, d_q, K, index, measure), ref,
                            (K, sel, "auto"))
            else:
                d_q = _cast(q[picks], "f32")
                ref = ref[0][picks], ref[1][picks]
                chosen = ({"label_sets": _i32(SETS[picks])} if sel == "sets"
                          else {"label_ranges": _i32(RANGES[picks])})
            for slices in (1, 3, 4) if picks is None else (3,):
                with _lib.hooks(LABEL_INDEX_SLICES=slices):
                    got = through_index(ops, sel, d_base, d_q, K, index, measure, sel=chosen)
                assert_same(got, ref, (K, sel, measure, slices))


# ---- classify -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 1000, 70000])
def test_classify(ops, nq):
    """routed and rest lists against numpy, order preserved; cutoffs 0, 16, 17, the largest total and
    2^31 - 1; 70000 queries take the compaction's second round of 65536; the totals are resolve's"""
    torch = _torch()
    labels = data(32, 0)[2]
    keys, offsets, _ = device_index(ops, labels)
    pool_totals = numpy_resolve(keys.cpu().numpy(), offsets.cpu().numpy(), label_sets=SETS)[1]
    assert pool_totals[5] == len(labels) and pool_totals[6] == 0       # the wildcard; no key
    pick = np.random.default_rng(nq).integers(0, NQ, nq)
    variants = [np.array([i]) for i in (0, 5, 6, 4)] if nq == 1 else [pick]
    for pick in variants:
        spans, totals = ops.label_spans_resolve(keys, offsets, label_sets=_i32(SETS[pick]))
        want_totals = pool_totals[pick]
        assert np.array_equal(totals.cpu().numpy(), want_totals)
        n = np.arange(len(pick), dtype=np.int32)
        for cutoff in (0, 16, 17, int(pool_totals.max()), 2 ** 31 - 1):
            routed, rest = ops.label_spans_classify(totals, cutoff)
            want = want_totals <= cutoff
            assert np.array_equal(routed.cpu().numpy(), n[want]), (nq, cutoff, "routed")
            assert np.array_equal(rest.cpu().numpy(), n[~want]), (nq, cutoff, "rest")
            again = ops.label_spans_classify(totals, cutoff)
            assert torch.equal(again[0], routed) and torch.equal(again[1], rest)
        # a wildcard set is routed only by a cutoff of at least N
        routed = ops.label_spans_classify(totals, len(labels) - 1)[0].cpu().numpy()
        assert not np.isin(np.nonzero(pick == 5)[0], routed).any()


# ---- edges ------------------------------------------------------------------------------------------------
def test_edges(ops, orc):
    torch = _torch()
    D, measure, K = 32, 0, 10
    base, q, labels, _ = spans_data(D, measure)
    d_base, d_q = _cast(base, "f32"), _cast(q, "f32")
    keys, offsets, rows = index = device_index(ops, labels)
    # Nq = 0 in all three
    spans, totals = ops.label_spans_resolve(keys, offsets, label_sets=_i32(np.zeros((0, 3))))
    assert tuple(spans.shape) == (0, 8, 2) and totals.numel() == 0
    spans, totals = ops.label_spans_resolve(keys, offsets, label_ranges=_i32(np.zeros((0, 2, 2))))
    assert tuple(spans.shape) == (0, 8, 2) and totals.numel() == 0
    ids, d = ops.bf_query_label_spans(d_base, d_q[:0], K, rows, spans)
    assert tuple(ids.shape) == (0, K) and tuple(d.shape) == (0, K)
    routed, rest = ops.label_spans_classify(totals, 5)
    assert routed.numel() == 0 and rest.numel() == 0
    # a batch whose every span is empty
    empty = _i32(np.full((NQ, 2), UNUSED))
    spans, totals = ops.label_spans_resolve(keys, offsets, label_sets=empty)
    assert not spans.any() and not totals.any()
    for k in (K, 300):
        ids, d = ops.bf_query_label_spans(d_base, d_q, k, rows, spans)
        assert (ids.cpu().numpy() == -1).all() and np.isinf(d.cpu().numpy()).all()
    # span_limit smaller than a query's total changes nothing in the result
    ref = reference(orc, D, measure, K, "sets")
    for limit in (1, 64, 2 ** 31 - 1):
        assert_same(through_index(ops, "sets", d_base, d_q, K, index, measure, span_limit=limit),
                    ref, ("span_limit", limit))
    # the argument checks of the ops surface that need device tensors
    with pytest.raises(ValueError):
        ops.label_spans_resolve(keys, offsets, label_sets=_i32(np.zeros((4, 9))))
    with pytest.raises(ValueError):
        ops.label_spans_resolve(keys, offsets, label_ranges=_i32(np.zeros((4, 5, 2))))
    with pytest.raises(ValueError):
        ops.bf_query_label_spans(d_base, d_q, K, rows[:-1], spans)
    with pytest.raises(ValueError):
        ops.bf_query_label_spans(d_base, d_q, K, rows, spans[:-1])
    with pytest.raises(TypeError):
        ops.label_spans_classify(totals.float(), 3)
    short = torch.zeros((2, (len(base) + 31) // 32 - 1), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.bf_query_label_spans(d_base, d_q, K, rows, spans, filter_table=short)
