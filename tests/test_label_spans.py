"""CPU tests of the label spans (include/ggnn_c.h, the three ggnn_op_*label_spans* operators): the status
codes that need no device, the ops surface, a numpy model of the resolve rule on hand-written columns
(tests/test_gpu_label_spans.py holds the kernel to this model), and the new kernels in the built
library (all five element types, no private segment)."""
import ctypes as C
import re

import numpy as np
import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture: the built library's code objects)
from test_kernel_resources import pytestmark as needs_built_library

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
SETS, RANGES = 0, 1


def _lib():
    from ggnn_amd import _lib
    return _lib


# ---- the numpy model of the resolve rule ------------------------------------------------------------
def numpy_resolve(keys, offsets, label_sets=None, label_ranges=None):
    """(spans [Nq, 8, 2], totals [Nq]) int32 of label sets [Nq, w] or label ranges [Nq, r, 2] over the
    index (keys, offsets): every entry's run of positions, empty ones dropped, sorted by begin,
    overlapping and touching runs merged, (0, 0) at the tail"""
    assert (label_sets is None) != (label_ranges is None)
    keys = np.asarray(keys, np.int64)
    offsets = np.asarray(offsets, np.int64)
    sel = np.asarray(label_sets if label_sets is not None else label_ranges, np.int64)
    spans = np.zeros((len(sel), 8, 2), np.int64)
    totals = np.zeros(len(sel), np.int64)
    for n, row in enumerate(sel):
        raw = []
        if label_sets is not None:
            for L in row:
                if L == -1:
                    raw.append((0, int(offsets[len(keys)])))
                    continue
                j = int(np.searchsorted(keys, L))
                if j < len(keys) and keys[j] == L:
                    raw.append((int(offsets[j]), int(offsets[j + 1])))
        else:
            for lo, hi in row:
                if lo <= hi:
                    raw.append((int(offsets[np.searchsorted(keys, lo, side="left")]),
                                int(offsets[np.searchsorted(keys, hi, side="right")])))
        merged = []
        for b, e in sorted(s for s in raw if s[0] < s[1]):
            if merged and b <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], e)
            else:
                merged.append([b, e])
        assert len(merged) <= 8
        for j, (b, e) in enumerate(merged):
            spans[n, j] = b, e
        totals[n] = sum(e - b for b, e in merged)
    return spans.astype(np.int32), totals.astype(np.int32)


# keys, and how many rows each has
HAND_KEYS = np.array([INT32_MIN, -7, -1, 0, 3, 4, 10, INT32_MAX], np.int32)
HAND_LEN = np.array([2, 1, 3, 5, 1, 4, 2, 6])
HAND_OFFSETS = np.concatenate([[0], np.cumsum(HAND_LEN)]).astype(np.int32)   # 0 2 3 6 11 12 16 18 24


def _padded(spans):
    out = np.zeros((8, 2), np.int32)
    out[:len(spans)] = np.asarray(spans, np.int32).reshape(-1, 2)
    return out


HAND_SETS = [
    # (set, spans)
    ([3], [(11, 12)]),
    ([3, 3, 3], [(11, 12)]),                                  # repeats: one span
    ([4, 3], [(11, 16)]),                                     # touching keys merge, input order is free
    ([10, 0], [(6, 11), (16, 18)]),
    ([5], []),                                                # no key
    ([5, 6, -8], []),
    ([-1], [(0, 24)]),                                        # the wildcard, not the key -1 ...
    ([0, -1, 10], [(0, 24)]),                                 # ... wherever it stands
    ([INT32_MIN, INT32_MAX], [(0, 2), (18, 24)]),
    ([INT32_MAX, 10, 4, 3, 0, -7, INT32_MIN, 0], [(0, 3), (6, 24)]),
    ([INT32_MIN, -7, 0, 3, 4, 10, INT32_MAX, 3], [(0, 3), (6, 24)]),
    ([-7, 0, 4, INT32_MAX], [(2, 3), (6, 11), (12, 16), (18, 24)]),
]
HAND_RANGES = [
    ([(3, 3)], [(11, 12)]),                                   # a single key
    ([(3, 4)], [(11, 16)]),
    ([(4, 3)], []),                                           # lo > hi
    ([(5, 9)], []),                                           # between two keys
    ([(1, 9)], [(11, 16)]),
    ([(-1, -1)], [(3, 6)]),                                   # -1 is an ordinary label here
    ([(INT32_MIN, INT32_MAX)], [(0, 24)]),
    ([(INT32_MIN, INT32_MIN), (INT32_MAX, INT32_MAX)], [(0, 2), (18, 24)]),
    ([(0, 10), (3, 4)], [(6, 18)]),                           # nested
    ([(0, 3), (3, 10)], [(6, 18)]),                           # overlapping
    ([(4, 10), (-1, 3)], [(3, 18)]),                          # touching, given in reverse
    ([(10, 10), (-7, -7), (3, 3), (0, 0)], [(2, 3), (6, 12), (16, 18)]),
    ([(2, 1), (11, INT32_MAX - 1), (-6, -2), (20, 30)], []),
]


def test_model_on_hand_written_columns():
    for row, want in HAND_SETS:
        spans, totals = numpy_resolve(HAND_KEYS, HAND_OFFSETS, label_sets=[row])
        assert np.array_equal(spans[0], _padded(want)), row
        assert totals[0] == sum(e - b for b, e in want), row
    for row, want in HAND_RANGES:
        spans, totals = numpy_resolve(HAND_KEYS, HAND_OFFSETS, label_ranges=[row])
        assert np.array_equal(spans[0], _padded(want)), row
        assert totals[0] == sum(e - b for b, e in want), row


def test_model_covers_every_admitted_position_once():
    """on a random column: the positions of a query's spans are exactly the positions of rows[] whose
    label the set / the ranges admit, each once, and the spans are in normal form"""
    rng = np.random.default_rng(5)
    labels = rng.integers(-6, 30, 400).astype(np.int32)
    keys = np.unique(labels)
    rows = np.argsort(labels, kind="stable")
    offsets = np.concatenate([np.searchsorted(labels[rows], keys), [len(labels)]])
    sets = rng.integers(-8, 34, (60, 8))
    ranges = rng.integers(-8, 34, (60, 4, 2))
    for kind, sel in (("sets", sets), ("ranges", ranges)):
        spans, totals = numpy_resolve(keys, offsets, **{"label_" + kind: sel})
        for n in range(len(sel)):
            if kind == "sets":
                want = np.ones(400, bool) if -1 in sel[n] else np.isin(labels[rows], sel[n])
            else:
                want = np.zeros(400, bool)
                for lo, hi in sel[n]:
                    want |= (labels[rows] >= lo) & (labels[rows] <= hi)
            hit = np.zeros(400, int)
            live = [(b, e) for b, e in spans[n] if e > b]
            for b, e in live:
                hit[b:e] += 1
            assert np.array_equal(hit, want.astype(int)), (kind, n)
            assert totals[n] == want.sum()
            assert all(live[i][1] < live[i + 1][0] for i in range(len(live) - 1)), (kind, n)
            assert (spans[n, len(live):] == 0).all()


# ---- status codes that need no device ---------------------------------------------------------------
def _host(n=64, dtype=np.int32):
    """some aligned host memory to stand for a device pointer that is never read"""
    a = np.zeros(n + 8, dtype)
    off = (-a.ctypes.data % 16) // a.itemsize
    return a[off:off + n]


def test_resolve_status_codes():
    _l = _lib()
    f = _l.lib().ggnn_op_label_spans_resolve
    k, o, s, sp, t = (_host() for _ in range(5))
    p = lambda a: a.ctypes.data  # noqa: E731
    for width in (0, 9, 2 ** 31):
        assert f(p(k), 3, p(o), SETS, p(s), width, 4, p(sp), p(t), None) == _l.INVALID_ARGUMENT
    for n_ranges in (0, 5, 8):
        assert f(p(k), 3, p(o), RANGES, p(s), n_ranges, 4, p(sp), p(t), None) == _l.INVALID_ARGUMENT
    for mode in (-1, 2):
        assert f(p(k), 3, p(o), mode, p(s), 1, 4, p(sp), p(t), None) == _l.INVALID_ARGUMENT
    for hole in range(5):
        args = [p(k), p(o), p(s), p(sp), p(t)]
        args[hole] = None
        assert f(args[0], 3, args[1], SETS, args[2], 2, 4, args[3], args[4], None) == \
            _l.INVALID_ARGUMENT, hole
    assert f(p(k), 0, p(o), SETS, p(s), 2, 4, p(sp), p(t), None) == _l.INVALID_ARGUMENT
    # Nq == 0 launches nothing (and needs no pointer), in both modes
    assert f(None, 0, None, SETS, None, 8, 0, None, None, None) == _l.OK
    assert f(None, 0, None, RANGES, None, 4, 0, None, None, None) == _l.OK
    assert f(None, 0, None, RANGES, None, 5, 0, None, None, None) == _l.INVALID_ARGUMENT


def _scan(_l, **kw):
    a = dict(base=_host(64, np.float32).ctypes.data, dtype=_l.F32, N=16, D=4,
             query=_host(64, np.float32).ctypes.data, Nq=2, k=4, measure=0,
             rows=_host().ctypes.data, spans=_host().ctypes.data, span_limit=0, table=None, F=0,
             n_bits=0, fids=None, ids=_host().ctypes.data, dists=_host().ctypes.data)
    a.update(kw)
    return _l.lib().ggnn_op_bf_query_label_spans(
        a["base"], a["dtype"], a["N"], a["D"], a["query"], a["Nq"], a["k"], a["measure"], a["rows"],
        a["spans"], a["span_limit"], a["table"], a["F"], a["n_bits"], a["fids"], a["ids"],
        a["dists"], None)


def test_scan_status_codes():
    _l = _lib()
    for k in (0, 6001, 2 ** 31):
        assert _scan(_l, k=k) == _l.INVALID_ARGUMENT, k
        assert _scan(_l, k=k, Nq=0) == _l.INVALID_ARGUMENT, k
    assert _scan(_l, N=2 ** 30 + 1) == _l.UNSUPPORTED
    assert _scan(_l, N=2 ** 30 + 1, dtype=_l.I8, D=16) == _l.UNSUPPORTED
    for hole in ("base", "query", "rows", "spans", "ids", "dists"):
        assert _scan(_l, **{hole: None}) == _l.INVALID_ARGUMENT, hole
    table = _host().ctypes.data
    # a table shorter than the base is refused; table and num_filters go together
    assert _scan(_l, table=table, F=2, n_bits=15, fids=_host().ctypes.data) == _l.INVALID_ARGUMENT
    assert _scan(_l, table=table, F=2, n_bits=15) == _l.INVALID_ARGUMENT
    assert _scan(_l, table=table, F=0, n_bits=32) == _l.INVALID_ARGUMENT
    assert _scan(_l, table=None, F=2, n_bits=32) == _l.INVALID_ARGUMENT
    assert _scan(_l, D=5) == _l.UNSUPPORTED                      # (the row layout rule of every scan)
    # Nq == 0 launches nothing: every element type, with and without a table, no pointer needed
    for dtype in (_l.F32, _l.U8, _l.I8, _l.F16, _l.BF16):
        assert _scan(_l, Nq=0, dtype=dtype, D=16) == _l.OK
    assert _scan(_l, Nq=0, base=None, query=None, rows=None, spans=None, ids=None, dists=None) == _l.OK
    assert _scan(_l, Nq=0, table=table, F=2, n_bits=16) == _l.OK


def test_classify_status_codes():
    _l = _lib()
    f = _l.lib().ggnn_op_label_spans_classify
    t, a, b = _host(), _host(), _host()
    assert f(t.ctypes.data, 4, 10, a.ctypes.data, b.ctypes.data, None, None) == _l.INVALID_ARGUMENT
    assert f(None, 0, 10, None, None, None, None) == _l.INVALID_ARGUMENT
    c = _host().ctypes.data
    assert f(None, 4, 10, a.ctypes.data, b.ctypes.data, c, None) == _l.INVALID_ARGUMENT
    assert f(t.ctypes.data, 4, 10, None, b.ctypes.data, c, None) == _l.INVALID_ARGUMENT
    assert f(t.ctypes.data, 4, 10, a.ctypes.data, None, c, None) == _l.INVALID_ARGUMENT


# ---- the ops surface ----------------------------------------------------------------------------------
def test_ops_surface():
    import inspect

    import torch
    from ggnn_amd import ops
    for name in ("label_spans_resolve", "bf_query_label_spans", "label_spans_classify",
                 "bf_query_label_index_in", "bf_query_label_index_range"):
        assert callable(getattr(ops, name)), name
    sig = inspect.signature(ops.bf_query_label_spans)
    assert list(sig.parameters) == ["base", "query", "k_query", "rows", "spans", "filter_table",
                                    "filter_ids", "measure", "span_limit"]
    assert sig.parameters["span_limit"].default == 0 and sig.parameters["measure"].default == 0
    assert list(inspect.signature(ops.label_spans_resolve).parameters) == \
        ["keys", "offsets", "label_sets", "label_ranges"]
    keys, offsets = torch.from_numpy(HAND_KEYS), torch.from_numpy(HAND_OFFSETS)
    sets = torch.zeros((3, 2), dtype=torch.int32)
    ranges = torch.zeros((3, 2, 2), dtype=torch.int32)
    # exactly one of the two selections
    with pytest.raises(ValueError, match="one of the two"):
        ops.label_spans_resolve(keys, offsets)
    with pytest.raises(ValueError, match="one of the two"):
        ops.label_spans_resolve(keys, offsets, label_sets=sets, label_ranges=ranges)
    # host tensors are refused before anything is called
    with pytest.raises(ValueError, match="CUDA"):
        ops.label_spans_resolve(keys, offsets, label_sets=sets)
    with pytest.raises(ValueError, match="CUDA"):
        ops.label_spans_classify(torch.zeros(4, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="CUDA"):
        ops.bf_query_label_spans(torch.zeros((8, 4)), torch.zeros((2, 4)), 2,
                                 torch.zeros(8, dtype=torch.int32),
                                 torch.zeros((2, 8, 2), dtype=torch.int32))


def test_header_declares_the_operators():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ggnn_c.h")).read()
    for name in ("ggnn_op_label_spans_resolve", "ggnn_op_bf_query_label_spans",
                 "ggnn_op_label_spans_classify"):
        assert re.search(r"ggnn_status\s+" + name + r"\(", header), name
        assert hasattr(_lib().lib(), name), name


# ---- the built library ----------------------------------------------------------------------------------
@needs_built_library
def test_library_has_the_kernels_without_a_private_segment(kernels):  # noqa: F811
    """label_spans_scan_kernel / label_spans_scan_lds_kernel for all five element types and both
    measures, R = 1, 2, 4 on the headline layout, and the resolve, flags and merge kernels; none
    carries a private segment or spills"""
    mine = {n: k for n, k in kernels.items() if n.startswith("label_spans_")}
    assert mine, "no label_spans_ kernel in the library"
    first_args = set()
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
        m = re.match(r"label_spans_scan(_lds)?_kernel<([^,]+), (\d+), (\d+), (.*)>$", name)
        if m:
            tail = [int(x) for x in m.group(5).split(", ")]
            first_args.add((bool(m.group(1)), m.group(2), tail[-1]))
    types = {t for _, t, _ in first_args}
    assert len(types) == 5, types            # (how the 16-bit types are spelled is the compiler's)
    assert {"float", "unsigned char", "signed char"} <= types
    for lds in (False, True):
        for t in types:
            for mode in (0, 1):
                assert (lds, t, mode) in first_args, (lds, t, mode)
    for plain in ("label_spans_resolve_kernel", "label_spans_flags_kernel",
                  "label_spans_merge_kernel<4>", "label_spans_merge_lds_kernel"):
        assert plain in mine, plain
    for R in (1, 2, 4):
        assert f"label_spans_scan_kernel<float, 16, 2, {R}, 0>" in mine
    assert "label_spans_scan_lds_kernel<float, 16, 2, 0>" in mine


@needs_built_library
def test_kernel_names_stay_clear_of_the_enumerated_prefixes(kernels):  # noqa: F811
    """the coverage tests list the library's kernels by the prefixes query_, bf_query_ and
    label_index_: every kernel of label_spans.hip is named label_spans_*"""
    src = open(__file__.replace("tests/test_label_spans.py",
                                "ggnn_amd/csrc/label_spans.hip")).read()
    names = re.findall(r"__global__[^;{]*?\b(\w+_kernel)\s*\(", src, flags=re.S)
    assert len(names) == 6, names
    for n in names:
        assert n.startswith("label_spans_"), n
        assert any(k == n or k.startswith(n + "<") for k in kernels), n
