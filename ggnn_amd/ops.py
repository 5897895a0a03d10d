"""Operator seam of the engine on torch CUDA tensors (include/ggnn_c.h section 2).

Mirrors the reference's internal operator interface -- QueryKernels::{query, bruteForceQuery}
(include/ggnn/query/query_kernels.cuh:47-57) and the kernels GraphConstruction drives
(src/ggnn/construction/graph_construction.cu:128-379) -- one function per kernel, all on the
current torch stream.  torch is only the owner of the device memory here.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import GraphConfig, check, lib

EUCLIDEAN, COSINE = 0, 1


_DTYPE_CODES = {torch.float32: _lib.F32, torch.uint8: _lib.U8, torch.float16: _lib.F16,
                torch.bfloat16: _lib.BF16, torch.int8: _lib.I8}


def _dtype_code(t):
    code = _DTYPE_CODES.get(t.dtype)
    if code is None:
        raise TypeError("base/query must be int8, float32, uint8, float16 or bfloat16")
    return code


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need(t, dtype=None, name="tensor"):
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous CUDA tensor")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}")
    return t


def _cfg(cfg):
    """accept any structure with the ggnn_graph_config fields"""
    if isinstance(cfg, GraphConfig):
        return cfg
    out = GraphConfig()
    for name, _ in GraphConfig._fields_:
        v = getattr(cfg, name)
        if hasattr(v, "__len__"):
            for i in range(4):
                getattr(out, name)[i] = v[i]
        else:
            setattr(out, name, v)
    return out


def graph_config(N, D, KBuild):
    cfg = GraphConfig()
    check(lib().ggnn_graph_config_init(N, D, KBuild, cfg))
    return cfg


def query_sizing(D, k_query, max_iterations):
    import ctypes as C
    cache, sorted_ = C.c_uint32(), C.c_uint32()
    check(lib().ggnn_query_sizing(D, k_query, max_iterations, C.byref(cache), C.byref(sorted_)))
    return cache.value, sorted_.value


def dist_layout(D, dtype):
    """(lanes per row, 16-byte chunks per lane) of the distance kernels for rows of D elements of
    `dtype` (torch.float32 / torch.uint8 / torch.int8 / torch.float16 / torch.bfloat16)"""
    import ctypes as C
    code = _DTYPE_CODES[dtype]
    lpr, nch = C.c_uint32(), C.c_uint32()
    check(lib().ggnn_op_dist_layout(D, code, C.byref(lpr), C.byref(nch)))
    return lpr.value, nch.value


def prescreen_sizes(N, D, measure=EUCLIDEAN):
    import ctypes as C
    dc, pf, sf = C.c_uint32(), C.c_size_t(), C.c_size_t()
    check(lib().ggnn_prescreen_sizes(N, D, measure, C.byref(dc), C.byref(pf), C.byref(sf)))
    return dc.value, pf.value, sf.value


def prescreen_encode(base, measure=EUCLIDEAN):
    """8-bit pre-screen copy of a float32 base for `measure`:
    (codes [N, code_dim] uint8, params float32)."""
    _need(base, torch.float32, "base")
    dc, pf, sf = prescreen_sizes(base.shape[0], base.shape[1], measure)
    codes = torch.empty((base.shape[0], dc), dtype=torch.uint8, device=base.device)
    params = torch.empty(pf, dtype=torch.float32, device=base.device)
    scratch = torch.empty(sf, dtype=torch.float32, device=base.device)
    check(lib().ggnn_op_prescreen_encode(_ptr(base), base.shape[0], base.shape[1], measure,
                                         _ptr(codes), _ptr(params), _ptr(scratch), _stream()))
    return codes, params


def prescreen_probe(codes, params, query, cand, crit, measure=EUCLIDEAN):
    """reject [Nq, M] int32 and coded squared distances [Nq, M] for explicit triples."""
    _need(codes, torch.uint8, "codes"), _need(params, torch.float32, "params")
    _need(query, torch.float32, "query"), _need(cand, torch.int32, "cand")
    _need(crit, torch.float32, "crit")
    Nq, M = cand.shape
    reject = torch.empty((Nq, M), dtype=torch.int32, device=codes.device)
    s_out = torch.empty((Nq, M), dtype=torch.float32, device=codes.device)
    check(lib().ggnn_op_prescreen_probe(_ptr(codes), _ptr(params), query.shape[1], measure,
                                        _ptr(query), Nq, _ptr(cand), M, _ptr(crit), _ptr(reject),
                                        _ptr(s_out), _stream()))
    return reject, s_out


def query(base, query, graph0, start, nn1_stats, k_query, tau_query, max_iterations=400,
          measure=EUCLIDEAN, shards_per_gpu=1, on_gpu_shard=0, out=None, counters=False,
          prescreen=None, rows_read=None):
    """prescreen: optional (codes, params) of prescreen_encode(base, measure) (float32);
    rows_read: optional int32 [Nq, 2] tensor receiving the float / code rows read per query."""
    _need(base, name="base"), _need(query, base.dtype, "query")
    _need(graph0, torch.int32, "graph0"), _need(start, torch.int32, "start")
    _need(nn1_stats, torch.float32, "nn1_stats")
    Nq = query.shape[0]
    if out is None:
        ids = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.int32, device=base.device)
        dists = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.float32,
                            device=base.device)
    else:
        ids, dists = out
    nd = npop = None
    if counters:
        nd = torch.zeros(Nq, dtype=torch.int32, device=base.device)
        npop = torch.zeros(Nq, dtype=torch.int32, device=base.device)
    if prescreen is not None:
        codes, params = prescreen
        _need(base, torch.float32, "base"), _need(codes, torch.uint8, "codes")
        _need(params, torch.float32, "params")
        check(lib().ggnn_op_query_prescreened(
            _ptr(base), base.shape[0], base.shape[1], _ptr(codes), _ptr(params), _ptr(query), Nq,
            _ptr(graph0), graph0.shape[1], _ptr(start), start.numel(), _ptr(nn1_stats), k_query,
            tau_query, max_iterations, measure, shards_per_gpu, on_gpu_shard, _ptr(ids),
            _ptr(dists),
            _ptr(nd), _ptr(npop), _ptr(rows_read), _stream()))
    else:
        check(lib().ggnn_op_query(_ptr(base), _dtype_code(base), base.shape[0], base.shape[1],
                                  _ptr(query), Nq, _ptr(graph0), graph0.shape[1], _ptr(start),
                                  start.numel(), _ptr(nn1_stats), k_query, tau_query,
                                  max_iterations, measure, shards_per_gpu, on_gpu_shard,
                                  _ptr(ids), _ptr(dists), _ptr(nd), _ptr(npop), _stream()))
    if counters:
        return ids, dists, nd, npop
    return ids, dists


def query_filtered(base, query, graph0, start, nn1_stats, k_query, tau_query, filter_bits,
                   max_iterations=400, measure=EUCLIDEAN, filter_bit_offset=0, shards_per_gpu=1,
                   on_gpu_shard=0, counters=False, prescreen=None, rows_read=None):
    """`query` restricted to an allowed-id bitset: filter_bits is a packed int32 CUDA tensor
    (ggnn_amd.pack_filter), key k of this shard is allowed iff bit k + filter_bit_offset is set.
    prescreen: optional (codes, params) of prescreen_encode(base, measure) (float32)."""
    _need(base, name="base"), _need(query, base.dtype, "query")
    _need(graph0, torch.int32, "graph0"), _need(start, torch.int32, "start")
    _need(nn1_stats, torch.float32, "nn1_stats"), _need(filter_bits, torch.int32, "filter_bits")
    if filter_bits.numel() * 32 < filter_bit_offset + base.shape[0]:
        raise ValueError("filter_bits is shorter than filter_bit_offset + N bits")
    Nq = query.shape[0]
    ids = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.float32, device=base.device)
    nd = npop = None
    if counters:
        nd = torch.zeros(Nq, dtype=torch.int32, device=base.device)
        npop = torch.zeros(Nq, dtype=torch.int32, device=base.device)
    codes, params = prescreen if prescreen is not None else (None, None)
    if prescreen is not None:
        _need(base, torch.float32, "base"), _need(codes, torch.uint8, "codes")
        _need(params, torch.float32, "params")
    check(lib().ggnn_op_query_filtered(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(codes), _ptr(params),
        _ptr(query), Nq, _ptr(graph0), graph0.shape[1], _ptr(start), start.numel(),
        _ptr(nn1_stats), k_query, tau_query, max_iterations, measure, shards_per_gpu,
        on_gpu_shard, _ptr(ids), _ptr(dists), _ptr(nd), _ptr(npop), _ptr(rows_read),
        _ptr(filter_bits), filter_bit_offset, _stream()))
    if counters:
        return ids, dists, nd, npop
    return ids, dists


def _certified(call, base, *args):
    """run a ggnn_op_bf_query_*_certified entry point: (rescanned, matrix_path)"""
    n = torch.zeros(1, dtype=torch.int32, device=base.device)
    path = C.c_int(0)
    check(call(*args, _ptr(n), C.byref(path), _stream()))
    return int(n.item()), int(path.value)


def bf_query_filtered(base, query, k_query, filter_bits, measure=EUCLIDEAN, filter_bit_offset=0,
                      rescanned=False):
    """the exact k nearest among the rows the bitset allows (row i: bit i + filter_bit_offset);
    slots beyond the number of allowed rows are (-1, +inf).
    rescanned=True: returns (ids, dists, rescanned, matrix_path) -- how many queries the
    matrix-core path handed to the scan, and 1 if the launch ran the tile kernels at all (0: scan)"""
    _need(base, name="base"), _need(query, base.dtype, "query")
    _need(filter_bits, torch.int32, "filter_bits")
    if filter_bits.numel() * 32 < filter_bit_offset + base.shape[0]:
        raise ValueError("filter_bits is shorter than filter_bit_offset + N bits")
    Nq = query.shape[0]
    ids = torch.empty((Nq, k_query), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query), dtype=torch.float32, device=base.device)
    if rescanned:
        return (ids, dists) + _certified(
            lib().ggnn_op_bf_query_filtered_certified, base, _ptr(base), _dtype_code(base),
            base.shape[0], base.shape[1], _ptr(query), Nq, k_query, measure, _ptr(ids), _ptr(dists),
            _ptr(filter_bits), filter_bit_offset)
    check(lib().ggnn_op_bf_query_filtered(_ptr(base), _dtype_code(base), base.shape[0],
                                          base.shape[1], _ptr(query), Nq, k_query, measure,
                                          _ptr(ids), _ptr(dists), _ptr(filter_bits),
                                          filter_bit_offset, _stream()))
    return ids, dists


def _need_filter_table(filter_table, filter_ids, Nq, n_bits_min):
    _need(filter_table, torch.int32, "filter_table"), _need(filter_ids, torch.int32, "filter_ids")
    if filter_table.dim() != 2 or filter_table.shape[0] == 0:
        raise ValueError("filter_table must be [F, words] with F >= 1")
    if filter_table.shape[1] * 32 < n_bits_min:
        raise ValueError("the rows of filter_table are shorter than filter_bit_offset + N bits")
    if filter_ids.dim() != 1 or filter_ids.numel() != Nq:
        raise ValueError("filter_ids must be 1-dimensional with one entry per query")


def query_filtered_by(base, query, graph0, start, nn1_stats, k_query, tau_query, filter_table,
                      filter_ids, max_iterations=400, measure=EUCLIDEAN, filter_bit_offset=0,
                      shards_per_gpu=1, on_gpu_shard=0, counters=False, prescreen=None,
                      rows_read=None):
    """`query_filtered` with one filter per query: filter_table is [F, words] packed int32 bitsets
    (ggnn_amd.pack_filters), query n searches under row filter_ids[n] (int32 CUDA tensor); id -1
    searches unfiltered and any other id outside [0, F) gives an empty result."""
    _need(base, name="base"), _need(query, base.dtype, "query")
    _need(graph0, torch.int32, "graph0"), _need(start, torch.int32, "start")
    _need(nn1_stats, torch.float32, "nn1_stats")
    Nq = query.shape[0]
    _need_filter_table(filter_table, filter_ids, Nq, filter_bit_offset + base.shape[0])
    ids = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.float32, device=base.device)
    nd = npop = None
    if counters:
        nd = torch.zeros(Nq, dtype=torch.int32, device=base.device)
        npop = torch.zeros(Nq, dtype=torch.int32, device=base.device)
    codes, params = prescreen if prescreen is not None else (None, None)
    if prescreen is not None:
        _need(base, torch.float32, "base"), _need(codes, torch.uint8, "codes")
        _need(params, torch.float32, "params")
    check(lib().ggnn_op_query_filtered_by(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(codes), _ptr(params),
        _ptr(query), Nq, _ptr(graph0), graph0.shape[1], _ptr(start), start.numel(),
        _ptr(nn1_stats), k_query, tau_query, max_iterations, measure, shards_per_gpu,
        on_gpu_shard, _ptr(ids), _ptr(dists), _ptr(nd), _ptr(npop), _ptr(rows_read),
        _ptr(filter_table), filter_table.shape[0], filter_table.shape[1] * 32, _ptr(filter_ids),
        filter_bit_offset, _stream()))
    if counters:
        return ids, dists, nd, npop
    return ids, dists


def bf_query_filtered_by(base, query, k_query, filter_table, filter_ids, measure=EUCLIDEAN,
                         filter_bit_offset=0, rescanned=False):
    """`bf_query_filtered` with one filter per query (see query_filtered_by)"""
    _need(base, name="base"), _need(query, base.dtype, "query")
    Nq = query.shape[0]
    _need_filter_table(filter_table, filter_ids, Nq, filter_bit_offset + base.shape[0])
    ids = torch.empty((Nq, k_query), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query), dtype=torch.float32, device=base.device)
    if rescanned:
        return (ids, dists) + _certified(
            lib().ggnn_op_bf_query_filtered_by_certified, base, _ptr(base), _dtype_code(base),
            base.shape[0], base.shape[1], _ptr(query), Nq, k_query, measure, _ptr(ids), _ptr(dists),
            _ptr(filter_table), filter_table.shape[0], filter_table.shape[1] * 32, _ptr(filter_ids),
            filter_bit_offset)
    check(lib().ggnn_op_bf_query_filtered_by(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(query), Nq, k_query,
        measure, _ptr(ids), _ptr(dists), _ptr(filter_table), filter_table.shape[0],
        filter_table.shape[1] * 32, _ptr(filter_ids), filter_bit_offset, _stream()))
    return ids, dists


def _need_labels(labels, query_labels, Nq, n_min):
    _need(labels, torch.int32, "labels"), _need(query_labels, torch.int32, "query_labels")
    if labels.dim() != 1 or labels.numel() < n_min:
        raise ValueError("labels must be 1-dimensional with at least bit_offset + N entries")
    if query_labels.dim() != 1 or query_labels.numel() != Nq:
        raise ValueError("query_labels must be 1-dimensional with one entry per query")


def query_labeled(base, query, graph0, start, nn1_stats, k_query, tau_query, labels,
                  query_labels, max_iterations=400, measure=EUCLIDEAN, bit_offset=0,
                  shards_per_gpu=1, on_gpu_shard=0, counters=False, prescreen=None,
                  rows_read=None):
    """`query_filtered` under label filters: labels is the int32 label column over the global ids
    (local id i has labels[i + bit_offset]), query n may be given the rows whose label equals
    query_labels[n] (int32 CUDA tensor); label -1 searches unfiltered."""
    _need(base, name="base"), _need(query, base.dtype, "query")
    _need(graph0, torch.int32, "graph0"), _need(start, torch.int32, "start")
    _need(nn1_stats, torch.float32, "nn1_stats")
    Nq = query.shape[0]
    _need_labels(labels, query_labels, Nq, bit_offset + base.shape[0])
    ids = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.float32, device=base.device)
    nd = npop = None
    if counters:
        nd = torch.zeros(Nq, dtype=torch.int32, device=base.device)
        npop = torch.zeros(Nq, dtype=torch.int32, device=base.device)
    codes, params = prescreen if prescreen is not None else (None, None)
    if prescreen is not None:
        _need(base, torch.float32, "base"), _need(codes, torch.uint8, "codes")
        _need(params, torch.float32, "params")
    check(lib().ggnn_op_query_labeled(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(codes), _ptr(params),
        _ptr(query), Nq, _ptr(graph0), graph0.shape[1], _ptr(start), start.numel(),
        _ptr(nn1_stats), k_query, tau_query, max_iterations, measure, shards_per_gpu,
        on_gpu_shard, _ptr(ids), _ptr(dists), _ptr(nd), _ptr(npop), _ptr(rows_read),
        _ptr(labels), labels.numel(), _ptr(query_labels), bit_offset, _stream()))
    if counters:
        return ids, dists, nd, npop
    return ids, dists


def bf_query_labeled(base, query, k_query, labels, query_labels, measure=EUCLIDEAN, bit_offset=0,
                     rescanned=False):
    """`bf_query_filtered` under label filters (see query_labeled)"""
    _need(base, name="base"), _need(query, base.dtype, "query")
    Nq = query.shape[0]
    _need_labels(labels, query_labels, Nq, bit_offset + base.shape[0])
    ids = torch.empty((Nq, k_query), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query), dtype=torch.float32, device=base.device)
    if rescanned:
        return (ids, dists) + _certified(
            lib().ggnn_op_bf_query_labeled_certified, base, _ptr(base), _dtype_code(base),
            base.shape[0], base.shape[1], _ptr(query), Nq, k_query, measure, _ptr(ids), _ptr(dists),
            _ptr(labels), labels.numel(), _ptr(query_labels), bit_offset)
    check(lib().ggnn_op_bf_query_labeled(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(query), Nq, k_query,
        measure, _ptr(ids), _ptr(dists), _ptr(labels), labels.numel(), _ptr(query_labels),
        bit_offset, _stream()))
    return ids, dists


def range_radii(radius, Nq, device=None):
    """`radius` of a range search as the float32 [Nq] tensor the kernels take: a scalar is broadcast
    to every query, a sequence / tensor must have one entry per query."""
    r = torch.as_tensor(radius, dtype=torch.float32)
    if r.dim() == 0:
        r = r.expand(Nq)
    if r.dim() != 1 or r.numel() != Nq:
        raise ValueError(f"radius must be a scalar or hold one entry per query ({Nq})")
    return r.to(device if device is not None else r.device).contiguous()


def sort_segments(lims, ids, dists):
    """Reorder every segment [lims[n], lims[n + 1]) of a range-search result by (distance, id) --
    what bf_query would list first.  The segments arrive in ascending id, so two stable sorts do it:
    by distance, then by segment."""
    lims = lims.to(torch.int64)
    total = int(ids.numel())
    if total == 0:
        return ids, dists
    seg = torch.repeat_interleave(torch.arange(lims.numel() - 1, device=ids.device),
                                  (lims[1:] - lims[:-1]).to(ids.device))
    by_d = torch.sort(dists, stable=True).indices
    order = by_d[torch.sort(seg[by_d], stable=True).indices]
    return ids[order], dists[order]


def bf_range_query(base, query, radius, measure=EUCLIDEAN, capacity=None, filter_bits=None,
                   filter_table=None, filter_ids=None, labels=None, query_labels=None,
                   filter_bit_offset=0, out=None):
    """Exact range search: every base row i whose filter admits it and whose distance to query n is
    <= radius[n] (float32).  The distance is the one `bf_query`'s scan reports, bit for bit: under
    EUCLIDEAN the SQUARED L2 distance -- so the radius is in squared units -- under COSINE |1 - cos|.
    radius: a scalar or [Nq]; +inf admits every allowed row, a negative or NaN radius none.
    Returns (lims, ids, dists) on the device, CSR-shaped: lims int64 [Nq + 1], the rows of query n at
    [lims[n], lims[n + 1]) in ascending id.
      capacity=None  a count-only call, one read of lims[-1] on the host, an exact allocation and a
                     second call: three distance passes in all
      capacity=c     one call into buffers of c entries (two passes; c = 0: count only, one pass),
                     nothing waits for the host: if lims[-1] > c the buffers are left untouched --
                     compare before reading them.  out=(ids, dists) gives the buffers to use.
    Filters (at most one): filter_bits (row i: bit i + filter_bit_offset), filter_table + filter_ids
    (see bf_query_filtered_by), labels + query_labels (see bf_query_labeled)."""
    _need(base, name="base"), _need(query, base.dtype, "query")
    Nq, N = query.shape[0], base.shape[0]
    radii = range_radii(radius, Nq, base.device)
    kinds = (filter_bits is not None) + (filter_ids is not None) + (query_labels is not None)
    if kinds > 1:
        raise ValueError("give at most one of filter_bits, filter_ids, query_labels")
    if filter_bits is not None:
        _need(filter_bits, torch.int32, "filter_bits")
        if filter_bits.numel() * 32 < filter_bit_offset + N:
            raise ValueError("filter_bits is shorter than filter_bit_offset + N bits")
        fn = lib().ggnn_op_bf_range_query_filtered
        tail = (_ptr(filter_bits), filter_bit_offset)
    elif filter_ids is not None:
        _need_filter_table(filter_table, filter_ids, Nq, filter_bit_offset + N)
        fn = lib().ggnn_op_bf_range_query_filtered_by
        tail = (_ptr(filter_table), filter_table.shape[0], filter_table.shape[1] * 32,
                _ptr(filter_ids), filter_bit_offset)
    elif query_labels is not None:
        _need_labels(labels, query_labels, Nq, filter_bit_offset + N)
        fn = lib().ggnn_op_bf_range_query_labeled
        tail = (_ptr(labels), labels.numel(), _ptr(query_labels), filter_bit_offset)
    else:
        fn, tail = lib().ggnn_op_bf_range_query, ()
    lims = torch.empty(Nq + 1, dtype=torch.int64, device=base.device)

    def call(cap, ids, dists):
        check(fn(_ptr(base), _dtype_code(base), N, base.shape[1], _ptr(query), Nq, _ptr(radii),
                 measure, cap, _ptr(lims), _ptr(ids), _ptr(dists), *tail, _stream()))

    if out is not None:
        ids, dists = out
        _need(ids, torch.int32, "ids"), _need(dists, torch.float32, "dists")
        cap = min(ids.numel(), dists.numel()) if capacity is None else int(capacity)
        if cap > min(ids.numel(), dists.numel()):
            raise ValueError("capacity exceeds the buffers of `out`")
        call(cap, ids, dists)
        return lims, ids, dists
    counted = capacity is None
    if counted:
        call(0, None, None)
        capacity = int(lims[-1].item())
    capacity = int(capacity)
    ids = torch.empty(capacity, dtype=torch.int32, device=base.device)
    dists = torch.empty(capacity, dtype=torch.float32, device=base.device)
    if capacity:
        call(capacity, ids, dists)
    elif not counted:
        call(0, None, None)
    return lims, ids, dists


def label_index_build(labels):
    """The index of an int32 label column (host; any CPU tensor or array of n labels, 1 <= n <= 2^30):
    (keys [L], offsets [L + 1], rows [n]) as int32 CPU tensors -- the distinct labels ascending, the
    start of every label's segment in `rows`, and the row ids sorted by (label, id).  `.cuda()` them
    for bf_query_label_index / label_index_classify."""
    import numpy as np
    col = np.ascontiguousarray(labels.cpu().numpy() if isinstance(labels, torch.Tensor) else labels)
    if col.dtype != np.int32 or col.ndim != 1:
        raise TypeError("labels must be a 1-dimensional int32 array")
    n = col.size
    keys, rows = np.empty(n, np.int32), np.empty(n, np.int32)
    offsets = np.empty(n + 1, np.uint32)
    L = C.c_uint32(0)
    check(lib().ggnn_label_index_build(col.ctypes.data, n, keys.ctypes.data, offsets.ctypes.data,
                                       rows.ctypes.data, C.byref(L)))
    L = int(L.value)
    return (torch.from_numpy(keys[:L].copy()), torch.from_numpy(offsets[:L + 1].astype(np.int32)),
            torch.from_numpy(rows))


def _need_label_index(keys, offsets, rows, query_labels, Nq, N):
    _need(keys, torch.int32, "keys"), _need(offsets, torch.int32, "offsets")
    _need(query_labels, torch.int32, "query_labels")
    if keys.dim() != 1 or keys.numel() < 1 or offsets.dim() != 1 or offsets.numel() != keys.numel() + 1:
        raise ValueError("keys [L] and offsets [L + 1] must be 1-dimensional, L >= 1")
    if rows is not None:
        _need(rows, torch.int32, "rows")
        if rows.dim() != 1 or rows.numel() != N:
            raise ValueError("rows must be 1-dimensional with one entry per base row")
    if query_labels.dim() != 1 or query_labels.numel() != Nq:
        raise ValueError("query_labels must be 1-dimensional with one entry per query")


def bf_query_label_index(base, query, k_query, keys, offsets, rows, query_labels,
                         measure=EUCLIDEAN):
    """`bf_query_labeled` through a label index (label_index_build of the column, on the device):
    every query reads only the rows of its label; every output bit equals bf_query_labeled's."""
    _need(base, name="base"), _need(query, base.dtype, "query")
    Nq = query.shape[0]
    _need_label_index(keys, offsets, rows, query_labels, Nq, base.shape[0])
    ids = torch.empty((Nq, k_query), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query), dtype=torch.float32, device=base.device)
    check(lib().ggnn_op_bf_query_label_index(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(query), Nq, k_query,
        measure, _ptr(keys), keys.numel(), _ptr(offsets), _ptr(rows), _ptr(query_labels), _ptr(ids),
        _ptr(dists), _stream()))
    return ids, dists


def label_index_classify(keys, offsets, query_labels, cutoff):
    """(routed, rest): the queries whose label is not -1 and has at most `cutoff` rows in the index
    (a label that is no key has none), and the others, each in ascending order (int32 CUDA tensors)"""
    Nq = query_labels.numel()
    _need_label_index(keys, offsets, None, query_labels, Nq, 0)
    lists = torch.empty((2, max(Nq, 1)), dtype=torch.int32, device=keys.device)
    counts = torch.zeros(2, dtype=torch.int32, device=keys.device)
    check(lib().ggnn_op_label_index_classify(
        _ptr(keys), keys.numel(), _ptr(offsets), _ptr(query_labels), Nq, int(cutoff),
        _ptr(lists[0]), _ptr(lists[1]), _ptr(counts), _stream()))
    n_routed, n_rest = (int(v) for v in counts.tolist())
    return lists[0, :n_routed], lists[1, :n_rest]


MAX_LABEL_SET = 8  # GGNN_MAX_LABEL_SET


def _need_label_rows(labels, rows, n_rows, filter_table, filter_ids, Nq, n_min):
    """the column, per-query rows (label sets or ranges, checked by the caller), table and ids of a
    seam call as the C-ABI takes them: (labels ptr, n_labels, rows ptr, n_rows, table ptr, F,
    n_bits, ids ptr)"""
    _need(labels, torch.int32, "labels")
    if labels.dim() != 1 or labels.numel() < n_min:
        raise ValueError("labels must be 1-dimensional with at least bit_offset + N entries")
    F = n_bits = 0
    if filter_table is not None:
        _need(filter_table, torch.int32, "filter_table")
        if filter_table.dim() != 2 or filter_table.shape[0] == 0:
            raise ValueError("filter_table must be [F, words] with F >= 1")
        if filter_table.shape[1] * 32 < n_min:
            raise ValueError("the rows of filter_table are shorter than bit_offset + N bits")
        F, n_bits = filter_table.shape[0], filter_table.shape[1] * 32
    if filter_ids is not None:
        _need(filter_ids, torch.int32, "filter_ids")
        if filter_ids.dim() != 1 or filter_ids.numel() != Nq:
            raise ValueError("filter_ids must be 1-dimensional with one entry per query")
    return (_ptr(labels), labels.numel(), _ptr(rows), n_rows, _ptr(filter_table), F, n_bits,
            _ptr(filter_ids))


def _need_label_sets(labels, label_sets, filter_table, filter_ids, Nq, n_min):
    """the label-set arguments of a seam call as the C-ABI takes them: (labels ptr, n_labels, sets
    ptr, set width, table ptr, F, n_bits, ids ptr)"""
    _need(label_sets, torch.int32, "label_sets")
    if label_sets.dim() != 2 or label_sets.shape[0] != Nq or \
            not 1 <= label_sets.shape[1] <= MAX_LABEL_SET:
        raise ValueError(f"label_sets must be [Nq, 1..{MAX_LABEL_SET}]")
    return _need_label_rows(labels, label_sets, label_sets.shape[1], filter_table, filter_ids, Nq,
                            n_min)


def query_labeled_in(base, query, graph0, start, nn1_stats, k_query, tau_query, labels,
                     label_sets, filter_table=None, filter_ids=None, max_iterations=400,
                     measure=EUCLIDEAN, bit_offset=0, shards_per_gpu=1, on_gpu_shard=0,
                     counters=False, prescreen=None, rows_read=None):
    """`query_labeled` with a label SET per query and, optionally, a filter id per query: labels is
    the int32 label column over the global ids (local id i has labels[i + bit_offset]), label_sets
    is [Nq, 1..8] int32 and query n may be given the rows whose label equals one of its entries (an
    entry -1 admits every label; entries may repeat) AND whose bit i + bit_offset of row
    filter_ids[n] of filter_table is set -- id -1 admits every row, any other id outside [0, F)
    none.  filter_ids=None: labels only (filter_table is then not read)."""
    _need(base, name="base"), _need(query, base.dtype, "query")
    _need(graph0, torch.int32, "graph0"), _need(start, torch.int32, "start")
    _need(nn1_stats, torch.float32, "nn1_stats")
    Nq = query.shape[0]
    tail = _need_label_sets(labels, label_sets, filter_table, filter_ids, Nq,
                            bit_offset + base.shape[0])
    ids = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.float32, device=base.device)
    nd = npop = None
    if counters:
        nd = torch.zeros(Nq, dtype=torch.int32, device=base.device)
        npop = torch.zeros(Nq, dtype=torch.int32, device=base.device)
    codes, params = prescreen if prescreen is not None else (None, None)
    if prescreen is not None:
        _need(base, torch.float32, "base"), _need(codes, torch.uint8, "codes")
        _need(params, torch.float32, "params")
    check(lib().ggnn_op_query_labeled_in(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(codes), _ptr(params),
        _ptr(query), Nq, _ptr(graph0), graph0.shape[1], _ptr(start), start.numel(),
        _ptr(nn1_stats), k_query, tau_query, max_iterations, measure, shards_per_gpu,
        on_gpu_shard, _ptr(ids), _ptr(dists), _ptr(nd), _ptr(npop), _ptr(rows_read),
        *tail, bit_offset, _stream()))
    if counters:
        return ids, dists, nd, npop
    return ids, dists


def bf_query_labeled_in(base, query, k_query, labels, label_sets, filter_table=None,
                        filter_ids=None, measure=EUCLIDEAN, bit_offset=0):
    """`bf_query_filtered` under label sets (see query_labeled_in); always the scan kernels"""
    _need(base, name="base"), _need(query, base.dtype, "query")
    Nq = query.shape[0]
    tail = _need_label_sets(labels, label_sets, filter_table, filter_ids, Nq,
                            bit_offset + base.shape[0])
    ids = torch.empty((Nq, k_query), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query), dtype=torch.float32, device=base.device)
    check(lib().ggnn_op_bf_query_labeled_in(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(query), Nq, k_query,
        measure, _ptr(ids), _ptr(dists), *tail, bit_offset, _stream()))
    return ids, dists


MAX_LABEL_RANGES = 4  # GGNN_MAX_LABEL_RANGES


def _need_label_ranges(labels, label_ranges, filter_table, filter_ids, Nq, n_min):
    """the label-range arguments of a seam call as the C-ABI takes them: (labels ptr, n_labels,
    ranges ptr, n_ranges, table ptr, F, n_bits, ids ptr)"""
    _need(label_ranges, torch.int32, "label_ranges")
    if label_ranges.dim() != 3 or label_ranges.shape[0] != Nq or label_ranges.shape[2] != 2 or \
            not 1 <= label_ranges.shape[1] <= MAX_LABEL_RANGES:
        raise ValueError(f"label_ranges must be [Nq, 1..{MAX_LABEL_RANGES}, 2]")
    return _need_label_rows(labels, label_ranges, label_ranges.shape[1], filter_table, filter_ids,
                            Nq, n_min)


def query_labeled_range(base, query, graph0, start, nn1_stats, k_query, tau_query, labels,
                        label_ranges, filter_table=None, filter_ids=None, max_iterations=400,
                        measure=EUCLIDEAN, bit_offset=0, shards_per_gpu=1, on_gpu_shard=0,
                        counters=False, prescreen=None, rows_read=None):
    """`query_labeled_in` with label RANGES in place of label sets: label_ranges is [Nq, 1..4, 2]
    int32, closed intervals (lo, hi), and query n may be given the rows with lo <= labels[i +
    bit_offset] <= hi (signed) for one of its intervals AND whose bit i + bit_offset of row
    filter_ids[n] of filter_table is set -- id -1 admits every row, any other id outside [0, F)
    none.  lo > hi is an empty interval; there is no wildcard value (-1 is an ordinary label).
    filter_ids=None: ranges only (filter_table is then not read)."""
    _need(base, name="base"), _need(query, base.dtype, "query")
    _need(graph0, torch.int32, "graph0"), _need(start, torch.int32, "start")
    _need(nn1_stats, torch.float32, "nn1_stats")
    Nq = query.shape[0]
    tail = _need_label_ranges(labels, label_ranges, filter_table, filter_ids, Nq,
                              bit_offset + base.shape[0])
    ids = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.float32, device=base.device)
    nd = npop = None
    if counters:
        nd = torch.zeros(Nq, dtype=torch.int32, device=base.device)
        npop = torch.zeros(Nq, dtype=torch.int32, device=base.device)
    codes, params = prescreen if prescreen is not None else (None, None)
    if prescreen is not None:
        _need(base, torch.float32, "base"), _need(codes, torch.uint8, "codes")
        _need(params, torch.float32, "params")
    check(lib().ggnn_op_query_labeled_range(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(codes), _ptr(params),
        _ptr(query), Nq, _ptr(graph0), graph0.shape[1], _ptr(start), start.numel(),
        _ptr(nn1_stats), k_query, tau_query, max_iterations, measure, shards_per_gpu,
        on_gpu_shard, _ptr(ids), _ptr(dists), _ptr(nd), _ptr(npop), _ptr(rows_read),
        *tail, bit_offset, _stream()))
    if counters:
        return ids, dists, nd, npop
    return ids, dists


def bf_query_labeled_range(base, query, k_query, labels, label_ranges, filter_table=None,
                           filter_ids=None, measure=EUCLIDEAN, bit_offset=0):
    """`bf_query_filtered` under label ranges (see query_labeled_range); always the scan kernels"""
    _need(base, name="base"), _need(query, base.dtype, "query")
    Nq = query.shape[0]
    tail = _need_label_ranges(labels, label_ranges, filter_table, filter_ids, Nq,
                              bit_offset + base.shape[0])
    ids = torch.empty((Nq, k_query), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query), dtype=torch.float32, device=base.device)
    check(lib().ggnn_op_bf_query_labeled_range(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(query), Nq, k_query,
        measure, _ptr(ids), _ptr(dists), *tail, bit_offset, _stream()))
    return ids, dists


MAX_LABEL_SPANS = 8


def label_spans_resolve(keys, offsets, label_sets=None, label_ranges=None):
    """The label sets ([Nq, 1..8] int32, as query_labeled_in takes them) or the label ranges ([Nq,
    1..4, 2] int32, as query_labeled_range) of a batch as spans of positions into `rows` of a label
    index: (spans [Nq, 8, 2] int32, totals [Nq] int32).  Exactly one of the two is given.  The spans
    of a query are sorted, disjoint, never touching and non-empty, unused slots are (0, 0) at the
    tail, and totals[n] is the number of rows query n will read."""
    if (label_sets is None) == (label_ranges is None):
        raise ValueError("give label_sets or label_ranges, one of the two")
    _need(keys, torch.int32, "keys"), _need(offsets, torch.int32, "offsets")
    if keys.dim() != 1 or keys.numel() < 1 or offsets.dim() != 1 or offsets.numel() != keys.numel() + 1:
        raise ValueError("keys [L] and offsets [L + 1] must be 1-dimensional, L >= 1")
    if label_sets is not None:
        sel, mode = _need(label_sets, torch.int32, "label_sets"), 0
        if sel.dim() != 2 or not 1 <= sel.shape[1] <= MAX_LABEL_SET:
            raise ValueError(f"label_sets must be [Nq, 1..{MAX_LABEL_SET}]")
    else:
        sel, mode = _need(label_ranges, torch.int32, "label_ranges"), 1
        if sel.dim() != 3 or sel.shape[2] != 2 or not 1 <= sel.shape[1] <= MAX_LABEL_RANGES:
            raise ValueError(f"label_ranges must be [Nq, 1..{MAX_LABEL_RANGES}, 2]")
    Nq = sel.shape[0]
    spans = torch.empty((Nq, MAX_LABEL_SPANS, 2), dtype=torch.int32, device=keys.device)
    totals = torch.empty(Nq, dtype=torch.int32, device=keys.device)
    check(lib().ggnn_op_label_spans_resolve(_ptr(keys), keys.numel(), _ptr(offsets), mode, _ptr(sel),
                                            sel.shape[1], Nq, _ptr(spans), _ptr(totals), _stream()))
    return spans, totals


def bf_query_label_spans(base, query, k_query, rows, spans, filter_table=None, filter_ids=None,
                         measure=EUCLIDEAN, span_limit=0):
    """The exact k_query nearest of every query among the rows at the positions of its spans
    (label_spans_resolve) of `rows` (label_index_build), and -- with filter_ids -- whose bit of row
    filter_ids[n] of filter_table is set (id -1 admits every row, any other id outside [0, F) none).
    Ranked by (distance, id): every output bit equals bf_query_labeled_in / bf_query_labeled_range on
    the same column.  Every element type, int8 included.  span_limit: the cutoff the batch was
    classified with (0: unknown); it sizes the slices only."""
    _need(base, name="base"), _need(query, base.dtype, "query")
    Nq, N = query.shape[0], base.shape[0]
    _need(rows, torch.int32, "rows"), _need(spans, torch.int32, "spans")
    if rows.dim() != 1 or rows.numel() != N:
        raise ValueError("rows must be 1-dimensional with one entry per base row")
    if spans.dim() != 3 or tuple(spans.shape) != (Nq, MAX_LABEL_SPANS, 2):
        raise ValueError(f"spans must be [Nq, {MAX_LABEL_SPANS}, 2]")
    F = n_bits = 0
    if filter_table is not None:
        _need(filter_table, torch.int32, "filter_table")
        if filter_table.dim() != 2 or filter_table.shape[0] == 0:
            raise ValueError("filter_table must be [F, words] with F >= 1")
        if filter_table.shape[1] * 32 < N:
            raise ValueError("the rows of filter_table are shorter than N bits")
        F, n_bits = filter_table.shape[0], filter_table.shape[1] * 32
    if filter_ids is not None:
        _need(filter_ids, torch.int32, "filter_ids")
        if filter_ids.dim() != 1 or filter_ids.numel() != Nq:
            raise ValueError("filter_ids must be 1-dimensional with one entry per query")
    ids = torch.empty((Nq, k_query), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query), dtype=torch.float32, device=base.device)
    check(lib().ggnn_op_bf_query_label_spans(
        _ptr(base), _dtype_code(base), N, base.shape[1], _ptr(query), Nq, k_query, measure,
        _ptr(rows), _ptr(spans), int(span_limit), _ptr(filter_table), F, n_bits, _ptr(filter_ids),
        _ptr(ids), _ptr(dists), _stream()))
    return ids, dists


def label_spans_classify(totals, cutoff):
    """(routed, rest): the queries with totals[n] <= cutoff and the others, each in ascending order
    (int32 CUDA tensors); totals as label_spans_resolve gives them"""
    _need(totals, torch.int32, "totals")
    if totals.dim() != 1:
        raise ValueError("totals must be 1-dimensional")
    Nq = totals.numel()
    lists = torch.empty((2, max(Nq, 1)), dtype=torch.int32, device=totals.device)
    counts = torch.zeros(2, dtype=torch.int32, device=totals.device)
    check(lib().ggnn_op_label_spans_classify(_ptr(totals), Nq, int(cutoff), _ptr(lists[0]),
                                             _ptr(lists[1]), _ptr(counts), _stream()))
    n_routed, n_rest = (int(v) for v in counts.tolist())
    return lists[0, :n_routed], lists[1, :n_rest]


def bf_query_label_index_in(base, query, k_query, keys, offsets, rows, label_sets,
                            filter_table=None, filter_ids=None, measure=EUCLIDEAN, span_limit=0):
    """`bf_query_labeled_in` through a label index: label_spans_resolve, then bf_query_label_spans"""
    spans, _ = label_spans_resolve(keys, offsets, label_sets=label_sets)
    return bf_query_label_spans(base, query, k_query, rows, spans, filter_table, filter_ids, measure,
                                span_limit)


def bf_query_label_index_range(base, query, k_query, keys, offsets, rows, label_ranges,
                               filter_table=None, filter_ids=None, measure=EUCLIDEAN, span_limit=0):
    """`bf_query_labeled_range` through a label index: label_spans_resolve, then
    bf_query_label_spans"""
    spans, _ = label_spans_resolve(keys, offsets, label_ranges=label_ranges)
    return bf_query_label_spans(base, query, k_query, rows, spans, filter_table, filter_ids, measure,
                                span_limit)


MAX_LABEL_MASKS = 2  # GGNN_MAX_LABEL_MASKS


def _need_label_masks(labels, label_masks, filter_table, filter_ids, Nq, n_min):
    """the label-mask arguments of a seam call as the C-ABI takes them: (labels ptr, n_labels,
    clauses ptr, n_masks, table ptr, F, n_bits, ids ptr)"""
    _need(label_masks, torch.int32, "label_masks")
    if label_masks.dim() != 3 or label_masks.shape[0] != Nq or label_masks.shape[2] != 3 or \
            not 1 <= label_masks.shape[1] <= MAX_LABEL_MASKS:
        raise ValueError(f"label_masks must be [Nq, 1..{MAX_LABEL_MASKS}, 3]")
    return _need_label_rows(labels, label_masks, label_masks.shape[1], filter_table, filter_ids,
                            Nq, n_min)


def query_labeled_mask(base, query, graph0, start, nn1_stats, k_query, tau_query, labels,
                       label_masks, filter_table=None, filter_ids=None, max_iterations=400,
                       measure=EUCLIDEAN, bit_offset=0, shards_per_gpu=1, on_gpu_shard=0,
                       counters=False, prescreen=None, rows_read=None):
    """`query_labeled_range` with label MASKS in place of label ranges: the label is read as 32 tag
    bits, label_masks is [Nq, 1..2, 3] int32, clauses (mask, value, any), and query n may be given
    the rows whose label L = labels[i + bit_offset] has (L & mask) == value and (any == 0 or
    (L & any) != 0) for one of its clauses AND whose bit i + bit_offset of row filter_ids[n] of
    filter_table is set -- id -1 admits every row, any other id outside [0, F) none.  value is
    never pre-masked (a bit outside mask admits nothing); there is no wildcard value.
    filter_ids=None: clauses only (filter_table is then not read)."""
    _need(base, name="base"), _need(query, base.dtype, "query")
    _need(graph0, torch.int32, "graph0"), _need(start, torch.int32, "start")
    _need(nn1_stats, torch.float32, "nn1_stats")
    Nq = query.shape[0]
    tail = _need_label_masks(labels, label_masks, filter_table, filter_ids, Nq,
                             bit_offset + base.shape[0])
    ids = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query * shards_per_gpu), dtype=torch.float32, device=base.device)
    nd = npop = None
    if counters:
        nd = torch.zeros(Nq, dtype=torch.int32, device=base.device)
        npop = torch.zeros(Nq, dtype=torch.int32, device=base.device)
    codes, params = prescreen if prescreen is not None else (None, None)
    if prescreen is not None:
        _need(base, torch.float32, "base"), _need(codes, torch.uint8, "codes")
        _need(params, torch.float32, "params")
    check(lib().ggnn_op_query_labeled_mask(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(codes), _ptr(params),
        _ptr(query), Nq, _ptr(graph0), graph0.shape[1], _ptr(start), start.numel(),
        _ptr(nn1_stats), k_query, tau_query, max_iterations, measure, shards_per_gpu,
        on_gpu_shard, _ptr(ids), _ptr(dists), _ptr(nd), _ptr(npop), _ptr(rows_read),
        *tail, bit_offset, _stream()))
    if counters:
        return ids, dists, nd, npop
    return ids, dists


def bf_query_labeled_mask(base, query, k_query, labels, label_masks, filter_table=None,
                          filter_ids=None, measure=EUCLIDEAN, bit_offset=0):
    """`bf_query_filtered` under label masks (see query_labeled_mask); always the scan kernels"""
    _need(base, name="base"), _need(query, base.dtype, "query")
    Nq = query.shape[0]
    tail = _need_label_masks(labels, label_masks, filter_table, filter_ids, Nq,
                             bit_offset + base.shape[0])
    ids = torch.empty((Nq, k_query), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query), dtype=torch.float32, device=base.device)
    check(lib().ggnn_op_bf_query_labeled_mask(
        _ptr(base), _dtype_code(base), base.shape[0], base.shape[1], _ptr(query), Nq, k_query,
        measure, _ptr(ids), _ptr(dists), *tail, bit_offset, _stream()))
    return ids, dists


def pack_filters(masks):
    """[F, N] boolean CUDA masks -> [F, ceil(N / 32)] int32 bitset words on the same GPU (bit
    i & 31 of word i >> 5 is mask i; padding bits zero)"""
    _need(masks, torch.bool, "masks")
    if masks.dim() != 2:
        raise ValueError("masks must be [F, N]")
    F, N = masks.shape
    words = torch.empty((F, (N + 31) // 32), dtype=torch.int32, device=masks.device)
    with torch.cuda.device(masks.device):
        check(lib().ggnn_op_pack_filters(_ptr(masks), F, N, _ptr(words), _stream()))
    return words


def bf_query(base, query, k_query, measure=EUCLIDEAN, rescanned=False):
    """rescanned=True: also return how many queries the matrix-core path handed to the scan"""
    _need(base, name="base"), _need(query, base.dtype, "query")
    Nq = query.shape[0]
    ids = torch.empty((Nq, k_query), dtype=torch.int32, device=base.device)
    dists = torch.empty((Nq, k_query), dtype=torch.float32, device=base.device)
    if rescanned:
        n = torch.zeros(1, dtype=torch.int32, device=base.device)
        check(lib().ggnn_op_bf_query_certified(_ptr(base), _dtype_code(base), base.shape[0],
                                               base.shape[1], _ptr(query), Nq, k_query, measure,
                                               _ptr(ids), _ptr(dists), _ptr(n), _stream()))
        return ids, dists, int(n.item())
    check(lib().ggnn_op_bf_query(_ptr(base), _dtype_code(base), base.shape[0], base.shape[1],
                                 _ptr(query), Nq, k_query, measure, _ptr(ids), _ptr(dists),
                                 _stream()))
    return ids, dists


def top(base, KBuild, translation_layer, N_layer, S, S_offset, layer, measure=EUCLIDEAN):
    _need(base, name="base")
    graph = torch.empty((N_layer, KBuild), dtype=torch.int32, device=base.device)
    nn1 = torch.empty(N_layer, dtype=torch.float32, device=base.device)
    check(lib().ggnn_op_top(_ptr(base), _dtype_code(base), base.shape[1], measure, KBuild,
                            _ptr(translation_layer), N_layer, S, S_offset, layer, _ptr(graph),
                            _ptr(nn1), _stream()))
    return graph, nn1


def merge(base, cfg, graph_all, translation_all, selection_all, nn1_stats, tau_build, layer_top,
          layer_btm, measure=EUCLIDEAN, counters=False, prescreen=None):
    _need(base, name="base"), _need(graph_all, torch.int32, "graph_all")
    _need(translation_all, torch.int32), _need(selection_all, torch.int32)
    Nb = cfg.Ns[layer_btm]
    gb = torch.empty((Nb, cfg.KBuild), dtype=torch.int32, device=base.device)
    nn1 = torch.zeros(Nb, dtype=torch.float32, device=base.device)
    nd = torch.zeros(Nb, dtype=torch.int32, device=base.device) if counters else None
    if prescreen is not None:
        codes, params = prescreen
        _need(base, torch.float32, "base"), _need(codes, torch.uint8, "codes")
        _need(params, torch.float32, "params")
        check(lib().ggnn_op_merge_prescreened(
            _ptr(base), _ptr(codes), _ptr(params), measure, _cfg(cfg), _ptr(graph_all),
            _ptr(translation_all), _ptr(selection_all), _ptr(nn1_stats), tau_build, layer_top,
            layer_btm, _ptr(gb), _ptr(nn1), _ptr(nd), _stream()))
    else:
        check(lib().ggnn_op_merge(_ptr(base), _dtype_code(base), measure, _cfg(cfg),
                                  _ptr(graph_all), _ptr(translation_all), _ptr(selection_all),
                                  _ptr(nn1_stats), tau_build, layer_top, layer_btm, _ptr(gb),
                                  _ptr(nn1), _ptr(nd), _stream()))
    if counters:
        return gb, nn1, nd
    return gb, nn1


def select(cfg, layer, nn1_dist_buffer, rng, translation_all, selection_all):
    check(lib().ggnn_op_select(_cfg(cfg), layer, _ptr(nn1_dist_buffer), _ptr(rng),
                               _ptr(translation_all), _ptr(selection_all), _stream()))


def uniform(n, seed=1234, stream_id=0, device="cuda"):
    out = torch.empty(n, dtype=torch.float32, device=device)
    check(lib().ggnn_op_uniform(_ptr(out), n, seed, stream_id, _stream()))
    return out


def sym(base, KBuild, graph_layer, translation_layer, nn1_stats, tau_build, sym_buffer,
        sym_atomic, measure=EUCLIDEAN, first_n=0, count=None, prescreen=None, requests=None):
    """prescreen: optional (codes, params) of prescreen_encode(base, measure) (float32);
    requests: optional int32 [N_layer, KL, KF] tensor: the request pass of the deterministic sym
    schedule, which fills it and leaves sym_buffer / sym_atomic alone (ggnn_op_sym_requests)"""
    N_layer = graph_layer.shape[0]
    if count is None:
        count = N_layer
    if requests is not None:
        KF = KBuild // 2
        _need(requests, torch.int32, "requests")
        if requests.numel() != N_layer * (KBuild - KF) * KF:
            raise ValueError("requests must have N_layer x KL x KF entries")
        codes, params = prescreen if prescreen is not None else (None, None)
        check(lib().ggnn_op_sym_requests(_ptr(base), _dtype_code(base), _ptr(codes), _ptr(params),
                                         measure, base.shape[1], KBuild, _ptr(graph_layer),
                                         _ptr(translation_layer), N_layer, _ptr(nn1_stats),
                                         tau_build, _ptr(sym_buffer), _ptr(sym_atomic),
                                         _ptr(requests), first_n, count, _stream()))
        return
    if prescreen is not None:
        codes, params = prescreen
        check(lib().ggnn_op_sym_prescreened(_ptr(base), _ptr(codes), _ptr(params), measure,
                                            base.shape[1], KBuild, _ptr(graph_layer),
                                            _ptr(translation_layer), N_layer, _ptr(nn1_stats),
                                            tau_build, _ptr(sym_buffer), _ptr(sym_atomic), first_n,
                                            count, _stream()))
        return
    check(lib().ggnn_op_sym(_ptr(base), _dtype_code(base), measure, base.shape[1], KBuild,
                            _ptr(graph_layer), _ptr(translation_layer), N_layer, _ptr(nn1_stats),
                            tau_build, _ptr(sym_buffer), _ptr(sym_atomic), first_n, count,
                            _stream()))


def sym_assign(KBuild, requests, sym_atomic, sym_buffer):
    """assign step of the deterministic sym schedule (ggnn_op_sym_assign), in place on sym_atomic
    [N_layer] / sym_buffer [N_layer, KF]"""
    _need(requests, torch.int32, "requests"), _need(sym_buffer, torch.int32, "sym_buffer")
    _need(sym_atomic, torch.int32, "sym_atomic")
    N_layer, KF = sym_atomic.numel(), KBuild // 2
    if sym_buffer.numel() != N_layer * KF or requests.numel() != N_layer * (KBuild - KF) * KF:
        raise ValueError("sym_assign: sym_buffer is [N, KF], requests [N, KL, KF]")
    check(lib().ggnn_op_sym_assign(KBuild, N_layer, _ptr(requests), _ptr(sym_atomic),
                                   _ptr(sym_buffer), _stream()))


def sym_buffer_merge(KBuild, sym_buffer, sym_atomic, graph_layer):
    check(lib().ggnn_op_sym_buffer_merge(KBuild, graph_layer.shape[0], _ptr(sym_buffer),
                                         _ptr(sym_atomic), _ptr(graph_layer), _stream()))


def nn1_stats(nn1_dist_buffer):
    scratch = torch.empty(lib().ggnn_nn1_stats_scratch_floats(), dtype=torch.float32,
                          device=nn1_dist_buffer.device)
    out = torch.empty(2, dtype=torch.float32, device=nn1_dist_buffer.device)
    check(lib().ggnn_op_nn1_stats(_ptr(nn1_dist_buffer), nn1_dist_buffer.numel(), _ptr(scratch),
                                  _ptr(out), _stream()))
    return out


def sort_shard_results(ids, dists):
    """in place"""
    check(lib().ggnn_op_sort_shard_results(ids.shape[0], ids.shape[1], _ptr(ids), _ptr(dists),
                                           _stream()))
    return ids, dists


def merge_results(parts_ids, parts_dists, k, id_offset_per_part):
    """parts_*: [num_parts, Nq, stride] (e.g. the all-gather buffer)"""
    _need(parts_ids, torch.int32), _need(parts_dists, torch.float32)
    P, Nq, stride = parts_ids.shape
    ids = torch.empty((Nq, k), dtype=torch.int32, device=parts_ids.device)
    dists = torch.empty((Nq, k), dtype=torch.float32, device=parts_ids.device)
    check(lib().ggnn_op_merge_results(Nq, k, P, stride, id_offset_per_part, _ptr(parts_ids),
                                      _ptr(parts_dists), _ptr(ids), _ptr(dists), _stream()))
    return ids, dists
