"""Python surface of the engine: same names, argument order and defaults as the reference's
nanobind module (src/ggnn/python/nanobind.cu:131-301), implemented over the C-ABI.

    import ggnn_amd as ggnn            # or `import ggnn` through the shim package
    g = ggnn.GGNN(); g.set_base(base); g.build(24, 0.5)
    indices, dists = g.query(query, 10, 0.64, 400)

Inputs may be numpy arrays or torch tensors (CPU or CUDA), C-contiguous 2-D float32/uint8/int8/
float16/bfloat16 (bfloat16 through torch only: numpy has no such type);
results are torch tensors like the reference's (nb::pytorch ndarrays), int32 ids and float32
SQUARED L2 (or |1-cos|) distances.
"""
import ctypes as C
import enum
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, lib


class DistanceMeasure(enum.IntEnum):
    """include/ggnn/base/def.h:27-30"""
    Euclidean = 0
    Cosine = 1


def set_log_level(level: int) -> None:
    """nanobind.cu:151"""
    lib().ggnn_set_log_level(int(level))


_NP_OF = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int8: np.int8,
          torch.int32: np.int32}


def _as_tensor(data, dtype=None, what="data"):
    """ndarray_to_dataset (nanobind.cu:102-110): 2-D, C-contiguous, CPU or CUDA."""
    if isinstance(data, _Dataset):
        data = data._t
    if isinstance(data, np.ndarray):
        data = torch.from_numpy(np.ascontiguousarray(data))
    if not isinstance(data, torch.Tensor):
        raise TypeError(f"{what} must be a numpy array, a torch tensor or a ggnn dataset")
    if data.dim() != 2:
        raise TypeError(f"{what} must be 2-dimensional")
    if dtype is not None and data.dtype != dtype:
        raise TypeError(f"{what} must have dtype {dtype}")
    if not data.is_contiguous():
        raise TypeError(f"{what} must be C-contiguous")
    return data


def _loc(t):
    if t.is_cuda:
        torch.cuda.current_stream(t.device).synchronize()
        return _lib.GPU, t.device.index if t.device.index is not None else 0
    return _lib.CPU, 0


_DTYPE_CODES = {torch.float32: _lib.F32, torch.uint8: _lib.U8, torch.float16: _lib.F16,
                torch.bfloat16: _lib.BF16, torch.int8: _lib.I8}


def _dtype_code(t):
    code = _DTYPE_CODES.get(t.dtype)
    if code is None:
        raise TypeError("unsupported datatype (int8, float32, uint8, float16 and bfloat16 are "
                        "supported)")
    return code


def _host_rows(t):
    """numpy rows of a CPU tensor; 16-bit rows widened to float32 (exact; numpy has no
    bfloat16)"""
    if t.dtype in (torch.float16, torch.bfloat16):
        t = t.float()
    return t.numpy()


def pack_filter(mask):
    """Pack a boolean mask over the base ids (numpy / torch, length N) into the bitset of the
    filtered calls: int32 words, id i is allowed iff bit (i & 31) of word (i >> 5) is set,
    ceil(N / 32) words, padding bits zero.  Returns a CPU torch.int32 tensor."""
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().cpu().numpy()
    mask = np.asarray(mask)
    if mask.dtype != np.bool_ or mask.ndim != 1:
        raise TypeError("mask must be a 1-dimensional boolean array")
    packed = np.packbits(mask, bitorder="little")
    words = np.zeros((mask.size + 31) // 32 * 4, np.uint8)
    words[:packed.size] = packed
    return torch.from_numpy(words.view(np.int32).copy())


def pack_filters(masks):
    """Pack F boolean masks over the base ids ([F, N], numpy / torch) into a filter table for
    `GGNN.set_filters`: int32 words [F, ceil(N / 32)], row f is `pack_filter(masks[f])`.  The
    result lives where the masks live: CUDA masks are packed on their GPU (one ballot per 64
    rows, no host round trip), anything else on the host."""
    if isinstance(masks, np.ndarray):
        masks = torch.from_numpy(np.ascontiguousarray(masks))
    if not isinstance(masks, torch.Tensor) or masks.dtype != torch.bool or masks.dim() != 2:
        raise TypeError("masks must be a 2-dimensional boolean array [F, N]")
    F, N = masks.shape
    words = (N + 31) // 32
    if masks.is_cuda:
        from . import ops
        return ops.pack_filters(masks)
    m = masks.detach().numpy()
    out = np.zeros((F, words * 4), np.uint8)
    if N:
        packed = np.packbits(m, axis=1, bitorder="little")
        out[:, :packed.shape[1]] = packed
    return torch.from_numpy(out.view(np.int32).reshape(F, words).copy())


def _filter_table(filters, N):
    """the `filters` argument of set_filters as a contiguous int32 tensor [F, ceil(N / 32)] (CPU or
    CUDA): boolean masks [F, N] are packed where they live, int32 / uint32 words are taken as
    already packed"""
    if isinstance(filters, np.ndarray) and filters.dtype == np.uint32:
        filters = filters.view(np.int32)
    if isinstance(filters, np.ndarray):
        filters = torch.from_numpy(np.ascontiguousarray(filters))
    if not isinstance(filters, torch.Tensor) or filters.dim() != 2:
        raise TypeError("filters must be a 2-dimensional numpy array or torch tensor")
    if filters.dtype == torch.bool:
        if filters.shape[1] != N:
            raise ValueError(f"boolean filters need one column per base vector ({N})")
        return pack_filters(filters)
    if hasattr(torch, "uint32") and filters.dtype == torch.uint32:
        filters = filters.view(torch.int32)
    if filters.dtype != torch.int32:
        raise TypeError("filters must be boolean, or int32 / uint32 words of packed bitsets")
    if filters.shape[1] != (N + 31) // 32:
        raise ValueError(f"packed filters need ceil(N / 32) = {(N + 31) // 32} words per row")
    return filters.contiguous()


def _filter_ids(filter_ids, Nq):
    """the `filter_ids` argument as a contiguous 1-D int32 tensor of length Nq (int64 is converted)"""
    if isinstance(filter_ids, np.ndarray):
        filter_ids = torch.from_numpy(np.ascontiguousarray(filter_ids))
    if not isinstance(filter_ids, torch.Tensor) or filter_ids.dim() != 1:
        raise TypeError("filter_ids must be a 1-dimensional numpy array or torch tensor")
    if filter_ids.dtype == torch.int64:
        filter_ids = filter_ids.to(torch.int32)
    if filter_ids.dtype != torch.int32:
        raise TypeError("filter_ids must be int32 (or int64)")
    if filter_ids.numel() != Nq:
        raise ValueError(f"filter_ids needs one entry per query ({Nq})")
    return filter_ids.contiguous()


_INT32_MIN, _INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _labels(labels, n, what="labels", per="base vector"):
    """a label argument as a contiguous 1-D int32 tensor of length n (CPU or CUDA): int32 is taken
    as it is, int64 is converted when every value fits int32 (ValueError otherwise)"""
    if isinstance(labels, np.ndarray):
        labels = torch.from_numpy(np.ascontiguousarray(labels))
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1:
        raise TypeError(f"{what} must be a 1-dimensional numpy array or torch tensor")
    if labels.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what} must be int32 (or int64 with values that fit int32)")
    if labels.numel() != n:
        raise ValueError(f"{what} needs one entry per {per} ({n})")
    if labels.dtype == torch.int64:
        if labels.numel() and (int(labels.min()) < _INT32_MIN or int(labels.max()) > _INT32_MAX):
            raise ValueError(f"{what} has values outside the int32 range")
        labels = labels.to(torch.int32)
    return labels.contiguous()


MAX_LABEL_SET = 8  # GGNN_MAX_LABEL_SET


def _label_sets(label_sets, Nq):
    """the `label_sets` argument as a contiguous [Nq, 1..8] int32 tensor (CPU or CUDA): a 2-D int32 /
    int64 array or tensor is taken as it is (int64 must fit int32); anything else is read as one
    sequence of 1..8 labels per query and padded to the longest row by repeating each row's first
    entry"""
    if isinstance(label_sets, np.ndarray):
        label_sets = torch.from_numpy(np.ascontiguousarray(label_sets))
    if not isinstance(label_sets, torch.Tensor):
        rows = [[int(v) for v in (r.tolist() if hasattr(r, "tolist") else r)] for r in label_sets]
        for n, r in enumerate(rows):
            if not 1 <= len(r) <= MAX_LABEL_SET:
                raise ValueError(f"the label set of query {n} has {len(r)} entries: 1 to "
                                 f"{MAX_LABEL_SET} are allowed")
        width = max((len(r) for r in rows), default=1)
        label_sets = torch.tensor([r + r[:1] * (width - len(r)) for r in rows],
                                  dtype=torch.int64).reshape(len(rows), width)
    if label_sets.dim() != 2:
        raise TypeError("label_sets must be 2-dimensional, or a sequence of per-query sequences")
    if label_sets.dtype not in (torch.int32, torch.int64):
        raise TypeError("label_sets must be int32 (or int64 with values that fit int32)")
    if label_sets.shape[0] != Nq:
        raise ValueError(f"label_sets needs one row per query ({Nq})")
    if not 1 <= label_sets.shape[1] <= MAX_LABEL_SET:
        raise ValueError(f"a label set has 1 to {MAX_LABEL_SET} entries, not "
                         f"{label_sets.shape[1]}")
    if label_sets.dtype == torch.int64:
        if label_sets.numel() and (int(label_sets.min()) < _INT32_MIN or
                                   int(label_sets.max()) > _INT32_MAX):
            raise ValueError("label_sets has values outside the int32 range")
        label_sets = label_sets.to(torch.int32)
    return label_sets.contiguous()


MAX_LABEL_RANGES = 4  # GGNN_MAX_LABEL_RANGES
_EMPTY_RANGE = (1, 0)  # lo > hi: contains nothing


def _label_ranges(label_ranges, Nq):
    """the `label_ranges` argument as a contiguous [Nq, 1..4, 2] int32 tensor (CPU or CUDA) of closed
    intervals (lo, hi): a 3-D int32 / int64 array or tensor is taken as it is (int64 must fit int32);
    anything else is read as one sequence of 1..4 (lo, hi) pairs per query and padded to the longest
    row with an empty interval"""
    if isinstance(label_ranges, np.ndarray):
        label_ranges = torch.from_numpy(np.ascontiguousarray(label_ranges))
    if not isinstance(label_ranges, torch.Tensor):
        rows = [[tuple(int(v) for v in (p.tolist() if hasattr(p, "tolist") else p)) for p in r]
                for r in label_ranges]
        for n, r in enumerate(rows):
            if not 1 <= len(r) <= MAX_LABEL_RANGES:
                raise ValueError(f"query {n} has {len(r)} label ranges: 1 to "
                                 f"{MAX_LABEL_RANGES} are allowed")
            if any(len(p) != 2 for p in r):
                raise ValueError(f"the label ranges of query {n} must be (lo, hi) pairs")
        width = max((len(r) for r in rows), default=1)
        label_ranges = torch.tensor([r + [_EMPTY_RANGE] * (width - len(r)) for r in rows],
                                    dtype=torch.int64).reshape(len(rows), width, 2)
    if label_ranges.dim() != 3 or label_ranges.shape[2] != 2:
        raise TypeError("label_ranges must be [Nq, R, 2], or a sequence of per-query sequences of "
                        "(lo, hi) pairs")
    if label_ranges.dtype not in (torch.int32, torch.int64):
        raise TypeError("label_ranges must be int32 (or int64 with values that fit int32)")
    if label_ranges.shape[0] != Nq:
        raise ValueError(f"label_ranges needs one row per query ({Nq})")
    if not 1 <= label_ranges.shape[1] <= MAX_LABEL_RANGES:
        raise ValueError(f"a query has 1 to {MAX_LABEL_RANGES} label ranges, not "
                         f"{label_ranges.shape[1]}")
    if label_ranges.dtype == torch.int64:
        if label_ranges.numel() and (int(label_ranges.min()) < _INT32_MIN or
                                     int(label_ranges.max()) > _INT32_MAX):
            raise ValueError("label_ranges has values outside the int32 range")
        label_ranges = label_ranges.to(torch.int32)
    return label_ranges.contiguous()


MAX_LABEL_MASKS = 2  # GGNN_MAX_LABEL_MASKS
_UINT32_MAX = 2 ** 32 - 1


def _wrap_int32(v):
    """an integer in [-2**31, 2**32) as the int32 with the same low 32 bits"""
    return v - 2 ** 32 if v > _INT32_MAX else v


def _label_masks(label_masks, Nq):
    """the `label_masks` argument as a contiguous [Nq, 1..2, 3] int32 tensor (CPU or CUDA) of clauses
    (mask, value, any): a 3-D [Nq, 1..2, 3] or 2-D [Nq, 3] int32 / int64 array or tensor is taken as
    it is; anything else is read as one sequence of 1 or 2 triples per query and padded to the
    longest row by repeating the row's first triple.  Values in [-2**31, 2**32) are accepted and
    wrapped to int32, so 0x80000000 can be written as it reads."""
    if isinstance(label_masks, np.ndarray):
        if label_masks.dtype in (np.uint32, np.uint64):
            raise TypeError("label_masks must be int32 or int64 (values up to 2**32 - 1 wrap)")
        label_masks = torch.from_numpy(np.ascontiguousarray(label_masks))
    if not isinstance(label_masks, torch.Tensor):
        rows = [[tuple(int(v) for v in (c.tolist() if hasattr(c, "tolist") else c)) for c in r]
                for r in label_masks]
        for n, r in enumerate(rows):
            if not 1 <= len(r) <= MAX_LABEL_MASKS:
                raise ValueError(f"query {n} has {len(r)} label mask clauses: 1 to "
                                 f"{MAX_LABEL_MASKS} are allowed")
            if any(len(c) != 3 for c in r):
                raise ValueError(f"the label masks of query {n} must be (mask, value, any) triples")
            if any(not _INT32_MIN <= v <= _UINT32_MAX for c in r for v in c):
                raise ValueError("label_masks has values outside [-2**31, 2**32)")
        width = max((len(r) for r in rows), default=1)
        label_masks = torch.tensor([r + [r[0]] * (width - len(r)) for r in rows],
                                   dtype=torch.int64).reshape(len(rows), width, 3)
    if label_masks.dim() == 2 and label_masks.shape[1] == 3:
        label_masks = label_masks.reshape(label_masks.shape[0], 1, 3)
    if label_masks.dim() != 3 or label_masks.shape[2] != 3:
        raise TypeError("label_masks must be [Nq, M, 3] or [Nq, 3], or a sequence of per-query "
                        "sequences of (mask, value, any) triples")
    if label_masks.dtype not in (torch.int32, torch.int64):
        raise TypeError("label_masks must be int32 or int64 (values up to 2**32 - 1 wrap)")
    if label_masks.shape[0] != Nq:
        raise ValueError(f"label_masks needs one row per query ({Nq})")
    if not 1 <= label_masks.shape[1] <= MAX_LABEL_MASKS:
        raise ValueError(f"a query has 1 to {MAX_LABEL_MASKS} label mask clauses, not "
                         f"{label_masks.shape[1]}")
    if label_masks.dtype == torch.int64:
        if label_masks.numel() and (int(label_masks.min()) < _INT32_MIN or
                                    int(label_masks.max()) > _UINT32_MAX):
            raise ValueError("label_masks has values outside [-2**31, 2**32)")
        label_masks = torch.where(label_masks > _INT32_MAX, label_masks - 2 ** 32,
                                  label_masks).to(torch.int32)
    return label_masks.contiguous()


def label_mask(all_of=0, none_of=0, any_of=0, field_mask=0, field_value=0):
    """one clause (mask, value, any) for `query_labeled_mask`, from sets of tag bits: the row has
    every bit of `all_of`, no bit of `none_of`, at least one bit of `any_of` (0: no such condition),
    and its bits under `field_mask` equal `field_value` (given at the field's position) --

        (all_of | none_of | field_mask,  all_of | field_value,  any_of)

    wrapped to int32.  The arguments are bit sets in [0, 2**32) (or their int32 form).  ValueError
    where the clause would silently mean something else: `all_of` and `none_of` share a bit,
    `field_value` has a bit outside `field_mask`, or `field_mask` overlaps `all_of | none_of`."""
    bits = []
    for name, v in (("all_of", all_of), ("none_of", none_of), ("any_of", any_of),
                    ("field_mask", field_mask), ("field_value", field_value)):
        v = int(v)
        if not _INT32_MIN <= v <= _UINT32_MAX:
            raise ValueError(f"label_mask: {name} is outside [-2**31, 2**32)")
        bits.append(v & _UINT32_MAX)
    all_of, none_of, any_of, field_mask, field_value = bits
    if all_of & none_of:
        raise ValueError("label_mask: all_of and none_of share a bit: no row could pass")
    if field_value & ~field_mask:
        raise ValueError("label_mask: field_value has a bit outside field_mask")
    if field_mask & (all_of | none_of):
        raise ValueError("label_mask: field_mask overlaps all_of | none_of")
    return (_wrap_int32(all_of | none_of | field_mask), _wrap_int32(all_of | field_value),
            _wrap_int32(any_of))


def ordered_int32(x):
    """float32 values (array, tensor or scalar) as int32 values in the same order, for a float
    attribute -- a price, a float timestamp -- in the int32 label column:

        eng.set_labels(ordered_int32(price))
        eng.query_labeled_range(q, 10, 0.5, label_ranges=[[(ordered_int32(lo), ordered_int32(hi))]])

    a < b iff ordered_int32(a) < ordered_int32(b): the bits b of the float become
    b ^ ((b >> 31) & 0x7fffffff) (arithmetic shift), -0.0 counts as +0.0, -inf / +inf map to the
    outermost values used, and NaN is a ValueError.  An array gives an int32 array, a tensor an int32
    tensor on the same device, a scalar an int."""
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float32:
            raise TypeError("ordered_int32 takes float32 values")
        if bool(torch.isnan(x).any()):
            raise ValueError("ordered_int32: NaN has no place in the order")
        b = (x + 0.0).contiguous().view(torch.int32)  # (-0.0 + 0.0 is +0.0)
        return b ^ ((b >> 31) & 0x7fffffff)
    a = np.asarray(x)
    if a.dtype != np.float32 and a.ndim:
        raise TypeError("ordered_int32 takes float32 values")
    a = a.astype(np.float32)
    if np.isnan(a).any():
        raise ValueError("ordered_int32: NaN has no place in the order")
    b = np.ascontiguousarray(np.atleast_1d(a) + np.float32(0.0)).view(np.int32)
    out = b ^ ((b >> 31) & np.int32(0x7fffffff))
    return out.reshape(a.shape) if a.ndim else int(out[0])


def _filter_words(filter, N):
    """the `filter` argument of query_filtered / bf_query_filtered as a contiguous int32 tensor of
    ceil(N / 32) words (CPU or CUDA): a boolean mask of length N is packed on the host, an
    int32 / uint32 array is taken as already packed"""
    if isinstance(filter, np.ndarray) and filter.dtype == np.uint32:
        filter = filter.view(np.int32)
    if isinstance(filter, np.ndarray):
        filter = torch.from_numpy(np.ascontiguousarray(filter))
    if not isinstance(filter, torch.Tensor) or filter.dim() != 1:
        raise TypeError("filter must be a 1-dimensional numpy array or torch tensor")
    if filter.dtype == torch.bool:
        if filter.numel() != N:
            raise ValueError(f"a boolean filter needs one entry per base vector ({N})")
        return pack_filter(filter)
    if hasattr(torch, "uint32") and filter.dtype == torch.uint32:
        filter = filter.view(torch.int32)
    if filter.dtype != torch.int32:
        raise TypeError("filter must be boolean, or int32 / uint32 words of a packed bitset")
    if filter.numel() != (N + 31) // 32:
        raise ValueError(f"a packed filter needs ceil(N / 32) = {(N + 31) // 32} words")
    return filter.contiguous()


# ---------------------------------------------------------------------------------------------
# Datasets (nanobind.cu:153-181; Dataset<T>::load/store, src/ggnn/base/dataset.cu:118-233)
# ---------------------------------------------------------------------------------------------
class _Dataset:
    _torch_dtype = None
    _suffix = None

    def __init__(self, data):
        self._t = _as_tensor(data, self._torch_dtype).clone()

    @classmethod
    def _wrap(cls, t):
        obj = cls.__new__(cls)
        obj._t = t
        return obj

    @classmethod
    def load(cls, file, from_=0, num=2 ** 32 - 1, pin_memory=False, **kw):
        """XVECS files: per vector a uint32 dimension followed by D values."""
        from_ = kw.get("from", from_)
        npdt = np.dtype(_NP_OF[cls._torch_dtype])
        with open(file, "rb") as f:
            head = np.fromfile(f, dtype=np.uint32, count=1)
            if head.size != 1:
                raise RuntimeError(f"cannot read {file}")
            D = int(head[0])
            rec = 4 + D * npdt.itemsize
            total = os.path.getsize(file) // rec
            n = max(0, min(int(num), total - int(from_)))
            f.seek(int(from_) * rec)
            raw = np.fromfile(f, dtype=np.uint8, count=n * rec).reshape(n, rec)
        data = np.ascontiguousarray(raw[:, 4:]).view(npdt).reshape(n, D)
        t = torch.from_numpy(data.copy())
        if pin_memory and torch.cuda.is_available():
            t = t.pin_memory()
        return cls._wrap(t)

    def store(self, file):
        a = self._t.cpu().numpy()
        n, D = a.shape
        rec = np.empty((n, 4 + D * a.dtype.itemsize), np.uint8)
        rec[:, :4] = np.frombuffer(np.uint32(D).tobytes(), np.uint8)
        rec[:, 4:] = a.view(np.uint8).reshape(n, -1)
        rec.tofile(file)

    @property
    def N(self):
        return int(self._t.shape[0])

    @property
    def D(self):
        return int(self._t.shape[1])

    def numel(self):
        return int(self._t.numel())

    def clone(self):
        return self._t.clone()

    @property
    def view(self):
        return self._t

    @property
    def device(self):
        return f"cuda:{self._t.device.index}" if self._t.is_cuda else "cpu"


class FloatDataset(_Dataset):
    _torch_dtype = torch.float32


class UCharDataset(_Dataset):
    _torch_dtype = torch.uint8


class CharDataset(_Dataset):
    """Signed 8-bit rows (torch.int8).  This project's extension: the reference has no such
    dataset.  `store` / `load` use the bvecs record layout of `UCharDataset` (per vector a uint32
    dimension, then D bytes) with the bytes read as signed."""
    _torch_dtype = torch.int8


class IntDataset(_Dataset):
    _torch_dtype = torch.int32


class Graph:
    """Graph views (include/ggnn/base/graph.h:38-71, nanobind.cu:295-300); copies on the host."""

    def __init__(self, graph, selection, translation, nn1_stats, config):
        self.graph = graph
        self.selection = selection
        self.translation = translation
        self.nn1_stats = nn1_stats
        self.config = config


# ---------------------------------------------------------------------------------------------
# GGNN (nanobind.cu:184-268 over ggnn.cuh:42-182)
# ---------------------------------------------------------------------------------------------
_ASYNC_SLOTS = 4   # DeviceCtx::kShardStreams: slots that map to the same engine stream
_MAX_TICKETS_PER_SLOT = 64   # query_async batches whose tensors are held per slot before it is drained


class QueryTicket:
    """Result of `GGNN.query_async`: `ids, dists = ticket` works as before; `query` keeps the
    input alive (and `filter_ids` the filter ids, or the query labels, of a batch that has some);
    `done` is set by `synchronize()`."""
    __slots__ = ("query", "ids", "dists", "slot", "done", "filter_ids", "label_sets",
                 "label_ranges", "label_masks")

    def __init__(self, query, ids, dists, slot, filter_ids=None, label_sets=None,
                 label_ranges=None, label_masks=None):
        self.query, self.ids, self.dists, self.slot, self.done = query, ids, dists, slot, False
        self.filter_ids = filter_ids
        self.label_sets = label_sets
        self.label_ranges = label_ranges
        self.label_masks = label_masks

    def __iter__(self):
        return iter((self.ids, self.dists))

    def __getitem__(self, i):
        return (self.ids, self.dists)[i]

    def __len__(self):
        return 2


class GGNN:
    """GGNN main class. Provides functionality for building, loading, storing, and querying
    nearest neighbor graphs on the GPU."""

    def __init__(self):
        h = C.c_void_p()
        check(lib().ggnn_create(C.byref(h)))
        self._h = h
        self._destroy = lib().ggnn_destroy
        self._keepalive = None
        self._return_results_on_gpu = False
        self._shards = 1
        self._inflight = {}   # slot -> QueryTickets whose kernels may still be running
        self._num_gpus = 1
        self._collect_counters = False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._destroy(h)

    def _check(self, status):
        check(status, self._h)

    def set_base(self, base):
        t = _as_tensor(base, what="base")
        loc, dev = _loc(t)
        # the binding clones its argument (nanobind.cu:102-110): the engine takes a copy
        self._check(lib().ggnn_set_base(self._h, t.data_ptr(), t.shape[0], t.shape[1],
                                        _dtype_code(t), loc, dev, 1))
        self._base_shape = tuple(t.shape)

    def set_base_reference(self, base):
        """GGNN::setBaseReference (ggnn.cuh:116-123): borrow; the tensor is kept alive here."""
        t = _as_tensor(base, what="base")
        loc, dev = _loc(t)
        self._check(lib().ggnn_set_base(self._h, t.data_ptr(), t.shape[0], t.shape[1],
                                        _dtype_code(t), loc, dev, 0))
        self._keepalive = t
        self._base_shape = tuple(t.shape)

    def set_working_directory(self, dir):
        self._check(lib().ggnn_set_working_directory(self._h, os.fspath(dir).encode()))

    def set_cpu_memory_limit(self, memory_limit):
        self._check(lib().ggnn_set_cpu_memory_limit(self._h, int(memory_limit)))

    def set_reserved_gpu_memory(self, reserved_memory):
        self._check(lib().ggnn_set_reserved_gpu_memory(self._h, int(reserved_memory)))

    def set_gpus(self, gpu_ids):
        ids = [int(g) for g in gpu_ids]
        arr = (C.c_int * len(ids))(*ids)
        self._check(lib().ggnn_set_gpus(self._h, arr, len(ids)))
        self._num_gpus = max(1, len(ids))

    def set_shard_size(self, n_shard):
        self._check(lib().ggnn_set_shard_size(self._h, int(n_shard)))
        self._n_shard = int(n_shard)

    def set_return_results_on_gpu(self, return_results_on_gpu=True):
        self._check(lib().ggnn_set_return_results_on_gpu(self._h, int(bool(return_results_on_gpu))))
        self._return_results_on_gpu = bool(return_results_on_gpu)

    def build(self, k_build, tau_build, refinement_iterations=2,
              measure=DistanceMeasure.Euclidean):
        """Build a GGNN graph."""
        self._check(lib().ggnn_build(self._h, int(k_build), float(tau_build),
                                     int(refinement_iterations), int(measure)))
        self._update_shards()

    def load(self, k_build):
        """Load a GGNN graph."""
        self._check(lib().ggnn_load(self._h, int(k_build)))
        self._update_shards()

    def store(self):
        """Store a GGNN graph."""
        self._check(lib().ggnn_store(self._h))

    def _update_shards(self):
        # shards per GPU as laid out by the engine: width factor of results kept on the GPU
        per_gpu = C.c_uint32(1)
        self._check(lib().ggnn_get_shard_layout(self._h, None, C.byref(per_gpu), None))
        self._shards = int(per_gpu.value)

    def _out(self, Nq, width, on_gpu, device):
        dev = device if on_gpu else "cpu"
        ids = torch.empty((Nq, width), dtype=torch.int32, device=dev)
        dists = torch.empty((Nq, width), dtype=torch.float32, device=dev)
        if on_gpu:
            # the blocks come from torch's caching allocator, which orders their reuse on torch's
            # stream; the engine writes them on its own stream, so work torch has queued on a
            # recycled block must have finished before the engine touches it
            torch.cuda.current_stream(device).synchronize()
        return ids, dists

    def _result_device(self, t):
        if t.is_cuda:
            return t.device
        view = _lib.GraphView()
        if lib().ggnn_get_graph(self._h, 0, C.byref(view)) == _lib.OK:
            return torch.device("cuda", view.gpu_id)
        return torch.device("cuda", torch.cuda.current_device())

    def _blocking(self, call, t, params, tail=(), shards=1):
        """one blocking call of the C-ABI: query tensor `t`, its location, the result tensors, then
        `call` with the search parameters `params` (k first) and the filter arguments `tail`.
        `shards`: rows per query that results kept on the GPU have (a graph search: one per shard)"""
        loc, dev = _loc(t)
        on_gpu = self._return_results_on_gpu
        width = params[0] * (shards if on_gpu else 1)
        ids, dists = self._out(t.shape[0], width, on_gpu, self._result_device(t) if on_gpu else None)
        self._check(call(self._h, t.data_ptr(), t.shape[0], t.shape[1], _dtype_code(t), loc, dev,
                         *params, ids.data_ptr(), dists.data_ptr(),
                         _lib.GPU if on_gpu else _lib.CPU, *tail))
        return ids, dists

    @staticmethod
    def _search(k_query, tau_query, max_iterations, measure):
        return int(k_query), float(tau_query), int(max_iterations), int(measure)

    @staticmethod
    def _where(x):
        """a filter tensor as the C-ABI takes it: pointer, location, GPU"""
        return (x.data_ptr(), *_loc(x))

    def query(self, query, k_query, tau_query, max_iterations=400,
              measure=DistanceMeasure.Euclidean):
        """Run a query and return indices and distances."""
        return self._blocking(lib().ggnn_query, _as_tensor(query, what="query"),
                              self._search(k_query, tau_query, max_iterations, measure),
                              shards=self._shards)

    @property
    def _N(self):
        return self._base_shape[0] if hasattr(self, "_base_shape") else 0

    def set_filters(self, filters):
        """Extension: make `filters` the resident filter table of this engine -- boolean masks
        [F, N] (packed where they live) or packed bitsets [F, ceil(N / 32)] int32 / uint32
        (`pack_filters`), CPU or GPU.  The engine copies the table and keeps it on every GPU it
        drives, also across `build` / `load`; queries then name a row per query (`filter_ids=` of
        `query_filtered_by`, `bf_query_filtered_by` and `query_async`).
        `None` drops the table.  Waits for batches in flight."""
        if filters is None:
            self._check(lib().ggnn_set_filters(self._h, None, 0, 0, _lib.CPU, 0))
            return
        N = self._N
        f = _filter_table(filters, N)
        if f.shape[0] == 0:
            raise ValueError("the filter table is empty (set_filters(None) drops it)")
        floc, fdev = _loc(f)
        self._check(lib().ggnn_set_filters(self._h, f.data_ptr(), f.shape[0], N, floc, fdev))

    def update_filter(self, i, filter):
        """Extension: replace row `i` of the filter table (`filter` as in `query_filtered`) on
        every GPU.  Waits for batches in flight."""
        N = self._N
        f = _filter_words(filter, N)
        floc, fdev = _loc(f)
        self._check(lib().ggnn_update_filter(self._h, int(i), f.data_ptr(), N, floc, fdev))

    @property
    def num_filters(self):
        """rows of the resident filter table (0: none)"""
        n = C.c_uint32(0)
        self._check(lib().ggnn_get_num_filters(self._h, C.byref(n)))
        return int(n.value)

    def set_labels(self, labels):
        """Extension: label filters.  `labels` is one int32 label per base vector -- 1-D int32 or
        int64 (values must fit int32) of length N, numpy / torch, CPU or GPU.  The engine copies the
        column and keeps it on every GPU it drives (4 * N bytes, whatever the number of distinct
        labels), also across `build` / `load`; queries then carry one label each (`labels=` of
        `query_labeled`, `bf_query_labeled` and `query_async_labeled`) and are given base vectors of that
        label only.  `None` drops the labels.  Waits for batches in flight."""
        if labels is None:
            self._check(lib().ggnn_set_labels(self._h, None, 0, _lib.CPU, 0))
            return
        N = self._N
        lab = _labels(labels, N)
        lloc, ldev = _loc(lab)
        self._check(lib().ggnn_set_labels(self._h, lab.data_ptr(), N, lloc, ldev))

    def update_labels(self, ids, labels):
        """Extension: relabel some rows, `labels[ids[i]] = labels_new[i]` in order (the last pair
        of a repeated id wins), on every GPU.  `ids`: 1-D int32 / int64 base ids, `labels`: as many
        int32 / int64 labels.  Waits for batches in flight."""
        if isinstance(ids, np.ndarray):
            ids = torch.from_numpy(np.ascontiguousarray(ids))
        if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or \
                ids.dtype not in (torch.int32, torch.int64):
            raise TypeError("ids must be a 1-dimensional int32 / int64 numpy array or torch tensor")
        lab = _labels(labels, ids.numel(), per="id")
        ids = ids.to(device=lab.device, dtype=torch.int64).contiguous()
        lloc, ldev = _loc(lab)
        self._check(lib().ggnn_update_labels(self._h, ids.data_ptr(), lab.data_ptr(), ids.numel(),
                                             lloc, ldev))

    @property
    def num_labels(self):
        """length of the resident label column (N), 0 without labels"""
        n = C.c_uint64(0)
        self._check(lib().ggnn_get_num_labels(self._h, C.byref(n)))
        return int(n.value)

    def query_labeled(self, query, k_query, tau_query, max_iterations=400,
                      measure=DistanceMeasure.Euclidean, labels=None):
        """Extension: `query` under label filters (`set_labels`).  `labels`: one label per query,
        1-D int32 / int64 of length Nq, CPU or GPU; query n is given base vectors whose label
        equals labels[n] -- bit for bit `query_filtered` with the mask `base_labels == labels[n]`
        -- and label -1 searches unfiltered.  A label no base vector carries gives an empty
        result (ids -1, distances +inf).  `labels=None` is `query`."""
        if labels is None:
            return self.query(query, k_query, tau_query, max_iterations, measure)
        t = _as_tensor(query, what="query")
        ql = _labels(labels, t.shape[0], per="query")
        return self._blocking(lib().ggnn_query_labeled, t,
                              self._search(k_query, tau_query, max_iterations, measure),
                              self._where(ql), self._shards)

    def bf_query_labeled(self, query, k_gt=100, measure=DistanceMeasure.Euclidean, labels=None):
        """Extension: the exact `k_gt` nearest among the base vectors that carry the query's label
        (`labels`: see `query_labeled`); slots beyond their number are (-1, +inf).  `labels=None`
        is `bf_query`."""
        if labels is None:
            return self.bf_query(query, k_gt, measure)
        t = _as_tensor(query, what="query")
        ql = _labels(labels, t.shape[0], per="query")
        return self._blocking(lib().ggnn_bf_query_labeled, t, (int(k_gt), int(measure)),
                              self._where(ql))

    def _labeled_in_tail(self, ls, fi):
        """the filter arguments of the *_labeled_in / *_labeled_range / *_labeled_mask calls: the
        sets (or ranges, or clauses: shape[1] is their number either way), then the ids (or null)"""
        ids = self._where(fi) if fi is not None else (None, _lib.CPU, 0)
        return (ls.data_ptr(), ls.shape[1], *_loc(ls), *ids)

    def query_labeled_in(self, query, k_query, tau_query, max_iterations=400,
                         measure=DistanceMeasure.Euclidean, label_sets=None, filter_ids=None):
        """Extension: `query` under label SETS (`set_labels`), combined with a filter id per query
        (`set_filters`).  `label_sets`: for every query the labels it accepts -- a 2-D int32 / int64
        array or tensor [Nq, 1..8], CPU or GPU, or a sequence of per-query sequences of 1 to 8
        labels (padded by repeating a row's first entry; an empty or longer row is a ValueError).
        Query n is given base vectors whose label equals one of its entries (an entry -1 accepts
        every label) AND that row `filter_ids[n]` of the filter table allows (`filter_ids` as in
        `query_filtered_by`; `None`: no bitset) -- bit for bit `query_filtered` with the mask
        `isin(base_labels, label_sets[n]) & table[filter_ids[n]]`.  `label_sets=None` is no label
        restriction (`query_filtered_by`); both `None` is `query`."""
        if label_sets is None:
            return self.query_filtered_by(query, k_query, tau_query, max_iterations, measure,
                                          filter_ids=filter_ids)
        t = _as_tensor(query, what="query")
        ls = _label_sets(label_sets, t.shape[0])
        fi = None if filter_ids is None else _filter_ids(filter_ids, t.shape[0])
        return self._blocking(lib().ggnn_query_labeled_in, t,
                              self._search(k_query, tau_query, max_iterations, measure),
                              self._labeled_in_tail(ls, fi), self._shards)

    def bf_query_labeled_in(self, query, k_gt=100, measure=DistanceMeasure.Euclidean,
                            label_sets=None, filter_ids=None):
        """Extension: the exact `k_gt` nearest among the base vectors `label_sets` and `filter_ids`
        admit (see `query_labeled_in`); slots beyond their number are (-1, +inf).  Always the scan
        kernels.  `label_sets=None` is `bf_query_filtered_by`; both `None` is `bf_query`."""
        if label_sets is None:
            return self.bf_query_filtered_by(query, k_gt, measure, filter_ids=filter_ids)
        t = _as_tensor(query, what="query")
        ls = _label_sets(label_sets, t.shape[0])
        fi = None if filter_ids is None else _filter_ids(filter_ids, t.shape[0])
        return self._blocking(lib().ggnn_bf_query_labeled_in, t, (int(k_gt), int(measure)),
                              self._labeled_in_tail(ls, fi))

    def query_labeled_range(self, query, k_query, tau_query, max_iterations=400,
                            measure=DistanceMeasure.Euclidean, label_ranges=None, filter_ids=None):
        """Extension: `query` under label RANGES (`set_labels`), combined with a filter id per
        query (`set_filters`).  `label_ranges`: for every query up to 4 closed intervals (lo, hi) of
        int32 labels -- a 3-D int32 / int64 array or tensor [Nq, 1..4, 2], CPU or GPU, or a sequence
        of per-query sequences of 1 to 4 pairs (padded with an empty interval; an empty or longer
        row is a ValueError).  Query n is given base vectors whose label lies in one of its
        intervals, compared as signed int32 -- lo > hi is an empty interval, and there is no
        wildcard: -1 is an ordinary label, (-2**31, 2**31 - 1) admits every label -- AND that row
        `filter_ids[n]` of the filter table allows (`filter_ids` as in `query_filtered_by`; `None`:
        no bitset) -- bit for bit `query_filtered` with the mask
        `any_j(lo_j <= base_labels <= hi_j) & table[filter_ids[n]]`.  `label_ranges=None` is no
        label restriction (`query_filtered_by`); both `None` is `query`.  Float attributes:
        `ordered_int32`."""
        if label_ranges is None:
            return self.query_filtered_by(query, k_query, tau_query, max_iterations, measure,
                                          filter_ids=filter_ids)
        t = _as_tensor(query, what="query")
        lr = _label_ranges(label_ranges, t.shape[0])
        fi = None if filter_ids is None else _filter_ids(filter_ids, t.shape[0])
        return self._blocking(lib().ggnn_query_labeled_range, t,
                              self._search(k_query, tau_query, max_iterations, measure),
                              self._labeled_in_tail(lr, fi), self._shards)

    def bf_query_labeled_range(self, query, k_gt=100, measure=DistanceMeasure.Euclidean,
                               label_ranges=None, filter_ids=None):
        """Extension: the exact `k_gt` nearest among the base vectors `label_ranges` and
        `filter_ids` admit (see `query_labeled_range`); slots beyond their number are (-1, +inf).
        Always the scan kernels.  `label_ranges=None` is `bf_query_filtered_by`; both `None` is
        `bf_query`."""
        if label_ranges is None:
            return self.bf_query_filtered_by(query, k_gt, measure, filter_ids=filter_ids)
        t = _as_tensor(query, what="query")
        lr = _label_ranges(label_ranges, t.shape[0])
        fi = None if filter_ids is None else _filter_ids(filter_ids, t.shape[0])
        return self._blocking(lib().ggnn_bf_query_labeled_range, t, (int(k_gt), int(measure)),
                              self._labeled_in_tail(lr, fi))

    def query_labeled_mask(self, query, k_query, tau_query, max_iterations=400,
                           measure=DistanceMeasure.Euclidean, label_masks=None, filter_ids=None):
        """Extension: `query` under label MASKS -- the int32 label of `set_labels` read as 32 tag
        bits -- combined with a filter id per query (`set_filters`).  `label_masks`: for every query
        1 or 2 clauses (mask, value, any) -- a [Nq, 1..2, 3] or [Nq, 3] int32 / int64 array or
        tensor, CPU or GPU, or a sequence of per-query sequences of 1 or 2 triples (a shorter row is
        padded by repeating its first triple; an empty or longer row is a ValueError); values in
        [-2**31, 2**32) wrap to int32; `label_mask` builds a triple.  A base vector with label L
        passes a clause iff (L & mask) == value and (any == 0 or (L & any) != 0); query n is given
        the vectors that pass one of its clauses AND that row `filter_ids[n]` of the filter table
        allows (`filter_ids` as in `query_filtered_by`; `None`: no bitset) -- bit for bit
        `query_filtered` with that mask.  (0, 0, 0) admits every vector, a value with a bit outside
        its mask none (value is never pre-masked), there is no wildcard value and bit 31 is a bit
        like any other.  `label_masks=None` is no label restriction (`query_filtered_by`); both
        `None` is `query`."""
        if label_masks is None:
            return self.query_filtered_by(query, k_query, tau_query, max_iterations, measure,
                                          filter_ids=filter_ids)
        t = _as_tensor(query, what="query")
        lm = _label_masks(label_masks, t.shape[0])
        fi = None if filter_ids is None else _filter_ids(filter_ids, t.shape[0])
        return self._blocking(lib().ggnn_query_labeled_mask, t,
                              self._search(k_query, tau_query, max_iterations, measure),
                              self._labeled_in_tail(lm, fi), self._shards)

    def bf_query_labeled_mask(self, query, k_gt=100, measure=DistanceMeasure.Euclidean,
                              label_masks=None, filter_ids=None):
        """Extension: the exact `k_gt` nearest among the base vectors `label_masks` and `filter_ids`
        admit (see `query_labeled_mask`); slots beyond their number are (-1, +inf).  Always the scan
        kernels.  `label_masks=None` is `bf_query_filtered_by`; both `None` is `bf_query`."""
        if label_masks is None:
            return self.bf_query_filtered_by(query, k_gt, measure, filter_ids=filter_ids)
        t = _as_tensor(query, what="query")
        lm = _label_masks(label_masks, t.shape[0])
        fi = None if filter_ids is None else _filter_ids(filter_ids, t.shape[0])
        return self._blocking(lib().ggnn_bf_query_labeled_mask, t, (int(k_gt), int(measure)),
                              self._labeled_in_tail(lm, fi))

    def query_filtered(self, query, k_query, tau_query, max_iterations=400,
                       measure=DistanceMeasure.Euclidean, filter=None):
        """Extension: `query` among the base vectors `filter` allows -- a boolean mask of length N
        (numpy / torch) or an already packed bitset (`pack_filter`: int32 / uint32, ceil(N / 32)
        words, CPU or GPU), shared by all queries of the batch.  Denied vectors still route the
        search but are never reported; slots that could not be filled hold id -1 and distance
        +inf.  `filter=None` is `query`.  A filter per query: `query_filtered_by`."""
        return self.query_filtered_by(query, k_query, tau_query, max_iterations, measure,
                                      filter=filter)

    def query_filtered_by(self, query, k_query, tau_query, max_iterations=400,
                          measure=DistanceMeasure.Euclidean, filter_ids=None, filter=None):
        """Extension: `query_filtered` with a filter per query.  `filter_ids`: one row of the
        filter table (`set_filters`) per query -- 1-D int32 / int64 of length Nq, CPU or GPU; -1
        searches unfiltered, and an id in device memory that names no row gives an empty result
        (on the host it is an error).  `filter` (instead of `filter_ids`) is the one bitset of
        `query_filtered`; giving both is a ValueError, giving neither is `query`."""
        if filter is not None and filter_ids is not None:
            raise ValueError("give either filter or filter_ids, not both")
        if filter is None and filter_ids is None:
            return self.query(query, k_query, tau_query, max_iterations, measure)
        t = _as_tensor(query, what="query")
        params = self._search(k_query, tau_query, max_iterations, measure)
        if filter_ids is not None:
            fi = _filter_ids(filter_ids, t.shape[0])
            return self._blocking(lib().ggnn_query_filtered_by, t, params, self._where(fi),
                                  self._shards)
        f = _filter_words(filter, self._N)
        ptr, floc, fdev = self._where(f)
        return self._blocking(lib().ggnn_query_filtered, t, params, (ptr, self._N, floc, fdev),
                              self._shards)

    def bf_query_filtered(self, query, k_gt=100, measure=DistanceMeasure.Euclidean, filter=None):
        """Extension: the exact `k_gt` nearest among the base vectors `filter` allows (see
        `query_filtered`); slots beyond the number of allowed vectors are (-1, +inf)."""
        return self.bf_query_filtered_by(query, k_gt, measure, filter=filter)

    def bf_query_filtered_by(self, query, k_gt=100, measure=DistanceMeasure.Euclidean,
                             filter_ids=None, filter=None):
        """Extension: `bf_query_filtered` with a filter per query (`filter_ids`, `filter`: see
        `query_filtered_by`)."""
        if filter is not None and filter_ids is not None:
            raise ValueError("give either filter or filter_ids, not both")
        if filter is None and filter_ids is None:
            return self.bf_query(query, k_gt, measure)
        t = _as_tensor(query, what="query")
        params = (int(k_gt), int(measure))
        if filter_ids is not None:
            fi = _filter_ids(filter_ids, t.shape[0])
            return self._blocking(lib().ggnn_bf_query_filtered_by, t, params, self._where(fi))
        f = _filter_words(filter, self._N)
        ptr, floc, fdev = self._where(f)
        return self._blocking(lib().ggnn_bf_query_filtered, t, params, (ptr, self._N, floc, fdev))

    def query_async(self, query, k_query, tau_query, max_iterations=400,
                    measure=DistanceMeasure.Euclidean, slot=0, filter_ids=None):
        """Extension for serving: enqueue a batch and return a `QueryTicket` (unpacks like the
        `(ids, dists)` pair) whose GPU tensors are valid after `synchronize()`.  Batches with
        different `slot`s overlap on the device (one GPU, query on that GPU); the result has the
        results-on-GPU shape [Nq, k_query * shards].

        Lifetime: the kernels run on the engine's own streams, which torch's caching allocator
        knows nothing about.  The engine object therefore keeps the query tensor and both
        result tensors referenced until `synchronize()` (of that slot) has returned, whatever
        the caller does with its own references -- a temporary passed as `query`, or a
        rebound loop variable, cannot be recycled under a running kernel.  At most
        `_MAX_TICKETS_PER_SLOT` batches are held per slot: enqueueing one more first synchronises
        that slot and releases them.

        `filter_ids`: one row of the filter table (`set_filters`) per query, as in
        `query_filtered_by`; the ids live where the query lives (they are moved there otherwise) and
        are kept alive with it.  A label per query: `query_async_labeled`."""
        return self._query_async(query, k_query, tau_query, max_iterations, measure, slot,
                                 filter_ids, None)

    def query_async_labeled(self, query, k_query, tau_query, max_iterations=400,
                            measure=DistanceMeasure.Euclidean, slot=0, labels=None):
        """Extension: `query_async` under label filters (`set_labels`).  `labels`: one label per
        query, as in `query_labeled`, with the memory and lifetime rules of the `filter_ids` of
        `query_async` (kept alive on the ticket, `ticket.filter_ids`).  A method of its own, like
        `query_labeled`: `query_async` keeps its signature.  `labels=None` is `query_async`."""
        return self._query_async(query, k_query, tau_query, max_iterations, measure, slot, None,
                                 labels)

    def query_async_labeled_in(self, query, k_query, tau_query, max_iterations=400,
                               measure=DistanceMeasure.Euclidean, slot=0, label_sets=None,
                               filter_ids=None):
        """Extension: `query_async` under label sets and filter ids (`query_labeled_in`), both with
        the memory and lifetime rules of the `filter_ids` of `query_async` (kept alive on the
        ticket: `ticket.filter_ids`, `ticket.label_sets`).  `label_sets=None` is `query_async`."""
        return self._query_async(query, k_query, tau_query, max_iterations, measure, slot,
                                 filter_ids, None, label_sets)

    def query_async_labeled_range(self, query, k_query, tau_query, max_iterations=400,
                                  measure=DistanceMeasure.Euclidean, slot=0, label_ranges=None,
                                  filter_ids=None):
        """Extension: `query_async` under label ranges and filter ids (`query_labeled_range`), both
        with the memory and lifetime rules of the `filter_ids` of `query_async` (kept alive on the
        ticket: `ticket.filter_ids`, `ticket.label_ranges`).  `label_ranges=None` is
        `query_async`."""
        return self._query_async(query, k_query, tau_query, max_iterations, measure, slot,
                                 filter_ids, None, None, label_ranges)

    def query_async_labeled_mask(self, query, k_query, tau_query, max_iterations=400,
                                 measure=DistanceMeasure.Euclidean, slot=0, label_masks=None,
                                 filter_ids=None):
        """Extension: `query_async` under label masks and filter ids (`query_labeled_mask`), both
        with the memory and lifetime rules of the `filter_ids` of `query_async` (kept alive on the
        ticket: `ticket.filter_ids`, `ticket.label_masks`).  `label_masks=None` is `query_async`."""
        return self._query_async(query, k_query, tau_query, max_iterations, measure, slot,
                                 filter_ids, None, None, None, label_masks)

    def _query_async(self, query, k_query, tau_query, max_iterations, measure, slot, filter_ids,
                     labels, label_sets=None, label_ranges=None, label_masks=None):
        t = _as_tensor(query, what="query")
        fi = None if filter_ids is None else _filter_ids(filter_ids, t.shape[0])
        if labels is not None:
            fi = _labels(labels, t.shape[0], per="query")
        ls = None if label_sets is None else _label_sets(label_sets, t.shape[0])
        lr = None if label_ranges is None else _label_ranges(label_ranges, t.shape[0])
        lm = None if label_masks is None else _label_masks(label_masks, t.shape[0])

        def follow(x, pinned):
            # sets and ids follow the query's memory rule: its GPU, or page-locked host memory
            if x is None:
                return None
            x = x.to(t.device) if t.is_cuda else (x.cpu() if x.is_cuda else x)
            if pinned and not x.is_cuda and not x.is_pinned():
                x = x.pin_memory()
            return x
        if self._num_gpus > 1 or _lib.get_hook("EXCHANGE") == 1:
            # several GPUs (or the forced RCCL path of the tests): merged [Nq, k] results; host-side tensors are page-locked so that the
            # engine's copies stay asynchronous
            if not t.is_cuda and not t.is_pinned():
                t = t.pin_memory()
            fi, ls, lr = follow(fi, True), follow(ls, True), follow(lr, True)
            lm = follow(lm, True)
            dev = t.device.index if t.is_cuda else -1
            if t.is_cuda:
                ids, dists = self._out(t.shape[0], int(k_query), True, t.device)
            else:
                ids = torch.empty((t.shape[0], int(k_query)), dtype=torch.int32, pin_memory=True)
                dists = torch.empty((t.shape[0], int(k_query)), dtype=torch.float32,
                                    pin_memory=True)
        else:
            if not t.is_cuda:
                raise RuntimeError("query_async needs the query on the GPU")
            loc, dev = _loc(t)
            fi, ls, lr = follow(fi, False), follow(ls, False), follow(lr, False)
            lm = follow(lm, False)
            ids, dists = self._out(t.shape[0], int(k_query) * self._shards, True, t.device)
        if ls is not None or lr is not None or lm is not None:
            # (sets, ranges or clauses: [Nq, width] / [Nq, n_ranges, 2] / [Nq, n_masks, 3], the same
            # argument list)
            if lm is not None:
                rows, call = lm, lib().ggnn_query_async_labeled_mask
            elif lr is not None:
                rows, call = lr, lib().ggnn_query_async_labeled_range
            else:
                rows, call = ls, lib().ggnn_query_async_labeled_in
            for x in (rows, fi):
                if x is not None and x.is_cuda:
                    torch.cuda.current_stream(x.device).synchronize()
            self._check(call(
                self._h, t.data_ptr(), t.shape[0], t.shape[1], _dtype_code(t), dev, int(k_query),
                float(tau_query), int(max_iterations), int(measure), ids.data_ptr(),
                dists.data_ptr(), int(slot), rows.data_ptr(), rows.shape[1],
                None if fi is None else fi.data_ptr()))
        elif fi is not None:
            if fi.is_cuda:
                torch.cuda.current_stream(fi.device).synchronize()
            call = (lib().ggnn_query_async_labeled if labels is not None
                    else lib().ggnn_query_async_filtered_by)
            self._check(call(
                self._h, t.data_ptr(), t.shape[0], t.shape[1], _dtype_code(t), dev, int(k_query),
                float(tau_query), int(max_iterations), int(measure), ids.data_ptr(),
                dists.data_ptr(), int(slot), fi.data_ptr()))
        else:
            self._check(lib().ggnn_query_async(self._h, t.data_ptr(), t.shape[0], t.shape[1],
                                               _dtype_code(t), dev, int(k_query), float(tau_query),
                                               int(max_iterations), int(measure), ids.data_ptr(),
                                               dists.data_ptr(), int(slot)))
        ticket = QueryTicket(t, ids, dists, int(slot), fi, ls, lr, lm)
        held = self._inflight.setdefault(int(slot) % _ASYNC_SLOTS, [])
        if len(held) >= _MAX_TICKETS_PER_SLOT:
            # a serving loop that waits some other way (its own events, torch.cuda.synchronize)
            # never calls synchronize(): the references held for the kernels' sake must not grow
            # without bound -- the slot is drained (its batches ran long ago) and released
            self.synchronize(slot)
            held = self._inflight.setdefault(int(slot) % _ASYNC_SLOTS, [])
        held.append(ticket)
        return ticket

    def synchronize(self, slot=None):
        """wait for every batch enqueued with query_async (or only for those of one slot); the
        tensors of the finished batches are released to their owners"""
        if slot is None:
            self._check(lib().ggnn_synchronize(self._h))
            done = [t for ts in self._inflight.values() for t in ts]
            self._inflight.clear()
        else:
            self._check(lib().ggnn_synchronize_slot(self._h, int(slot)))
            done = self._inflight.pop(int(slot) % _ASYNC_SLOTS, [])
        for t in done:
            t.done = True

    def bf_query(self, query, k_gt=100, measure=DistanceMeasure.Euclidean):
        """Run a brute-force query and indices and distances."""
        return self._blocking(lib().ggnn_bf_query, _as_tensor(query, what="query"),
                              (int(k_gt), int(measure)))

    def _range(self, call, query, radius, measure, max_results, sort, tail=()):
        """one exact range search through the C-ABI: (lims int64 [Nq + 1], ids int32, dists float32)"""
        from .ops import range_radii, sort_segments
        t = _as_tensor(query, what="query")
        Nq = t.shape[0]
        radii = range_radii(radius, Nq, "cpu")
        loc, dev = _loc(t)
        on_gpu = self._return_results_on_gpu
        out_dev = self._result_device(t) if on_gpu else "cpu"
        lims = torch.zeros(Nq + 1, dtype=torch.int64)

        def run(capacity, ids, dists):
            self._check(call(self._h, t.data_ptr(), Nq, t.shape[1], _dtype_code(t), loc, dev,
                             radii.data_ptr(), int(measure), capacity, lims.data_ptr(),
                             ids.data_ptr() if capacity else None,
                             dists.data_ptr() if capacity else None,
                             _lib.GPU if on_gpu else _lib.CPU, *tail))
            return int(lims[-1])

        def buffers(capacity):
            ids = torch.empty(capacity, dtype=torch.int32, device=out_dev)
            dists = torch.empty(capacity, dtype=torch.float32, device=out_dev)
            if on_gpu:
                torch.cuda.current_stream(out_dev).synchronize()  # (see _out)
            return ids, dists

        if max_results is None:
            total = run(0, None, None)
            ids, dists = buffers(total)
            if total:
                run(total, ids, dists)
        else:
            max_results = int(max_results)
            ids, dists = buffers(max_results)
            total = run(max_results, ids, dists)
            if total > max_results:
                raise RuntimeError(f"range query: {total} results do not fit max_results="
                                   f"{max_results}; call again with max_results >= {total}")
            ids, dists = ids[:total], dists[:total]
        if sort:
            ids, dists = sort_segments(lims, ids, dists)
        return lims, ids, dists

    def bf_range_query(self, query, radius, measure=DistanceMeasure.Euclidean, max_results=None,
                       sort=True):
        """Extension: exact range search -- EVERY base vector within `radius` of each query, where
        `bf_query` returns the k best.  Returns (lims, ids, dists): lims is int64 [Nq + 1] on the
        CPU, and the results of query n are ids[lims[n]:lims[n + 1]] / dists[...] (on the GPU with
        `set_return_results_on_gpu`).

        **Under the Euclidean measure distances are SQUARED L2 distances, and so is the radius**:
        pass r * r to get everything within Euclidean distance r.  Under Cosine it is |1 - cos|.  A
        vector belongs to the answer iff distance <= radius in float32, with exactly the distance
        `bf_query` reports.  `radius`: a scalar for all queries, or one value per query; +inf
        admits everything, a negative radius nothing, NaN is an error.

        `max_results=None` counts first (one distance pass), allocates exactly and calls again (two
        more passes: three in all).  An integer `max_results` makes one call (two passes) into
        buffers of that many entries and raises RuntimeError, naming the needed total, if they are
        too small.  `sort=True` orders each query's results by (distance, id), as `bf_query` would
        list them; `sort=False` keeps the engine's order, ascending id."""
        return self._range(lib().ggnn_bf_range_query, query, radius, measure, max_results, sort)

    def bf_range_query_filtered(self, query, radius, measure=DistanceMeasure.Euclidean,
                                max_results=None, sort=True, filter=None):
        """Extension: `bf_range_query` among the base vectors `filter` allows (see
        `query_filtered`).  `filter=None` is `bf_range_query`."""
        return self.bf_range_query_filtered_by(query, radius, measure, max_results, sort,
                                               filter=filter)

    def bf_range_query_filtered_by(self, query, radius, measure=DistanceMeasure.Euclidean,
                                   max_results=None, sort=True, filter_ids=None, filter=None):
        """Extension: `bf_range_query` with a filter per query (`filter_ids`, `filter`: see
        `query_filtered_by`)."""
        if filter is not None and filter_ids is not None:
            raise ValueError("give either filter or filter_ids, not both")
        if filter_ids is not None:
            fi = _filter_ids(filter_ids, _as_tensor(query, what="query").shape[0])
            return self._range(lib().ggnn_bf_range_query_filtered_by, query, radius, measure,
                               max_results, sort, self._where(fi))
        if filter is not None:
            f = _filter_words(filter, self._N)
            ptr, floc, fdev = self._where(f)
            return self._range(lib().ggnn_bf_range_query_filtered, query, radius, measure,
                               max_results, sort, (ptr, self._N, floc, fdev))
        return self.bf_range_query(query, radius, measure, max_results, sort)

    def bf_range_query_labeled(self, query, radius, measure=DistanceMeasure.Euclidean,
                               max_results=None, sort=True, labels=None):
        """Extension: `bf_range_query` among the base vectors that carry the query's label
        (`labels`: see `query_labeled`; -1 admits every vector).  `labels=None` is
        `bf_range_query`."""
        if labels is None:
            return self.bf_range_query(query, radius, measure, max_results, sort)
        ql = _labels(labels, _as_tensor(query, what="query").shape[0], per="query")
        return self._range(lib().ggnn_bf_range_query_labeled, query, radius, measure, max_results,
                           sort, self._where(ql))

    def range_query(self, query, radius, k_query, tau_query, max_iterations=400,
                    measure=DistanceMeasure.Euclidean):
        """Extension: the APPROXIMATE counterpart of `bf_range_query`: the graph search `query`,
        cut at the radius.  Returns the same (lims, ids, dists) triple, each query's results in
        ascending distance: the prefix of its `query` row with distance <= radius (squared units
        under Euclidean), unfilled slots (id -1) dropped.

        It can return AT MOST `k_query` vectors per query.  A query whose count lims[n + 1] -
        lims[n] equals `k_query` was cut by the list length, not by the radius: raise `k_query`
        (or use `bf_range_query`) for those."""
        from .ops import range_radii
        ids, dists = self.query(query, k_query, tau_query, max_iterations, measure)
        Nq = ids.shape[0]
        k = int(k_query)
        if ids.shape[1] != k:
            raise RuntimeError("range_query needs merged results: one shard per GPU, or results "
                               "returned on the host")
        r = range_radii(radius, Nq, dists.device)
        if bool(torch.isnan(r).any()):
            raise ValueError("a radius is NaN")
        ok = (dists <= r[:, None]) & (ids >= 0)
        keep = torch.cumprod(ok.to(torch.int32), dim=1).bool()   # the prefix only
        lims = torch.zeros(Nq + 1, dtype=torch.int64)
        lims[1:] = torch.cumsum(keep.sum(dim=1), dim=0).cpu()
        return lims, ids[keep], dists[keep]

    def get_graph(self, on_gpu_shard_id=0):
        """Access the GGNN graph."""
        view = _lib.GraphView()
        self._check(lib().ggnn_get_graph(self._h, int(on_gpu_shard_id), C.byref(view)))
        cfg = view.config
        K = cfg.KBuild

        def fetch(ptr, count, dtype):
            if count == 0:
                return torch.empty(0, dtype=dtype)
            out = torch.empty(count, dtype=dtype)
            nbytes = count * out.element_size()
            with torch.cuda.device(view.gpu_id):
                tmp = torch.empty(count, dtype=dtype, device="cuda")
                _hip_memcpy_d2d(tmp.data_ptr(), ptr, nbytes)
                out.copy_(tmp)
            return out

        graph_all = fetch(view.graph, cfg.N_all * K, torch.int32).view(cfg.N_all, K)
        tr_all = fetch(view.translation, cfg.ST_all, torch.int32)
        sel_all = fetch(view.selection, cfg.ST_all, torch.int32)
        stats = fetch(view.nn1_stats, 2, torch.float32).view(2, 1)
        graph, selection, translation = [], [], []
        for l in range(4):
            g = graph_all[cfg.Ns_offsets[l]:cfg.Ns_offsets[l] + cfg.Ns[l]]
            graph.append(IntDataset._wrap(g))
            if l:
                s = slice(cfg.STs_offsets[l], cfg.STs_offsets[l] + cfg.Ns[l])
                selection.append(IntDataset._wrap(sel_all[s].view(-1, 1)))
                translation.append(IntDataset._wrap(tr_all[s].view(-1, 1)))
            else:
                selection.append(IntDataset._wrap(torch.empty((0, 1), dtype=torch.int32)))
                translation.append(IntDataset._wrap(torch.empty((0, 1), dtype=torch.int32)))
        return Graph(graph, selection, translation, FloatDataset._wrap(stats), cfg.as_dict())

    # tracing helpers (not part of the reference surface)
    def last_timing_ms(self):
        b, q, f = C.c_float(), C.c_float(), C.c_float()
        self._check(lib().ggnn_last_timing_ms(self._h, C.byref(b), C.byref(q), C.byref(f)))
        return {"build_ms": b.value, "query_ms": q.value, "bf_query_ms": f.value}

    def set_collect_counters(self, enable=True):
        self._check(lib().ggnn_set_collect_counters(self._h, int(bool(enable))))
        self._collect_counters = bool(enable)

    def last_query_parts(self):
        """half-batches the last blocking multi-GPU query() was searched in (2: the second half's
        search overlapped the exchange and merge of the first)"""
        n = C.c_uint32()
        self._check(lib().ggnn_last_query_parts(self._h, C.byref(n)))
        return int(n.value)

    def rccl_ranks(self):
        """ranks of the RCCL communicator behind the handle's exchange (0: none in use)"""
        n = C.c_uint32()
        self._check(lib().ggnn_rccl_ranks(self._h, C.byref(n)))
        return int(n.value)

    def last_build_work(self):
        """work counters and kernel times of the merge / sym launches of the last build()
        (set_collect_counters(True) before the build): {"merge": {...}, "sym": {...}}"""
        w = _lib.BuildWork()
        self._check(lib().ggnn_last_build_work(self._h, C.byref(w)))
        return {"merge": w.merge.as_dict(), "sym": w.sym.as_dict()}

    def set_prescreen(self, enable=True):
        """Exact pre-screen of float32/Euclidean queries on an 8-bit copy of the base (an
        extension: same results, less memory traffic; costs N x D bytes per shard)."""
        self._check(lib().ggnn_set_prescreen(self._h, int(bool(enable))))

    def set_build_hooks(self, rng=None, serial_sym=False, deterministic_sym=False):
        """Deterministic build (see ggnn_set_build_hooks): `rng` = [3, N_shard] float32 uniform
        (0, 1] numbers for the selection kernel, `serial_sym` = sym one point per launch in
        ascending order.  Used to compare a whole build with a CPU restatement bit for bit.
        `deterministic_sym` instead: concurrent sym searches that ignore the inverse links of
        their own pass, slots handed out in ascending order -- the same graph on every run."""
        mode = 1 if serial_sym else (2 if deterministic_sym else 0)
        if rng is None:
            self._check(lib().ggnn_set_build_hooks(self._h, None, 0, mode))
            return
        arr = np.ascontiguousarray(np.asarray(rng, dtype=np.float32))
        self._check(lib().ggnn_set_build_hooks(self._h, arr.ctypes.data, arr.size, mode))

    def last_exchange(self):
        """how the last query combined per-GPU results: "none", "rccl" or "copy" """
        return lib().ggnn_last_exchange(self._h).decode()

    def last_bf_query_rescanned(self):
        """queries of the last bf_query answered by the exhaustive scan because the matrix-core
        pre-selection could not be certified exact (results are exact either way)"""
        n = C.c_uint32()
        self._check(lib().ggnn_last_bf_query_rescanned(self._h, C.byref(n)))
        return int(n.value)

    def last_bf_query_matrix_path(self):
        """1 if the last bf_query* call (filtered or not) ran the matrix-core tile kernel on every
        shard, else 0 (the scan kernels); results are bit-identical on either path"""
        n = C.c_int()
        self._check(lib().ggnn_last_bf_query_matrix_path(self._h, C.byref(n)))
        return int(n.value)

    def last_query_counters(self):
        d, p = C.c_uint64(), C.c_uint64()
        self._check(lib().ggnn_last_query_counters(self._h, C.byref(d), C.byref(p)))
        return {"n_dist": d.value, "n_pop": p.value}

    def last_query_rows_read(self):
        """float rows and 8-bit pre-screen rows read by the last query (with collect_counters)"""
        f, c = C.c_uint64(), C.c_uint64()
        self._check(lib().ggnn_last_query_rows_read(self._h, C.byref(f), C.byref(c)))
        return {"float_rows": f.value, "code_rows": c.value}


_hip = None


def _hip_memcpy_d2d(dst, src, nbytes):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    rc = _hip.hipMemcpy(dst, src, nbytes, 3)  # hipMemcpyDeviceToDevice
    if rc != 0:
        raise RuntimeError(f"hipMemcpy failed with {rc}")


# ---------------------------------------------------------------------------------------------
# Evaluator (include/ggnn/base/eval.h:31-65, src/ggnn/base/eval.cpp:37-242)
# ---------------------------------------------------------------------------------------------
class Evaluation:
    def __init__(self, k_query, c1, c1_dup, c_k_query, c_k_query_dup, r_k_query, r_k_query_dup):
        self.k_query = k_query
        self.c1 = c1
        self.c1_dup = c1_dup
        self.c_k_query = c_k_query
        self.c_k_query_dup = c_k_query_dup
        self.r_k_query = r_k_query
        self.r_k_query_dup = r_k_query_dup

    def __repr__(self):
        # operator<<, eval.cpp:67-86
        def dup(v, nl):
            if not np.isnan(v):
                return f" +duplicates: {v:g}" + ("\n" if nl else "")
            return " (duplicates unknown)" + ("\n" if nl else "")
        return (f"c@1 (=r@1): {self.c1:g}" + dup(self.c1_dup, True) +
                f"c@{self.k_query}: {self.c_k_query:g}" + dup(self.c_k_query_dup, True) +
                f"r@{self.k_query}: {self.r_k_query:g}" + dup(self.r_k_query_dup, False))


def _eval_distance(base_rows, query_rows, measure):
    """compute_distance, eval.cpp:37-65 incl. its quirks (Euclidean WITH sqrt; the cosine
    variant uses the base vector for both norms)."""
    a = base_rows.astype(np.float32)
    b = query_rows.astype(np.float32)
    if measure == DistanceMeasure.Euclidean:
        return np.sqrt(((a - b) ** 2).sum(-1, dtype=np.float32))
    dot = (a * b).sum(-1, dtype=np.float32)
    na = (a * a).sum(-1, dtype=np.float32)
    prod = na * na
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(np.float32(1.0) - dot / np.sqrt(prod))
    return np.where(prod > 0, d, np.float32(1.0)).astype(np.float32)


class Evaluator:
    def __init__(self, base, query, gt, k_query, measure=DistanceMeasure.Euclidean):
        self.k_query = int(k_query)
        self.measure = DistanceMeasure(measure)
        gt_t = _as_tensor(gt, torch.int32, "gt")
        if gt_t.is_cuda:
            raise RuntimeError("Ground truth data needs to be given on the CPU for evaluation.")
        self.gt = gt_t.numpy().copy()
        self.top1_end = None
        self.topk_end = None
        base_t = _as_tensor(base, what="base")
        query_t = _as_tensor(query, what="query")
        if base_t.shape[0] == 0 or query_t.shape[0] == 0 or base_t.is_cuda or query_t.is_cuda:
            return  # duplicates unknown (eval.cpp:93-102)
        if base_t.dtype != query_t.dtype:
            raise RuntimeError("base and query need to have the same data type")
        b, q = _host_rows(base_t), _host_rows(query_t)
        Nq, gtD, K = q.shape[0], self.gt.shape[1], self.k_query
        eps = np.float32(0.000001)
        # distances of all ground-truth entries, [Nq, gtD]
        gd = np.stack([_eval_distance(b[self.gt[:, k]], q, self.measure) for k in range(gtD)], 1)

        def run_length(ref, start):
            # number of consecutive entries from `start` whose distance stays within eps
            within = (gd[:, start:] - ref[:, None]) <= eps
            if within.shape[1] == 0:
                return np.zeros(Nq, np.uint32)
            stop = np.where(within.all(1), within.shape[1], np.argmin(within, 1))
            return stop.astype(np.uint32)

        self.top1_end = 1 + run_length(gd[:, 0], 1)
        if K <= gtD:
            self.topk_end = K + run_length(gd[:, K - 1], K)
        else:
            self.topk_end = np.full(Nq, gtD, np.uint32)

    def evaluate_results(self, results):
        """Evaluate the accuracy of a query result."""
        res_t = _as_tensor(results, torch.int32, "results")
        if res_t.is_cuda:
            raise RuntimeError("Results need to be given on the CPU for evaluation.")
        res = res_t.numpy()
        K, gt = self.k_query, self.gt
        if gt.shape[1] == 0:
            raise RuntimeError("No ground truth data loaded. cannot compute accuracy.")
        N = res.shape[0]
        has_dup = self.top1_end is not None
        end1 = self.top1_end[:N] if has_dup else np.ones(N, np.uint32)
        endk = self.topk_end[:N] if has_dup else np.full(N, K, np.uint32)
        gtD = gt.shape[1]
        kg = np.arange(gtD)[None, None, :]                       # [1,1,gtD]
        match = res[:N, :K, None] == gt[:N, None, :]             # [N,K,gtD]
        match &= kg < endk[:, None, None]
        first_res = np.zeros((1, K, 1), bool)
        first_res[0, 0, 0] = True
        c1 = int((match[:, :, :1] & first_res).sum())
        r_k_dup = int(match[:, :, 0].sum())
        r_k = r_k_dup if K > 0 else 0
        c1_dup = int((match & first_res & (kg < end1[:, None, None])).sum())
        c_k = int((match & (kg < K)).sum())
        c_k_dup = int(match.sum())
        inv_q = np.float32(1.0) / np.float32(N)
        inv_r = np.float32(1.0) / np.float32(N * K)
        nan = float("nan")
        return Evaluation(K, float(c1 * inv_q), float(c1_dup * inv_q) if has_dup else nan,
                          float(c_k * inv_r), float(c_k_dup * inv_r) if has_dup else nan,
                          float(r_k * inv_q), float(r_k_dup * inv_q) if has_dup else nan)
