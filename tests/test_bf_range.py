"""Range search without a GPU: argument checks of the C interface that never reach a device, the
Python helpers (radius broadcasting, the segment sort against numpy's lexsort), and the private
segment of every bf_range_kernel instantiation, from the built library's metadata."""
import ctypes as C

import numpy as np
import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture: the library's kernel metadata)

torch = pytest.importorskip("torch")


@pytest.fixture()
def handle():
    from ggnn_amd import _lib
    h = C.c_void_p()
    assert _lib.lib().ggnn_create(C.byref(h)) == _lib.OK
    yield h
    _lib.lib().ggnn_destroy(h)


def _call(h, q, radii, lims, capacity=0):
    from ggnn_amd import _lib
    return _lib.lib().ggnn_bf_range_query(
        h, q.ctypes.data, q.shape[0], q.shape[1], _lib.F32, _lib.CPU, 0,
        None if radii is None else radii.ctypes.data, 0, capacity,
        None if lims is None else lims.ctypes.data, None, None, _lib.CPU)


def test_nan_radius_is_invalid_argument(handle):
    from ggnn_amd import _lib
    q = np.zeros((3, 32), np.float32)
    lims = np.full(4, 99, np.uint64)
    st = _call(handle, q, np.array([1.0, np.nan, 2.0], np.float32), lims)
    assert st == _lib.INVALID_ARGUMENT
    assert b"NaN" in _lib.lib().ggnn_last_error(handle)
    assert b"query 1" in _lib.lib().ggnn_last_error(handle)


def test_null_lims_and_null_radii_are_invalid_argument(handle):
    from ggnn_amd import _lib
    q = np.zeros((3, 32), np.float32)
    assert _call(handle, q, np.ones(3, np.float32), None) == _lib.INVALID_ARGUMENT
    assert _call(handle, q, None, np.zeros(4, np.uint64)) == _lib.INVALID_ARGUMENT
    # capacity without buffers
    assert _call(handle, q, np.ones(3, np.float32), np.zeros(4, np.uint64), capacity=5) == \
        _lib.INVALID_ARGUMENT
    assert _lib.lib().ggnn_bf_range_query(None, None, 0, 0, 0, 0, 0, None, 0, 0, None, None, None,
                                          0) == _lib.INVALID_ARGUMENT


def test_without_a_base_is_invalid_state(handle):
    from ggnn_amd import _lib
    q = np.zeros((3, 32), np.float32)
    assert _call(handle, q, np.ones(3, np.float32), np.zeros(4, np.uint64)) == _lib.INVALID_STATE


def test_wrong_radii_length():
    import ggnn_amd as ggnn
    from ggnn_amd import ops
    eng = ggnn.GGNN()
    q = np.zeros((3, 32), np.float32)
    for bad in (np.ones(2, np.float32), np.ones(4, np.float32), np.ones((3, 1), np.float32)):
        with pytest.raises(ValueError, match="one entry per query"):
            eng.bf_range_query(q, bad)
        with pytest.raises(ValueError, match="one entry per query"):
            ops.range_radii(bad, 3)


def test_radius_broadcasting():
    from ggnn_amd import ops
    r = ops.range_radii(2.5, 4)
    assert r.dtype == torch.float32 and r.tolist() == [2.5] * 4 and r.is_contiguous()
    assert ops.range_radii(np.float64(3), 2).tolist() == [3.0, 3.0]
    r = ops.range_radii([1, 2, 3], 3)
    assert r.dtype == torch.float32 and r.tolist() == [1.0, 2.0, 3.0]
    r = ops.range_radii(torch.tensor([np.inf, -1.0], dtype=torch.float64), 2)
    assert r.dtype == torch.float32 and r.tolist() == [np.inf, -1.0]
    assert ops.range_radii(1.0, 0).numel() == 0


@pytest.mark.parametrize("seed", range(4))
def test_segment_sort_is_numpy_lexsort(seed):
    from ggnn_amd import ops
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 40, 23)
    counts[rng.integers(0, 23, 4)] = 0                     # empty segments, first and last included
    counts[0] = counts[-1] = 0 if seed % 2 else 5
    lims = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    # ascending ids inside a segment, few distinct distances: many ties
    ids = np.concatenate([np.sort(rng.choice(1000, c, replace=False)) for c in counts] +
                         [np.empty(0, np.int64)]).astype(np.int32)
    d = rng.integers(0, 4, ids.size).astype(np.float32)
    d[rng.random(ids.size) < 0.1] = np.inf
    seg = np.repeat(np.arange(23), counts)
    o = np.lexsort((ids, d, seg))
    got_ids, got_d = ops.sort_segments(torch.from_numpy(lims), torch.from_numpy(ids),
                                       torch.from_numpy(d))
    assert np.array_equal(got_ids.numpy(), ids[o])
    assert got_d.numpy().tobytes() == d[o].tobytes()


def test_segment_sort_of_nothing():
    from ggnn_amd import ops
    ids, d = ops.sort_segments(torch.zeros(4, dtype=torch.int64), torch.empty(0, dtype=torch.int32),
                               torch.empty(0, dtype=torch.float32))
    assert ids.numel() == 0 and d.numel() == 0


def test_range_kernels_have_no_private_segment(kernels):  # noqa: F811
    mine = {n: v for n, v in kernels.items() if n.startswith("bf_range_kernel<")}
    # 5 element types x 7 layouts (int8: 6) x 2 measures x 3 filter forms x 2 passes
    assert len(mine) == (4 * 7 + 6) * 2 * 3 * 2, len(mine)
    bad = {n: v for n, v in mine.items()
           if v.get("private_segment_fixed_size") != 0 or v.get("vgpr_spill_count", 0) != 0}
    assert not bad, bad
    assert kernels["bf_range_prefix_kernel"]["private_segment_fixed_size"] == 0
