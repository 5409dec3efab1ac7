"""Exact k-nearest-neighbour search on the device (C ABI: dgr_knn_build, dgr_knn_search; the rule is stated in include/dgr_hip.h)
and simple-knn's `distCUDA2` on top of it."""
import math as _math
import struct as _struct
from typing import NamedTuple as _NamedTuple

import torch

from . import _capi

_MAX = 1 << 24


class KnnIndex(_NamedTuple):
    """What `knn_build` leaves on the device: `points` float32 [P,3] (the tensor indexed; the index holds a copy of its
    coordinates as they were), `index` and `scratch` uint8 (opaque)."""
    points: torch.Tensor
    index: torch.Tensor
    scratch: torch.Tensor


class KnnResult(_NamedTuple):
    """`dist2` float32 [Q,k] ascending, `idx` int32 [Q,k] (rows of the indexed points; -1 and +inf past `count`), `count` int32
    [Q] or None, `mean_dist2` float32 [Q] or None."""
    dist2: torch.Tensor
    idx: torch.Tensor
    count: torch.Tensor
    mean_dist2: torch.Tensor


def _points(what, name, t):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, not {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, not {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: {name} is [N,3], not {tuple(t.shape)}")
    if not 1 <= t.shape[0] <= _MAX:
        raise ValueError(f"{what}: {name} must hold 1 .. 2^24 rows, not {t.shape[0]}")


def _check_gpu(what, *tensors):
    if any(not t.is_cuda for t in tensors):
        raise ValueError(f"{what}: the points must be GPU tensors (there is no CPU fallback)")
    if any(t.device != tensors[0].device for t in tensors):
        raise ValueError(f"{what}: the tensors are on different devices")


def _bytes(n, device):
    return torch.empty((n,), dtype=torch.uint8, device=device)


def knn_build(points):
    """The search index of `points` ([P,3] float32 on the GPU; rows with a non-finite coordinate are left out): a Morton sort and
    256-point leaves with their boxes, 16 launches, nothing read on the host, capturable into a hipGraph.  Returns a
    KnnIndex for `knn_search`; build again after the points have moved."""
    what = "knn_build"
    _points(what, "points", points)
    _check_gpu(what, points)
    points = points.detach().contiguous()
    P, dev, lib = points.shape[0], points.device, _capi.load()
    index = _bytes(lib.dgr_knn_index_bytes(P), dev)
    scratch = _bytes(lib.dgr_knn_scratch_bytes(P, P), dev)
    _capi.call("dgr_knn_build", dev, P, points.data_ptr(), index.data_ptr(), scratch.data_ptr())
    return KnnIndex(points, index, scratch)


def _square(max_distance):
    """a distance, squared in float64 and rounded once to float32"""
    d = float(max_distance)
    if d != d or d < 0.0:
        raise ValueError(f"knn_search: max_distance must not be NaN or negative, not {d}")
    if _math.isinf(d):
        return d
    sq = d * d
    try:
        return _struct.unpack("f", _struct.pack("f", sq))[0]
    except OverflowError:
        return float("inf")


def knn_search(index, queries=None, k=3, *, exclude_self=None, max_distance=float("inf"), return_count=False, return_mean=False):
    """The `k` nearest indexed points of every query, exactly: candidates ordered by (squared distance in float32 with every
    operation rounded once, index), those within `max_distance` (inclusive) admitted, the first `k` returned in ascending order.
    `queries` [Q,3] float32, or None: the indexed points themselves (query i is point i); `exclude_self` (self mode only, there
    the default) leaves a point out of its own neighbours, other coincident points stay.  1 <= k <= 16.
    Returns KnnResult(dist2, idx, count, mean_dist2): slots past a query's `count` hold -1 / +inf; `count` and `mean_dist2`
    (the mean of the k squared distances, +inf with fewer than k) are None unless asked for.  Same bits on every run, nothing
    read on the host, capturable into a hipGraph."""
    what = "knn_search"
    if not isinstance(index, KnnIndex):
        raise ValueError(f"{what}: index must be what knn_build returned, not {type(index).__name__}")
    self_mode = queries is None
    if not self_mode:
        _points(what, "queries", queries)
    k = int(k)
    if not 1 <= k <= _capi.KNN_MAX_K:
        raise ValueError(f"{what}: k must be 1 .. {_capi.KNN_MAX_K}, not {k}")
    if exclude_self is None:
        exclude_self = self_mode
    if exclude_self and not self_mode:
        raise ValueError(f"{what}: exclude_self is defined in self mode only (queries=None)")
    max_d2 = _square(max_distance)
    _check_gpu(what, index.points, *(() if self_mode else (queries,)))
    dev, P, lib = index.points.device, index.points.shape[0], _capi.load()
    if self_mode:
        Q, q_ptr, scratch = P, None, index.scratch
    else:
        queries = queries.detach().contiguous()
        Q, q_ptr = queries.shape[0], queries.data_ptr()
        need = lib.dgr_knn_scratch_bytes(P, Q)
        scratch = index.scratch if index.scratch.numel() >= need else _bytes(need, dev)
    dist2 = torch.empty((Q, k), dtype=torch.float32, device=dev)
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    count = torch.empty((Q,), dtype=torch.int32, device=dev) if return_count else None
    mean = torch.empty((Q,), dtype=torch.float32, device=dev) if return_mean else None
    params = _capi.KnnParams(k, 1 if exclude_self else 0, max_d2)
    _capi.call("dgr_knn_search", dev, index.index.data_ptr(), P, index.points.data_ptr(), Q, q_ptr, params, scratch.data_ptr(),
               dist2.data_ptr(), idx.data_ptr(), _capi.ptr(count), _capi.ptr(mean))
    return KnnResult(dist2, idx, count, mean)


def dist2(points):
    """simple-knn's `distCUDA2`: for every point the mean squared distance to its three nearest other points, float32 [P].
    +inf where fewer than three other valid points exist (simple-knn returns a FLT_MAX-derived value there) and for a row with a
    non-finite coordinate; the reference is the brute-force model of the rule, not simple-knn's bits."""
    index = knn_build(points)  # (which checks `points`)
    P, dev = index.points.shape[0], index.points.device
    mean = torch.empty((P,), dtype=torch.float32, device=dev)
    _capi.call("dgr_knn_search", dev, index.index.data_ptr(), P, index.points.data_ptr(), P, None, _capi.KnnParams(3, 1, float("inf")),
               index.scratch.data_ptr(), None, None, None, mean.data_ptr())
    return mean
