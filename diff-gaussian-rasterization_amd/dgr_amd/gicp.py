"""Generalized ICP over the kNN index on the device (C ABI: dgr_point_covariances, dgr_gicp_step; the rules are stated in
include/dgr_hip.h): per-point neighbourhood covariances, one fused Gauss-Newton iteration over nearest-neighbour pairs, and
`gicp_align`, the chain of iterations that registers two clouds which need not overlap pixel for pixel -- a loop edge for
`pose_graph_optimize`, or a frame against a Gaussian map's own covariances (GS-ICP SLAM's scan-to-map form)."""
from typing import NamedTuple as _NamedTuple

import torch

from . import _capi
from ._align import INF, _Chain, _number, _pose
from .knn import KnnIndex, _check_gpu, _points, knn_build, knn_search

_MODES = {"raw": _capi.COV_RAW, "plane": _capi.COV_PLANE}


class PointCovariances(_NamedTuple):
    """What `point_covariances` leaves on the device: `cov` float32 [P,8] rows (c00, c01, c02, c11, c12, c22, sigma, n), n = 0
    on an invalid row; `normals` float32 [P,4] = (v_0, sigma) or None; `log_scales` [P,3] (largest first) and `quats` [P,4]
    (r, x, y, z) or None; `flags` uint8 [P] (bit 0 valid); `index`, the KnnIndex the neighbourhoods came from."""
    cov: torch.Tensor
    normals: torch.Tensor
    log_scales: torch.Tensor
    quats: torch.Tensor
    flags: torch.Tensor
    index: KnnIndex


class GicpResult(_NamedTuple):
    """What `gicp_align` leaves on the device: `transform` float32 [4,4], source to target coordinates, stored transposed with
    the translation in its last row (`relative_pose`'s layout); `quat` [4] (r, x, y, z; unit, r >= 0) and `trans` [3] of the same
    motion; `stats` float64 [iterations, 32] per iteration: A (21, the upper triangle row-major), b (6), sum w s^2 [27], count
    [28], ok [29], |omega| [30], |v| [31]; `idx` int32 [S] (the last iteration's association, -1: none) and `flags` uint8 [S]
    (bit 0 valid, bit 1 associated, bit 2 singular), each None unless asked for."""
    transform: torch.Tensor
    quat: torch.Tensor
    trans: torch.Tensor
    stats: torch.Tensor
    idx: torch.Tensor
    flags: torch.Tensor


def point_covariances(points, index=None, *, k=10, include_self=True, mode="plane", epsilon=1e-3, min_neighbours=4, viewpoint=None,
                      scale_floor=1e-4, return_normals=False, return_gaussians=False):
    """The covariance of every point's `k` nearest neighbours (`include_self`: the point itself among them): `cov` [P,8] rows
    (c00, c01, c02, c11, c12, c22, sigma, n) for `gicp_align`.  `mode` "plane" is Generalized ICP's regularised form,
    I - (1 - epsilon) n n^T with n the neighbourhood's normal (variance `epsilon` along it, 1 across); "raw" the covariance
    itself.  sigma = lambda_0 / (lambda_0 + lambda_1 + lambda_2), the surface variation.  A row with a non-finite point, fewer
    than `min_neighbours` (>= 3) neighbours or a zero covariance is invalid: all zeros, flag 0, never paired by `gicp_align`.
    `return_normals`: `normals` [P,4] = (n, sigma), n turned toward `viewpoint` (three numbers; the origin for a camera-frame
    cloud gives `depth_normals`' facing convention) or, without one, so that its largest component is positive.
    `return_gaussians`: `log_scales` [P,3] = log of the standard deviations along the principal axes, largest first and not below
    log(`scale_floor`), and `quats` [P,4] of that frame: the anisotropic Gaussians GS-ICP SLAM seeds.
    `points` [P,3] float32 on the GPU; `index`: what `knn_build(points)` returned (built here when None).  One search and one
    launch, nothing read on the host, the same bits on every run.  Returns PointCovariances."""
    what = "point_covariances"
    _points(what, "points", points)
    if index is not None and not isinstance(index, KnnIndex):
        raise ValueError(f"{what}: index must be what knn_build returned, not {type(index).__name__}")
    k = int(k)
    if not 1 <= k <= _capi.KNN_MAX_K:
        raise ValueError(f"{what}: k must be 1 .. {_capi.KNN_MAX_K}, not {k}")
    if mode not in _MODES:
        raise ValueError(f"{what}: mode must be 'plane' or 'raw', not {mode!r}")
    epsilon = _number(what, "epsilon", epsilon)
    if not 0.0 < epsilon <= 1.0:
        raise ValueError(f"{what}: epsilon must lie in (0, 1], not {epsilon}")
    min_neighbours = int(min_neighbours)
    if not 3 <= min_neighbours <= k:
        raise ValueError(f"{what}: min_neighbours must be 3 .. k = {k}, not {min_neighbours}")
    scale_floor = _number(what, "scale_floor", scale_floor)
    view = (0.0, 0.0, 0.0)
    if viewpoint is not None:
        view = tuple(_number(what, "viewpoint", v) for v in viewpoint)
        if len(view) != 3:
            raise ValueError(f"{what}: viewpoint is three numbers, not {len(view)}")
    if index is not None and index.points.shape[0] != points.shape[0]:
        raise ValueError(f"{what}: index was built for {index.points.shape[0]} points, not {points.shape[0]}")
    _check_gpu(what, points, *(() if index is None else (index.points,)))
    points = points.detach().contiguous()
    if index is None:
        index = knn_build(points)
    P, dev = points.shape[0], points.device
    idx = knn_search(index, None, k, exclude_self=not include_self).idx
    cov = torch.empty((P, 8), dtype=torch.float32, device=dev)
    normals = torch.empty((P, 4), dtype=torch.float32, device=dev) if return_normals else None
    log_scales = torch.empty((P, 3), dtype=torch.float32, device=dev) if return_gaussians else None
    quats = torch.empty((P, 4), dtype=torch.float32, device=dev) if return_gaussians else None
    flags = torch.empty((P,), dtype=torch.uint8, device=dev)
    params = _capi.CovarianceParams(_MODES[mode], epsilon, min_neighbours, scale_floor, (_capi._f * 3)(*view), 0 if viewpoint is None else 1)
    _capi.call("dgr_point_covariances", dev, P, points.data_ptr(), k, idx.data_ptr(), params, cov.data_ptr(), _capi.ptr(normals),
               _capi.ptr(log_scales), _capi.ptr(quats), flags.data_ptr())
    return PointCovariances(cov, normals, log_scales, quats, flags, index)


def gaussian_covariances(scales, rotations):
    """The packed `[N,8]` covariance rows of a Gaussian map for `gicp_align`'s target side: Sigma = R S S^T R^T from `scales`
    [N,3] (standard deviations, activated) and `rotations` [N,4] (r, x, y, z; normalised here), sigma from the scales' squares,
    n = 1.  Torch ops; rows with a non-finite entry get n = 0."""
    if not (isinstance(scales, torch.Tensor) and isinstance(rotations, torch.Tensor)):
        raise ValueError("gaussian_covariances: scales and rotations must be tensors")
    if scales.dim() != 2 or scales.shape[1] != 3 or rotations.dim() != 2 or rotations.shape[1] != 4 or scales.shape[0] != rotations.shape[0]:
        raise ValueError(f"gaussian_covariances: scales is [N,3] and rotations [N,4], not {tuple(scales.shape)} and {tuple(rotations.shape)}")
    s, q = scales.detach().double(), rotations.detach().double()
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    var = s * s
    C = (R * var[:, None, :]) @ R.transpose(1, 2)
    sigma = var.min(dim=1).values / var.sum(dim=1)
    rows = torch.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2], sigma, torch.ones_like(sigma)], 1)
    ok = torch.isfinite(rows).all(dim=1, keepdim=True)
    return torch.where(ok, rows, torch.zeros_like(rows)).float().contiguous()


def unproject_depth(depth, fx, fy, cx, cy, stride=1, depth_range=(0.0, INF)):
    """The camera-frame cloud [S,3] of a depth image's stride grid (pixels x, y = 0, stride, ..; the ICP steps' candidates):
    ((x - cx) / fx d, (y - cy) / fy d, d).  A pixel whose depth is not inside `depth_range` (exclusive) becomes a NaN row, which the
    kNN index, `point_covariances` and `gicp_align` all leave out: no compaction, nothing read on the host.  Torch ops."""
    what = "unproject_depth"
    if not isinstance(depth, torch.Tensor):
        raise ValueError(f"{what}: depth must be a tensor, not {type(depth).__name__}")
    if depth.dtype != torch.float32:
        raise ValueError(f"{what}: depth must be float32, not {depth.dtype}")
    if depth.dim() == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if depth.dim() != 2 or depth.numel() == 0:
        raise ValueError(f"{what}: depth is [H,W] or [1,H,W], not {tuple(depth.shape)}")
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"{what}: stride must be positive, not {stride}")
    fx, fy, cx, cy = (_number(what, n, v) for n, v in (("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy)))
    if not (0.0 < fx < INF and 0.0 < fy < INF):
        raise ValueError(f"{what}: fx and fy must be finite and positive")
    lo, hi = (_number(what, "depth_range", v) for v in depth_range)
    d = depth.detach()[::stride, ::stride]
    H, W = d.shape
    x = torch.arange(W, dtype=torch.float32, device=d.device) * stride
    y = torch.arange(H, dtype=torch.float32, device=d.device) * stride
    ok = (d > lo) & (d < hi)
    d = torch.where(ok, d, torch.full_like(d, float("nan")))
    return torch.stack([(x[None, :] - cx) / fx * d, (y[:, None] - cy) / fy * d, d], -1).reshape(-1, 3).contiguous()


def _cov_rows(what, name, t, n):
    if t is None:
        return None
    if isinstance(t, PointCovariances):
        t = t.cov
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (n, 8) or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous float32 tensor [{n},8] (point_covariances' cov) or None")
    return t


def _transform(what, name, t):
    return _pose(what, name, t, "the motion transposed, relative_pose's layout")


def _step_numbers(what, max_distance, huber_delta, damping, rcond, min_points):
    out = [_number(what, n, v, 0.0) for n, v in (("max_distance", max_distance), ("huber_delta", huber_delta), ("damping", damping),
                                                  ("rcond", rcond))]
    min_points = int(min_points)
    if min_points < 1:
        raise ValueError(f"{what}: min_points must be at least 1, not {min_points}")
    return _capi.GicpParams(*out, min_points)


def _scratch(what, N, S, dev):
    size = _capi.load().dgr_gicp_scratch_bytes(N, S)
    if not size:
        raise ValueError(f"{what}: source and target must hold 1 .. 2^24 points each")
    return torch.zeros((size,), dtype=torch.uint8, device=dev)


def _target(what, target, target_index):
    if target_index is not None and not isinstance(target_index, KnnIndex):
        raise ValueError(f"{what}: target_index must be what knn_build returned, not {type(target_index).__name__}")
    if target_index is not None and target_index.points.shape[0] != target.shape[0]:
        raise ValueError(f"{what}: target_index was built for {target_index.points.shape[0]} points, not {target.shape[0]}")


def gicp_step(source, target_index, transform_in, *, transform_out=None, source_cov=None, target_cov=None, max_distance=INF,
              huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6, return_idx=False, return_flags=False, scratch=None):
    """One Gauss-Newton iteration (include/dgr_hip.h: dgr_gicp_step) of `source` [S,3] against the points of `target_index`
    (what `knn_build(target)` returned) at the estimate `transform_in`.  Returns GicpResult with `stats` [1, 32];
    `transform_out` (a contiguous float32 [4,4] GPU tensor, which may be `transform_in`) receives the motion when given.
    `scratch`: a zero-filled uint8 tensor of dgr_gicp_scratch_bytes to reuse; None allocates one."""
    what = "gicp_step"
    _points(what, "source", source)
    if not isinstance(target_index, KnnIndex):
        raise ValueError(f"{what}: target_index must be what knn_build returned, not {type(target_index).__name__}")
    target = target_index.points
    S, N = source.shape[0], target.shape[0]
    source_cov, target_cov = _cov_rows(what, "source_cov", source_cov, S), _cov_rows(what, "target_cov", target_cov, N)
    transform_in = _transform(what, "transform_in", transform_in)
    params = _step_numbers(what, max_distance, huber_delta, damping, rcond, min_points)
    _check_gpu(what, source, target, transform_in, *(t for t in (source_cov, target_cov) if t is not None))
    dev = source.device
    source, transform_in = source.detach().contiguous(), transform_in.contiguous()
    chain = _Chain(torch, what, dev, 1, 32, out=transform_out, out_name="transform_out", flags=S if return_flags else None,
                   idx=S if return_idx else None)
    if scratch is None:
        scratch = _scratch(what, N, S, dev)
    _capi.call("dgr_gicp_step", dev, target_index.index.data_ptr(), N, target.data_ptr(), _capi.ptr(target_cov), S, source.data_ptr(),
               _capi.ptr(source_cov), transform_in.data_ptr(), params, scratch.data_ptr(), *chain.tail(0))
    return chain.result(GicpResult)


def gicp_align(source, target, *, transform=None, source_cov=None, target_cov=None, target_index=None, iterations=15,
               max_distance=INF, huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6, return_idx=False, return_flags=False):
    """Generalized ICP: the rigid motion that takes `source` [S,3] onto `target` [N,3], from a first estimate `transform`
    (None: the identity).  Every iteration moves the source by the current estimate, pairs each of its points with the nearest
    target point within `max_distance` (the exact kNN search; `target_index`: what `knn_build(target)` returned, built here when
    None), and takes one 6 x 6 Gauss-Newton step over sum e^T (C_B + R C_A R^T)^-1 e with the pairs' covariances --
    `source_cov`, `target_cov`: `point_covariances(...)` or its `cov`, any [*,8] rows of that packing (`gaussian_covariances`
    of a map), or None: a side without covariances contributes nothing, and with neither the step is point-to-point ICP.
    `huber_delta` (on the Mahalanobis length), `damping`, `rcond`, `min_points`: as `icp_align`'s; a refused step keeps the motion.
    `transform` is the motion transposed with the translation in its last row -- `relative_pose`'s layout: with the source a
    cloud in camera j's frame and the target one in camera i's, the result is the measurement Z_ij `pose_graph_optimize` takes.
    `iterations` steps (a fixed number: nothing is read on the host) run in place on one device tensor, so the whole call
    records into a hipGraph; the bits are the same on every run.  Rows with a non-finite coordinate (`unproject_depth`'s
    unusable pixels) take no part.  Returns GicpResult(transform, quat, trans, stats, idx, flags)."""
    what = "gicp_align"
    _points(what, "source", source)
    _points(what, "target", target)
    _target(what, target, target_index)
    S, N = source.shape[0], target.shape[0]
    source_cov, target_cov = _cov_rows(what, "source_cov", source_cov, S), _cov_rows(what, "target_cov", target_cov, N)
    if transform is not None:
        transform = _transform(what, "transform", transform)
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError(f"{what}: iterations must be at least 1, not {iterations}")
    params = _step_numbers(what, max_distance, huber_delta, damping, rcond, min_points)
    tensors = [t for t in (source, target, transform, source_cov, target_cov) if t is not None]
    if target_index is not None:
        tensors.append(target_index.points)
    _check_gpu(what, *tensors)
    dev = source.device
    source = source.detach().contiguous()
    if target_index is None:
        target_index = knn_build(target)
    target = target_index.points
    chain = _Chain(torch, what, dev, iterations, 32, first=torch.eye(4, dtype=torch.float32, device=dev) if transform is None else transform,
                   flags=S if return_flags else None, idx=S if return_idx else None)
    scratch = _scratch(what, N, S, dev)
    with _capi.StepCalls(dev) as abi:
        for k in range(iterations):
            abi.call("dgr_gicp_step", target_index.index.data_ptr(), N, target.data_ptr(), _capi.ptr(target_cov), S, source.data_ptr(),
                     _capi.ptr(source_cov), chain.pose.data_ptr(), params, scratch.data_ptr(), *chain.tail(k))
    return chain.result(GicpResult)
