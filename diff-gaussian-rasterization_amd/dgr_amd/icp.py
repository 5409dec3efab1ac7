"""Frame-to-model ICP pose alignment on the device (C ABI: dgr_depth_normals, dgr_icp_step): the packed vertex-normal map of a
depth image, one fused Gauss-Newton iteration of projective point-to-plane ICP, and `icp_align`, the chain of iterations that
initialises the photometric tracker's pose from the sensor depth and the model's rendered depth."""
from typing import NamedTuple as _NamedTuple

import torch

from . import _capi
from ._align import INF, _Chain, _pose, _scalars, _step_scratch
from .losses import _check_gpu


class IcpResult(_NamedTuple):
    """What `icp_align` leaves on the device: `viewmatrix` float32 [4,4] (W2C^T) with `quat` [4] (r, x, y, z; unit, r >= 0) and
    `trans` [3] of the same pose (pose_to_camera's convention); `stats` float64 [iterations, 32] per iteration: A (21, the upper
    triangle row-major), b (6), sum w r^2 [27], count [28], ok [29], |omega| [30], |v| [31]; `flags` uint8 [S] of the LAST
    iteration's candidates (bit 0 valid, bit 1 inside, bit 2 associated) or None."""
    viewmatrix: torch.Tensor
    quat: torch.Tensor
    trans: torch.Tensor
    stats: torch.Tensor
    flags: torch.Tensor


def _image(what, name, t, shape=None):
    """a float32 [H,W] (or [1,H,W]) image tensor as [H,W]"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, not {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, not {t.dtype}")
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"{what}: {name} is [H,W] or [1,H,W], not {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} {tuple(t.shape)} is not [H,W] = {tuple(shape)}")
    return t


def _depth_range(what, depth_range):
    lo, hi = (float(x) for x in depth_range)
    if lo != lo or hi != hi:
        raise ValueError(f"{what}: depth_range must not be NaN")
    return lo, hi


def _normals_into(abi, vnmap, depth, mask_image, s, lo, hi):
    H, W = depth.shape
    abi.call("dgr_depth_normals", W, H, depth.data_ptr(), _capi.ptr(mask_image), s["mask_threshold"], s["fx"], s["fy"], s["cx"],
             s["cy"], lo, hi, s["max_jump"], vnmap.data_ptr())


def depth_normals(depth, fx, fy, cx, cy, *, depth_range=(0.0, INF), max_jump=0.1, mask_image=None, mask_threshold=0.99):
    """The packed vertex-normal map of a depth image: `vnmap` float32 [H,W,4] = (nx, ny, nz, d), one launch.  A pixel is usable
    when it and its four neighbours x +- 1, y +- 1 lie inside the image with a depth in `depth_range` (exclusive), its own
    `mask_image` (e.g. the rasterizer's `opacity_map`) exceeds `mask_threshold`, and every neighbour's depth is within
    `max_jump * d` of its own; its normal is the normalised cross product of the central differences of the unprojected
    neighbours ((x - cx) / fx d, (y - cy) / fy d, d), turned to face the camera, and `d` is its depth.  Every other pixel -- the
    border among them -- is four zeros.  `depth`, `mask_image`: [H,W] or [1,H,W] float32 GPU tensors.  What `icp_align`
    gathers from (one 16-byte load per pixel); on its own: normal regularisers, visualisation."""
    what = "depth_normals"
    depth = _image(what, "depth", depth)
    tensors = [depth]
    if mask_image is not None:
        mask_image = _image(what, "mask_image", mask_image, depth.shape)
        tensors.append(mask_image)
    s = _scalars(what, fx, fy, cx=(cx, None), cy=(cy, None), max_jump=(max_jump, 0.0), mask_threshold=(mask_threshold, None))
    lo, hi = _depth_range(what, depth_range)
    _check_gpu(what, *tensors)
    depth = depth.detach().contiguous()
    if mask_image is not None:
        mask_image = mask_image.detach().contiguous()
    vnmap = torch.empty((depth.shape[0], depth.shape[1], 4), dtype=torch.float32, device=depth.device)
    with _capi.StepCalls(depth.device) as abi:
        _normals_into(abi, vnmap, depth, mask_image, s, lo, hi)
    return vnmap


def icp_step(depth_obs, vn_obs, vn_model, model_viewmatrix, viewmatrix_in, fx, fy, cx, cy, *, viewmatrix_out=None, stride=1,
             depth_range=(0.0, INF), dist_max=0.1, normal_cos_min=0.8, huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6,
             return_flags=False, scratch=None):
    """One Gauss-Newton iteration (include/dgr_hip.h: dgr_icp_step) on maps the caller made with `depth_normals`: `vn_obs`
    [H,W,4] or None, `vn_model` [H,W,4].  Returns IcpResult with `stats` [1, 32]; `viewmatrix_out` (a contiguous float32 [4,4]
    GPU tensor, which may be `viewmatrix_in`) receives the pose when given.  `scratch`: a zero-filled uint8 tensor of
    dgr_icp_scratch_bytes to reuse; None allocates one."""
    what = "icp_step"
    depth_obs = _image(what, "depth_obs", depth_obs)
    H, W = depth_obs.shape
    maps = [("vn_model", vn_model)] + ([("vn_obs", vn_obs)] if vn_obs is not None else [])
    for n, t in maps:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (H, W, 4) or not t.is_contiguous():
            raise ValueError(f"{what}: {n} must be a contiguous float32 tensor [H,W,4] = {(H, W, 4)}")
    model_viewmatrix, viewmatrix_in = _pose(what, "model_viewmatrix", model_viewmatrix), _pose(what, "viewmatrix_in", viewmatrix_in)
    s, lo, hi, stride, min_points = _step_arguments(what, fx, fy, cx, cy, depth_range, dist_max, normal_cos_min, huber_delta,
                                                    damping, rcond, min_points, [stride])
    _check_gpu(what, depth_obs, model_viewmatrix, viewmatrix_in, *(t for _, t in maps))
    dev = depth_obs.device
    depth_obs, model_viewmatrix, viewmatrix_in = depth_obs.detach().contiguous(), model_viewmatrix.contiguous(), viewmatrix_in.contiguous()
    S = -(-W // stride[0]) * -(-H // stride[0])
    chain = _Chain(torch, what, dev, 1, 32, out=viewmatrix_out, out_name="viewmatrix_out", flags=S if return_flags else None)
    if scratch is None:
        scratch = _step_scratch(torch, what, "dgr_icp_scratch_bytes", W, H, stride, dev)
    params = _params(s, lo, hi, min_points, stride[0])
    _capi.call("dgr_icp_step", dev, W, H, depth_obs.data_ptr(), _capi.ptr(vn_obs), vn_model.data_ptr(), model_viewmatrix.data_ptr(),
               viewmatrix_in.data_ptr(), params, scratch.data_ptr(), *chain.tail(0))
    return chain.result(IcpResult)


def _step_arguments(what, fx, fy, cx, cy, depth_range, dist_max, normal_cos_min, huber_delta, damping, rcond, min_points, strides):
    s = _scalars(what, fx, fy, cx=(cx, None), cy=(cy, None), dist_max=(dist_max, 0.0), normal_cos_min=(normal_cos_min, -1.0),
                 huber_delta=(huber_delta, 0.0), damping=(damping, 0.0), rcond=(rcond, 0.0))
    if s["normal_cos_min"] > 1.0:
        raise ValueError(f"{what}: normal_cos_min must lie in [-1, 1], not {s['normal_cos_min']}")
    lo, hi = _depth_range(what, depth_range)
    strides = [int(x) for x in strides]
    if any(x < 1 for x in strides):
        raise ValueError(f"{what}: stride must be positive, not {min(strides)}")
    min_points = int(min_points)
    if min_points < 1:
        raise ValueError(f"{what}: min_points must be at least 1, not {min_points}")
    return s, lo, hi, strides, min_points


def _params(s, lo, hi, min_points, stride):
    return _capi.IcpParams(s["fx"], s["fy"], s["cx"], s["cy"], lo, hi, s["dist_max"], s["normal_cos_min"], s["huber_delta"],
                           s["damping"], s["rcond"], min_points, stride)


def icp_align(depth_obs, model_depth, viewmatrix, model_viewmatrix, fx, fy, cx, cy, *, iterations=10, strides=None,
              opacity_map=None, silhouette_threshold=0.99, depth_range=(0.0, INF), max_jump=0.1, dist_max=0.1, normal_cos_min=0.8,
              use_obs_normals=True, huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6, return_flags=False):
    """Frame-to-model ICP: the pose of the frame that measured `depth_obs`, from the model's depth `model_depth` rendered at
    `model_viewmatrix` and a first estimate `viewmatrix` (None: `model_viewmatrix`, the usual "render at the predicted pose, then
    align").  KinectFusion's projective point-to-plane ICP, as RTG-SLAM and GS-ICP SLAM run it on a Gaussian map in front of the
    photometric refinement: every candidate pixel of `depth_obs` is taken into the model's camera by the current estimate,
    associated with the model pixel it lands on (closer than `dist_max`, normals within `normal_cos_min` when
    `use_obs_normals`), and the point-to-plane residuals give one 6 x 6 Gauss-Newton step per iteration (`huber_delta`: robust
    weights; `damping`: Levenberg-Marquardt; a step is refused -- the pose kept -- with fewer than `min_points` pairs or a pivot
    below `rcond` of the largest diagonal entry).  `strides`: None = every pixel in every iteration, or one stride per iteration,
    coarse to fine (e.g. `(4,) * 4 + (2,) * 3 + (1,) * 3`); the maps stay full resolution, only the candidate grid thins.
    `opacity_map` with `silhouette_threshold` masks the model's map to the well-observed pixels; `depth_range` (exclusive) and
    `max_jump` bound the depths and depth steps either map uses (`depth_normals`).
    Launches: one normals launch for the model, one for the observation when `use_obs_normals`, then `iterations` steps chained
    through one device pose buffer: nothing is read on the host, the bits are the same on every run, and the whole call records
    into a hipGraph (include/dgr_hip.h: dgr_depth_normals, dgr_icp_step).  Images [H,W] or [1,H,W], poses [4,4] holding W2C^T,
    float32 GPU tensors.  Returns IcpResult(viewmatrix, quat, trans, stats, flags); `flags` is None unless `return_flags`."""
    what = "icp_align"
    depth_obs = _image(what, "depth_obs", depth_obs)
    H, W = depth_obs.shape
    model_depth = _image(what, "model_depth", model_depth, (H, W))
    tensors = [depth_obs, model_depth]
    if opacity_map is not None:
        opacity_map = _image(what, "opacity_map", opacity_map, (H, W))
        tensors.append(opacity_map)
    model_viewmatrix = _pose(what, "model_viewmatrix", model_viewmatrix)
    viewmatrix = model_viewmatrix if viewmatrix is None else _pose(what, "viewmatrix", viewmatrix)
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError(f"{what}: iterations must be at least 1, not {iterations}")
    if strides is None:
        strides = (1,) * iterations
    strides = tuple(strides)
    if len(strides) != iterations:
        raise ValueError(f"{what}: strides must hold one stride per iteration ({iterations}), not {len(strides)}")
    s, lo, hi, strides, min_points = _step_arguments(what, fx, fy, cx, cy, depth_range, dist_max, normal_cos_min, huber_delta,
                                                     damping, rcond, min_points, strides)
    s.update(_scalars(what, fx, fy, max_jump=(max_jump, 0.0), mask_threshold=(silhouette_threshold, None)))
    _check_gpu(what, *tensors, model_viewmatrix, viewmatrix)
    dev = depth_obs.device
    depth_obs, model_depth = depth_obs.detach().contiguous(), model_depth.detach().contiguous()
    if opacity_map is not None:
        opacity_map = opacity_map.detach().contiguous()
    model_viewmatrix = model_viewmatrix.detach().contiguous()
    maps = torch.empty((2 if use_obs_normals else 1, H, W, 4), dtype=torch.float32, device=dev)
    S = -(-W // strides[-1]) * -(-H // strides[-1])
    chain = _Chain(torch, what, dev, iterations, 32, first=viewmatrix, flags=S if return_flags else None)
    scratch = _step_scratch(torch, what, "dgr_icp_scratch_bytes", W, H, strides, dev)
    with _capi.StepCalls(dev) as abi:
        _normals_into(abi, maps[0], model_depth, opacity_map, s, lo, hi)
        if use_obs_normals:
            _normals_into(abi, maps[1], depth_obs, None, s, lo, hi)
        for k, stride in enumerate(strides):
            abi.call("dgr_icp_step", W, H, depth_obs.data_ptr(), maps[1].data_ptr() if use_obs_normals else None,
                     maps[0].data_ptr(), model_viewmatrix.data_ptr(), chain.pose.data_ptr(), _params(s, lo, hi, min_points, stride),
                     scratch.data_ptr(), *chain.tail(k))
    return chain.result(IcpResult)
