"""Hybrid RGB-D pose alignment on the device (C ABI: dgr_intensity_map, dgr_frame_halve, dgr_rgbd_step): the packed
intensity-gradient map of an image, one pyramid level of a frame, one fused Gauss-Newton iteration of point-to-plane ICP with a
photometric term beside it, and `rgbd_align`, the coarse-to-fine chain of iterations that initialises the photometric tracker's
pose where the geometry alone cannot: on planar scenes and on maps too unstructured to find pairs."""
from typing import NamedTuple as _NamedTuple

import torch

from . import _capi
from ._align import INF, _Chain, _pose, _scalars, _step_scratch
from .icp import _depth_range, _image, _normals_into, _step_arguments
from .losses import _check_gpu


class RgbdResult(_NamedTuple):
    """What `rgbd_align` leaves on the device: `viewmatrix` float32 [4,4] (W2C^T) with `quat` [4] (r, x, y, z; unit, r >= 0) and
    `trans` [3] of the same pose; `stats` float64 [iterations, 40] per iteration in the order they ran (coarsest level first):
    A (21, the upper triangle row-major), b (6), sum w r^2 [27], count_g [28], sum w_p r_p^2 [29], count_p [30], ok [31],
    |omega| [32], |v| [33], zeros; `flags` uint8 [S] of the LAST iteration's candidates (bit 0 valid, bit 1 inside, bit 2
    associated, bit 3 photometric) or None."""
    viewmatrix: torch.Tensor
    quat: torch.Tensor
    trans: torch.Tensor
    stats: torch.Tensor
    flags: torch.Tensor


def _color(what, name, t, shape=None):
    """a float32 [C,H,W] (C = 1 or 3) or [H,W] image tensor as [C,H,W]"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, not {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, not {t.dtype}")
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[0] not in (1, 3) or t.numel() == 0:
        raise ValueError(f"{what}: {name} is [C,H,W] with C = 1 or 3, or [H,W], not {tuple(t.shape)}")
    if shape is not None and tuple(t.shape[1:]) != tuple(shape):
        raise ValueError(f"{what}: {name} {tuple(t.shape)} is not [C,H,W] with [H,W] = {tuple(shape)}")
    return t


def _intensity_into(abi, image, mask_image, mask_threshold, imap, intensity):
    C_, H, W = image.shape
    abi.call("dgr_intensity_map", W, H, C_, image.data_ptr(), _capi.ptr(mask_image), mask_threshold, _capi.ptr(imap),
             _capi.ptr(intensity))


def intensity_map(image, *, mask_image=None, mask_threshold=0.99):
    """The packed intensity-gradient map of an image: `imap` float32 [H,W,4] = (I, I_x, I_y, u), one launch.  I = 0.299 R +
    0.587 G + 0.114 B (or the single channel), I_x and I_y the 3 x 3 Sobel responses divided by 8, u = 1 where the pixel is
    interior, its nine intensities are finite and -- with `mask_image`, e.g. the rasterizer's `opacity_map` -- all nine mask values
    exceed `mask_threshold`; every other pixel is four zeros.  `image`: [C,H,W] (C = 1 or 3) or [H,W], `mask_image`: [H,W] or
    [1,H,W], float32 GPU tensors.  What `rgbd_align` gathers from (one 16-byte load per pixel)."""
    what = "intensity_map"
    image = _color(what, "image", image)
    tensors = [image]
    if mask_image is not None:
        mask_image = _image(what, "mask_image", mask_image, image.shape[1:])
        tensors.append(mask_image)
    mask_threshold = float(mask_threshold)
    if mask_threshold != mask_threshold:
        raise ValueError(f"{what}: mask_threshold must not be NaN")
    _check_gpu(what, *tensors)
    image = image.detach().contiguous()
    if mask_image is not None:
        mask_image = mask_image.detach().contiguous()
    imap = torch.empty((image.shape[1], image.shape[2], 4), dtype=torch.float32, device=image.device)
    with _capi.StepCalls(image.device) as abi:
        _intensity_into(abi, image, mask_image, mask_threshold, imap, None)
    return imap


def _halve_into(abi, planes, depth, lo, hi, max_jump, planes_out, depth_out):
    H, W = (planes if planes is not None else depth).shape[-2:]
    abi.call("dgr_frame_halve", W, H, 0 if planes is None else planes.shape[0], _capi.ptr(planes), _capi.ptr(depth), lo, hi, max_jump,
             _capi.ptr(planes_out), _capi.ptr(depth_out))


def level_intrinsics(fx, fy, cx, cy, level=1):
    """The intrinsics of pyramid level `level` (each level halves the one below): pixel centres sit at integers, so the centre of
    an output pixel lies half an input pixel beyond twice its index: fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2 per level."""
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    for _ in range(int(level)):
        fx, fy, cx, cy = 0.5 * fx, 0.5 * fy, 0.5 * (cx - 0.5), 0.5 * (cy - 0.5)
    return fx, fy, cx, cy


def halve_frame(planes=None, depth=None, *, depth_range=(0.0, INF), max_jump=0.1):
    """One pyramid level, one launch: `planes` [N,H,W] (intensities, a silhouette) -> [N,H//2,W//2], each value the mean of its
    2 x 2 block; `depth` [H,W] -> [H//2,W//2], the mean of the block's depths inside `depth_range` (exclusive) where there is one
    and the largest exceeds the smallest by at most `max_jump` times the smallest, else 0.  An odd last row or column is dropped.
    Returns (planes_out or None, depth_out or None).  The level's intrinsics: `level_intrinsics`."""
    what = "halve_frame"
    if planes is None and depth is None:
        raise ValueError(f"{what}: nothing to halve: planes and depth are both None")
    tensors = []
    shape = None
    if planes is not None:
        if not isinstance(planes, torch.Tensor) or planes.dtype != torch.float32 or planes.dim() != 3 or planes.numel() == 0:
            raise ValueError(f"{what}: planes must be a float32 tensor [N,H,W]")
        if planes.shape[0] > 64:
            raise ValueError(f"{what}: at most 64 planes, not {planes.shape[0]}")
        shape = tuple(planes.shape[1:])
        tensors.append(planes)
    if depth is not None:
        depth = _image(what, "depth", depth, shape)
        shape = tuple(depth.shape)
        tensors.append(depth)
    if min(shape) < 2:
        raise ValueError(f"{what}: a frame of {shape[1]} x {shape[0]} cannot be halved")
    lo, hi = _depth_range(what, depth_range)
    max_jump = float(max_jump)
    if not max_jump >= 0.0:
        raise ValueError(f"{what}: max_jump must not be NaN or negative, not {max_jump}")
    _check_gpu(what, *tensors)
    dev = tensors[0].device
    H2, W2 = shape[0] // 2, shape[1] // 2
    planes_out = depth_out = None
    if planes is not None:
        planes = planes.detach().contiguous()
        planes_out = torch.empty((planes.shape[0], H2, W2), dtype=torch.float32, device=dev)
    if depth is not None:
        depth = depth.detach().contiguous()
        depth_out = torch.empty((H2, W2), dtype=torch.float32, device=dev)
    with _capi.StepCalls(dev) as abi:
        _halve_into(abi, planes, depth, lo, hi, max_jump, planes_out, depth_out)
    return planes_out, depth_out


def _photo_arguments(what, geo_weight, photo_weight, photo_max, photo_huber):
    named = dict(geo_weight=float(geo_weight), photo_weight=float(photo_weight), photo_max=float(photo_max),
                 photo_huber=float(photo_huber))
    for n, v in named.items():
        if v != v:
            raise ValueError(f"{what}: {n} must not be NaN")
        if v < 0.0:
            raise ValueError(f"{what}: {n} must not be negative, not {v}")
    return named


def _params(s, lo, hi, min_points, stride, ph, intr=None):
    fx, fy, cx, cy = intr if intr is not None else (s["fx"], s["fy"], s["cx"], s["cy"])
    return _capi.RgbdParams(fx, fy, cx, cy, lo, hi, s["dist_max"], s["normal_cos_min"], s["huber_delta"], s["damping"], s["rcond"],
                            min_points, stride, ph["geo_weight"], ph["photo_weight"], ph["photo_max"], ph["photo_huber"])


def rgbd_step(depth_obs, vn_obs, vn_model, intensity_obs, imap_model, model_viewmatrix, viewmatrix_in, fx, fy, cx, cy, *,
              viewmatrix_out=None, stride=1, depth_range=(0.0, INF), dist_max=0.1, normal_cos_min=0.8, huber_delta=INF,
              geo_weight=1.0, photo_weight=1.0, photo_max=INF, photo_huber=INF, damping=0.0, rcond=1e-8, min_points=6,
              return_flags=False, scratch=None):
    """One hybrid Gauss-Newton iteration (include/dgr_hip.h: dgr_rgbd_step) on maps the caller made: `vn_obs` [H,W,4] or None and
    `vn_model` [H,W,4] (`depth_normals`), `intensity_obs` [H,W], `imap_model` [H,W,4] (`intensity_map`).  Returns RgbdResult with
    `stats` [1, 40]; `viewmatrix_out` (a contiguous float32 [4,4] GPU tensor, which may be `viewmatrix_in`) receives the pose when
    given.  `scratch`: a zero-filled uint8 tensor of dgr_rgbd_scratch_bytes to reuse; None allocates one."""
    what = "rgbd_step"
    depth_obs = _image(what, "depth_obs", depth_obs)
    H, W = depth_obs.shape
    intensity_obs = _image(what, "intensity_obs", intensity_obs, (H, W))
    maps = [("vn_model", vn_model), ("imap_model", imap_model)] + ([("vn_obs", vn_obs)] if vn_obs is not None else [])
    for n, t in maps:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (H, W, 4) or not t.is_contiguous():
            raise ValueError(f"{what}: {n} must be a contiguous float32 tensor [H,W,4] = {(H, W, 4)}")
    model_viewmatrix, viewmatrix_in = _pose(what, "model_viewmatrix", model_viewmatrix), _pose(what, "viewmatrix_in", viewmatrix_in)
    s, lo, hi, stride, min_points = _step_arguments(what, fx, fy, cx, cy, depth_range, dist_max, normal_cos_min, huber_delta,
                                                    damping, rcond, min_points, [stride])
    ph = _photo_arguments(what, geo_weight, photo_weight, photo_max, photo_huber)
    _check_gpu(what, depth_obs, intensity_obs, model_viewmatrix, viewmatrix_in, *(t for _, t in maps))
    dev = depth_obs.device
    depth_obs, intensity_obs = depth_obs.detach().contiguous(), intensity_obs.detach().contiguous()
    model_viewmatrix, viewmatrix_in = model_viewmatrix.contiguous(), viewmatrix_in.contiguous()
    S = -(-W // stride[0]) * -(-H // stride[0])
    chain = _Chain(torch, what, dev, 1, 40, out=viewmatrix_out, out_name="viewmatrix_out", flags=S if return_flags else None)
    if scratch is None:
        scratch = _step_scratch(torch, what, "dgr_rgbd_scratch_bytes", W, H, stride, dev)
    _capi.call("dgr_rgbd_step", dev, W, H, depth_obs.data_ptr(), _capi.ptr(vn_obs), vn_model.data_ptr(), intensity_obs.data_ptr(),
               imap_model.data_ptr(), model_viewmatrix.data_ptr(), viewmatrix_in.data_ptr(), _params(s, lo, hi, min_points, stride[0], ph),
               scratch.data_ptr(), *chain.tail(0))
    return chain.result(RgbdResult)


def _level_plan(what, W, H, levels, iterations, strides):
    """[(level, stride)] in the order the iterations run: the coarsest level first"""
    levels = int(levels)
    if levels < 1:
        raise ValueError(f"{what}: levels must be at least 1, not {levels}")
    if min(W, H) >> (levels - 1) < 3:
        raise ValueError(f"{what}: {levels} levels leave a {W} x {H} frame without an interior pixel (3 x 3 at least)")
    per_level = (int(iterations),) * levels if isinstance(iterations, int) else tuple(int(k) for k in iterations)
    if len(per_level) != levels:
        raise ValueError(f"{what}: iterations must be one number or one per level ({levels}, coarsest first), not {len(per_level)}")
    if any(k < 1 for k in per_level):
        raise ValueError(f"{what}: iterations must be at least 1, not {min(per_level)}")
    total = sum(per_level)
    strides = (1,) * total if strides is None else tuple(strides)
    if len(strides) != total:
        raise ValueError(f"{what}: strides must hold one stride per iteration ({total}), not {len(strides)}")
    order = [level for level, k in zip(range(levels - 1, -1, -1), per_level) for _ in range(k)]
    return levels, order, strides


def rgbd_align(color_obs, depth_obs, model_color, model_depth, viewmatrix, model_viewmatrix, fx, fy, cx, cy, *, levels=1,
               iterations=10, strides=None, opacity_map=None, silhouette_threshold=0.99, geo_weight=1.0, photo_weight=1.0,
               photo_max=INF, photo_huber=INF, depth_range=(0.0, INF), max_jump=0.1, dist_max=0.1, normal_cos_min=0.8,
               use_obs_normals=True, huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6, return_flags=False):
    """Frame-to-model hybrid RGB-D alignment: `icp_align` with a photometric term beside the point-to-plane one.  The pose of the
    frame that measured `color_obs`, `depth_obs`, from the model's colour and depth `model_color`, `model_depth` rendered at
    `model_viewmatrix` and a first estimate `viewmatrix` (None: `model_viewmatrix`).  What Kerl's DVO, Open3D's hybrid odometry
    and the front ends of Gaussian-SLAM and LoopSplat run: per candidate pixel the geometric residual n_m . (q - v_m) of
    `icp_align` and the intensity residual I_model(landing position) - I_obs, the second with the class weight `photo_weight`
    (intensity^-2 against `geo_weight`'s metres^-2), its own bound `photo_max` on |r_p| and Huber threshold `photo_huber`, summed
    into one 6 x 6 Gauss-Newton step per iteration.  The photometric rows constrain what a plane leaves free (rotation about its
    normal, translation in it); `geo_weight=0` is a purely photometric step, `photo_weight=0` is `icp_align` bit for bit.
    `levels`: the pyramid's depth; level l halves level l - 1 (`halve_frame`, `level_intrinsics`); the coarsest level runs first
    and widens the basin of convergence to 2^(levels - 1) pixels of image motion.  `iterations`: per level, or one number per
    level coarsest first; `strides`: None or one per iteration in the order they run.  `opacity_map` with `silhouette_threshold`
    masks both of the model's maps.  Every other keyword is `icp_align`'s.
    Launches: per level two halvings (above level 0), the intensity map, one or two normal maps, then its iterations, all chained
    through one device pose buffer inside one block of calls: nothing is read on the host, the bits are the same on every run,
    and the whole call records into a hipGraph.  Colours [C,H,W] (C = 1 or 3) or [H,W], depths [H,W] or [1,H,W], poses [4,4]
    holding W2C^T, float32 GPU tensors.  Returns RgbdResult(viewmatrix, quat, trans, stats, flags)."""
    what = "rgbd_align"
    depth_obs = _image(what, "depth_obs", depth_obs)
    H, W = depth_obs.shape
    model_depth = _image(what, "model_depth", model_depth, (H, W))
    color_obs, model_color = _color(what, "color_obs", color_obs, (H, W)), _color(what, "model_color", model_color, (H, W))
    tensors = [color_obs, depth_obs, model_color, model_depth]
    if opacity_map is not None:
        opacity_map = _image(what, "opacity_map", opacity_map, (H, W))
        tensors.append(opacity_map)
    model_viewmatrix = _pose(what, "model_viewmatrix", model_viewmatrix)
    viewmatrix = model_viewmatrix if viewmatrix is None else _pose(what, "viewmatrix", viewmatrix)
    levels, order, strides = _level_plan(what, W, H, levels, iterations, strides)
    s, lo, hi, strides, min_points = _step_arguments(what, fx, fy, cx, cy, depth_range, dist_max, normal_cos_min, huber_delta,
                                                     damping, rcond, min_points, strides)
    s.update(_scalars(what, fx, fy, max_jump=(max_jump, 0.0), mask_threshold=(silhouette_threshold, None)))
    ph = _photo_arguments(what, geo_weight, photo_weight, photo_max, photo_huber)
    _check_gpu(what, *tensors, model_viewmatrix, viewmatrix)
    dev = depth_obs.device
    color_obs, model_color = color_obs.detach().contiguous(), model_color.detach().contiguous()
    depth_obs, model_depth = depth_obs.detach().contiguous(), model_depth.detach().contiguous()
    if opacity_map is not None:
        opacity_map = opacity_map.detach().contiguous()
    model_viewmatrix = model_viewmatrix.detach().contiguous()
    # one arena for every level's images: per level 3 mean planes (I_obs, I_model, the silhouette), 2 depths, 3 packed maps
    sizes = [(H >> level, W >> level) for level in range(levels)]
    arena = torch.empty((sum(-(-17 * h * w // 4) * 4 for h, w in sizes),), dtype=torch.float32, device=dev)
    S = -(-W // strides[-1]) * -(-H // strides[-1])
    chain = _Chain(torch, what, dev, len(order), 40, first=viewmatrix, flags=S if return_flags else None)
    scratch = _step_scratch(torch, what, "dgr_rgbd_scratch_bytes", W, H, [1], dev)  # (the finest level at stride 1: the largest grid any iteration has)
    frames, at = [], 0
    for h, w in sizes:
        n = h * w
        # (the packed maps first: each starts at a multiple of 16 bytes)
        f = dict(maps=arena[at:at + 12 * n].view(3, h, w, 4), obs=arena[at + 12 * n:at + 13 * n].view(1, h, w),
                 model=arena[at + 13 * n:at + 15 * n].view(2, h, w), depth_obs=arena[at + 15 * n:at + 16 * n].view(h, w),
                 depth_model=arena[at + 16 * n:at + 17 * n].view(h, w))
        frames.append(f)
        at += -(-17 * n // 4) * 4
    with _capi.StepCalls(dev) as abi:
        # level 0: the intensities of both colours as planes; the given depths and silhouette are used where they are
        top = frames[0]
        _intensity_into(abi, color_obs, None, 0.0, None, top["obs"])
        _intensity_into(abi, model_color, opacity_map, s["mask_threshold"], top["maps"][2], top["model"][0])
        top["depth_obs"], top["depth_model"], mask = depth_obs, model_depth, opacity_map
        masks = [mask]
        for level in range(1, levels):
            below, f = frames[level - 1], frames[level]
            _halve_into(abi, below["obs"], below["depth_obs"], lo, hi, s["max_jump"], f["obs"], f["depth_obs"])
            if mask is not None and level == 1:
                below["model"][1].copy_(mask)  # (beside the model's intensity: one launch halves both)
            planes = below["model"] if mask is not None else below["model"][:1]
            _halve_into(abi, planes, below["depth_model"], lo, hi, s["max_jump"], f["model"], f["depth_model"])
            masks.append(f["model"][1] if mask is not None else None)
            _intensity_into(abi, f["model"][:1], masks[level], s["mask_threshold"], f["maps"][2], None)
        k = 0
        for level in range(levels - 1, -1, -1):
            f = frames[level]
            h, w = sizes[level]
            intr = level_intrinsics(s["fx"], s["fy"], s["cx"], s["cy"], level)
            sl = dict(s, fx=intr[0], fy=intr[1], cx=intr[2], cy=intr[3])
            _normals_into(abi, f["maps"][0], f["depth_model"], masks[level], sl, lo, hi)
            if use_obs_normals:
                _normals_into(abi, f["maps"][1], f["depth_obs"], None, sl, lo, hi)
            while k < len(order) and order[k] == level:
                abi.call("dgr_rgbd_step", w, h, f["depth_obs"].data_ptr(), f["maps"][1].data_ptr() if use_obs_normals else None,
                         f["maps"][0].data_ptr(), f["obs"].data_ptr(), f["maps"][2].data_ptr(), model_viewmatrix.data_ptr(),
                         chain.pose.data_ptr(), _params(s, lo, hi, min_points, strides[k], ph, intr), scratch.data_ptr(),
                         *chain.tail(k))
                k += 1
    return chain.result(RgbdResult)
