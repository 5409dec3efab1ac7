"""The losses of a tracking or mapping step as fused HIP launches (C ABI: dgr_l1_loss_*, dgr_ssim_loss_*, dgr_masked_loss_*):
the plain L1 loss, SSIM and the L1 + D-SSIM mapping loss, and the masked L1 loss with the on-device median.  None of them adds a
float atomically: the same bits on every run, and capturable into a hipGraph."""
from typing import NamedTuple as _NamedTuple

import torch

from . import _capi


class _L1Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, depth, color_obs, depth_obs, w_color, w_depth):
        color, depth, color_obs, depth_obs = (x.contiguous() for x in (color, depth, color_obs, depth_obs))
        buf = torch.empty((_capi.load().dgr_l1_loss_scratch_floats() + 1,), dtype=torch.float32, device=color.device)
        _capi.call("dgr_l1_loss_forward", color.device, color.numel(), color.data_ptr(), color_obs.data_ptr(), depth.numel(),
                   depth.data_ptr(), depth_obs.data_ptr(), float(w_color), float(w_depth), buf[1:].data_ptr(), buf.data_ptr())
        ctx.save_for_backward(color, depth, color_obs, depth_obs)
        ctx.weights = (float(w_color), float(w_depth))
        return buf[0]

    @staticmethod
    def backward(ctx, upstream):
        color, depth, color_obs, depth_obs = ctx.saved_tensors
        dc, dd = torch.empty_like(color), torch.empty_like(depth)
        upstream = upstream.contiguous()
        _capi.call("dgr_l1_loss_backward", color.device, color.numel(), color.data_ptr(), color_obs.data_ptr(), depth.numel(),
                   depth.data_ptr(), depth_obs.data_ptr(), ctx.weights[0], ctx.weights[1], upstream.data_ptr(), dc.data_ptr(),
                   dd.data_ptr())
        return dc, dd, None, None, None, None


def l1_loss(color, depth, color_obs, depth_obs, w_color=1.0, w_depth=0.5):
    """w_color * mean|color - color_obs| + w_depth * mean|depth - depth_obs| as one fused reduction, with both gradient
    images written by one launch in the backward (float32 GPU tensors, each image of its observation's shape; the observations
    carry no gradient)."""
    _check_pair("color", color, color_obs, "l1_loss")
    _check_pair("depth", depth, depth_obs, "l1_loss")
    _check_gpu("l1_loss", color, color_obs, depth, depth_obs)
    return _L1Loss.apply(color, depth, color_obs, depth_obs, w_color, w_depth)


def _check_pair(name, a, b, what):
    """ValueError unless `a`, `b` are float32 tensors of one shape (with _check_gpu: all on the host, before any device call)."""
    for t, n in ((a, name), (b, name + "_obs")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {n} must be a tensor, not {type(t).__name__}")
    if a.shape != b.shape:
        raise ValueError(f"{what}: {name} {tuple(a.shape)} and {name}_obs {tuple(b.shape)} differ in shape")
    for t, n in ((a, name), (b, name + "_obs")):
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {n} must be float32, not {t.dtype}")


def _check_gpu(what, *tensors):
    if any(not t.is_cuda for t in tensors):
        raise ValueError(f"{what}: the images must be GPU tensors (there is no CPU fallback)")
    if any(t.device != tensors[0].device for t in tensors):
        raise ValueError(f"{what}: the images are on different devices")


def _image_stack(img, what):
    """(V, C, H, W) of a [C,H,W] or [V,C,H,W] image tensor the SSIM kernels can read."""
    if img.dim() not in (3, 4):
        raise ValueError(f"{what}: images are [C,H,W] or [V,C,H,W], not {tuple(img.shape)}")
    V, (C, H, W) = (img.shape[0] if img.dim() == 4 else 1), img.shape[-3:]
    if min(V, C, H, W) < 1 or V * C > 65535:
        raise ValueError(f"{what}: cannot read a stack of shape {tuple(img.shape)} (empty, or more than 65535 image planes)")
    return V, C, H, W


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class _SsimLoss(torch.autograd.Function):
    """w_l1 mean|img - ref| + w_ssim (1 - SSIM(img, ref)) + w_depth mean|depth - depth_obs| (C ABI: dgr_ssim_loss_forward /
    _backward; csrc/ssim.hip).  `depth` / `depth_obs` may be None.  `want_ssim`: return the mean SSIM the forward leaves in its
    scratch header instead of the loss (with weights (0, -1, 0) the loss is SSIM - 1, whose gradient is SSIM's).  `want_maps`:
    whether a backward will follow (the forward then writes the three derivative maps it needs)."""

    @staticmethod
    def forward(ctx, img, depth, ref, depth_obs, shape, w_l1, w_ssim, w_depth, want_maps, want_ssim):
        img, ref = img.contiguous(), ref.contiguous()
        if depth is not None:
            depth, depth_obs = depth.contiguous(), depth_obs.contiguous()
        n_depth = depth.numel() if depth is not None else 0
        floats = _capi.load().dgr_ssim_scratch_floats(*shape)
        if not want_maps:  # the inference form: the scratch ends where the derivative maps would begin
            floats -= 3 * img.numel()
        buf = torch.empty((floats + 4,), dtype=torch.float32, device=img.device)
        weights = (float(w_l1), float(w_ssim), float(w_depth))
        _capi.call("dgr_ssim_loss_forward", img.device, *shape, img.data_ptr(), ref.data_ptr(), n_depth, _capi.ptr(depth),
                   _capi.ptr(depth_obs), *weights, buf.data_ptr(), int(want_maps), buf[floats:].data_ptr())
        ctx.save_for_backward(img, ref, depth, depth_obs, buf)
        ctx.call = (shape, n_depth, weights)
        return buf[0] if want_ssim else buf[floats]

    @staticmethod
    def backward(ctx, upstream):
        img, ref, depth, depth_obs, buf = ctx.saved_tensors
        shape, n_depth, weights = ctx.call
        dimg = torch.empty_like(img)
        ddepth = torch.empty_like(depth) if n_depth else None
        upstream = upstream.contiguous()
        _capi.call("dgr_ssim_loss_backward", img.device, *shape, img.data_ptr(), ref.data_ptr(), n_depth, _capi.ptr(depth),
                   _capi.ptr(depth_obs), *weights, buf.data_ptr(), upstream.data_ptr(), dimg.data_ptr(), _capi.ptr(ddepth))
        return dimg, ddepth, None, None, None, None, None, None, None, None


def ssim(img, ref):
    """Mean SSIM of `img` against `ref` as 3DGS's `ssim(img1, img2, window_size=11, size_average=True)` computes it (11 x 11
    Gaussian window of sigma 1.5 over the zero-padded images, per channel and per image), as a scalar differentiable with respect
    to `img`: one tiled kernel each way instead of five depthwise convolutions and their elementwise trail.  float32 GPU tensors
    [C,H,W] or [V,C,H,W] of one shape; `ref` carries no gradient."""
    _check_pair("img", img, ref, "ssim")
    shape = _image_stack(img, "ssim")
    _check_gpu("ssim", img, ref)
    return _SsimLoss.apply(img, None, ref, None, shape, 0.0, -1.0, 0.0, _wants_grad(img), True)


def l1_ssim_loss(color, depth, color_obs, depth_obs, w_color=1.0, w_depth=0.5, lambda_dssim=0.2):
    """The mapping loss of 3DGS and the SLAM systems built on it,
        w_color * ((1 - lambda) * mean|color - color_obs| + lambda * (1 - SSIM(color, color_obs))) + w_depth * mean|depth - depth_obs|,
    in at most three launches, with both gradient images written by at most two in the backward, none of them with atomics: the
    same bits on every run, and capturable into a hipGraph.  `color` is [C,H,W] or a stack [V,C,H,W] (then the loss is the mean over
    the stack: multiply the weights by V for a sum over keyframes); `depth` and `depth_obs` may both be None.  float32 GPU tensors;
    the observations carry no gradient.  When no input requires a gradient the forward skips the derivative maps."""
    _check_pair("color", color, color_obs, "l1_ssim_loss")
    shape = _image_stack(color, "l1_ssim_loss")
    if (depth is None) != (depth_obs is None):
        raise ValueError("l1_ssim_loss: depth and depth_obs are given together or both None")
    if depth is not None:
        _check_pair("depth", depth, depth_obs, "l1_ssim_loss")
    _check_gpu("l1_ssim_loss", *(t for t in (color, color_obs, depth, depth_obs) if t is not None))
    if depth is not None and depth.numel() == 0:
        depth = depth_obs = None
    lam = float(lambda_dssim)
    return _SsimLoss.apply(color, depth, color_obs, depth_obs, shape, float(w_color) * (1.0 - lam), float(w_color) * lam,
                           float(w_depth) if depth is not None else 0.0, _wants_grad(color, depth), False)


class MaskedLossStats(_NamedTuple):
    """What `masked_l1_loss(..., return_stats=True)` leaves on the device (views into the call's scratch, nothing read on the host):
    `mask` bool [V,H,W] -- the kept set K; `median` float32 [V] -- the lower median of |depth - depth_obs| over each view's base
    set (0 for an empty one, NaN when rejection is off); `base`, `kept` int32 [V] -- |B_v| and |K_v|.  `median[v:v + 1] * 50` is a
    valid device-tensor `depth_error_min` for `optim.seed_from_frame`."""
    mask: torch.Tensor
    median: torch.Tensor
    base: torch.Tensor
    kept: torch.Tensor


def _round16(n):
    return (n + 15) & ~15


class _MaskedL1Loss(torch.autograd.Function):
    """C ABI: dgr_masked_loss_forward / _backward (csrc/masked_loss.hip).  Returns (loss, scratch): the scratch (uint8, the layout
    include/dgr_hip.h documents) holds the statistics and the mask bytes the backward reads."""

    @staticmethod
    def forward(ctx, color, depth, color_obs, depth_obs, opacity_map, mask, shape, params):
        color, depth, color_obs, depth_obs = (x.contiguous() for x in (color, depth, color_obs, depth_obs))
        if opacity_map is not None:
            opacity_map = opacity_map.detach().contiguous()
        if mask is not None:
            mask = mask.contiguous()
        V, C, H, W = shape
        scratch = torch.empty((_capi.load().dgr_masked_loss_scratch_bytes(V, H, W),), dtype=torch.uint8, device=color.device)
        loss = scratch[8:12].view(torch.float32)  # (a free word of the stats header)
        _capi.call("dgr_masked_loss_forward", color.device, V, C, H, W, color.data_ptr(), color_obs.data_ptr(), depth.data_ptr(),
                   depth_obs.data_ptr(), _capi.ptr(opacity_map), _capi.ptr(mask), params, scratch.data_ptr(), loss.data_ptr())
        ctx.save_for_backward(color, depth, color_obs, depth_obs, opacity_map, mask, scratch)
        ctx.call = (shape, params)
        ctx.mark_non_differentiable(scratch)
        return loss[0], scratch

    @staticmethod
    def backward(ctx, upstream, _dscratch):
        color, depth, color_obs, depth_obs, opacity_map, mask, scratch = ctx.saved_tensors
        (V, C, H, W), params = ctx.call
        dcolor = torch.empty_like(color) if ctx.needs_input_grad[0] else None
        ddepth = torch.empty_like(depth) if ctx.needs_input_grad[1] else None
        if dcolor is None and ddepth is None:
            return (None,) * 8
        upstream = upstream.contiguous()
        _capi.call("dgr_masked_loss_backward", color.device, V, C, H, W, color.data_ptr(), color_obs.data_ptr(), depth.data_ptr(),
                   depth_obs.data_ptr(), _capi.ptr(opacity_map), _capi.ptr(mask), params, scratch.data_ptr(), upstream.data_ptr(),
                   _capi.ptr(dcolor), _capi.ptr(ddepth))
        return dcolor, ddepth, None, None, None, None, None, None


def masked_l1_loss(color, depth, color_obs, depth_obs, opacity_map=None, mask=None, *, silhouette_threshold=0.99,
                   depth_range=(0.0, float("inf")), outlier_factor=10.0, mask_color=True, w_color=1.0, w_depth=0.5,
                   reduction="sum", return_stats=False):
    """The masked L1 loss of the RGB-D SLAM systems (SplaTAM's `get_loss`, CG-SLAM's tracking), fused: at most six launches
    forward, one backward, no host read, the same bits on every run, capturable into a hipGraph.  Per pixel of every view of the
    stack, in single fp32 operations:
        e = |depth - depth_obs|
        B = lo < depth_obs < hi  and  e finite  [and opacity_map > silhouette_threshold]  [and mask != 0]
        K = B and e <= outlier_factor * median_v         median_v: the exact lower median of e over B of view v (torch.median's,
                                                          by a radix select on the device; 0 for an empty B)
        loss = w_depth * sum_K e / N_d + w_color * sum |color - color_obs| / N_c
    The colour sum runs over the channels and over K, or over every pixel with `mask_color=False` (the mapping form).
    `reduction="sum"` (SplaTAM's): N_d = N_c = 1; `"mean"`: N_d = |K| over the whole stack, N_c = C |K| (or C H W V unmasked),
    the counts read on the device; a zero count gives a zero term.  `outlier_factor=None` turns the rejection off (K = B; no
    median is computed).  The comparison is `<=`: a perfectly fitted frame (median 0) keeps its pixels.  NaN in any image drops
    the pixel.  Gradients go to `color` and `depth` (sign(.) on their set, zero outside); the mask is piecewise constant, so
    `opacity_map`, the observations and the median receive none.
    `color`, `color_obs`: [V,C,H,W] or [C,H,W]; `depth`, `depth_obs`, `opacity_map`: [V,1,H,W], [1,H,W] or [H,W]; `mask`: uint8 or
    bool of the depth's pixel shape.  float32 GPU tensors.
    `return_stats=True`: returns (loss, MaskedLossStats(mask, median, base, kept)), device tensors; `stats.median * 50` (one view)
    is a valid device-tensor `depth_error_min` for `optim.seed_from_frame`."""
    what = "masked_l1_loss"
    _check_pair("color", color, color_obs, what)
    _check_pair("depth", depth, depth_obs, what)
    V, C, H, W = _image_stack(color, what)
    pixels = {(V, 1, H, W)} if color.dim() == 4 else {(1, H, W), (H, W)}
    if tuple(depth.shape) not in pixels:
        raise ValueError(f"{what}: depth {tuple(depth.shape)} does not match color {tuple(color.shape)} "
                         "([V,1,H,W] beside [V,C,H,W]; [1,H,W] or [H,W] beside [C,H,W])")
    if opacity_map is not None:
        if not isinstance(opacity_map, torch.Tensor) or opacity_map.dtype != torch.float32:
            raise ValueError(f"{what}: opacity_map must be a float32 tensor")
        if tuple(opacity_map.shape) not in pixels:
            raise ValueError(f"{what}: opacity_map {tuple(opacity_map.shape)} does not have the depth's shape {tuple(depth.shape)}")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"{what}: mask must be a uint8 or bool tensor")
        if tuple(mask.shape) not in pixels and tuple(mask.shape) != (V, H, W):
            raise ValueError(f"{what}: mask {tuple(mask.shape)} does not have the depth's pixel shape {tuple(depth.shape)}")
    if reduction not in ("sum", "mean"):
        raise ValueError(f"{what}: reduction must be 'sum' or 'mean', not {reduction!r}")
    lo, hi = (float(x) for x in depth_range)
    factor = 0.0 if outlier_factor is None else float(outlier_factor)
    if any(x != x for x in (lo, hi, float(silhouette_threshold), factor)) or factor < 0.0:
        raise ValueError(f"{what}: depth_range, silhouette_threshold and outlier_factor must not be NaN, outlier_factor not negative")
    _check_gpu(what, *(t for t in (color, color_obs, depth, depth_obs, opacity_map, mask) if t is not None))
    if _capi.load().dgr_masked_loss_scratch_bytes(V, H, W) == 0:
        raise ValueError(f"{what}: cannot read a stack of shape {tuple(color.shape)} (more than 2^30 pixels per view)")
    params = _capi.MaskedLossParams(lo, hi, float(silhouette_threshold), factor, int(outlier_factor is not None), int(bool(mask_color)),
                                    _capi.MASKED_LOSS_MEAN if reduction == "mean" else _capi.MASKED_LOSS_SUM, float(w_color),
                                    float(w_depth))
    if mask is not None and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    loss, scratch = _MaskedL1Loss.apply(color, depth, color_obs, depth_obs, opacity_map, mask, (V, C, H, W), params)
    if not return_stats:
        return loss
    pad, n = _round16(4 * V), V * H * W  # (the scratch layout of include/dgr_hip.h)
    end = scratch.numel() - _round16(n)
    return loss, MaskedLossStats(scratch[end:end + n].view(torch.bool).view(V, H, W),
                                 scratch[64:64 + 4 * V].view(torch.float32), scratch[64 + pad:64 + pad + 4 * V].view(torch.int32),
                                 scratch[64 + 2 * pad:64 + 2 * pad + 4 * V].view(torch.int32))
