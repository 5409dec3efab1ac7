"""Host-side mirror of diff-gaussian-rasterization-light/diff_gaussian_rasterization/__init__.py.

Same names, argument order, return arity and error behaviour as the reference module
(`GaussianRasterizationSettings`, `GaussianRasterizer`, `rasterize_gaussians`, `_RasterizeGaussians`),
with `_C.*` replaced by calls into the gfx950 C ABI (include/dgr_hip.h).  Differences, all invisible
to a caller of the autograd surface:
  * the per-pixel [H*W,4,4] pose-gradient buffer and its torch.sum (reference __init__.py:160-161)
    do not exist; the C ABI returns the reduced [4,4];
  * forward runs without a mid-pipeline host sync when a binning capacity is known from an earlier
    call of the same shape (one status read at the end instead); DGR_FORWARD_MODE=callback selects the
    strict mirror with allocation callbacks and the reference's blocking read;
  * the debug path's NameError (`deoth_var`, reference __init__.py:93) is not reproduced.
"""
import os
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _binning, _capi, _frontend
# The binning status policy and its state live in dgr_amd._binning; the names outside code reads are the same objects here
# (mutated in place there, never rebound).  The lazy depth is reached through lazy_depth() / set_lazy_depth() only.
from ._binning import (_capacity_cache, _capture_keepalive, _check, _check_oldest, _last_status, _pending_status,  # noqa: F401
                       _unsettled, check_async_errors, check_captured_status, lazy_depth, set_lazy_depth)
# What this module shares with dgr_amd.full and the batch surfaces lives in dgr_amd._frontend; the names outside code reads stay here.
from ._frontend import (LIGHT, SPAN_SEGMENTS, _EMPTY, _checked_inputs, _consume_post_backward_wait, _device_guarded,  # noqa: F401
                        _drop_post_backward_wait, _f32c, _forward_r, _set_post_backward_wait, check_means2D_abs,
                        set_complete_pose_gradient, set_silhouette_gradient, set_tight_culling)


def cpu_deep_copy_tuple(input_tuple):
    copied_tensors = [item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple]
    return tuple(copied_tensors)


def _grad_arena(P, M, f32):
    """dgr_amd._frontend._grad_arena, allocated through this module's `torch`."""
    return _frontend._grad_arena(P, M, f32, torch)


class _C:
    """Functions with the signatures of the reference's pybind11 module `_C` (L/ext.cpp:15-19).  Their device buffers are
    allocated through this module's `torch` and `_grad_arena`, read at call time."""

    @staticmethod
    def rasterize_gaussians(*args):
        # L/rasterize_points.cu:35-129.  The tuple's num_rendered is the count last read for the shape (a lazy forward's own
        # count is read one call late); the autograd Function takes its backward's R from rasterize_gaussians_r.
        return _CtypesC.rasterize_gaussians_r(*args)[1]

    @_device_guarded(1)
    def rasterize_gaussians_r(*args):
        """(R for the backward, the `rasterize_gaussians` tuple) of rasterize_gaussians' arguments.  R is the exact count of a
        strict forward and the capacity the binning buffer was carved with of a lazy one (dgr_amd._binning.record)."""
        R, rendered, _, out, geom, binning, img = _forward_r(LIGHT, torch, *args)
        color, depth, median, var, alpha, radii, unc, px = out
        return R, (rendered, color, depth, median, var, alpha, radii, geom, binning, img, unc, px)

    @_device_guarded(1)
    def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                     cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                     dL_dout_depth, dL_dout_median_depth, dL_dout_depth_var, gt_depth, sh, degree,
                                     campos, geomBuffer, R, binningBuffer, imageBuffer, alphas, debug,
                                     perspec_matrix, track_off, map_off, need_gaussian_grads=True, absgrad=False,
                                     silhouette=None):
        # L/rasterize_points.cu:131-236.  `need_gaussian_grads=False` (an extension: the autograd Function passes it when
        # no Gaussian input requires a gradient, i.e. tracking) returns None for the eight per-Gaussian gradients and lets
        # the library skip their dense rows; the pose gradient is the same.  `absgrad=True` (dgr_light_backward_absgrad)
        # appends a tenth result, the absolute screen-space gradient [P,3].  `silhouette` (dgr_light_backward_silhouette):
        # the opacity_map gradient [1,H,W], or None (no image).
        p = _capi.ptr

        def abi_args(st, P, M, W, H, i, g, dL_dview, scratch, scratch_bytes):  # include/dgr_hip.h: dgr_light_backward
            (means3D_, sh_, gC, background_, colors_, scales_, rotations_, cov3D_precomp_, viewmatrix_, projmatrix_, campos_, gt_depth_,
             alphas_, perspec_matrix_, gD, gM, gV) = i
            (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations) = g
            return (st, P, int(degree), M, int(R), background_, W, H, means3D_, sh_, colors_, alphas_, scales_,
                    float(scale_modifier), rotations_, cov3D_precomp_, viewmatrix_, projmatrix_, campos_, float(tan_fovx),
                    float(tan_fovy), p(radii), p(geomBuffer), p(binningBuffer), p(imageBuffer), gC, gD, gM, gV, dL_dmeans2D, None,
                    dL_dopacity, dL_dcolors, None, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, int(bool(debug)), None,
                    perspec_matrix_, dL_dview, None, gt_depth_, *_frontend._tracking_tail(track_off, map_off, need_gaussian_grads),
                    scratch, scratch_bytes)
        # [1,4,4]: the reference binding returns the per-pixel [H*W,4,4] buffer and its __init__.py sums dim 0
        # (L/rasterize_points.cu:186,235, L/__init__.py:160-161); one already-reduced "pixel" keeps that code working
        return _frontend._backward_one(LIGHT, torch, _grad_arena, abi_args, (1, 4, 4), R, need_gaussian_grads, absgrad, silhouette,
                                       means3D, sh, dL_dout_color, background, colors, scales, rotations, cov3D_precomp, viewmatrix,
                                       projmatrix, campos, gt_depth, alphas, perspec_matrix, dL_dout_depth, dL_dout_median_depth,
                                       dL_dout_depth_var)

    mark_visible = _frontend._mark_visible  # L/rasterize_points.cu:238-256


class _CompiledC:
    """The same three functions over the compiled torch extension (csrc/torch_ext.cpp -> dgr_amd/_dgr_torch_ext.so), the
    counterpart of the reference's pybind11 `_C` (L/ext.cpp:15-19): tensor allocation, argument marshalling and the C-ABI
    call happen in C++; only the capacity / status policy stays in Python.  Selected when the extension is built
    (DGR_BINDING=ctypes forces the ctypes class)."""

    ext = _frontend.ext

    @staticmethod
    def rasterize_gaussians(*args):
        return _CompiledC.rasterize_gaussians_r(*args)[1]

    @staticmethod
    def rasterize_gaussians_r(*args):
        """(R for the backward, the `rasterize_gaussians` tuple): see _C.rasterize_gaussians_r."""
        # tensors: color, depth, median, var, alpha, radii, geom, binning, img, unc, px
        R, rendered, _, tensors = _frontend._compiled_forward_r(LIGHT, *args)
        return R, (rendered, *tensors)

    @staticmethod
    def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                     viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_depth,
                                     dL_dout_median_depth, dL_dout_depth_var, gt_depth, sh, degree, campos, geomBuffer, R,
                                     binningBuffer, imageBuffer, alphas, debug, perspec_matrix, track_off, map_off,
                                     need_gaussian_grads=True, absgrad=False, silhouette=None):
        args = (background, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp, viewmatrix,
                projmatrix, float(tan_fovx), float(tan_fovy), dL_dout_color, dL_dout_depth, dL_dout_median_depth,
                dL_dout_depth_var, gt_depth, sh, int(degree), campos, geomBuffer, int(R), binningBuffer, imageBuffer, alphas,
                bool(debug), perspec_matrix, bool(track_off), bool(map_off), bool(need_gaussian_grads),
                _EMPTY if silhouette is None else silhouette, bool(absgrad))
        return tuple(_CompiledC.ext.light_backward(*args))

    mark_visible = _frontend._mark_visible_compiled


# DGR_AUTOGRAD=python keeps the Python autograd.Function over the compiled `_C` (the A/B for profiles/host_breakdown.py)
_USE_NODE = os.environ.get("DGR_AUTOGRAD", "compiled") != "python"
_CtypesC = _C
if _frontend.ext is not None:  # (dgr_amd._frontend decided: DGR_BINDING, DGR_HIP_LIB, extension built)
    _C = _CompiledC


def _rasterize_compiled(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix,
                        gt_depth, rs):
    """`_RasterizeGaussians.apply` through the autograd node compiled into the extension (csrc/torch_ext.cpp: Node<Light>):
    one Python -> C++ crossing per forward, the backward runs inside the autograd engine without the interpreter.  Same
    inputs, outputs, saved state and gradients as the Python Function below, which stays for the debug path and the ctypes
    binding."""
    P, H, W = (means3D.size(0) if means3D.dim() == 2 else 0), rs.image_height, rs.image_width
    args = (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, gt_depth, rs.bg,
            rs.projmatrix, rs.campos, rs.perspec_matrix, rs.scale_modifier, rs.tanfovx, rs.tanfovy, H, W, rs.sh_degree,
            rs.prefiltered, rs.track_off, rs.map_off)
    return tuple(_binning.compiled_forward(_CompiledC.ext.light_apply, args, means3D.device.index, P, H, W, False)[3])


def rasterize_gaussians(
    means3D,
    means2D,
    sh,
    colors_precomp,
    opacities,
    scales,
    rotations,
    cov3Ds_precomp,
    viewmatrix,
    gt_depth,
    raster_settings,
):
    if _C is _CompiledC and not raster_settings.debug and _USE_NODE:
        return _rasterize_compiled(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                   viewmatrix, gt_depth, raster_settings)
    return _RasterizeGaussians.apply(
        means3D,
        means2D,
        sh,
        colors_precomp,
        opacities,
        scales,
        rotations,
        cov3Ds_precomp,
        viewmatrix,
        gt_depth,
        raster_settings,
    )


class _RasterizeGaussians(torch.autograd.Function):
    """`means2D_abs` (absgrad, an extension): one more leaf [P,3] whose gradient is the absolute screen-space gradient
    (include/dgr_hip.h: dgr_light_backward_absgrad); None when absent.  Over either binding's forward and backward: the
    compiled node has no such input.  With the option "silhouette_grad" on at the forward, the opacity_map gradient goes to the
    backward as the silhouette image (dgr_light_backward_silhouette); without it, it is dropped, as the reference does.  What
    the forward records and what the backward does with it: dgr_amd._frontend._record_forward, _run_backward."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                viewmatrix, gt_depth, raster_settings, means2D_abs=None):
        # argument packing of L/diff_gaussian_rasterization/__init__.py:66-87
        args = (
            raster_settings.bg,
            means3D,
            colors_precomp,
            opacities,
            scales,
            rotations,
            raster_settings.scale_modifier,
            cov3Ds_precomp,
            viewmatrix,
            gt_depth,
            raster_settings.projmatrix,
            raster_settings.tanfovx,
            raster_settings.tanfovy,
            raster_settings.image_height,
            raster_settings.image_width,
            sh,
            raster_settings.sh_degree,
            raster_settings.campos,
            raster_settings.prefiltered,
            raster_settings.debug,
        )
        if raster_settings.debug:
            cpu_args = cpu_deep_copy_tuple(args)
            try:
                R, out = _C.rasterize_gaussians_r(*args)
            except Exception as ex:
                torch.save(cpu_args, "snapshot_fw.dump")
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
                raise ex
        else:
            R, out = _C.rasterize_gaussians_r(*args)
        # (color, radii, depth, depth_median, depth_var, opacity_map, gau_uncertainty, gau_related_pixels)
        return _frontend._record_forward(ctx, LIGHT, raster_settings, R, means2D_abs, colors_precomp, means3D, scales, rotations,
                                         cov3Ds_precomp, viewmatrix, sh, gt_depth, out[1:])

    @staticmethod
    def backward(ctx, *grad_outputs):
        def call(saved, images, need_gaussian_grads, silhouette):
            raster_settings = ctx.raster_settings
            (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrix, radii, sh, geomBuffer,
             binningBuffer, imgBuffer, opacity_map, gt_depth) = saved
            grad_color, grad_depth, grad_depth_median, grad_depth_var = images
            # argument packing of L/diff_gaussian_rasterization/__init__.py:116-146
            args = (raster_settings.bg,
                    means3D,
                    radii,
                    colors_precomp,
                    scales,
                    rotations,
                    raster_settings.scale_modifier,
                    cov3Ds_precomp,
                    viewmatrix,
                    raster_settings.projmatrix,
                    raster_settings.tanfovx,
                    raster_settings.tanfovy,
                    grad_color,
                    grad_depth,
                    grad_depth_median,
                    grad_depth_var,
                    gt_depth,
                    sh,
                    raster_settings.sh_degree,
                    raster_settings.campos,
                    geomBuffer,
                    ctx.num_rendered,
                    binningBuffer,
                    imgBuffer,
                    opacity_map,
                    raster_settings.debug,
                    raster_settings.perspec_matrix,
                    raster_settings.track_off,
                    raster_settings.map_off)
            debug = raster_settings.debug
            cpu_args = cpu_deep_copy_tuple(args) if debug else None
            try:
                out = _C.rasterize_gaussians_backward(*args, need_gaussian_grads=debug or need_gaussian_grads, absgrad=ctx.absgrad,
                                                      silhouette=silhouette)
            except Exception:
                if debug:
                    torch.save(cpu_args, "snapshot_bw.dump")
                    print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
                raise
            # reference: torch.sum(grad_viewmatrix, dim=0) over a [H*W,4,4] buffer (__init__.py:160-161);
            # here the buffer is [1,4,4], already reduced: a view instead of a reduction kernel.
            return out[:8] + (out[8].view(4, 4),) + out[9:]
        return _frontend._run_backward(ctx, LIGHT, False, grad_outputs, call)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    perspec_matrix: torch.Tensor
    track_off: bool
    map_off: bool


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        # Mark visible points (based on frustum culling for camera) with a boolean
        with torch.no_grad():
            raster_settings = self.raster_settings
            visible = _C.mark_visible(
                positions,
                raster_settings.viewmatrix,
                raster_settings.projmatrix)
        return visible

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, viewmatrix=None, gt_depth=None, *, means2D_abs=None):
        raster_settings = self.raster_settings
        shs, colors_precomp, scales, rotations, cov3D_precomp = _frontend._rasterizer_inputs(
            means3D, means2D_abs, raster_settings.map_off, shs, colors_precomp, scales, rotations, cov3D_precomp)
        if means2D_abs is not None:
            return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                             cov3D_precomp, viewmatrix, gt_depth, raster_settings, means2D_abs)
        return rasterize_gaussians(
            means3D,
            means2D,
            shs,
            colors_precomp,
            opacities,
            scales,
            rotations,
            cov3D_precomp,
            viewmatrix,
            gt_depth,
            raster_settings,
        )
