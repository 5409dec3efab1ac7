"""Host-side mirror of diff-gaussian-rasterization-full/diff_gaussian_rasterization/__init__.py.

Same names, argument order and return arity as the reference module of the -full variant
(`GaussianRasterizationSettings` without debug / track_off / map_off, forward returning
`(color, radii, depth, uncertainty)`), with `_C.*` replaced by the gfx950 C ABI (include/dgr_hip.h).
`num_related_gaussians` (the reference's NG, which sizes its pair lists) is still produced and threaded
through the autograd context, but nothing here is sized by it.
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _binning, _capi, _frontend
from . import light as _light  # (for the switch point light._USE_NODE alone)
from ._frontend import FULL, _EMPTY, _device_guarded, set_tight_culling  # noqa: F401  (set_tight_culling: shared)


def _grad_arena(P, M, f32):
    """dgr_amd._frontend._grad_arena, allocated through this module's `torch`."""
    return _frontend._grad_arena(P, M, f32, torch)


class _C:
    """Functions with the signatures of the full variant's pybind11 module (F/ext.cpp:15-19).  Their device buffers are
    allocated through this module's `torch`, read at call time."""

    @staticmethod
    def rasterize_gaussians(*args):
        # F/rasterize_points.cu:35-120.  The tuple's num_rendered / num_related are the values last read for the shape (a lazy
        # forward's own are read one call late); the autograd Function takes its backward's R from rasterize_gaussians_r.
        return _CtypesC.rasterize_gaussians_r(*args)[1]

    @_device_guarded(1)
    def rasterize_gaussians_r(*args):
        """(R for the backward, the `rasterize_gaussians` tuple): see dgr_amd.light._C.rasterize_gaussians_r.  num_related is
        the callback forward's NG, the strict forward's status word [3] and, for a lazy forward, the last one read."""
        R, rendered, related, out, geom, binning, img = _frontend._forward_r(FULL, torch, *args)
        color, depth, unc, radii = out
        return R, (rendered, related, color, depth, unc, radii, geom, binning, img)

    @_device_guarded(1)
    def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                     cov3D_precomp, viewmatrix, gt_depth, projmatrix, tan_fovx, tan_fovy,
                                     dL_dout_color, dL_dout_depth, dL_dout_uncertainty, sh, degree, campos, geomBuffer,
                                     R, binningBuffer, imageBuffer, NG, perspec_matrix, need_gaussian_grads=True, absgrad=False,
                                     silhouette=None):
        # F/rasterize_points.cu:122-239.  need_gaussian_grads=False (tracking: no Gaussian input requires a gradient) returns
        # None for the eight per-Gaussian gradients and skips their dense rows; the pose gradient is the same.  absgrad=True
        # (dgr_full_backward_absgrad) appends a tenth result, the absolute screen-space gradient [P,3].  `silhouette`
        # (dgr_full_backward_silhouette): the exact silhouette gradient image [1,H,W], or None; dL_dout_uncertainty keeps the
        # reference's variance form.
        p = _capi.ptr

        def abi_args(st, P, M, W, H, i, g, dL_dview, scratch, scratch_bytes):  # include/dgr_hip.h: dgr_full_backward
            (means3D_, sh_, gC, background_, colors_, scales_, rotations_, cov3D_precomp_, viewmatrix_, projmatrix_, campos_, gt_depth_,
             perspec_matrix_, gD, gU) = i
            (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations) = g
            return (st, P, int(degree), M, int(R), background_, W, H, means3D_, sh_, colors_, scales_, float(scale_modifier),
                    rotations_, cov3D_precomp_, viewmatrix_, projmatrix_, campos_, float(tan_fovx), float(tan_fovy), p(radii),
                    p(geomBuffer), p(binningBuffer), p(imageBuffer), gC, gD, dL_dmeans2D, None, dL_dopacity, dL_dcolors, dL_dmeans3D,
                    dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, None, None, None, None, None, perspec_matrix_, None, None, None,
                    dL_dview, None, None, None, gt_depth_, gU, scratch, scratch_bytes)
        return _frontend._backward_one(FULL, torch, _grad_arena, abi_args, (4, 4), R, need_gaussian_grads, absgrad, silhouette,
                                       means3D, sh, dL_dout_color, background, colors, scales, rotations, cov3D_precomp, viewmatrix,
                                       projmatrix, campos, gt_depth, perspec_matrix, dL_dout_depth, dL_dout_uncertainty)

    mark_visible = _frontend._mark_visible


class _CompiledC:
    """The same functions over the compiled torch extension (csrc/torch_ext.cpp), the counterpart of F/ext.cpp:15-19;
    see dgr_amd.light._CompiledC."""

    ext = _frontend.ext

    @staticmethod
    def rasterize_gaussians(*args):
        return _CompiledC.rasterize_gaussians_r(*args)[1]

    @staticmethod
    def rasterize_gaussians_r(*args):
        """(R for the backward, the `rasterize_gaussians` tuple): see dgr_amd.light._C.rasterize_gaussians_r."""
        # tensors: color, depth, uncertainty, radii, geom, binning, img
        R, rendered, related, tensors = _frontend._compiled_forward_r(FULL, *args)
        return R, (rendered, related, *tensors)

    @staticmethod
    def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                     viewmatrix, gt_depth, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_depth,
                                     dL_dout_uncertainty, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, NG,
                                     perspec_matrix, need_gaussian_grads=True, absgrad=False, silhouette=None):
        args = (background, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp, viewmatrix, gt_depth,
                projmatrix, float(tan_fovx), float(tan_fovy), dL_dout_color, dL_dout_depth, dL_dout_uncertainty, sh, int(degree),
                campos, geomBuffer, int(R), binningBuffer, imageBuffer, int(NG), perspec_matrix, bool(need_gaussian_grads),
                _EMPTY if silhouette is None else silhouette, bool(absgrad))
        return tuple(_CompiledC.ext.full_backward(*args))

    mark_visible = _frontend._mark_visible_compiled


_CtypesC = _C
if _frontend.ext is not None:  # (dgr_amd._frontend decided: DGR_BINDING, DGR_HIP_LIB, extension built)
    _C = _CompiledC


def _rasterize_compiled(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix,
                        gt_depth, rs):
    """`_RasterizeGaussians.apply` through the autograd node compiled into the extension (csrc/torch_ext.cpp: Node<Full>); see
    dgr_amd.light._rasterize_compiled."""
    P, H, W = (means3D.size(0) if means3D.dim() == 2 else 0), rs.image_height, rs.image_width
    args = (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, gt_depth, rs.bg,
            rs.projmatrix, rs.campos, rs.perspec_matrix, rs.scale_modifier, rs.tanfovx, rs.tanfovy, H, W, rs.sh_degree,
            rs.prefiltered, False, False)  # (track_off, map_off: the light variant's)
    # (the strict node does not wait for num_related -- csrc/torch_ext.cpp: Full::after_strict -- and reports -1: the record keeps
    #  the last one read)
    return tuple(_binning.compiled_forward(_CompiledC.ext.full_apply, args, means3D.device.index, P, H, W, True)[3])


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        viewmatrix, gt_depth, raster_settings):
    if _C is _CompiledC and _light._USE_NODE:
        return _rasterize_compiled(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                   viewmatrix, gt_depth, raster_settings)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, viewmatrix, gt_depth, raster_settings)


class _RasterizeGaussians(torch.autograd.Function):
    """`means2D_abs`: one more leaf [P,3] or None (absgrad: dgr_amd.light._RasterizeGaussians).  With the option
    "silhouette_grad" on at the forward, the uncertainty gradient goes to the backward as the exact silhouette image and
    dL_duncertainties is NULL (dgr_full_backward_silhouette); without it, it is the reference's variance form."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix,
                gt_depth, raster_settings, means2D_abs=None):
        # argument packing of F/diff_gaussian_rasterization/__init__.py:62-83
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
        )
        R, out = _C.rasterize_gaussians_r(*args)
        ctx.num_related_gaussians = out[1]
        # (color, radii, depth, uncertainty)
        return _frontend._record_forward(ctx, FULL, raster_settings, R, means2D_abs, colors_precomp, means3D, scales, rotations,
                                         cov3Ds_precomp, viewmatrix, sh, gt_depth, out[2:])

    @staticmethod
    def backward(ctx, *grad_outputs):
        def call(saved, images, need_gaussian_grads, silhouette):
            raster_settings = ctx.raster_settings
            (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrix, radii, sh, geomBuffer, binningBuffer,
             imgBuffer, gt_depth) = saved
            grad_out_color, grad_out_depth, grad_out_uncertainty = images
            # argument packing of F/diff_gaussian_rasterization/__init__.py:104-131
            args = (raster_settings.bg,
                    means3D,
                    radii,
                    colors_precomp,
                    scales,
                    rotations,
                    raster_settings.scale_modifier,
                    cov3Ds_precomp,
                    viewmatrix,
                    gt_depth,
                    raster_settings.projmatrix,
                    raster_settings.tanfovx,
                    raster_settings.tanfovy,
                    grad_out_color,
                    grad_out_depth,
                    grad_out_uncertainty,
                    sh,
                    raster_settings.sh_degree,
                    raster_settings.campos,
                    geomBuffer,
                    ctx.num_rendered,
                    binningBuffer,
                    imgBuffer,
                    ctx.num_related_gaussians,
                    raster_settings.perspec_matrix)
            return _C.rasterize_gaussians_backward(*args, need_gaussian_grads=need_gaussian_grads, absgrad=ctx.absgrad,
                                                   silhouette=silhouette)
        return _frontend._run_backward(ctx, FULL, False, grad_outputs, call)


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
    perspec_matrix: torch.Tensor


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
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
            means3D, means2D_abs, False, shs, colors_precomp, scales, rotations, cov3D_precomp)
        if means2D_abs is not None:
            return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                             cov3D_precomp, viewmatrix, gt_depth, raster_settings, means2D_abs)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   viewmatrix, gt_depth, raster_settings)
