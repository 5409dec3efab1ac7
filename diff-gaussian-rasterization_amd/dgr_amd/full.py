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

from . import _binning, _capi
from . import light as _light
from .light import _check, _device_guarded, _f32c, _grad_arena, set_tight_culling  # noqa: F401  (set_tight_culling: shared)


def _full_outputs(P, H, W, gt_depth, f32, i32):
    """The full forward's output tensors, and their pointers in the order of its entry points' output arguments."""
    color = torch.empty((3, H, W), **f32)
    depth = torch.empty((1, H, W), **f32)
    unc = torch.empty((1, H, W), **f32)
    radii = torch.zeros((P,), **i32)
    p = _capi.ptr
    return (color, depth, unc, radii), (p(color), p(depth), p(gt_depth), p(unc), p(radii))


class _C:
    """Functions with the signatures of the full variant's pybind11 module (F/ext.cpp:15-19)."""

    @staticmethod
    def rasterize_gaussians(*args):
        # F/rasterize_points.cu:35-120.  The tuple's num_rendered / num_related are the values last read for the shape (a lazy
        # forward's own are read one call late); the autograd Function takes its backward's R from rasterize_gaussians_r.
        return _CtypesC.rasterize_gaussians_r(*args)[1]

    @_device_guarded(1)
    def rasterize_gaussians_r(background, means3D, colors, opacity, scales, rotations, scale_modifier,
                              cov3D_precomp, viewmatrix, gt_depth, projmatrix, tan_fovx, tan_fovy,
                              image_height, image_width, sh, degree, campos, prefiltered):
        """(R for the backward, the `rasterize_gaussians` tuple): see dgr_amd.light._C.rasterize_gaussians_r.  num_related is
        the callback forward's NG, the strict forward's status word [3] and, for a lazy forward, the last one read."""
        R, rendered, related, out, geom, binning, img = _light._forward_r(
            True, _full_outputs, background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
            viewmatrix, gt_depth, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered)
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
        lib = _capi.load()
        dev = means3D.device
        P = means3D.size(0)
        H, W = dL_dout_color.size(1), dL_dout_color.size(2)
        f32 = dict(dtype=torch.float32, device=dev)
        means3D = _f32c(means3D, dev)
        background, colors = _f32c(background, dev), _f32c(colors, dev)
        scales, rotations, cov3D_precomp = _f32c(scales, dev), _f32c(rotations, dev), _f32c(cov3D_precomp, dev)
        viewmatrix, projmatrix, campos = _f32c(viewmatrix, dev), _f32c(projmatrix, dev), _f32c(campos, dev)
        gt_depth, sh, perspec_matrix = _f32c(gt_depth, dev), _f32c(sh, dev), _f32c(perspec_matrix, dev)
        gC, gD, gU = _f32c(dL_dout_color, dev), _f32c(dL_dout_depth, dev), _f32c(dL_dout_uncertainty, dev)
        M = sh.size(1) if sh.numel() != 0 else 0
        names = ("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations")
        seg = _grad_arena(P, M, f32) if need_gaussian_grads else dict.fromkeys(names)
        dL_dview = torch.empty((4, 4), **f32)
        scratch = torch.empty((max(lib.dgr_light_backward_scratch_bytes_r(P, W, H, int(R)), 1),), dtype=torch.uint8, device=dev)
        p = _capi.ptr
        args = (_capi.stream_handle(dev.index), P, int(degree), M, int(R), p(background), W, H, p(means3D), p(sh), p(colors),
                p(scales), float(scale_modifier), p(rotations), p(cov3D_precomp), p(viewmatrix), p(projmatrix), p(campos),
                float(tan_fovx), float(tan_fovy), p(radii), p(geomBuffer), p(binningBuffer), p(imageBuffer), p(gC), p(gD),
                p(seg["means2D"]), None, p(seg["opacity"]), p(seg["colors"]), p(seg["means3D"]), p(seg["cov3D"]),
                p(seg["sh"]), p(seg["scales"]), p(seg["rotations"]), None, None, None, None, None, p(perspec_matrix), None,
                None, None, p(dL_dview), None, None, None, p(gt_depth), p(gU), p(scratch), scratch.numel())
        out = (seg["means2D"], seg["colors"], seg["opacity"], seg["means3D"], seg["cov3D"], seg["sh"], seg["scales"],
               seg["rotations"], dL_dview)
        dL_dmeans2D_abs = torch.empty((P, 3), **f32) if absgrad else None
        _check(_capi.call_backward("full", 0, args, dL_dmeans2D_abs, None if silhouette is None else _f32c(silhouette, dev)))
        return out + (dL_dmeans2D_abs,) if absgrad else out

    @_device_guarded(0)
    def mark_visible(means3D, viewmatrix, projmatrix):
        from .light import _C as _LC
        return _LC.mark_visible(means3D, viewmatrix, projmatrix)


class _CompiledC:
    """The same functions over the compiled torch extension (csrc/torch_ext.cpp), the counterpart of F/ext.cpp:15-19;
    see dgr_amd.light._CompiledC."""

    ext = None

    @staticmethod
    def rasterize_gaussians(*args):
        return _CompiledC.rasterize_gaussians_r(*args)[1]

    @staticmethod
    def rasterize_gaussians_r(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                              viewmatrix, gt_depth, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                              prefiltered):
        """(R for the backward, the `rasterize_gaussians` tuple): see dgr_amd.light._C.rasterize_gaussians_r."""
        P, H, W = means3D.size(0) if means3D.dim() else 0, int(image_height), int(image_width)
        args = (background, means3D, colors, opacity, scales, rotations, float(scale_modifier), cov3D_precomp, viewmatrix, gt_depth,
                projmatrix, float(tan_fovx), float(tan_fovy), H, W, sh, int(degree), campos, bool(prefiltered), False)  # (no debug)
        # tensors: color, depth, uncertainty, radii, geom, binning, img
        R, rendered, related, tensors = _binning.compiled_forward(_CompiledC.ext.full_forward, args, means3D.device.index, P, H, W, True)
        return R, (rendered, related, *tensors)

    @staticmethod
    def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                     viewmatrix, gt_depth, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_depth,
                                     dL_dout_uncertainty, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, NG,
                                     perspec_matrix, need_gaussian_grads=True, absgrad=False, silhouette=None):
        args = (background, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp, viewmatrix, gt_depth,
                projmatrix, float(tan_fovx), float(tan_fovy), dL_dout_color, dL_dout_depth, dL_dout_uncertainty, sh, int(degree),
                campos, geomBuffer, int(R), binningBuffer, imageBuffer, int(NG), perspec_matrix, bool(need_gaussian_grads),
                _light._EMPTY if silhouette is None else silhouette, bool(absgrad))
        return tuple(_CompiledC.ext.full_backward(*args))

    @staticmethod
    def mark_visible(means3D, viewmatrix, projmatrix):
        return _CompiledC.ext.mark_visible(means3D, viewmatrix, projmatrix)


_CtypesC = _C
if _light._C is getattr(_light, "_CompiledC", None):  # the light module decided (DGR_BINDING, DGR_HIP_LIB, extension built)
    _CompiledC.ext = _light._CompiledC.ext
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
        # (R: the backward's num_rendered -- the capacity of a lazy forward, which never learns its own count)
        R, (_, num_related_gaussians, color, depth, uncertainty, radii, geomBuffer, binningBuffer,
            imgBuffer) = _C.rasterize_gaussians_r(*args)
        ctx.raster_settings = raster_settings
        ctx.num_rendered = R
        ctx.absgrad = means2D_abs is not None
        ctx.dgr_options = _capi.load().dgr_thread_options_effective()  # the backward runs under the forward's options
        ctx.silhouette = _capi.silhouette_on(ctx.dgr_options)
        ctx.num_related_gaussians = num_related_gaussians
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrix, radii, sh,
                              geomBuffer, binningBuffer, imgBuffer, gt_depth)
        ctx.set_materialize_grads(False)  # no zero-filled gradient tensor for radii on every backward
        ctx.mark_non_differentiable(radii)
        return color, radii, depth, uncertainty

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_out_depth, grad_out_uncertainty):
        num_rendered = ctx.num_rendered
        num_related_gaussians = ctx.num_related_gaussians
        raster_settings = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrix, radii, sh, geomBuffer, binningBuffer,
         imgBuffer, gt_depth) = ctx.saved_tensors
        # outputs that did not take part in the loss arrive as None: zeros, as the reference's autograd would have passed
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        zeros = lambda c: torch.zeros((c, H, W), dtype=torch.float32, device=means3D.device)  # noqa: E731
        absgrad = ctx.absgrad
        grad_out_color = zeros(3) if grad_out_color is None else grad_out_color
        grad_out_depth = zeros(1) if grad_out_depth is None else grad_out_depth
        silhouette = None
        if ctx.silhouette:  # the exact silhouette gradient: the image (or NULL, unused) there, NULL as dL_duncertainties
            silhouette, grad_out_uncertainty = grad_out_uncertainty, _light._EMPTY
        if absgrad and grad_out_uncertainty is None:  # NULL: the lean blend backward (bit-identical to a zero image)
            grad_out_uncertainty = _light._EMPTY
        grad_out_uncertainty = zeros(1) if grad_out_uncertainty is None else grad_out_uncertainty
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
                num_rendered,
                binningBuffer,
                imgBuffer,
                num_related_gaussians,
                raster_settings.perspec_matrix)
        with _capi.under_options(ctx.dgr_options):  # (the autograd engine may run this on a thread of its own)
            out = _C.rasterize_gaussians_backward(*args, need_gaussian_grads=absgrad or any(ctx.needs_input_grad[:8]),
                                                  absgrad=absgrad, silhouette=silhouette)
        grad_means2D_abs = out[9] if absgrad else None
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_rotations, grad_viewmatrix) = out[:9]
        _light._consume_post_backward_wait()  # (dgr_amd.multiview.ViewStreams.before_backward)
        grads = (
            grad_means3D,
            grad_means2D,
            grad_sh,
            grad_colors_precomp,
            grad_opacities,
            grad_scales,
            grad_rotations,
            grad_cov3Ds_precomp,
            grad_viewmatrix,
            None,
            None,
            grad_means2D_abs,
        )
        return grads


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
        # means2D_abs (absgrad, an extension): as dgr_amd.light.GaussianRasterizer.forward's
        raster_settings = self.raster_settings
        if means2D_abs is not None:
            _light.check_means2D_abs(means2D_abs, means3D, False)
        shs, colors_precomp, scales, rotations, cov3D_precomp = _light._checked_inputs(shs, colors_precomp, scales, rotations,
                                                                                       cov3D_precomp)
        if means2D_abs is not None:
            return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                                cov3D_precomp, viewmatrix, gt_depth, raster_settings, means2D_abs)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   viewmatrix, gt_depth, raster_settings)
