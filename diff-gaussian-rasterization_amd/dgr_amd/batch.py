"""Batched multi-view surface of the light variant (BASELINE configs 4 and 5): V cameras over ONE set
of Gaussians per call.

The reference renders a keyframe batch as V calls of `GaussianRasterizer.forward` + `.backward`
(L/diff_gaussian_rasterization/__init__.py:36-176) and lets autograd add the V dense gradient sets.  `rasterize_gaussians_batch`
keeps that function's argument meaning with a leading view dimension on everything that belongs to a camera and goes through
the C ABI's batched entry points (include/dgr_hip.h: dgr_light_forward_batch / dgr_light_backward_batch):

  * per view the outputs are bit-identical to the one-view surface (`dgr_amd.light`);
  * the gradients of the Gaussians come back SUMMED over the views -- what autograd's accumulation of V one-view backward
    passes yields (same operations in the same order in the per-Gaussian stage; two runs differ only by the order of the
    blend backward's float atomics, as two one-view runs do) -- formed in registers and written once; `means2D` (the
    screen-space points 3DGS reads its densification statistics from) and `viewmatrices` keep their per-view gradients;
  * they are views of one flat arena (`dgr_amd._frontend._grad_arena`), so `dgr_amd.multiview.GradientArena` finds the fused
    all-reduce span of a multi-GPU mapping step in them as it does for a one-view backward.

torch supplies device memory and the current stream; every compute call goes through the C ABI.  There is no CPU fallback.
"""
from typing import NamedTuple

import torch

from . import _capi, _frontend
from ._frontend import LIGHT, MAX_VIEWS, _EMPTY, _backward_views, _ext, _forward_views, _row  # noqa: F401  (read from here too)


class BatchRasterizationSettings(NamedTuple):
    """`GaussianRasterizationSettings` (L/diff_gaussian_rasterization/__init__.py:180-195) for V cameras that share the
    image size, the field of view and the background: the three camera tensors carry a leading view dimension."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrices: torch.Tensor   # [V,4,4]
    projmatrices: torch.Tensor   # [V,4,4]
    sh_degree: int
    campos: torch.Tensor         # [V,3]
    prefiltered: bool
    debug: bool
    perspec_matrix: torch.Tensor  # [4,4] (one projection for the batch) or [V,4,4] (one per view, e.g. per-view cx, cy)
    track_off: bool
    map_off: bool


def _forward_batch(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, gt_depths,
                   projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered):
    """Returns (per-view R for the backward, color, depth, median, var, alpha, radii, geom, binning, img, unc, px)."""
    V = _frontend._check_batch(means3D, viewmatrices)
    R, out = _forward_views(LIGHT, V, bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                            gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered)
    return (R,) + tuple(out[1:])


def _backward_batch(bg, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices,
                    tanfovx, tanfovy, gC, gD, gM, gV, gt_depths, sh, degree, campos, geom, binning, img, alphas,
                    perspec_matrix, track_off, map_off, need_gaussian_grads, need_means2D, num_rendered=None, absgrad=False,
                    silhouette=None):
    """`num_rendered`: per view, what the one-view backward takes as R (>= the view's instance count); read by the library only
    under deterministic_grads, where it sizes the views' row buffers.  `absgrad=True` (dgr_light_backward_batch_absgrad) appends
    a tenth result, every view's absolute screen-space gradient [V,P,3].  `silhouette`: every view's opacity_map gradient
    [V,1,H,W] (dgr_light_backward_batch_silhouette), or None."""
    V_ = viewmatrices.size(0)
    num_rendered = [int(r) for r in (num_rendered if num_rendered is not None else [0] * V_)]
    ext = _ext()
    if ext is not None:
        args = (bg, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp,
                viewmatrices, projmatrices, float(tanfovx), float(tanfovy), gC, gD, gM, gV, gt_depths, sh,
                int(degree), campos, geom, binning, img, alphas, perspec_matrix, bool(track_off),
                bool(map_off), bool(need_gaussian_grads), bool(need_means2D), num_rendered,
                _EMPTY if silhouette is None else silhouette, bool(absgrad))
        return tuple(ext.light_backward_batch(*args))
    return _backward_views(LIGHT, {"alphas": alphas, "dL_dpix": gC, "dL_dpix_depth": gD, "dL_dpix_median_depth": gM,
                                   "dL_dpix_depth_var": gV},
                           _frontend._tracking_tail(track_off, map_off, need_gaussian_grads), bg, means3D, radii, colors, scales,
                           rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices, tanfovx, tanfovy, gt_depths, sh,
                           degree, campos, geom, binning, img, perspec_matrix, need_gaussian_grads, need_means2D, num_rendered,
                           absgrad, silhouette)


class _RasterizeGaussiansBatch(torch.autograd.Function):
    """`_RasterizeGaussians` (L/diff_gaussian_rasterization/__init__.py:48-176) over V cameras.  `means2D_abs`: one more leaf
    [V,P,3] whose gradient is every view's absolute screen-space gradient (absgrad, include/dgr_hip.h:
    dgr_light_backward_batch_absgrad), or None.  Option "silhouette_grad" at the forward: the opacity_map gradient is every
    view's silhouette image (dgr_light_backward_batch_silhouette)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrices,
                gt_depths, raster_settings, means2D_abs=None):
        rs = raster_settings
        with _capi.on_device(means3D.device):
            out = _forward_batch(rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                                 viewmatrices, gt_depths, rs.projmatrices, rs.tanfovx, rs.tanfovy, int(rs.image_height),
                                 int(rs.image_width), sh, rs.sh_degree, rs.campos, rs.prefiltered)
        # (color, radii, depth, depth_median, depth_var, opacity_map, unc, px)
        return _frontend._record_forward(ctx, LIGHT, rs, out[0], means2D_abs, colors_precomp, means3D, scales, rotations,
                                         cov3Ds_precomp, viewmatrices, sh, gt_depths, out[1:])

    @staticmethod
    def backward(ctx, *grad_outputs):
        def call(saved, images, need_gaussian_grads, silhouette):
            rs = ctx.raster_settings
            (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrices, radii, sh, geom, binning, img, opacity_map,
             gt_depths) = saved
            with _capi.on_device(means3D.device):
                return _backward_batch(
                    rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, viewmatrices,
                    rs.projmatrices, rs.tanfovx, rs.tanfovy, *images, gt_depths, sh, rs.sh_degree, rs.campos, geom, binning, img,
                    opacity_map, rs.perspec_matrix, rs.track_off, rs.map_off, need_gaussian_grads=need_gaussian_grads,
                    need_means2D=bool(ctx.needs_input_grad[1]), num_rendered=ctx.num_rendered, absgrad=ctx.absgrad,
                    silhouette=silhouette)
        return _frontend._run_backward(ctx, LIGHT, True, grad_outputs, call)


def rasterize_gaussians_batch(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrices,
                              gt_depths, raster_settings):
    """`rasterize_gaussians` (L/diff_gaussian_rasterization/__init__.py:22-46) for V cameras: `means2D` is [V,P,3] (or a
    tensor that requires no gradient), `viewmatrices` [V,4,4], `gt_depths` [V,H,W]; the eight outputs carry a leading view
    dimension."""
    return _RasterizeGaussiansBatch.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                          viewmatrices, gt_depths, raster_settings)


class GaussianRasterizerBatch(torch.nn.Module):
    """`GaussianRasterizer` (L/diff_gaussian_rasterization/__init__.py:197-258) over the V cameras of its settings."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, viewmatrices=None, gt_depths=None, *, means2D_abs=None):
        rs = self.raster_settings
        if viewmatrices is None:
            viewmatrices = rs.viewmatrices
        shs, colors_precomp, scales, rotations, cov3D_precomp = _frontend._rasterizer_inputs(
            means3D, means2D_abs, rs.map_off, shs, colors_precomp, scales, rotations, cov3D_precomp,
            None if means2D_abs is None else (viewmatrices.size(0), means3D.size(0), 3))
        if means2D_abs is not None:
            return _RasterizeGaussiansBatch.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                                  cov3D_precomp, viewmatrices, gt_depths, rs, means2D_abs)
        return rasterize_gaussians_batch(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                         viewmatrices, gt_depths, rs)
