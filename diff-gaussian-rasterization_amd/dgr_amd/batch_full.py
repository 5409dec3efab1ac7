"""Batched multi-view surface of the -full variant: V cameras over ONE set of Gaussians per call, through the C ABI's
dgr_full_forward_batch / dgr_full_backward_batch (include/dgr_hip.h).

The counterpart of `dgr_amd.batch` for the full variant's `_RasterizeGaussians` (F/diff_gaussian_rasterization/__init__.py):
per view the outputs (colour, radii, depth, uncertainty) are bit-identical to the one-view surface (`dgr_amd.full`); the
Gaussians' gradients come back SUMMED over the views, formed in registers by one per-Gaussian launch and written once, as views
of one flat arena (`dgr_amd._frontend._grad_arena`, so `dgr_amd.multiview.GradientArena` finds the all-reduce span); `means2D`
([V,P,3]) and `viewmatrices` ([V,4,4]) keep their per-view gradients.  Settings are `dgr_amd.batch.BatchRasterizationSettings`;
the full variant has no tracking / mapping switches, so `track_off` and `map_off` must be False.

The forward and the ctypes backward are the light batch's too (`dgr_amd._frontend._forward_views`, `_backward_views`), with the binning capacity and
status policy of `dgr_amd._binning` (`run_batch`: lazy mode follows the shape's growth guard and runs an unsettled shape strict;
a batch of V views leaves V status words unread).  A lazy forward hands its backward the capacity its binning buffers were carved
with as R (deterministic gradients size their row buffers by it), never the largest count seen.  There is no CPU fallback.
"""
import torch

from . import _capi, _frontend
from ._frontend import FULL, MAX_VIEWS, _backward_views, _ext, _forward_views  # noqa: F401  (read from here too)
from .batch import BatchRasterizationSettings  # noqa: F401  (the settings are shared)


def _forward_batch(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, gt_depths,
                   projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered):
    """Returns (per-view R for the backward, color, depth, uncertainty, radii, geom, binning, img, [V,4] device status words
    {num_rendered, overflow, prefiltered violation, num_related})."""
    V = _frontend._check_batch(means3D, viewmatrices)
    R, out = _forward_views(FULL, V, bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                            gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered)
    return (R,) + tuple(out[1:]) + (out[0],)


def _backward_batch(bg, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices,
                    tanfovx, tanfovy, gC, gD, gU, gt_depths, sh, degree, campos, geom, binning, img, perspec_matrix,
                    need_gaussian_grads, need_means2D, num_rendered, absgrad=False, silhouette=None):
    """gU None: no view's loss used the uncertainty image (the lean blend backward).  `num_rendered`: per view, the R of the
    one-view backward (>= the view's count; sizes the row buffers under deterministic_grads).  Returns (dL_dmeans2D [V,P,3] or
    None, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dL_dview [V,4,4]); absgrad=True
    (dgr_full_backward_batch_absgrad) appends every view's absolute screen-space gradient [V,P,3].  `silhouette`: every view's
    exact silhouette gradient [V,1,H,W] (dgr_full_backward_batch_silhouette), or None."""
    num_rendered = [int(r) for r in num_rendered]
    dev = means3D.device
    ext = _ext()
    if ext is not None:
        e = torch.empty(0, device=dev)
        args = (bg, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp,
                viewmatrices, projmatrices, float(tanfovx), float(tanfovy), gC, gD,
                e if gU is None else gU, gt_depths, sh, int(degree), campos, geom, binning, img,
                perspec_matrix, bool(need_gaussian_grads), bool(need_means2D), num_rendered,
                e if silhouette is None else silhouette, bool(absgrad))
        return tuple(ext.full_backward_batch(*args))
    return _backward_views(FULL, {"dL_dpix": gC, "dL_depths": gD, "dL_duncertainties": gU}, (), bg, means3D, radii, colors, scales,
                           rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices, tanfovx, tanfovy, gt_depths, sh,
                           degree, campos, geom, binning, img, perspec_matrix, need_gaussian_grads, need_means2D, num_rendered,
                           absgrad, silhouette)


class _RasterizeGaussiansBatchFull(torch.autograd.Function):
    """The full variant's `_RasterizeGaussians` (F/diff_gaussian_rasterization/__init__.py) over V cameras.  `means2D_abs`: one
    more leaf [V,P,3] or None (absgrad: dgr_amd.batch._RasterizeGaussiansBatch).  Option "silhouette_grad" at the forward: the
    uncertainty gradient is every view's exact silhouette image, and no view has a dL_duncertainties image."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrices,
                gt_depths, raster_settings, means2D_abs=None):
        rs = raster_settings
        with _capi.on_device(means3D.device):
            out = _forward_batch(rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                                 viewmatrices, gt_depths, rs.projmatrices, rs.tanfovx, rs.tanfovy, int(rs.image_height),
                                 int(rs.image_width), sh, rs.sh_degree, rs.campos, rs.prefiltered)
        # (color, radii, depth, unc)
        return _frontend._record_forward(ctx, FULL, rs, out[0], means2D_abs, colors_precomp, means3D, scales, rotations,
                                         cov3Ds_precomp, viewmatrices, sh, gt_depths, out[1:-1])

    @staticmethod
    def backward(ctx, *grad_outputs):
        def call(saved, images, need_gaussian_grads, silhouette):
            rs = ctx.raster_settings
            (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrices, radii, sh, geom, binning, img,
             gt_depths) = saved
            with _capi.on_device(means3D.device):
                return _backward_batch(
                    rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, viewmatrices,
                    rs.projmatrices, rs.tanfovx, rs.tanfovy, *images, gt_depths, sh, rs.sh_degree, rs.campos, geom, binning, img,
                    rs.perspec_matrix, need_gaussian_grads=need_gaussian_grads, need_means2D=bool(ctx.needs_input_grad[1]),
                    num_rendered=ctx.num_rendered, absgrad=ctx.absgrad, silhouette=silhouette)
        return _frontend._run_backward(ctx, FULL, True, grad_outputs, call)


def rasterize_gaussians_batch_full(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                   viewmatrices, gt_depths, raster_settings, means2D_abs=None):
    """The full variant's `rasterize_gaussians` for V cameras: `means2D` is [V,P,3] (or a tensor that requires no gradient),
    `viewmatrices` [V,4,4], `gt_depths` [V,H,W] (read by the backward); returns color [V,3,H,W], radii [V,P], depth [V,1,H,W]
    and uncertainty [V,1,H,W]."""
    if raster_settings.track_off or raster_settings.map_off:
        raise ValueError("the full variant has no track_off / map_off")
    if gt_depths is None:
        raise ValueError("the full variant's batch needs gt_depths (its backward reads them)")
    _frontend._check_batch(means3D, viewmatrices)
    if means2D_abs is not None:  # (absgrad: GaussianRasterizerBatchFull.forward)
        _frontend.check_means2D_abs(means2D_abs, means3D, False, shape=(viewmatrices.size(0), means3D.size(0), 3))
    return _RasterizeGaussiansBatchFull.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                              viewmatrices, gt_depths, raster_settings, means2D_abs)


class GaussianRasterizerBatchFull(torch.nn.Module):
    """The full variant's `GaussianRasterizer` over the V cameras of its settings."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, viewmatrices=None, gt_depths=None, *, means2D_abs=None):
        # means2D_abs (absgrad): a float32 [V,P,3] leaf whose .grad receives every view's absolute screen-space gradient
        shs, colors_precomp, scales, rotations, cov3D_precomp = _frontend._checked_inputs(shs, colors_precomp, scales, rotations,
                                                                                          cov3D_precomp)
        if viewmatrices is None:
            viewmatrices = self.raster_settings.viewmatrices
        return rasterize_gaussians_batch_full(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                              viewmatrices, gt_depths, self.raster_settings, means2D_abs=means2D_abs)
