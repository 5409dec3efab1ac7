"""Batched multi-view surface of the -full variant: V cameras over ONE set of Gaussians per call, through the C ABI's
dgr_full_forward_batch / dgr_full_backward_batch (include/dgr_hip.h).

The counterpart of `dgr_amd.batch` for the full variant's `_RasterizeGaussians` (F/diff_gaussian_rasterization/__init__.py):
per view the outputs (colour, radii, depth, uncertainty) are bit-identical to the one-view surface (`dgr_amd.full`); the
Gaussians' gradients come back SUMMED over the views, formed in registers by one per-Gaussian launch and written once, as views
of one flat arena (`dgr_amd.light._grad_arena`, so `dgr_amd.multiview.GradientArena` finds the all-reduce span); `means2D`
([V,P,3]) and `viewmatrices` ([V,4,4]) keep their per-view gradients.  Settings are `dgr_amd.batch.BatchRasterizationSettings`;
the full variant has no tracking / mapping switches, so `track_off` and `map_off` must be False.

The binning capacity and status policy is `dgr_amd.light`'s (`_binning_policy`: lazy mode follows the shape's growth guard and
runs an unsettled shape strict).  A lazy forward hands its backward the capacity its binning buffers were carved with as R
(deterministic gradients size their row buffers by it), never the largest count seen.  There is no CPU fallback.
"""
import ctypes as C

import torch

from . import _capi
from . import light as _light
from .batch import MAX_VIEWS, BatchRasterizationSettings, _ext, _policy, _row, _settle  # noqa: F401  (the settings are shared)

_View, _ViewGrad = _capi.FullView, _capi.FullViewGrad


def _check_inputs(means3D, viewmatrices):
    V = viewmatrices.size(0) if viewmatrices.dim() == 3 else 0
    if not 1 <= V <= MAX_VIEWS:
        raise RuntimeError(f"1 .. {MAX_VIEWS} views per batch")
    if means3D.device.type != "cuda":
        raise RuntimeError("dgr_hip runs on the GPU only (no CPU path exists, as in the reference)")
    return V


def _forward_batch(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, gt_depths,
                   projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered):
    """Returns (per-view R for the backward, color, depth, uncertainty, radii, geom, binning, img, [V,4] device status words
    {num_rendered, overflow, prefiltered violation, num_related})."""
    V = _check_inputs(means3D, viewmatrices)
    dev = means3D.device
    P = means3D.size(0)
    key = (dev.index, P, H, W)
    strict, use, cap = _policy(key, P)
    ext = _ext()
    while True:
        if ext is not None:
            out, tickets = ext.full_forward_batch(bg, means3D, colors, opacity, scales, rotations, float(scale_modifier),
                                                  cov3D_precomp, viewmatrices, gt_depths, projmatrices, float(tanfovx),
                                                  float(tanfovy), int(H), int(W), sh, int(degree), campos, bool(prefiltered),
                                                  use, not strict)
        else:
            out, tickets = _forward_batch_ctypes(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                                                 viewmatrices, gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree,
                                                 campos, prefiltered, use, V), None
        if P == 0:
            return ([0] * V,) + tuple(out[1:]) + (out[0],)
        R = _settle(out[0], key, strict, use, cap, V, tickets)
        if R is not None:
            return (R,) + tuple(out[1:]) + (out[0],)
        use = int(max(r[0] for r in out[0].tolist()) * 1.1) + 4096  # overflow: those views' tile lists were left empty


def _forward_batch_ctypes(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                          gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered, cap, V):
    lib = _capi.load()
    dev = means3D.device
    f32 = dict(dtype=torch.float32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    c = _light._f32c
    means3D, bg, colors, opacity = c(means3D, dev), c(bg, dev), c(colors, dev), c(opacity, dev)
    scales, rotations, cov3D_precomp, sh = c(scales, dev), c(rotations, dev), c(cov3D_precomp, dev), c(sh, dev)
    viewmatrices, projmatrices, campos, gt_depths = c(viewmatrices, dev), c(projmatrices, dev), c(campos, dev), c(gt_depths, dev)
    P = means3D.size(0)
    M = sh.size(1) if sh.numel() != 0 else 0
    color = torch.empty((V, 3, H, W), **f32)
    depth, unc = torch.empty((V, 1, H, W), **f32), torch.empty((V, 1, H, W), **f32)
    radii = (torch.empty if P else torch.zeros)((V, P), dtype=torch.int32, device=dev)
    geom = torch.empty((V, max(lib.dgr_geometry_bytes(P), 1)), **u8)
    img = torch.empty((V, max(lib.dgr_image_bytes(W, H), 1)), **u8)
    binning = torch.empty((V, max(lib.dgr_binning_bytes(cap, W, H), 1)), **u8)
    status = torch.zeros((V, 4), dtype=torch.int32, device=dev)
    views = (_View * V)()
    for v in range(V):
        w = views[v]
        w.geometry_buffer, w.binning_buffer, w.binning_capacity, w.image_buffer = _row(geom, v), _row(binning, v), cap, _row(img, v)
        w.status, w.viewmatrix, w.projmatrix, w.cam_pos = _row(status, v), _row(viewmatrices, v), _row(projmatrices, v), _row(campos, v)
        w.out_color, w.out_depth, w.gt_depth, w.out_uncertainty = _row(color, v), _row(depth, v), _row(gt_depths, v), _row(unc, v)
        w.radii = _row(radii, v)
    p = _capi.ptr
    _light._check(lib.dgr_full_forward_batch(_capi.stream_handle(dev.index), V, views, P, int(degree), M, p(bg), W, H, p(means3D),
                                             p(sh), p(colors), p(opacity), p(scales), float(scale_modifier), p(rotations),
                                             p(cov3D_precomp), float(tanfovx), float(tanfovy), int(bool(prefiltered))))
    return status, color, depth, unc, radii, geom, binning, img


def _backward_batch(bg, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices,
                    tanfovx, tanfovy, gC, gD, gU, gt_depths, sh, degree, campos, geom, binning, img, perspec_matrix,
                    need_gaussian_grads, need_means2D, num_rendered, absgrad=False):
    """gU None: no view's loss used the uncertainty image (the lean blend backward).  `num_rendered`: per view, the R of the
    one-view backward (>= the view's count; sizes the row buffers under deterministic_grads).  Returns (dL_dmeans2D [V,P,3] or
    None, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dL_dview [V,4,4]); absgrad=True
    (dgr_full_backward_batch_absgrad) appends every view's absolute screen-space gradient [V,P,3]."""
    num_rendered = [int(r) for r in num_rendered]
    dev = means3D.device
    ext = _ext()
    if ext is not None:
        e = torch.empty(0, device=dev)
        fn = ext.full_backward_batch_absgrad if absgrad else ext.full_backward_batch
        return tuple(fn(bg, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp,
                                             viewmatrices, projmatrices, float(tanfovx), float(tanfovy), gC, gD,
                                             e if gU is None else gU, gt_depths, sh, int(degree), campos, geom, binning, img,
                                             perspec_matrix, bool(need_gaussian_grads), bool(need_means2D), num_rendered))
    lib = _capi.load()
    V, P = viewmatrices.size(0), means3D.size(0)
    H, W = gC.size(2), gC.size(3)
    f32 = dict(dtype=torch.float32, device=dev)
    c = _light._f32c
    means3D, bg, colors = c(means3D, dev), c(bg, dev), c(colors, dev)
    scales, rotations, cov3D_precomp, sh = c(scales, dev), c(rotations, dev), c(cov3D_precomp, dev), c(sh, dev)
    viewmatrices, projmatrices, campos = c(viewmatrices, dev), c(projmatrices, dev), c(campos, dev)
    gt_depths, perspec_matrix = c(gt_depths, dev), c(perspec_matrix, dev)
    gC, gD = c(gC, dev), c(gD, dev)
    gU = None if gU is None else c(gU, dev)
    M = sh.size(1) if sh.numel() != 0 else 0
    if need_gaussian_grads:
        seg = _light._grad_arena(P, M, f32)
        seg["means2D"].zero_()  # the arena's one-view slot: the batch returns means2D gradients per view, beside the arena
        d3, dsh, dop, dsc, drot, dcov, dcol = (seg[k] for k in ("means3D", "sh", "opacity", "scales", "rotations", "cov3D", "colors"))
        d2 = torch.empty((V, P, 3), **f32) if need_means2D else None
    else:
        d3 = dsh = dop = dsc = drot = dcov = dcol = d2 = None
    dview = torch.empty((V, 4, 4), **f32)
    nscr = (max(lib.dgr_light_backward_scratch_bytes_r(P, W, H, max(num_rendered + [0])), 1) + 255) // 256 * 256
    scratch = torch.empty((V, nscr), dtype=torch.uint8, device=dev)
    views = (_ViewGrad * V)()
    pp = _capi.ptr(perspec_matrix)
    for v in range(V):
        w = views[v]
        w.geometry_buffer, w.binning_buffer, w.image_buffer = _row(geom, v), _row(binning, v), _row(img, v)
        w.viewmatrix, w.projmatrix, w.cam_pos, w.perspec_matrix = _row(viewmatrices, v), _row(projmatrices, v), _row(campos, v), pp
        w.gt_depth, w.radii = _row(gt_depths, v), _row(radii, v)
        w.dL_dpix, w.dL_depths, w.dL_duncertainties = _row(gC, v), _row(gD, v), _row(gU, v)
        w.dL_dmean2D, w.dL_dview, w.scratch, w.scratch_bytes = _row(d2, v), _row(dview, v), _row(scratch, v), nscr
        w.num_rendered = num_rendered[v]
    p = _capi.ptr
    q = lambda t: None if t is None else p(t)  # noqa: E731
    args = (_capi.stream_handle(dev.index), V, views, P, int(degree), M, p(bg), W, H, p(means3D), p(sh), p(colors), p(scales),
            float(scale_modifier), p(rotations), p(cov3D_precomp), float(tanfovx), float(tanfovy), q(dop), q(dcol), q(d3), q(dcov),
            q(dsh), q(dsc), q(drot))
    if not absgrad:
        _light._check(lib.dgr_full_backward_batch(*args))
        return d2, dcol, dop, d3, dcov, dsh, dsc, drot, dview
    dabs = torch.empty((V, P, 3), **f32)
    _light._check(lib.dgr_full_backward_batch_absgrad(*args, (C.c_void_p * V)(*(_row(dabs, v) for v in range(V)))))
    return d2, dcol, dop, d3, dcov, dsh, dsc, drot, dview, dabs


class _RasterizeGaussiansBatchFull(torch.autograd.Function):
    """The full variant's `_RasterizeGaussians` (F/diff_gaussian_rasterization/__init__.py) over V cameras."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrices,
                gt_depths, raster_settings):
        rs = raster_settings
        with _capi.on_device(means3D.device):
            (R, color, depth, unc, radii, geom, binning, img, _) = _forward_batch(
                rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, viewmatrices,
                gt_depths, rs.projmatrices, rs.tanfovx, rs.tanfovy, int(rs.image_height), int(rs.image_width), sh,
                rs.sh_degree, rs.campos, rs.prefiltered)
        ctx.raster_settings = rs
        ctx.num_rendered = R
        ctx.dgr_options = _capi.load().dgr_thread_options_effective()  # the backward runs under the forward's options
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrices, radii, sh, geom, binning,
                              img, gt_depths)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii)
        return color, radii, depth, unc

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_unc):
        rs = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrices, radii, sh, geom, binning, img,
         gt_depths) = ctx.saved_tensors
        V, H, W = viewmatrices.size(0), int(rs.image_height), int(rs.image_width)
        zeros = lambda ch: torch.zeros((V, ch, H, W), dtype=torch.float32, device=means3D.device)  # noqa: E731
        grad_color = zeros(3) if grad_color is None else grad_color
        grad_depth = zeros(1) if grad_depth is None else grad_depth
        need = ctx.needs_input_grad
        with _capi.on_device(means3D.device), _capi.under_options(ctx.dgr_options):
            absgrad = getattr(ctx, "absgrad", False)  # (_RasterizeGaussiansBatchFullAbs)
            g = _backward_batch(
                rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, viewmatrices,
                rs.projmatrices, rs.tanfovx, rs.tanfovy, grad_color, grad_depth, grad_unc, gt_depths, sh, rs.sh_degree,
                rs.campos, geom, binning, img, rs.perspec_matrix, need_gaussian_grads=any(need[:8]) or absgrad,
                need_means2D=bool(need[1]), num_rendered=ctx.num_rendered, **({"absgrad": True} if absgrad else {}))
        (g2, gcol, gop, g3, gcov, gsh, gsc, grot, gview) = g[:9]
        _light._consume_post_backward_wait()
        grads = (g3, g2, gsh, gcol, gop, gsc, grot, gcov, gview, None, None)
        return grads + (g[9],) if absgrad else grads


class _RasterizeGaussiansBatchFullAbs(torch.autograd.Function):
    """_RasterizeGaussiansBatchFull with one more leaf, means2D_abs [V,P,3] (absgrad: dgr_amd.batch._RasterizeGaussiansBatchAbs)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrices,
                gt_depths, raster_settings, means2D_abs):
        ctx.absgrad = True
        return _RasterizeGaussiansBatchFull.forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                                    cov3Ds_precomp, viewmatrices, gt_depths, raster_settings)

    @staticmethod
    def backward(ctx, *grads):
        return _RasterizeGaussiansBatchFull.backward(ctx, *grads)


def rasterize_gaussians_batch_full(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                   viewmatrices, gt_depths, raster_settings, means2D_abs=None):
    """The full variant's `rasterize_gaussians` for V cameras: `means2D` is [V,P,3] (or a tensor that requires no gradient),
    `viewmatrices` [V,4,4], `gt_depths` [V,H,W] (read by the backward); returns color [V,3,H,W], radii [V,P], depth [V,1,H,W]
    and uncertainty [V,1,H,W]."""
    if raster_settings.track_off or raster_settings.map_off:
        raise ValueError("the full variant has no track_off / map_off")
    if gt_depths is None:
        raise ValueError("the full variant's batch needs gt_depths (its backward reads them)")
    _check_inputs(means3D, viewmatrices)
    if means2D_abs is not None:  # (absgrad: GaussianRasterizerBatchFull.forward)
        _light.check_means2D_abs(means2D_abs, means3D, False, shape=(viewmatrices.size(0), means3D.size(0), 3))
        return _RasterizeGaussiansBatchFullAbs.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                                     cov3Ds_precomp, viewmatrices, gt_depths, raster_settings, means2D_abs)
    return _RasterizeGaussiansBatchFull.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                              viewmatrices, gt_depths, raster_settings)


class GaussianRasterizerBatchFull(torch.nn.Module):
    """The full variant's `GaussianRasterizer` over the V cameras of its settings."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, viewmatrices=None, gt_depths=None, *, means2D_abs=None):
        # means2D_abs (absgrad): a float32 [V,P,3] leaf whose .grad receives every view's absolute screen-space gradient
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        e = torch.Tensor([])
        shs = e if shs is None else shs
        colors_precomp = e if colors_precomp is None else colors_precomp
        scales = e if scales is None else scales
        rotations = e if rotations is None else rotations
        cov3D_precomp = e if cov3D_precomp is None else cov3D_precomp
        if viewmatrices is None:
            viewmatrices = self.raster_settings.viewmatrices
        return rasterize_gaussians_batch_full(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                              viewmatrices, gt_depths, self.raster_settings, means2D_abs=means2D_abs)
