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
  * they are views of one flat arena (`dgr_amd.light._grad_arena`), so `dgr_amd.multiview.GradientArena` finds the fused
    all-reduce span of a multi-GPU mapping step in them as it does for a one-view backward.

torch supplies device memory and the current stream; every compute call goes through the C ABI.  There is no CPU fallback.
"""
from typing import NamedTuple

import torch

from . import _binning, _capi
from . import light as _light

MAX_VIEWS = _capi.MAX_BATCH_VIEWS
_View, _ViewGrad = _capi.LightView, _capi.LightViewGrad
_lib = _capi.load


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


_row = _capi.row_ptr


def _ext():
    """the compiled torch extension (csrc/torch_ext.cpp: forward_batch<V> / backward_batch<V> -- allocation and
    marshalling in C++) when dgr_amd.light selected it, else None: the ctypes code below binds the same C ABI"""
    return _light._CompiledC.ext if _light._C is _light._CompiledC else None


def _forward_views(variant, View, outputs, V, bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                   viewmatrices, gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered):
    """The batch forward of both variants: the extension's <variant>_forward_batch when dgr_amd.light selected it, else
    dgr_<variant>_forward_batch through ctypes with `View` views; mode, capacity, retries and status words follow
    dgr_amd._binning.run_batch.  `outputs(V, P, H, W, f32, i32)` -> the variant's output tensors by their `View` field name, in
    the order of the extension's result, which carries the geometry, binning and image buffers after "radii".  Returns (per-view
    R for the backward, that result: the [V,4] status words, the outputs and the buffers)."""
    ext = _ext()
    P = means3D.size(0)

    def attempt(cap, lazy):
        if ext is not None:
            return getattr(ext, f"{variant}_forward_batch")(
                bg, means3D, colors, opacity, scales, rotations, float(scale_modifier), cov3D_precomp, viewmatrices, gt_depths,
                projmatrices, float(tanfovx), float(tanfovy), int(H), int(W), sh, int(degree), campos, bool(prefiltered), cap, lazy)
        return _attempt_ctypes(variant, View, outputs, bg, means3D, colors, opacity, scales, rotations, scale_modifier,
                               cov3D_precomp, viewmatrices, gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos,
                               prefiltered, cap, V), None
    return _binning.run_batch((means3D.device.index, P, H, W), P, V, attempt)


def _attempt_ctypes(variant, View, outputs, bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                    viewmatrices, gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered, cap, V):
    """One ctypes attempt of _forward_views with binning capacity `cap` per view; returns what the extension returns."""
    lib = _lib()
    dev = means3D.device
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    c = _light._f32c
    means3D, bg, colors, opacity = c(means3D, dev), c(bg, dev), c(colors, dev), c(opacity, dev)
    scales, rotations, cov3D_precomp, sh = c(scales, dev), c(rotations, dev), c(cov3D_precomp, dev), c(sh, dev)
    viewmatrices, projmatrices, campos, gt_depths = c(viewmatrices, dev), c(projmatrices, dev), c(campos, dev), c(gt_depths, dev)
    P = means3D.size(0)
    M = sh.size(1) if sh.numel() != 0 else 0
    out = outputs(V, P, H, W, f32, i32)
    geom = torch.empty((V, max(lib.dgr_geometry_bytes(P), 1)), **u8)
    img = torch.empty((V, max(lib.dgr_image_bytes(W, H), 1)), **u8)
    binning = torch.empty((V, max(lib.dgr_binning_bytes(cap, W, H), 1)), **u8)
    status = torch.zeros((V, 4), **i32)
    views = (View * V)()
    for v in range(V):
        w = views[v]
        w.geometry_buffer, w.binning_buffer, w.binning_capacity, w.image_buffer = _row(geom, v), _row(binning, v), cap, _row(img, v)
        w.status, w.viewmatrix, w.projmatrix, w.cam_pos = _row(status, v), _row(viewmatrices, v), _row(projmatrices, v), _row(campos, v)
        w.gt_depth = _row(gt_depths, v)
        for k, t in out.items():
            setattr(w, k, _row(t, v))
    p = _capi.ptr
    _light._check(getattr(lib, f"dgr_{variant}_forward_batch")(
        _capi.stream_handle(dev.index), V, views, P, int(degree), M, p(bg), W, H, p(means3D), p(sh), p(colors), p(opacity),
        p(scales), float(scale_modifier), p(rotations), p(cov3D_precomp), float(tanfovx), float(tanfovy), int(bool(prefiltered))))
    i, o = list(out).index("radii") + 1, list(out.values())
    return (status, *o[:i], geom, binning, img, *o[i:])


def _outputs(V, P, H, W, f32, i32):
    """The light batch's output tensors (_forward_views)."""
    mk = torch.empty if P else torch.zeros
    return {"out_color": torch.empty((V, 3, H, W), **f32), "out_depth": torch.empty((V, 1, H, W), **f32),
            "out_median_depth": torch.empty((V, 1, H, W), **f32), "out_depth_var": torch.empty((V, 1, H, W), **f32),
            "out_alpha": torch.empty((V, 1, H, W), **f32), "radii": mk((V, P), **i32), "gau_uncertainty": mk((V, P, 1), **f32),
            "gau_related_pixels": mk((V, P, 1), **i32)}


def _forward_batch(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, gt_depths,
                   projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered):
    """Returns (per-view R for the backward, color, depth, median, var, alpha, radii, geom, binning, img, unc, px)."""
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("dgr_hip runs on the GPU only (no CPU path exists, as in the reference)")
    V = viewmatrices.size(0)
    if not 1 <= V <= MAX_VIEWS:
        raise RuntimeError(f"1 .. {MAX_VIEWS} views per batch")
    R, out = _forward_views("light", _View, _outputs, V, bg, means3D, colors, opacity, scales, rotations, scale_modifier,
                            cov3D_precomp, viewmatrices, gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos,
                            prefiltered)
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
                _light._EMPTY if silhouette is None else silhouette, bool(absgrad))
        return tuple(ext.light_backward_batch(*args))
    if not need_gaussian_grads:
        map_off = True  # nobody reads the per-Gaussian sums: the blend kernels form the three pose sums only
    return _backward_views("light", _ViewGrad, {"alphas": alphas, "dL_dpix": gC, "dL_dpix_depth": gD, "dL_dpix_median_depth": gM,
                                                 "dL_dpix_depth_var": gV},
                           (int(bool(track_off)), int(bool(map_off))), bg, means3D, radii, colors, scales, rotations,
                           scale_modifier, cov3D_precomp, viewmatrices, projmatrices, tanfovx, tanfovy, gt_depths, sh, degree,
                           campos, geom, binning, img, perspec_matrix, need_gaussian_grads, need_means2D, num_rendered, absgrad,
                           silhouette)


def _backward_views(variant, ViewGrad, per_view, tail, bg, means3D, radii, colors, scales, rotations, scale_modifier,
                    cov3D_precomp, viewmatrices, projmatrices, tanfovx, tanfovy, gt_depths, sh, degree, campos, geom, binning,
                    img, perspec_matrix, need_gaussian_grads, need_means2D, num_rendered, absgrad, silhouette=None):
    """The ctypes batch backward of both variants: dgr_<variant>_backward_batch[_absgrad|_silhouette] with `ViewGrad` views
    (`silhouette`: every view's silhouette gradient image [V,1,H,W], or None).  `per_view`:
    the variant's own [V, ...] inputs by the view struct's field name (None: NULL; "dL_dpix" is the colour gradient [V,3,H,W]);
    `tail`: the entry point's arguments after the common ones.  Returns (dL_dmeans2D [V,P,3] or None, dL_dcolors, dL_dopacity,
    dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dL_dview [V,4,4]) and, with absgrad, every view's absolute
    screen-space gradient [V,P,3]."""
    lib = _lib()
    dev = means3D.device
    V, P = viewmatrices.size(0), means3D.size(0)
    H, W = per_view["dL_dpix"].size(2), per_view["dL_dpix"].size(3)
    f32 = dict(dtype=torch.float32, device=dev)
    c = _light._f32c
    means3D, bg, colors = c(means3D, dev), c(bg, dev), c(colors, dev)
    scales, rotations, cov3D_precomp, sh = c(scales, dev), c(rotations, dev), c(cov3D_precomp, dev), c(sh, dev)
    viewmatrices, projmatrices, campos = c(viewmatrices, dev), c(projmatrices, dev), c(campos, dev)
    gt_depths, perspec_matrix = c(gt_depths, dev), c(perspec_matrix, dev)
    per_view = {k: None if t is None else c(t, dev) for k, t in per_view.items()}
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
    views = (ViewGrad * V)()
    pp = _capi.ptr(perspec_matrix)
    for v in range(V):
        w = views[v]
        w.geometry_buffer, w.binning_buffer, w.image_buffer = _row(geom, v), _row(binning, v), _row(img, v)
        w.viewmatrix, w.projmatrix, w.cam_pos = _row(viewmatrices, v), _row(projmatrices, v), _row(campos, v)
        w.perspec_matrix = _row(perspec_matrix, v) if perspec_matrix.dim() == 3 else pp
        w.gt_depth, w.radii = _row(gt_depths, v), _row(radii, v)
        for k, t in per_view.items():
            setattr(w, k, _row(t, v))
        w.dL_dmean2D, w.dL_dview, w.scratch, w.scratch_bytes = _row(d2, v), _row(dview, v), _row(scratch, v), nscr
        w.num_rendered = num_rendered[v]
    p = _capi.ptr
    args = (_capi.stream_handle(dev.index), V, views, P, int(degree), M, p(bg), W, H, p(means3D), p(sh), p(colors), p(scales),
            float(scale_modifier), p(rotations), p(cov3D_precomp), float(tanfovx), float(tanfovy), p(dop), p(dcol), p(d3), p(dcov),
            p(dsh), p(dsc), p(drot)) + tail
    out = (d2, dcol, dop, d3, dcov, dsh, dsc, drot, dview)
    dabs = torch.empty((V, P, 3), **f32) if absgrad else None
    _light._check(_capi.call_backward(variant, V, args, dabs, None if silhouette is None else c(silhouette, dev)))
    return out + (dabs,) if absgrad else out


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
        (num_rendered, color, depth, depth_median, depth_var, opacity_map, radii, geom, binning, img, unc, px) = out
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        ctx.absgrad = means2D_abs is not None
        ctx.dgr_options = _capi.load().dgr_thread_options_effective()  # the backward runs under the forward's options
        ctx.silhouette = _capi.silhouette_on(ctx.dgr_options)
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrices, radii, sh, geom, binning,
                              img, opacity_map, gt_depths)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii, px)
        return color, radii, depth, depth_median, depth_var, opacity_map, unc, px

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_depth_median, grad_depth_var, grad_alpha, grad_unc, grad_px):
        rs = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrices, radii, sh, geom, binning, img, opacity_map,
         gt_depths) = ctx.saved_tensors
        V, H, W = viewmatrices.size(0), int(rs.image_height), int(rs.image_width)
        zeros = lambda ch: torch.zeros((V, ch, H, W), dtype=torch.float32, device=means3D.device)  # noqa: E731
        absgrad = ctx.absgrad
        grad_color = zeros(3) if grad_color is None else grad_color
        grad_depth = zeros(1) if grad_depth is None else grad_depth
        grad_depth_median = zeros(1) if grad_depth_median is None else grad_depth_median
        grad_depth_var = zeros(1) if grad_depth_var is None else grad_depth_var
        need = ctx.needs_input_grad
        with _capi.on_device(means3D.device), _capi.under_options(ctx.dgr_options):
            g = _backward_batch(
                rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, viewmatrices,
                rs.projmatrices, rs.tanfovx, rs.tanfovy, grad_color, grad_depth, grad_depth_median, grad_depth_var, gt_depths, sh,
                rs.sh_degree, rs.campos, geom, binning, img, opacity_map, rs.perspec_matrix, rs.track_off, rs.map_off,
                need_gaussian_grads=any(need[:8]) or absgrad, need_means2D=bool(need[1]), num_rendered=ctx.num_rendered,
                absgrad=absgrad, silhouette=grad_alpha if ctx.silhouette else None)
        (g2, gcol, gop, g3, gcov, gsh, gsc, grot, gview) = g[:9]
        _light._consume_post_backward_wait()
        return g3, g2, gsh, gcol, gop, gsc, grot, gcov, gview, None, None, g[9] if absgrad else None


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
        # means2D_abs (absgrad): a float32 [V,P,3] leaf whose .grad receives every view's absolute screen-space gradient
        # (dgr_amd.light.GaussianRasterizer.forward)
        shs, colors_precomp, scales, rotations, cov3D_precomp = _light._checked_inputs(shs, colors_precomp, scales, rotations,
                                                                                       cov3D_precomp)
        if viewmatrices is None:
            viewmatrices = self.raster_settings.viewmatrices
        if means2D_abs is not None:
            _light.check_means2D_abs(means2D_abs, means3D, self.raster_settings.map_off,
                                     shape=(viewmatrices.size(0), means3D.size(0), 3))
            return _RasterizeGaussiansBatch.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                                  cov3D_precomp, viewmatrices, gt_depths, self.raster_settings, means2D_abs)
        return rasterize_gaussians_batch(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                         viewmatrices, gt_depths, self.raster_settings)
