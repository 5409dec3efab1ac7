"""The caller's side of the rasterizer: CG-SLAM's `render()` and the camera tensors a tracking or
mapping step feeds it.

The reference repository documents this call but does not contain it (README.md:33-47, 71-96: `render(viewpoint_cam,
gaussians, pipe, background, viewmatrix=w2cT, fov=(tanfovx, tanfovy), HW=(H, W), gt_depth=..., track_off=...,
map_off=...)` returning a dict); it lives in CG-SLAM and follows the 3DGS `gaussian_renderer.render`.  This module
restates it over `dgr_amd.light` / `dgr_amd.full`, duck-typed on the 3DGS `GaussianModel` accessors, and adds the
differentiable pose -> matrices helpers, so that a whole tracking iteration (pose parameters -> viewmatrix -> render ->
loss -> backward -> pose update) can run without leaving the GPU.

Matrix convention (cuda_rasterizer/auxiliary.h:58-77 reads 16 floats column-major): the rasterizer takes W2C^T,
(Proj W2C)^T and Proj^T.  The analytic pose gradient is returned w.r.t. the `viewmatrix` tensor only; `projmatrix` and
`campos` are recomputed from the same pose but enter as constants, exactly as in the reference (its backward adds their
dependence inside the kernels: L/cuda_rasterizer/backward.cu:633-651, 683-751).
"""
import contextlib as _contextlib
from collections.abc import Mapping as _Mapping

import torch

from . import full as _full
from . import light as _light
from .contrib import ContributionAccumulator, ContributionStats, contribution_stats, render_contributions  # noqa: F401
from .fusion import TsdfMesh, TsdfRaycast, TsdfVolume, extract_mesh, tsdf_bricks, tsdf_integrate, tsdf_raycast  # noqa: F401
from .icp import IcpResult, depth_normals, icp_align  # noqa: F401
from .knn import KnnIndex, KnnResult, dist2, knn_build, knn_search  # noqa: F401
from .gicp import (GicpResult, PointCovariances, gaussian_covariances, gicp_align, gicp_step, point_covariances,  # noqa: F401
                   unproject_depth)
from .keyframes import KeyframeOverlap, keyframe_overlap, select_keyframes  # noqa: F401  (slam.X stays the public name)
from .posegraph import PgoPlan, PgoResult, pose_graph_optimize, pose_graph_plan, relative_pose  # noqa: F401
from .losses import MaskedLossStats, l1_loss, l1_ssim_loss, masked_l1_loss, ssim  # noqa: F401
from .rgbd import RgbdResult, halve_frame, intensity_map, level_intrinsics, rgbd_align  # noqa: F401
from .pose import (_Kept, _cameras_of, camera_tensors, pose_to_camera, projection_matrix, quat_to_rotmat,  # noqa: F401
                   w2c_from_quat_trans)


def _get(obj, name, default=None):
    v = getattr(obj, name, default)
    return v() if callable(v) and not isinstance(v, torch.Tensor) else v


_VIEWS_CACHE = _Kept(4)    # render_views: camera tensors of the last few keyframe batches (see there)
_VIEW_CACHE = _Kept(16)    # render: the same for single fixed poses
_ZERO_POINTS = _Kept(16)   # (device, P) -> a [P, 3] zero tensor for calls whose screen-space gradient nobody reads (tracking)


def _result(out, screenspace_points, abs_points):
    """The dict of `render()` / `render_views()` from the rasterizer's output tuple (eight entries: light; four: full)."""
    if len(out) == 8:
        color, radii, depth, depth_median, depth_var, opacity_map, gau_uncertainty, gau_related_pixels = out
        res = {"render": color, "depth": depth, "depth_median": depth_median, "opacity_map": opacity_map,
               "depth_var": depth_var, "gau_uncertainty": gau_uncertainty, "num_related_pixels": gau_related_pixels}
    else:
        color, radii, depth, uncertainty = out
        res = {"render": color, "depth": depth, "opacity_map": uncertainty}
    res.update(viewspace_points=screenspace_points, visibility_filter=radii > 0, radii=radii)
    if abs_points is not None:
        res["viewspace_points_abs"] = abs_points
    return res


def render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None, viewmatrix=None, fov=None,
           HW=None, gt_depth=None, track_off=False, map_off=False, variant="light", pose_tensors=None, absgrad=False,
           complete_pose=False, silhouette_grad=False):
    """CG-SLAM's `render()` (reference README.md:33,71).

    `pc`: anything with the 3DGS GaussianModel accessors `get_xyz`, `get_opacity`, `get_scaling`, `get_rotation`,
    `get_features` ([P, M, 3]) and `active_sh_degree`.  `viewmatrix` is W2C^T (differentiable for tracking); `fov` the
    two half-angle tangents; `HW` = (H, W).  `viewpoint_camera` may carry `projection_matrix` (Proj^T), `znear`, `zfar`;
    without it a symmetric frustum with znear 0.01 / zfar 100 is used.  `pipe.debug` is honoured.
    `pose_tensors` = what `pose_to_camera(q, t, ...)` returned for this `viewmatrix` -- (viewmatrix, projmatrix, perspec_matrix,
    campos): the projection, the full projection and the camera centre are then taken from there instead of being formed again
    from `viewmatrix` with a dozen small torch kernels (a 640x480 tracking iteration is bound by exactly those).
    Returns the reference's dict (light: render, depth, depth_median, opacity_map, depth_var, gau_uncertainty,
    num_related_pixels; full: render, depth, opacity_map) plus the 3DGS bookkeeping entries viewspace_points,
    visibility_filter, radii.  `absgrad=True` (AbsGS densification, a mapping render) adds `viewspace_points_abs`, a zero leaf
    shaped like `viewspace_points` whose `.grad` receives the absolute screen-space gradient (GaussianRasterizer.forward's
    `means2D_abs`): feed it to `optim.add_densification_stats` in place of `viewspace_points.grad`.
    `complete_pose=True`: the backward returns the complete pose gradient (library option "pose_grad" = 1: the view-matrix
    counterpart of the Gaussians' dL_dmeans3D, with the 2D-covariance, colour and depth terms the reference leaves out) instead
    of the reference's; the forward runs under it and its backward follows.  The campos used is the one formed from
    `viewmatrix` here (or `pose_tensors`), which is what makes the colour term exact.
    `silhouette_grad=True`: `res["opacity_map"]` carries the exact gradient of the silhouette sum alpha T in both variants
    (library option "silhouette_grad" = 1): a mask or opacity loss on it trains the Gaussians and the pose, instead of being
    dropped (light) or taken as the full variant's depth variance.  The full variant's pose gradient receives it only
    together with `complete_pose=True` (include/dgr_hip.h)."""
    if viewmatrix is None or fov is None or HW is None:
        raise ValueError("render() needs viewmatrix=W2C^T, fov=(tanfovx, tanfovy) and HW=(H, W)")
    mod = _light if variant == "light" else _full
    H, W = int(HW[0]), int(HW[1])
    tanfovx, tanfovy = float(fov[0]), float(fov[1])
    dev = viewmatrix.device
    znear = float(_get(viewpoint_camera, "znear", 0.01)) if viewpoint_camera is not None else 0.01
    zfar = float(_get(viewpoint_camera, "zfar", 100.0)) if viewpoint_camera is not None else 100.0
    if pose_tensors is not None:
        vm = viewmatrix.detach()
        projmatrix, perspec, campos = pose_tensors[1].detach(), pose_tensors[2], pose_tensors[3].detach()
    else:
        perspec_src = _get(viewpoint_camera, "projection_matrix") if viewpoint_camera is not None else None
        # a fixed keyframe pose (mapping) is rendered again and again: its derived tensors are kept while `viewmatrix` is the
        # same object at the same version (render_views does the same for a batch); a pose under optimisation is a new
        # tensor every iteration and is not kept; never while a hipGraph is being recorded (a replay re-derives them)
        keep = (not viewmatrix.requires_grad and viewmatrix.is_cuda and not torch.cuda.is_current_stream_capturing())
        key = (id(viewmatrix), viewmatrix._version, id(perspec_src), getattr(perspec_src, "_version", 0), tanfovx, tanfovy,
               znear, zfar) if keep else None
        hit = _VIEW_CACHE.get(key) if keep else None
        if hit is None:
            with torch.no_grad():
                hit = _cameras_of(viewmatrix.detach(), perspec_src, tanfovx, tanfovy, znear, zfar)
            if keep:  # (the sources too: ids are unique among live objects)
                _VIEW_CACHE.put(key, hit + (viewmatrix, perspec_src), dev)
        perspec, vm, projmatrix, campos = hit[:4]

    means3D = pc.get_xyz
    # 3DGS keeps a zero tensor whose .grad receives the screen-space gradient (densification statistics).  A tracking
    # step (map_off, or a map that carries no gradients) has no use for it, and without it the backward can skip every
    # per-Gaussian gradient row (dgr_amd.light: need_gaussian_grads).
    shs_or_colors = override_color if override_color is not None else pc.get_features
    opacity, scaling, rotation = pc.get_opacity, pc.get_scaling, pc.get_rotation
    mapping = (variant != "light" or not map_off) and any(
        t.requires_grad for t in (means3D, shs_or_colors, opacity, scaling, rotation))
    if mapping:
        screenspace_points = torch.zeros_like(means3D, requires_grad=True)
    else:  # never read, never written: one shared zero tensor per size instead of a fill per call
        key = (means3D.device, means3D.shape[0])
        screenspace_points = _ZERO_POINTS.get(key)
        if screenspace_points is None:
            screenspace_points = _ZERO_POINTS.put(key, torch.zeros_like(means3D), means3D.device)
    debug = bool(getattr(pipe, "debug", False)) if pipe is not None else False
    common = dict(image_height=H, image_width=W, tanfovx=tanfovx, tanfovy=tanfovy, bg=bg_color,
                  scale_modifier=scaling_modifier, viewmatrix=vm, projmatrix=projmatrix,
                  sh_degree=int(pc.active_sh_degree), campos=campos, prefiltered=False)
    if variant == "light":
        settings = mod.GaussianRasterizationSettings(**common, debug=debug, perspec_matrix=perspec, track_off=track_off,
                                                     map_off=map_off)
    else:
        settings = mod.GaussianRasterizationSettings(**common, perspec_matrix=perspec)
    rasterizer = mod.GaussianRasterizer(raster_settings=settings)
    shs, colors = (None, override_color) if override_color is not None else (shs_or_colors, None)
    abs_points = torch.zeros_like(means3D, requires_grad=True) if absgrad else None  # (None: the call is the plain one)
    with _pose_mode(complete_pose, silhouette_grad):
        out = rasterizer(means3D=means3D, means2D=screenspace_points, opacities=opacity, shs=shs, colors_precomp=colors,
                         scales=scaling, rotations=rotation, cov3D_precomp=None, viewmatrix=viewmatrix, gt_depth=gt_depth,
                         means2D_abs=abs_points)
    return _result(out, screenspace_points, abs_points)


def _pose_mode(complete_pose, silhouette_grad=False):
    """The block's rasterizer calls under pose_grad = 1 and / or silhouette_grad = 1 (their backwards follow through the
    forward's options snapshot)."""
    modes = dict(pose_grad=1) if complete_pose else {}
    if silhouette_grad:
        modes["silhouette_grad"] = 1
    if not modes:
        return _contextlib.nullcontext()
    from . import _capi
    return _capi.thread_options(**modes)


def render_views(cameras, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None, track_off=False, map_off=False,
                 variant="light", absgrad=False, complete_pose=False, silhouette_grad=False):
    """`render()` for the V cameras of a keyframe batch in ONE call of the batched entry points (`dgr_amd.batch`, SURVEY.md
    s8(f) item 2; `variant="full"`: `dgr_amd.batch_full`): the cameras share `fov` and `HW` (one sensor, V poses), every
    per-view entry of `render()`'s dict comes back with a leading view dimension, and one backward through it yields the
    Gaussians' gradients already summed over the views, the pose gradient per `viewmatrix` and `viewspace_points.grad`
    ([V,P,3]) per view.  `cameras`: sequence of dicts with `viewmatrix` (W2C^T), `fov`, `HW`, `gt_depth` and optionally
    `viewpoint_camera`.  The full variant has no track_off / map_off.  `absgrad=True`: as in `render()`, with
    `viewspace_points_abs` [V,P,3].  `complete_pose=True`: every view's pose gradient is the complete one, as in `render()`.
    `silhouette_grad=True`: every view's `opacity_map` carries the exact silhouette gradient, as in `render()`."""
    from . import batch as _batch
    if variant not in ("light", "full"):
        raise ValueError(f"unknown variant {variant!r}")
    if variant == "full" and (track_off or map_off):
        raise ValueError("the full variant has no track_off / map_off")
    cameras = list(cameras)
    if not 1 <= len(cameras) <= _batch.MAX_VIEWS:
        raise ValueError(f"1 .. {_batch.MAX_VIEWS} cameras per call")
    c0 = cameras[0]
    H, W = int(c0["HW"][0]), int(c0["HW"][1])
    tanfovx, tanfovy = float(c0["fov"][0]), float(c0["fov"][1])
    for c in cameras[1:]:
        if (int(c["HW"][0]), int(c["HW"][1])) != (H, W) or (float(c["fov"][0]), float(c["fov"][1])) != (tanfovx, tanfovy):
            raise ValueError("the cameras of a batch share fov and HW")
    cam0 = c0.get("viewpoint_camera")
    znear = float(_get(cam0, "znear", 0.01)) if cam0 is not None else 0.01
    zfar = float(_get(cam0, "zfar", 100.0)) if cam0 is not None else 100.0
    gts = [c.get("gt_depth") for c in cameras]
    if any(g is None for g in gts):
        raise ValueError(f"the {variant} variant's batch needs gt_depth for every camera")
    vms = [c["viewmatrix"] for c in cameras]
    perspec_src = _get(cam0, "projection_matrix") if cam0 is not None else None
    # A mapping loop renders the same keyframes iteration after iteration: the camera tensors derived from the poses (a dozen
    # small launches) are kept while the tensors they were made from are the same objects at the same version -- an optimiser
    # step on a pose, or a new depth image, changes the key.
    key = (H, W, tanfovx, tanfovy, znear, zfar, id(perspec_src), getattr(perspec_src, "_version", 0),
           tuple((id(v), v._version, id(g), g._version) for v, g in zip(vms, gts)))
    # (never while a hipGraph is being recorded: a replay must re-derive the cameras from whatever the poses hold then)
    capturing = vms[0].is_cuda and torch.cuda.is_current_stream_capturing()
    hit = None if capturing else _VIEWS_CACHE.get(key)
    if hit is None:
        with torch.no_grad():
            # (the operations of render(), in a fixed order: the cameras -- hence the images -- are those of the one-view
            #  path bit for bit)
            hit = _cameras_of(torch.stack([v.detach() for v in vms]), perspec_src, tanfovx, tanfovy, znear, zfar)
            hit += (torch.stack([g.reshape(H, W) for g in gts]),)
        # (the sources are held too: an id() is only unique among live objects)
        _VIEWS_CACHE.put(key, hit + (list(vms), list(gts), perspec_src), vms[0].device)
    perspec, vm, projmatrices, campos, gt_depths = hit[:5]
    dev = vm.device
    # (differentiable where a pose is a leaf: every pose keeps its gradient)
    viewmatrices = torch.stack(vms) if any(v.requires_grad for v in vms) else vm
    means3D = pc.get_xyz
    shs_or_colors = override_color if override_color is not None else pc.get_features
    opacity, scaling, rotation = pc.get_opacity, pc.get_scaling, pc.get_rotation
    mapping = not map_off and any(t.requires_grad for t in (means3D, shs_or_colors, opacity, scaling, rotation))
    screenspace_points = torch.zeros((len(cameras),) + tuple(means3D.shape), dtype=means3D.dtype, device=dev, requires_grad=mapping)
    # (absgrad: a [V,P,3] leaf of its own; None leaves the calls below as they are)
    abs_points = torch.zeros_like(screenspace_points, requires_grad=True) if absgrad else None
    debug = bool(getattr(pipe, "debug", False)) if pipe is not None else False
    settings = _batch.BatchRasterizationSettings(
        image_height=H, image_width=W, tanfovx=tanfovx, tanfovy=tanfovy, bg=bg_color, scale_modifier=scaling_modifier,
        viewmatrices=vm, projmatrices=projmatrices, sh_degree=int(pc.active_sh_degree), campos=campos, prefiltered=False,
        debug=debug, perspec_matrix=perspec, track_off=track_off, map_off=map_off)
    shs, colors = (None, override_color) if override_color is not None else (shs_or_colors, None)
    if variant == "full":
        from .batch_full import GaussianRasterizerBatchFull as rasterizer
    else:
        rasterizer = _batch.GaussianRasterizerBatch
    with _pose_mode(complete_pose, silhouette_grad):
        out = rasterizer(settings)(means3D, screenspace_points, opacity, shs=shs, colors_precomp=colors, scales=scaling,
                                   rotations=rotation, viewmatrices=viewmatrices, gt_depths=gt_depths, means2D_abs=abs_points)
    return _result(out, screenspace_points, abs_points)


class _ViewOf(_Mapping):
    """View k of `render_views`' dict: entry n is `out[n][k]`, sliced when it is first asked for (a loss reads two or three
    of the ten; every slice is an autograd node and a launch-free but not cost-free call) -- except `viewspace_points` (and
    `viewspace_points_abs`, with absgrad), which stays the whole [V,P,3] tensor: one backward fills every view's slice."""
    _NAMES = ("render", "depth", "depth_median", "opacity_map", "depth_var", "gau_uncertainty", "num_related_pixels",
              "visibility_filter", "radii", "viewspace_points")
    _FULL_NAMES = ("render", "depth", "opacity_map", "visibility_filter", "radii", "viewspace_points")  # (variant="full")

    def __init__(self, out, k):
        self._out, self._k, self._got = out, k, {}
        self._names = self._NAMES if "depth_median" in out else self._FULL_NAMES
        if "viewspace_points_abs" in out:
            self._names = self._names + ("viewspace_points_abs",)

    def __getitem__(self, n):
        v = self._got.get(n)
        if v is None:
            if n not in self._names:
                raise KeyError(n)
            whole = n == "viewspace_points" or n == "viewspace_points_abs"
            v = self._got[n] = self._out[n] if whole else self._out[n][self._k]
        return v

    def __iter__(self):
        return iter(self._names)

    def __len__(self):
        return len(self._names)


def render_batch_fused(cameras, pc, pipe, bg_color, loss_fn, batch_loss_fn=None, absgrad=False, silhouette_grad=False,
                       **render_kwargs):
    """`render_batch` through ONE batched forward and ONE batched backward (`render_views`): `loss_fn(out_k, k)` sees the
    dict of view k (slices of the batched outputs), the losses are summed and back-propagated once.  Same gradients as
    `render_batch` -- the sum over the keyframes in the Gaussians' `.grad`, one pose gradient per `viewmatrix` -- without V - 1
    accumulation passes over the dense gradient rows and with the camera-independent per-Gaussian work done once.
    `batch_loss_fn(out)`, if given, replaces the V calls of `loss_fn`: it sees the batched dict and returns the SUM of the
    views' losses as one scalar (then the returned list holds that one value).  `variant="full"` (a render_kwargs entry) renders
    through the full variant's batch.  `absgrad=True`: the returned dict carries `viewspace_points_abs` (render_views).
    `complete_pose=True` (a render_kwargs entry) passes through to `render_views`: complete pose gradients.
    `silhouette_grad=True`: the exact silhouette gradient of every view's `opacity_map` (render_views)."""
    if silhouette_grad:
        render_kwargs["silhouette_grad"] = True
    if absgrad:
        render_kwargs["absgrad"] = True
    out = render_views(cameras, pc, pipe, bg_color, **render_kwargs)
    if batch_loss_fn is not None:
        # ONE loss over the stacked outputs ([V,3,H,W], [V,1,H,W], ...): no per-view slice in the graph -- each is a node whose
        # backward zero-fills a tensor of the whole stack's size -- and one reduction instead of V
        total = batch_loss_fn(out)
        total.backward()
        return [total.detach()], out
    losses = [loss_fn(_ViewOf(out, k), k) for k in range(out["render"].size(0))]
    torch.stack(losses).sum().backward()
    return [l_.detach() for l_ in losses], out


def render_batch(cameras, pc, pipe, bg_color, loss_fn, views_in_flight=3, absgrad=False, silhouette_grad=False,
                 **render_kwargs):
    """One mapping step over a batch of keyframes: every camera is rendered, `loss_fn(out, k)`
    is evaluated on its output dict and back-propagated, each view's forward + loss + backward on its own HIP stream
    (`dgr_amd.multiview.ViewStreams`) so that the views overlap on the GPU; gradients accumulate in the `.grad` of the
    Gaussian parameters as usual.  Accumulation into a shared `.grad` from several streams needs an explicit order
    (PyTorch gives none): every view's backward waits for the end of the previous view (`views.before_backward()`), its
    forward and loss still overlap the previous view's backward.  `cameras`: sequence of dicts with `viewmatrix`
    (W2C^T), `fov`, `HW` and optionally `gt_depth`, `viewpoint_camera`.  Returns the list of detached loss values
    (device tensors); the caller's stream is ordered after all views on return.  `absgrad=True`: every view's dict carries
    `viewspace_points_abs` (render()), which `loss_fn` may keep for the densification statistics.  `silhouette_grad=True`: every
    view's `opacity_map` carries the exact silhouette gradient (render())."""
    if absgrad:
        render_kwargs["absgrad"] = True
    if silhouette_grad:
        render_kwargs["silhouette_grad"] = True
    from .multiview import ViewStreams
    cameras = list(cameras)
    if not cameras:
        return []
    views = ViewStreams(min(max(1, views_in_flight), len(cameras)), cameras[0]["viewmatrix"].device)

    def one_view(k, cam):  # (a function: no autograd graph of one view is kept alive into the next)
        out = render(cam.get("viewpoint_camera"), pc, pipe, bg_color, viewmatrix=cam["viewmatrix"], fov=cam["fov"],
                     HW=cam["HW"], gt_depth=cam.get("gt_depth"), **render_kwargs)
        loss = loss_fn(out, k)
        views.before_backward()
        loss.backward()
        return loss.detach()

    losses = []
    for k, cam in enumerate(cameras):
        with views.next():
            losses.append(one_view(k, cam))
    views.join()
    return losses
