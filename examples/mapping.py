#!/usr/bin/env python3
"""Mapping against a window of keyframes (CG-SLAM's mapping loop in miniature).

A synthetic map rendered from K poses gives the keyframes' observed colour and depth; a degraded copy of the map
(jittered positions, flattened colours, wrong opacities) is then refined.  One iteration =
  slam.render_batch      every keyframe's forward + loss + backward on its own HIP stream (light variant, track_off=True:
                         no pose gradient), gradients summed into the parameters' .grad
  add_densification_stats 3DGS's per-view bookkeeping (screen-space gradient norm, view count, largest radius), one launch
  SparseAdam.step        fused Adam over the rows some keyframe saw, one launch per tensor
all on the GPU, no host synchronisation inside the loop.  --densify-every N adds the step that changes the number of
Gaussians: every N iterations densify_and_prune consumes the statistics (clone, split, prune; three launches and one host read
for the whole model and its Adam moments) and the loop goes on with the new leaves.  --fused renders the keyframe batch through the batched entry points
instead (slam.render_batch_fused: one forward and one backward call for all keyframes, gradients summed in the kernels).
--variant full runs the same loop through the -full variant (uncertainty output; it has no track_off, so the pose gradients are
formed and left unused).  --ssim LAMBDA optimises the standard 3DGS mapping loss instead of plain L1: (1 - LAMBDA) L1 + LAMBDA (1 - SSIM)
on the colour images plus the depth L1 (slam.l1_ssim_loss: at most three launches forward, two backward, capturable).
--seed starts from an EMPTY map instead of the degraded copy: keyframe 0's observed colour and depth are unprojected into
Gaussians (optim.seed_from_frame: three launches and one host read for every leaf, moment and accumulator), and each further
keyframe is rendered before it joins the window and seeded where its silhouette (opacity_map) shows the map does not explain it.
--masked gives the observed depth the holes of a real sensor (0 where the true map does not cover the pixel) and optimises the
masked loss in its mapping form (slam.masked_l1_loss(mask_color=False): the depth term over the valid pixels whose error is at most
10 x the keyframe's median error, the colour term over every pixel); with --seed a joining keyframe is also seeded where the
rendered depth lies more than 50 x the median depth error behind the sensor's (`stats.median * 50`, a device tensor: no host read).
--select K treats the --keyframes poses as the session's keyframe POOL (one of which, as in a real session, looks at another part
of the room) and maps against a window of K of them: the newest keyframe and the K - 1 that overlap it most
(slam.keyframe_overlap: one launch scores the whole pool on the device; slam.select_keyframes: the top scores, read once).

--relocate-every N keeps a map of FIXED size healthy instead (3DGS-MCMC): every N iterations optim.relocate_dead moves each dead
Gaussian (opacity below --relocate-min-opacity) onto a live one drawn in proportion to its opacity and recomputes the copies'
opacity and scale (--relocate-start K: not before iteration K, the method's warm-up); --position-noise adds the gated SGLD noise after it (optim.inject_position_noise).  Neither changes P, reallocates
a tensor or reads anything on the host, so both go together with --graph and --fused: the step runs between replays, with no
re-recording.  The logged counts are the step's one host read.

--loop-close-at N (with --seed) is the pose-graph update of a SLAM back end: every keyframe is seeded before the first iteration,
each Gaussian remembering its keyframe in the role-less leaf "anchor" (seed_from_frame's `fill`); after iteration N the keyframes'
poses get seeded rigid corrections and optim.transform_map moves every Gaussian, with its Adam moments, by the correction of its
keyframe (optim.pose_corrections forms them from the old and new poses on the device).  In place and without a host read: it goes
together with --graph and --fused, between replays.  The losses before and after are logged.

--prune-unseen N (with --densify-every or --relocate-every) prunes by what the keyframes actually BLEND: every N iterations each
keyframe of the window goes through slam.render_contributions into one ContributionAccumulator, and the Gaussians that fewer than
--prune-min-views M keyframes observed (blended by at least one pixel: occluded and never-seen Gaussians, which get no gradient
and so never lose their opacity) have their opacity logit set far below the pruning threshold; that iteration's densify_and_prune
removes them, or its relocate_dead recycles them.  The count is logged.  Not together with --graph.

--tsdf VOXEL hands the run's result over as a surface: after the last iteration the window's keyframes are rendered once more,
their depth and colour are fused into a truncated signed distance volume of that voxel size around the map
(slam.tsdf_integrate: every keyframe in ONE pass over the volume, mask_image = the render's opacity_map) and the zero level is
extracted by marching tetrahedra (slam.extract_mesh); one line reports the volume, the triangles and their area.
--mesh-out PATH writes that mesh as an ASCII PLY (from the host, with numpy).
--raycast (with --tsdf) then looks at the fused volume from the fused keyframes' poses (slam.tsdf_raycast, all of them in one
launch) and reports the share of pixels that hit the surface and the mean |rendered depth - ray-cast depth| where both are valid:
how far the Gaussians' depth lies from the surface fused from it.
--knn-scale (with --seed) gives the Gaussians a seeding adds 3DGS's initial scale: log-scale = 0.5 log(max(dist2, 1e-7)), dist2 the
mean squared distance to the three nearest Gaussians of the whole map (slam.dist2, the distCUDA2 of simple-knn), written into the
new rows in place (their Adam moments are zero already).

  python examples/mapping.py [--graph] [--fused] [--variant light|full] [--absgrad] [--densify-every N] [--iters 100]
                             [--keyframes 4] [--ssim LAMBDA] [--seed] [--masked] [--select K]
                             [--relocate-every N [--relocate-start K] [--position-noise] [--relocate-min-opacity 0.005]]
                             [--loop-close-at N [--loop-close-seed S]] [--prune-unseen N [--prune-min-views M]]
                             [--tsdf VOXEL [--mesh-out PATH] [--raycast]] [--knn-scale]

--absgrad feeds the densification statistics with AbsGS's absolute screen-space gradient (`viewspace_points_abs.grad`) instead
of 3DGS's `viewspace_points.grad`; the densify step then uses a threshold 4x higher (0.0008 for 0.0002).
                             [--width 640 --height 480 --gaussians 100000]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


class MapModel:
    """3DGS's GaussianModel reduced to what a mapping step touches: raw leaves + the activations render() reads."""

    def __init__(self, s, dev, degrade=None):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        xyz, opac, scal, rot, shs = t(s.means), t(s.opac), t(s.scales), t(s.rots), t(s.shs)
        if degrade is not None:
            g = torch.Generator(device="cpu").manual_seed(degrade)
            xyz = xyz + 0.15 * scal.mean(1, keepdim=True) * torch.randn(xyz.shape, generator=g).to(dev)
            shs = shs * 0.5
            opac = (opac * 0.6).clamp(0.02, 0.98)
        opac = opac.clamp(1e-4, 1 - 1e-4)
        self._xyz = xyz.clone().requires_grad_()
        self._features = shs.clone().requires_grad_()
        self._opacity = torch.log(opac / (1 - opac)).requires_grad_()      # inverse sigmoid
        self._scaling = torch.log(scal).requires_grad_()
        self._rotation = rot.clone().requires_grad_()
        self.active_sh_degree = 3
        P = xyz.shape[0]
        self.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        self.denom = torch.zeros((P, 1), device=dev)
        self.max_radii2D = torch.zeros(P, device=dev)

    get_xyz = property(lambda self: self._xyz)
    get_features = property(lambda self: self._features)
    get_opacity = property(lambda self: torch.sigmoid(self._opacity))
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: torch.nn.functional.normalize(self._rotation))

    def leaves(self):
        """name -> raw leaf, under the role names densify_and_prune looks for"""
        return {"xyz": self._xyz, "features": self._features, "opacity": self._opacity, "scaling": self._scaling,
                "rotation": self._rotation}

    def replace(self, leaves, xyz_gradient_accum, denom, max_radii2D):
        self._xyz, self._features, self._opacity = leaves["xyz"], leaves["features"], leaves["opacity"]
        self._scaling, self._rotation = leaves["scaling"], leaves["rotation"]
        self.xyz_gradient_accum, self.denom, self.max_radii2D = xyz_gradient_accum, denom, max_radii2D

    def groups(self):
        return [{"params": [self._xyz], "lr": 1.6e-4}, {"params": [self._features], "lr": 2.5e-3},
                {"params": [self._opacity], "lr": 5e-2}, {"params": [self._scaling], "lr": 5e-3},
                {"params": [self._rotation], "lr": 1e-3}]


class SeededMapModel(MapModel):
    """A MapModel that starts empty and grows by seed_from_frame.  3DGS's own leaves: the SH coefficients are split into the
    degree-0 ones (f_dc, which a seed takes from the observed colour) and the rest."""

    def __init__(self, dev, anchored=False):
        empty = lambda *shape: torch.zeros(shape, device=dev).requires_grad_()  # noqa: E731
        self._anchor = torch.zeros(0, device=dev) if anchored else None  # the keyframe each Gaussian was seeded from (no gradient)
        self._xyz, self._f_dc, self._f_rest = empty(0, 3), empty(0, 1, 3), empty(0, 15, 3)
        self._opacity, self._scaling, self._rotation = empty(0, 1), empty(0, 3), empty(0, 4)
        self.active_sh_degree = 3
        self.xyz_gradient_accum = torch.zeros((0, 1), device=dev)
        self.denom = torch.zeros((0, 1), device=dev)
        self.max_radii2D = torch.zeros(0, device=dev)

    get_features = property(lambda self: torch.cat([self._f_dc, self._f_rest], dim=1))

    def leaves(self):
        leaves = {"xyz": self._xyz, "f_dc": self._f_dc, "f_rest": self._f_rest, "opacity": self._opacity, "scaling": self._scaling,
                  "rotation": self._rotation}
        return leaves if self._anchor is None else dict(leaves, anchor=self._anchor)

    def replace(self, leaves, xyz_gradient_accum, denom, max_radii2D):
        self._xyz, self._f_dc, self._f_rest = leaves["xyz"], leaves["f_dc"], leaves["f_rest"]
        self._opacity, self._scaling, self._rotation = leaves["opacity"], leaves["scaling"], leaves["rotation"]
        self._anchor = leaves.get("anchor")
        self.xyz_gradient_accum, self.denom, self.max_radii2D = xyz_gradient_accum, denom, max_radii2D

    def groups(self):
        return [{"params": [self._xyz], "lr": 1.6e-4}, {"params": [self._f_dc], "lr": 2.5e-3},
                {"params": [self._f_rest], "lr": 2.5e-3 / 20}, {"params": [self._opacity], "lr": 5e-2},
                {"params": [self._scaling], "lr": 5e-3}, {"params": [self._rotation], "lr": 1e-3}]


def mapping_loop(dev, P, W, H, keyframes, iters, views_in_flight=3, log=None, graph=False, fused=False, variant="light",
                 absgrad=False, densify_every=0, ssim_lambda=0.0, seed=False, masked=False, select=0, relocate_every=0,
                 position_noise=False, relocate_min_opacity=0.005, relocate_seed=0, relocate_start=0, loop_close_at=0,
                 loop_close_seed=0, loop_close_scale=0.1, loop_close_moves_map=True, loop_close_pgo=False, prune_unseen=0,
                 prune_min_views=1, tsdf=0.0, mesh_out=None, raycast=False, knn_scale=False, on_knn_scale=None):
    """Returns (losses of the first and last iteration, model, seconds per iteration).  graph=True records the whole
    iteration (renders, losses, backward passes, statistics, Adam) into one hipGraph after three eager iterations.
    absgrad=True: the statistics take the absolute screen-space gradient (slam.render*(absgrad=True)).
    densify_every=N: every N iterations the statistics are consumed by densify_and_prune (not with graph=True: the step
    changes the number of Gaussians).
    ssim_lambda > 0: the loss is slam.l1_ssim_loss with that lambda_dssim instead of slam.l1_loss (0.0: the L1 path, unchanged).
    seed=True: the map starts empty and is seeded from the keyframes (seed_from_frame), which join the window one by one, every
    iters // keyframes iterations (light variant, not with graph=True or fused=True: the step changes the number of Gaussians
    and the window grows).
    masked=True: the observed depth has holes and the loss is slam.masked_l1_loss in its mapping form (not with ssim_lambda > 0);
    with seed=True the seeding also takes `stats.median * 50` as its depth_error_min.
    select=K: the `keyframes` poses are a pool (keyframe 1 of three or more turned to look the opposite way); the window mapped
    against is the newest keyframe and the K - 1 others that overlap it most (slam.keyframe_overlap / select_keyframes; not with
    seed=True, whose window grows by itself).  The model's `window` attribute then lists the pool indices chosen.
    relocate_every=N: every N iterations relocate_dead moves the Gaussians whose opacity lies below `relocate_min_opacity` onto live
    ones (generator keyed by `relocate_seed`) and, with position_noise=True, inject_position_noise follows; in place, also with
    graph=True (between replays) and fused=True.  relocate_start=K: not before iteration K (3DGS-MCMC's warm-up: a split Gaussian
    moves twice as fast, which costs loss while the optimiser is still in its first descent).  The model's `relocations` attribute then lists each step's counts
    [dead, live, relocated, sources hit, largest hits].
    loop_close_at=N (with seed=True): a pose-graph update after iteration N.  Every keyframe is seeded before the first iteration
    (so the map and the window are fixed from then on, and graph=True and fused=True are allowed), with its index in the role-less
    leaf "anchor".  After iteration N the keyframes' poses change -- one rigid motion of size `loop_close_scale` (radians and scene
    units; 0: none) shared by all of them, as a loop closure moves a stretch of trajectory, followed by each keyframe's own of a
    hundredth of that, drawn from `loop_close_seed` -- and transform_map moves every Gaussian with its keyframe (between replays
    with graph=True; loop_close_moves_map=False leaves the map where it was).  The model's `loop_closure` attribute then holds the
    losses of iteration N and N + 1 (before, after) and the step's counts.
    loop_close_pgo=True: the drawn poses are the truth, and the poses the map follows are SOLVED for: slam.pose_graph_optimize gets
    the old poses with keyframe 0 set to its true pose and fixed, K - 1 chain edges and one loop edge K - 1 -> 0, each measured on
    the truth with slam.relative_pose; its result goes to pose_corrections and transform_map in place of the drawn poses (on the
    device, between replays with graph=True).  `loop_closure` then also holds "solved" and "truth" ([K,4,4] each) and "pgo_stats".
    prune_unseen=N (with densify_every or relocate_every; not with graph=True): every N iterations the window's keyframes are
    rendered through slam.render_contributions into one accumulator and the Gaussians observed by fewer than `prune_min_views` of
    them get an opacity logit far below the pruning threshold, ahead of that iteration's densify_and_prune / relocate_dead.  The
    model's `unseen` attribute then lists each step's [Gaussians, unseen ones].
    tsdf=VOXEL: after the last iteration the window's keyframes are rendered once more and fused into a TSDF volume of that voxel
    size around the map (slam.tsdf_integrate, one call for all of them, mask_image=opacity_map), and slam.extract_mesh gives its
    zero level; the model's `tsdf` attribute then holds dims, triangles, area and the mesh.  mesh_out=PATH (with tsdf) writes the
    mesh as an ASCII PLY.  raycast=True (with tsdf): the volume is ray-cast at the fused keyframes' poses (slam.tsdf_raycast) and
    `tsdf` also holds hit_share and depth_diff, the mean |rendered depth - ray-cast depth| over the pixels where both are valid.
    knn_scale=True (with seed): after each seeding the new rows' log-scales become 0.5 log(max(slam.dist2(xyz), 1e-7)) over the whole
    map (3DGS's initialisation); `on_knn_scale(rows_before, xyz, new_log_scales)`, if given, is called after each such write with
    views of the map's tensors."""
    if raycast and not tsdf:
        raise ValueError("raycast=True looks at the volume that tsdf=VOXEL fuses: give that too")
    if knn_scale and not seed:
        raise ValueError("knn_scale=True sets the scale of the Gaussians that seed=True adds: give that too")
    if mesh_out and not tsdf:
        raise ValueError("mesh_out=PATH writes the mesh that tsdf=VOXEL extracts: give that too")
    if tsdf < 0 or tsdf != tsdf:
        raise ValueError("tsdf=VOXEL takes a voxel size > 0 (0: no fusion)")
    if prune_unseen and (graph or not (densify_every or relocate_every)):
        raise ValueError("prune_unseen=N marks Gaussians for densify_and_prune or relocate_dead (give one of them), not with graph=True")
    from dgr_amd import light, slam
    from dgr_amd.optim import (SparseAdam, add_densification_stats, densify_and_prune, inject_position_noise, pose_corrections,
                               relocate_dead, seed_from_frame, transform_map)
    from dgr_amd.synth import make_scene

    scenes = [make_scene(P, W, H, 3, view_index=k) for k in range(keyframes)]
    s = scenes[0]
    bg, gt = torch.from_numpy(s.bg).to(dev), torch.from_numpy(s.gt).to(dev)
    cams = [dict(viewmatrix=torch.from_numpy(sc.view).to(dev), fov=(sc.tanfovx, sc.tanfovy), HW=(H, W), gt_depth=gt)
            for sc in scenes]
    if select and keyframes >= 3:  # a keyframe from elsewhere in the session: same centre, a half turn about the camera's y axis
        cams[1]["viewmatrix"] = cams[1]["viewmatrix"] * torch.tensor([-1.0, 1.0, -1.0, 1.0], device=dev)
    kw = dict(track_off=True, map_off=False) if variant == "light" else dict(variant="full")
    truth = MapModel(s, dev)
    with torch.no_grad():
        obs = [slam.render(None, truth, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"], HW=c["HW"], gt_depth=gt, **kw)
               for c in cams]
    window = None
    if select:  # the window: the newest keyframe and the select - 1 of the others that see most of what it sees
        newest = keyframes - 1
        sensor = torch.where(obs[newest]["opacity_map"] > 0.9, obs[newest]["depth"] / obs[newest]["opacity_map"],
                             torch.zeros_like(obs[newest]["depth"]))
        pool = torch.stack([c["viewmatrix"] for c in cams[:newest]])
        overlap = slam.keyframe_overlap(sensor, cams[newest]["viewmatrix"], pool, W / (2.0 * s.tanfovx), H / (2.0 * s.tanfovy),
                                        (W - 1) / 2.0, (H - 1) / 2.0, stride=max(1, min(16, W // 40)), edge=min(20.0, W / 32.0))
        chosen, count = slam.select_keyframes(overlap.score, select - 1)
        window = sorted(chosen[:int(count)].tolist()) + [newest]  # (the step's one host read; logging the scores below is a second)
        if log:
            log(f"select: overlap with keyframe {newest}: " + ", ".join(f"{x:.3f}" for x in overlap.score.tolist()) +
                f" -> window {window}")
        cams, obs, keyframes = [cams[k] for k in window], [obs[k] for k in window], len(window)
    if seed:  # the synthetic sensor: the truth's expected depth where the truth covers the pixel, a hole (0) elsewhere
        sensor_depth = [torch.where(o["opacity_map"] > 0.9, o["depth"] / o["opacity_map"], torch.zeros_like(o["depth"])).detach()
                        for o in obs]
    if masked:  # the same holes in the depth the loss compares with (the rasterizer's depth is alpha-weighted: obs keeps that form)
        obs = [(o["render"].detach(), torch.where(o["opacity_map"] > 0.9, o["depth"], torch.zeros_like(o["depth"])).detach())
               for o in obs]
    else:
        obs = [(o["render"].detach(), o["depth"].detach()) for o in obs]
    # the mapping renders: with absgrad their dicts carry `viewspace_points_abs`, which the statistics read instead
    mkw = dict(kw, absgrad=True) if absgrad else kw
    points = "viewspace_points_abs" if absgrad else "viewspace_points"

    if graph:
        views_in_flight = 1  # (branches of one graph do not overlap on this ROCm, and the leaves' gradient accumulation
                             #  belongs to the stream they were created on: keep the recorded iteration on one stream)
    if loop_close_at and not (seed and 3 <= loop_close_at < iters - 1):
        raise ValueError("loop_close_at=N needs seed=True and 3 <= N < iters - 1")
    pc = SeededMapModel(dev, anchored=bool(loop_close_at)) if seed else MapModel(s, dev, degrade=7)
    opt = SparseAdam(pc.groups(), eps=1e-15, capturable=graph)
    seen = torch.zeros(pc.get_xyz.shape[0], dtype=torch.int32, device=dev)
    outs = [None] * keyframes
    n_live = 0 if seed else keyframes  # the window: keyframes 0 .. n_live - 1

    def photometric(color, depth, color_obs, depth_obs, w_color, w_depth):
        if masked:  # depth over the valid, non-outlier pixels; colour over every pixel; means over their own counts
            return slam.masked_l1_loss(color, depth, color_obs, depth_obs, mask_color=False, w_color=w_color, w_depth=w_depth,
                                       reduction="mean")
        if ssim_lambda > 0.0:  # (1 - lambda) L1 + lambda (1 - SSIM) on the colour, L1 on the depth
            return slam.l1_ssim_loss(color, depth, color_obs, depth_obs, w_color, w_depth, ssim_lambda)
        return slam.l1_loss(color, depth, color_obs, depth_obs, w_color, w_depth)  # one fused reduction

    def loss_fn(out, k):
        outs[k] = out
        return photometric(out["render"], out["depth"], obs[k][0], obs[k][1], 1.0, 0.5)

    obs_color, obs_depth = torch.stack([o[0] for o in obs]), torch.stack([o[1] for o in obs])

    def batch_loss_fn(out):
        # the keyframes' losses summed, as ONE fused reduction over the stacked images: sum_k (mean_k |c - c_obs| + 0.5
        # mean_k |d - d_obs|) = V x the means over the whole stack (the keyframes share a size; SSIM's mean likewise)
        V = float(out["render"].size(0))
        return photometric(out["render"], out["depth"], obs_color, obs_depth, V * 1.0, V * 0.5)

    def iteration_fused():
        # the keyframe batch through ONE batched forward and ONE batched backward (dgr_amd.batch): the Gaussians' gradients
        # arrive summed over the keyframes, the screen-space gradients per view
        opt.zero_grad(set_to_none=True)
        losses, out = slam.render_batch_fused(cams, pc, None, bg, loss_fn, batch_loss_fn=batch_loss_fn, **mkw)
        pts = out[points].grad
        for k in range(keyframes):
            add_densification_stats(pts[k], out["radii"][k], pc.xyz_gradient_accum, pc.denom, pc.max_radii2D)
        torch.amax(out["radii"], dim=0, out=seen)
        if not graph:  # lazy status mode: every outstanding forward reports before the step (an overflowed one raises here)
            light.check_async_errors()
        opt.step(visible=seen)
        return losses[0] / keyframes   # (the batch loss is the sum over the keyframes)

    def iteration():
        if fused:
            return iteration_fused()
        opt.zero_grad(set_to_none=True)
        if views_in_flight > 1:
            losses = slam.render_batch(cams[:n_live], pc, None, bg, loss_fn, views_in_flight=views_in_flight, **mkw)
        else:  # one keyframe after the other on the caller's stream
            losses = []
            for k, c in enumerate(cams[:n_live]):
                loss = loss_fn(slam.render(None, pc, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"], HW=c["HW"],
                                           gt_depth=gt, **mkw), k)
                loss.backward()
                losses.append(loss.detach())
        seen.zero_()
        for out in outs[:n_live]:
            add_densification_stats(out[points].grad, out["radii"], pc.xyz_gradient_accum, pc.denom,
                                    pc.max_radii2D)
            torch.maximum(seen, out["radii"], out=seen)
        if not graph:
            light.check_async_errors()
        opt.step(visible=seen)
        return torch.stack(losses).mean()

    if densify_every:  # the scene's radius stands in for 3DGS's cameras_extent
        extent = float((truth.get_xyz.detach() - truth.get_xyz.detach().mean(dim=0)).norm(dim=1).max())

    def densify():
        nonlocal seen
        before = pc.get_xyz.shape[0]
        leaves, accum, denom, max_radii2D, counts = densify_and_prune(
            pc.leaves(), opt, pc.xyz_gradient_accum, pc.denom, pc.max_radii2D,
            grad_threshold=0.0008 if absgrad else 0.0002, extent=extent, max_screen_size=20.0)
        pc.replace(leaves, accum, denom, max_radii2D)
        seen = torch.zeros(counts.rows, dtype=torch.int32, device=dev)
        if log:
            log(f"densify: P {before} -> {counts.rows} ({counts.survivors} kept, {counts.clones} cloned, "
                f"{counts.split} split into {counts.children})")

    def seed_keyframe(k):
        """Keyframe k joins the window: what the map does not explain of it (all of it while the map is empty) becomes Gaussians."""
        nonlocal seen, n_live
        c, before = cams[k], pc.get_xyz.shape[0]
        silhouette, behind = None, {}
        if before:
            with torch.no_grad():
                r = slam.render(None, pc, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"], HW=c["HW"], gt_depth=gt, **kw)
                silhouette = r["opacity_map"]
                if masked:  # also where the map lies far behind the sensor: 50 x the median depth error of the explained pixels
                    expected = torch.where(silhouette > 0.5, r["depth"] / silhouette, torch.zeros_like(silhouette))
                    _, stats = slam.masked_l1_loss(r["render"], expected, obs[k][0], sensor_depth[k], silhouette,
                                                   silhouette_threshold=0.5, mask_color=False, return_stats=True)
                    behind = dict(depth=expected, depth_error_min=stats.median * 50)
        leaves, accum, denom, max_radii2D, counts = seed_from_frame(
            pc.leaves(), opt, obs[k][0], sensor_depth[k], c["viewmatrix"], W / (2.0 * s.tanfovx), H / (2.0 * s.tanfovy),
            (W - 1) / 2.0, (H - 1) / 2.0, opacity_map=silhouette, silhouette_threshold=0.5, init_opacity=0.5, **behind,
            **(dict(fill={"anchor": float(k)}) if loop_close_at else {}),
            xyz_gradient_accum=pc.xyz_gradient_accum, denom=pc.denom, max_radii2D=pc.max_radii2D)
        pc.replace(leaves, accum, denom, max_radii2D)
        if knn_scale and counts.rows > before:  # 3DGS's initial scale, over the whole map; the new rows' Adam moments are zero
            with torch.no_grad():
                d2 = slam.dist2(pc._xyz.detach())
                pc._scaling[before:] = (0.5 * torch.log(torch.clamp(d2[before:], min=1e-7)))[:, None].expand(-1, 3)
            if on_knn_scale:
                on_knn_scale(before, pc._xyz.detach(), pc._scaling.detach()[before:])
            if log:
                log(f"knn-scale: keyframe {k}: {counts.rows - before} new rows, mean scale {float(pc._scaling.detach()[before:].exp().mean()):.5f}")
        seen = torch.zeros(counts.rows, dtype=torch.int32, device=dev)
        n_live = k + 1
        if log:
            log(f"seed: keyframe {k}: P {before} -> {counts.rows} ({counts.new} new from {counts.valid} valid pixels"
                f"{f', {counts.unseen} of them unseen' if before else ''})")

    relocations = []

    def relocate(step):
        # in place: the leaves, the moments and the accumulators stay the tensors the recorded iteration reads and writes
        result = relocate_dead(pc.leaves(), opt, min_opacity=relocate_min_opacity, seed=relocate_seed, step=step,
                               xyz_gradient_accum=pc.xyz_gradient_accum, denom=pc.denom, max_radii2D=pc.max_radii2D)
        if position_noise:
            inject_position_noise(pc.leaves(), opt.param_groups[0]["lr"], seed=relocate_seed + 1, step=step)
        relocations.append(result.counts)
        if log:
            dead, live, moved, sources, most = result.counts.tolist()[:5]  # (the step's one host read)
            log(f"relocate: {dead} dead of {dead + live}, {moved} moved onto {sources} live Gaussians (at most {most} onto one)")

    unseen_steps = []

    def mark_unseen(step):
        """What no keyframe of the window blends gets an opacity no pruning rule keeps (sigmoid(-15) = 3e-7; the thresholds are 0.005)."""
        acc = slam.ContributionAccumulator(pc.get_xyz.shape[0], dev)
        with torch.no_grad():
            for c in cams[:n_live]:  # a window is a loop over its keyframes into one accumulator
                slam.render_contributions(None, pc, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"], HW=c["HW"], gt_depth=gt,
                                          variant=variant, into=acc, frame_id=step)
            unseen = ~acc.observed(min(prune_min_views, n_live))  # (a window that is still growing cannot ask for more views than it has)
            pc._opacity.masked_fill_(unseen[:, None], -15.0)
        unseen_steps.append([acc.P, int(unseen.sum())])  # (the step's one host read)
        if log:
            log(f"prune-unseen: {unseen_steps[-1][1]} of {acc.P} Gaussians blended by fewer than {min(prune_min_views, n_live)} of {n_live} keyframes")

    def rigid(rng, size):  # a rigid motion of about `size`: a rotation by that angle about a random axis, a translation of that length
        axis, shift = rng.standard_normal(3), rng.standard_normal(3)
        x, y, z = axis / np.linalg.norm(axis)
        K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = np.eye(3) + np.sin(size) * K + (1.0 - np.cos(size)) * K @ K, size * shift / np.linalg.norm(shift)
        return D

    def close_loop():
        # C2W_new = D_k C2W_old: the viewmatrix W2C^T becomes (D_k^-1)^T W2C^T.  The poses are rewritten in place (the recorded
        # iteration derives its cameras from these tensors on every replay), and the map follows them, in place as well
        rng = np.random.RandomState(loop_close_seed)
        shared = rigid(rng, loop_close_scale)
        deltas = np.stack([rigid(rng, loop_close_scale / 100.0) @ shared for _ in cams])
        old = torch.stack([c["viewmatrix"] for c in cams])
        new = (torch.from_numpy(np.linalg.inv(deltas).transpose(0, 2, 1)).to(dev) @ old.double()).float()
        if loop_close_pgo:
            K = len(cams)
            edges = torch.tensor([(k + 1, k) for k in range(K - 1)] + [(K - 1, 0)], dtype=torch.int32, device=dev)
            measured = slam.relative_pose(new[edges[:, 0].long()], new[edges[:, 1].long()])
            start = old.clone()
            start[0] = new[0]
            solved = slam.pose_graph_optimize(start, edges, measured, iterations=20)
            closure.update(truth=new, solved=solved.viewmatrices, pgo_stats=solved.stats)
            new = solved.viewmatrices
        corrections = pose_corrections(old, new)
        for c, v in zip(cams, new):
            c["viewmatrix"].copy_(v)
        return transform_map(pc.leaves(), opt, corrections) if loop_close_moves_map else None

    if seed:
        seed_keyframe(0)
    if loop_close_at:  # the whole window before the first iteration
        while n_live < keyframes:
            seed_keyframe(n_live)
    join_every = max(iters // keyframes, 1)
    closure = {}

    run = iteration
    if graph:  # (the three eager iterations run inside CapturedStep, on the stream the graph is recorded on)
        from dgr_amd.multiview import CapturedStep
        with torch.no_grad():
            first = float(torch.stack([photometric(*(slam.render(None, pc, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"],
                                                                 HW=c["HW"], gt_depth=gt, **kw)[k_] for k_ in ("render", "depth")),
                                                   obs[i][0], obs[i][1], 1.0, 0.5) for i, c in enumerate(cams)]).mean())
        step = CapturedStep(iteration, warmup=3)
        run = step.replay
    else:
        first = float(iteration())
        for _ in range(2):
            iteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters - 3):
        if seed and n_live < keyframes and (i + 3) % join_every == 0:
            seed_keyframe(n_live)
        loss = run()
        if prune_unseen and (i + 4) % prune_unseen == 0:
            mark_unseen(i + 3)
        if densify_every and (i + 4) % densify_every == 0:
            densify()
        if relocate_every and (i + 4) % relocate_every == 0 and i + 3 >= relocate_start:
            relocate(i + 3)
        if loop_close_at and i + 3 == loop_close_at:
            closure["before"], closure["counts"] = loss.detach().clone(), close_loop()
        elif loop_close_at and i + 3 == loop_close_at + 1:
            closure["after"] = loss.detach().clone()
        if log and (i + 3) % 20 == 0:
            log(f"iteration {i + 3:4d}: loss {float(loss):.4e}")
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / max(iters - 3, 1)
    if graph:
        step.check()
    if tsdf:
        pc.tsdf = fuse_window(slam, pc, cams[:max(n_live, 1)], bg, gt, kw, W, H, s.tanfovx, s.tanfovy, float(tsdf), mesh_out, raycast)
        if log:
            log(tsdf_line(pc.tsdf))
            if raycast:
                log(raycast_line(pc.tsdf))
    pc.window = window
    pc.relocations = [c.tolist()[:5] for c in relocations]
    pc.unseen = unseen_steps
    if loop_close_at:
        pc.loop_closure = dict(before=float(closure["before"]), after=float(closure["after"]),
                               counts=None if closure["counts"] is None else closure["counts"].tolist())
        if loop_close_pgo:
            pc.loop_closure.update(solved=closure["solved"], truth=closure["truth"], pgo_stats=closure["pgo_stats"].tolist())
        if log:
            log(f"loop closure after iteration {loop_close_at}: loss {pc.loop_closure['before']:.4e} before, "
                f"{pc.loop_closure['after']:.4e} after; counts {pc.loop_closure['counts']}")
    return (first, float(loss)), pc, dt


def fuse_window(slam, pc, cams, bg, gt, kw, W, H, tanfovx, tanfovy, voxel, mesh_out=None, raycast=False):
    """The map's surface: the keyframes `cams` rendered once more, fused into a TSDF volume of voxel size `voxel` around the map in
    one call and extracted.  Returns dict(dims, triangles, area, mesh); with `raycast` the volume is also ray-cast at the same
    poses, and hit_share and depth_diff (mean |rendered - ray-cast depth| where both are valid) join them."""
    with torch.no_grad():
        outs = [slam.render(None, pc, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"], HW=c["HW"], gt_depth=gt, **kw) for c in cams]
        alpha = torch.stack([o["opacity_map"].reshape(H, W) for o in outs])
        # the rasterizer's depth is alpha-weighted: the sensor's form is depth / alpha (where the map covers the pixel; 0 = a hole)
        depth = torch.stack([o["depth"].reshape(H, W) for o in outs])
        depth = torch.where(alpha > 0.5, depth / alpha.clamp_min(1e-6), torch.zeros_like(depth))
        color = torch.stack([o["render"] for o in outs]).clamp(0.0, 1.0)
        views = torch.stack([c["viewmatrix"] for c in cams])
        # around the scene: the map's positions without their outermost hundredth, a truncation's width more (one host read)
        xyz = pc.get_xyz.detach()
        q = torch.quantile(xyz[::max(1, xyz.shape[0] // 100000)], torch.tensor([0.01, 0.99], device=xyz.device), dim=0).tolist()
        pad = 4.0 * voxel
        vol = slam.TsdfVolume.from_bounds([v - pad for v in q[0]], [v + pad for v in q[1]], voxel, device=xyz.device)
        slam.tsdf_integrate(vol, depth, views, W / (2.0 * tanfovx), H / (2.0 * tanfovy), (W - 1) / 2.0, (H - 1) / 2.0, color=color,
                            mask_image=alpha)
        mesh = slam.extract_mesh(vol)
        tri = mesh.vertices.reshape(-1, 3, 3).double()
        area = float(0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1).sum())
        out = dict(dims=vol.dims, triangles=mesh.vertices.shape[0] // 3, area=area, mesh=mesh)
        if raycast:
            cast = slam.tsdf_raycast(vol, views, W / (2.0 * tanfovx), H / (2.0 * tanfovy), (W - 1) / 2.0, (H - 1) / 2.0, H, W,
                                     normals=False, color=False)
            both = (cast.depth > 0) & (depth > 0)
            diff = (cast.depth - depth).abs()[both]
            out.update(hit_share=float((cast.depth > 0).float().mean()), depth_diff=float(diff.mean()) if diff.numel() else float("nan"))
    if mesh_out:
        write_ply(mesh_out, mesh.vertices.cpu().numpy(), mesh.colors.cpu().numpy())
    return out


def tsdf_line(t):
    return f"tsdf: {t['dims'][0]}x{t['dims'][1]}x{t['dims'][2]} voxels, {t['triangles']} triangles, area {t['area']:.4f}"


def raycast_line(t):
    return f"raycast: hit share {t['hit_share']:.4f}, mean |rendered - ray-cast depth| {t['depth_diff']:.5f}"


def write_ply(path, vertices, colors):
    """an unindexed triangle list [3 T, 3] with colours in [0, 1] as an ASCII PLY"""
    n = len(vertices)
    rgb = np.clip(np.rint(colors * 255.0), 0, 255).astype(np.int64)
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
                f"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {n // 3}\n"
                "property list uchar int vertex_indices\nend_header\n")
        np.savetxt(f, np.concatenate([vertices.astype(np.float64), rgb], axis=1), fmt="%.7g %.7g %.7g %d %d %d")
        np.savetxt(f, np.concatenate([np.full((n // 3, 1), 3), np.arange(n).reshape(-1, 3)], axis=1), fmt="%d")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--keyframes", type=int, default=4)
    ap.add_argument("--views-in-flight", type=int, default=3)
    ap.add_argument("--graph", action="store_true", help="record the iteration into a hipGraph and replay it")
    ap.add_argument("--fused", action="store_true",
                    help="the keyframe batch through one batched forward + backward (slam.render_batch_fused) instead of one "
                         "rasterizer call per keyframe")
    ap.add_argument("--variant", choices=("light", "full"), default="light", help="which rasterizer variant maps")
    ap.add_argument("--absgrad", action="store_true",
                    help="densification statistics from the absolute screen-space gradient (AbsGS) instead of viewspace_points.grad")
    ap.add_argument("--densify-every", type=int, default=0, metavar="N",
                    help="every N iterations clone / split / prune from the accumulated statistics (densify_and_prune); "
                         "off by default, not together with --graph")
    ap.add_argument("--ssim", type=float, default=0.0, metavar="LAMBDA",
                    help="the 3DGS mapping loss (1 - LAMBDA) L1 + LAMBDA (1 - SSIM) on the colour images (slam.l1_ssim_loss; 3DGS "
                         "uses 0.2) instead of plain L1; 0 (default) keeps the L1 loss")
    ap.add_argument("--seed", action="store_true",
                    help="start from an empty map: seed Gaussians from keyframe 0's colour and depth, then from each further "
                         "keyframe's unexplained pixels before it joins the window (seed_from_frame); light variant, not together "
                         "with --graph or --fused")
    ap.add_argument("--masked", action="store_true",
                    help="observed depth with holes and the masked loss in its mapping form (slam.masked_l1_loss(mask_color=False)); "
                         "with --seed, stats.median * 50 becomes the seeding's depth_error_min; not together with --ssim")
    ap.add_argument("--select", type=int, default=0, metavar="K",
                    help="map against a window of K keyframes chosen from the --keyframes pool by their overlap with the newest one "
                         "(slam.keyframe_overlap + slam.select_keyframes); 0 (default) maps against every keyframe; not together "
                         "with --seed")
    ap.add_argument("--relocate-every", type=int, default=0, metavar="N",
                    help="every N iterations move the dead Gaussians onto live ones, in place (relocate_dead: 3DGS-MCMC's relocation "
                         "for a map of fixed size); off by default; goes together with --graph and --fused")
    ap.add_argument("--relocate-start", type=int, default=0, metavar="K",
                    help="with --relocate-every: no relocation before iteration K (3DGS-MCMC starts after a warm-up)")
    ap.add_argument("--position-noise", action="store_true",
                    help="with --relocate-every: add the gated SGLD position noise after each relocation (inject_position_noise)")
    ap.add_argument("--relocate-min-opacity", type=float, default=0.005, metavar="O",
                    help="a Gaussian whose opacity lies below O is dead (default 0.005)")
    ap.add_argument("--loop-close-at", type=int, default=0, metavar="N",
                    help="with --seed: after iteration N the keyframes' poses get seeded rigid corrections, as after a loop closure, and "
                         "every Gaussian follows the keyframe it was seeded from (pose_corrections + transform_map); all keyframes are "
                         "then seeded before the first iteration, so --graph and --fused are allowed")
    ap.add_argument("--loop-close-seed", type=int, default=0, help="the seed of --loop-close-at's corrections")
    ap.add_argument("--pgo", action="store_true",
                    help="with --loop-close-at: the corrected poses are solved for on the device (slam.pose_graph_optimize over chain "
                         "edges and one loop edge measured on the drawn poses) instead of being taken as drawn")
    ap.add_argument("--prune-unseen", type=int, default=0, metavar="N",
                    help="every N iterations give the Gaussians that fewer than --prune-min-views keyframes of the window blend "
                         "(slam.render_contributions) an opacity below the pruning threshold; needs --densify-every or "
                         "--relocate-every, which then removes or recycles them; not together with --graph")
    ap.add_argument("--prune-min-views", type=int, default=1, metavar="M", help="with --prune-unseen: the views a Gaussian needs (default 1)")
    ap.add_argument("--tsdf", type=float, default=0.0, metavar="VOXEL",
                    help="after the last iteration fuse the window's rendered keyframes into a TSDF volume of this voxel size around "
                         "the map (slam.tsdf_integrate) and extract its surface (slam.extract_mesh); 0 (default): off")
    ap.add_argument("--mesh-out", default=None, metavar="PATH", help="with --tsdf: write the mesh as an ASCII PLY")
    ap.add_argument("--raycast", action="store_true",
                    help="with --tsdf: ray-cast the fused volume at the fused keyframes' poses (slam.tsdf_raycast) and report the hit "
                         "share and the mean |rendered depth - ray-cast depth|")
    ap.add_argument("--knn-scale", action="store_true",
                    help="with --seed: the log-scale of the new Gaussians becomes 0.5 log(max(dist2, 1e-7)), dist2 the mean squared "
                         "distance to the three nearest Gaussians of the whole map (slam.dist2, simple-knn's distCUDA2): 3DGS's "
                         "initialisation")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--gaussians", type=int, default=100000)
    args = ap.parse_args()
    if not 0.0 <= args.ssim <= 1.0:
        ap.error("--ssim LAMBDA lies in [0, 1]")
    if args.masked and args.ssim > 0:
        ap.error("--masked replaces the photometric loss: drop --ssim")
    if args.densify_every < 0 or (args.densify_every and args.graph):
        ap.error("--densify-every changes the number of Gaussians: it cannot run inside a recorded hipGraph (drop --graph)")
    if args.loop_close_at and not args.seed:
        ap.error("--loop-close-at moves every Gaussian with the keyframe it was seeded from: it needs --seed")
    if args.pgo and not args.loop_close_at:
        ap.error("--pgo solves the pose graph of --loop-close-at: give that too")
    if args.seed and (((args.graph or args.fused) and not args.loop_close_at) or args.variant != "light"):
        ap.error("--seed changes the number of Gaussians and grows the window: it cannot run inside a recorded hipGraph (drop "
                 "--graph), and it maps through the per-keyframe light path (drop --fused / --variant full)")
    if args.select < 0 or args.select > args.keyframes or (args.select and args.seed):
        ap.error("--select K chooses 1 .. --keyframes keyframes of the pool; --seed grows its own window (drop one of the two)")
    if args.relocate_every < 0 or (args.position_noise and not args.relocate_every):
        ap.error("--relocate-every N takes N >= 0, and --position-noise goes with it")
    if args.relocate_every and args.seed:
        ap.error("--relocate-every keeps a map of fixed size; --seed grows one (drop one of the two)")
    if args.prune_unseen < 0 or args.prune_min_views < 1 or (args.prune_unseen and not (args.densify_every or args.relocate_every)):
        ap.error("--prune-unseen N marks Gaussians for removal: give --densify-every or --relocate-every too (N >= 0, --prune-min-views >= 1)")
    if args.prune_unseen and args.graph:
        ap.error("--prune-unseen renders the window outside the recorded iteration and reads a count: drop --graph")
    if args.tsdf < 0 or (args.mesh_out and not args.tsdf):
        ap.error("--tsdf VOXEL takes a voxel size > 0, and --mesh-out PATH writes its mesh: give --tsdf too")
    if args.knn_scale and not args.seed:
        ap.error("--knn-scale sets the scale of the Gaussians that --seed adds: give --seed too")
    if args.raycast and not args.tsdf:
        ap.error("--raycast looks at the volume that --tsdf VOXEL fuses: give --tsdf too")
    if not 0.0 <= args.relocate_min_opacity < 1.0:
        ap.error("--relocate-min-opacity lies in [0, 1)")
    import torch as _torch
    _torch.autograd.set_multithreading_enabled(False)  # one device, one thread: no engine-thread hand-off per backward
    if args.graph:
        os.environ["DGR_SYNC_MODE"] = "lazy"  # a blocking status read cannot be captured
    dev = torch.device("cuda:0")
    (l0, l1), pc, dt = mapping_loop(dev, args.gaussians, args.width, args.height, args.keyframes, args.iters,
                                    args.views_in_flight, log=None if args.graph else print, graph=args.graph, fused=args.fused,
                                    variant=args.variant, absgrad=args.absgrad, densify_every=args.densify_every, ssim_lambda=args.ssim,
                                    seed=args.seed, masked=args.masked, select=args.select, relocate_every=args.relocate_every,
                                    position_noise=args.position_noise, relocate_min_opacity=args.relocate_min_opacity,
                                    relocate_start=args.relocate_start, loop_close_at=args.loop_close_at,
                                    loop_close_seed=args.loop_close_seed, loop_close_pgo=args.pgo, prune_unseen=args.prune_unseen,
                                    prune_min_views=args.prune_min_views, tsdf=args.tsdf, mesh_out=args.mesh_out, raycast=args.raycast,
                                    knn_scale=args.knn_scale)
    if args.tsdf and args.graph:  # (otherwise the loop has logged it)
        print(tsdf_line(pc.tsdf))
        if args.raycast:
            print(raycast_line(pc.tsdf))
    if args.prune_unseen:
        print(f"prune-unseen: {sum(u for _, u in pc.unseen)} Gaussians marked unseen in {len(pc.unseen)} steps "
              f"(fewer than {args.prune_min_views} keyframes blended them)")
    if args.pgo:
        c = pc.loop_closure
        s = c["pgo_stats"]
        print(f"pose graph: {len(c['solved'])} poses solved in {s[3]:.0f} trials ({s[4]:.0f} accepted, {s[6]:.0f} CG iterations), cost "
              f"{s[0]:.4e} -> {s[1]:.4e}, ok {s[2]:.0f}, |solved - drawn| {float((c['solved'] - c['truth']).abs().max()):.3e}")
    if args.loop_close_at and args.graph:
        print(f"loop closure after iteration {args.loop_close_at}: loss {pc.loop_closure['before']:.4e} before, "
              f"{pc.loop_closure['after']:.4e} after; counts {pc.loop_closure['counts']}")
    for step, (dead, live, moved, sources, most) in enumerate(pc.relocations if args.graph else ()):
        print(f"relocation {step}: {dead} dead of {dead + live}, {moved} moved onto {sources} live Gaussians (at most {most} onto one)")
    if args.select:
        args.keyframes = len(pc.window)
    n = float(pc.denom.sum())
    print(("full variant: " if args.variant == "full" else "") + ("absgrad: " if args.absgrad else "") +
          (f"L1 + D-SSIM (lambda {args.ssim:g}): " if args.ssim > 0 else "") + ("masked L1: " if args.masked else "") +
          f"loss {l0:.4e} -> {l1:.4e}; {dt * 1e3:.3f} ms per mapping iteration over {args.keyframes} keyframes"
          f" ({dt / args.keyframes * 1e3:.3f} ms per keyframe); {int((pc.denom > 0).sum())} Gaussians seen,"
          f" {n:.0f} (Gaussian, view) statistics accumulated" +
          (f"; P {0 if args.seed else args.gaussians} -> {pc.get_xyz.shape[0]}" if args.densify_every or args.seed else ""))


if __name__ == "__main__":
    main()
