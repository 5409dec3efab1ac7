#!/usr/bin/env python3
"""Camera tracking against a fixed Gaussian map (CG-SLAM's tracking loop in miniature).

A synthetic map is rendered from the true pose to get the "observed" frame; the pose estimate starts perturbed and is
refined by Adam on (quaternion, translation) through the rasterizer's analytic viewmatrix gradient (tracking mode:
map_off=True, no Gaussian gradients).  With --graph the whole iteration -- pose -> matrices -> render -> loss -> backward ->
Adam step -- is recorded once into a hipGraph and replayed (dgr_amd.multiview.CapturedStep), which removes the host
from the loop.

With --complete-pose the pose gradient is the complete one (slam.render(complete_pose=True): 2D covariance, colour and every
depth term included) instead of the reference's.  --trace K prints the pose error every K iterations (the timing then includes
those reads).

With --masked the observed frame gets what a real depth sensor adds: holes (depth_obs = 0 on a seeded random 20 % of the pixels)
and gross outliers (2 % of the pixels, metres off).  The pose is then tracked twice from the same start, with the plain L1 loss and
with the masked loss (slam.masked_l1_loss: valid sensor depth, silhouette above 0.99, depth error at most 10 x the frame's median
error -- the median found on the device, so the iteration still records into a hipGraph), and both final pose errors are printed.

With --icp N the pose is first aligned geometrically (slam.icp_align: frame-to-model point-to-plane ICP): the model's depth is
rendered at the perturbed start pose, N Gauss-Newton iterations align the observed depth to it on the device, and the resulting
(quaternion, translation) replace the start pose of the Adam loop, device to device.  The pose error is printed at the start,
after ICP and at the end, with the time per ICP iteration.  --reach ROT TRANS additionally prints the first Adam iteration at which the
rotation error is at most ROT and the translation error at most TRANS (read once per iteration: the timing then includes those reads).

With --rgbd N [--rgbd-levels L] the pose is first aligned by the hybrid step instead (slam.rgbd_align: the point-to-plane term and
a photometric term on the rendered against the observed colour, N iterations on each of L pyramid levels, coarsest first); the
rest is --icp's, with which it cannot be combined.

  python examples/tracking.py [--graph] [--fused] [--masked] [--complete-pose] [--icp N | --rgbd N [--rgbd-levels L]]
                              [--reach ROT TRANS] [--trace K]
                              [--iters 150]
                              [--width 640 --height 480 --gaussians 100000]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--fused", action="store_true",
                    help="pose -> camera tensors, the L1 loss and the Adam step as single launches (slam.pose_to_camera, "
                         "slam.l1_loss, optim.SparseAdam)")
    ap.add_argument("--masked", action="store_true",
                    help="holes and outliers in the observed depth; track with the plain loss and with slam.masked_l1_loss")
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--gaussians", type=int, default=100000)
    ap.add_argument("--complete-pose", action="store_true", help="the complete pose gradient (library option pose_grad = 1)")
    ap.add_argument("--trace", type=int, default=0, help="print the pose error every K iterations")
    ap.add_argument("--icp", type=int, default=0,
                    help="N iterations of frame-to-model ICP (slam.icp_align) on the depth images before the Adam loop")
    ap.add_argument("--rgbd", type=int, default=0,
                    help="N iterations per level of hybrid RGB-D alignment (slam.rgbd_align) on the colour and depth images before "
                         "the Adam loop; not together with --icp")
    ap.add_argument("--rgbd-levels", type=int, default=1, help="pyramid levels of --rgbd, coarsest first")
    ap.add_argument("--reach", type=float, nargs=2, default=None, metavar=("ROT", "TRANS"),
                    help="print the first Adam iteration at which the pose errors are at most ROT and TRANS")
    args = ap.parse_args()
    if args.icp > 0 and args.rgbd > 0:
        ap.error("--rgbd cannot be combined with --icp")
    if args.graph or args.fused:
        # a blocking status read cannot be captured, and a tracking loop has no use for num_rendered on the host: no host wait
        os.environ.setdefault("DGR_SYNC_MODE", "lazy") if not args.graph else os.environ.__setitem__("DGR_SYNC_MODE", "lazy")
    from dgr_amd import light, slam
    from dgr_amd.multiview import CapturedStep
    from dgr_amd.synth import camera, make_scene
    from test_slam_render import Model, rot_to_quat

    dev = torch.device("cuda:0")
    W, H = args.width, args.height
    s = make_scene(args.gaussians, W, H, 3)
    pc = Model(s, dev)
    tanfovx, tanfovy, Rm, t_true, *_ = camera(W, H, 0.05)
    bg, gt_depth = torch.from_numpy(s.bg).to(dev), torch.from_numpy(s.gt).to(dev)
    kw = dict(fov=(tanfovx, tanfovy), HW=(H, W), gt_depth=gt_depth, track_off=False, map_off=True,
              complete_pose=args.complete_pose)

    # one device, one Python thread: the autograd engine's worker thread only adds a hand-off per backward (0.47 -> 0.32 ms per
    # iteration here); a switch of PyTorch, not of the rasterizer
    torch.autograd.set_multithreading_enabled(False)

    def pose(q, t):
        if args.fused:
            return slam.pose_to_camera(q, t, tanfovx, tanfovy)
        return slam.camera_tensors(slam.w2c_from_quat_trans(q, t), tanfovx, tanfovy)

    def render(cam):  # (fused: projmatrix / campos come from the pose kernel; otherwise render() forms them from the viewmatrix)
        return slam.render(None, pc, None, bg, viewmatrix=cam[0], pose_tensors=cam if args.fused else None, **kw)

    q_true = torch.tensor(rot_to_quat(Rm), dtype=torch.float32, device=dev)
    t_true = torch.tensor(t_true, dtype=torch.float32, device=dev)
    with torch.no_grad():
        obs = render(pose(q_true, t_true))
    obs_c, obs_d = obs["render"].detach(), obs["depth"].detach()

    if args.masked:
        g = torch.Generator().manual_seed(11)
        hole = (torch.rand(obs_d.shape, generator=g) < 0.20).to(dev)
        gross = (torch.rand(obs_d.shape, generator=g) < 0.02).to(dev)
        off = (1.0 + 2.0 * torch.rand(obs_d.shape, generator=g)).to(dev)
        obs_d = torch.where(hole, torch.zeros_like(obs_d), torch.where(gross, obs_d + off, obs_d)).contiguous()

    def track(masked):
        q = (q_true + torch.tensor([0.0, 0.004, -0.006, 0.003], device=dev)).requires_grad_()
        t = (t_true + torch.tensor([0.012, -0.009, 0.015], device=dev)).requires_grad_()
        groups = [{"params": [q], "lr": 5e-4}, {"params": [t], "lr": 1.5e-3}]
        if args.fused:  # one launch per tensor, step count on the device when the iteration is recorded into a graph
            from dgr_amd.optim import SparseAdam
            opt = SparseAdam(groups, capturable=args.graph)
        else:
            opt = torch.optim.Adam(groups, capturable=args.graph)

        def iteration():
            opt.zero_grad(set_to_none=True)
            out = render(pose(q, t))
            if masked:  # the means over the kept pixels, so that the step sizes compare with the plain loss's
                loss = slam.masked_l1_loss(out["render"], out["depth"], obs_c, obs_d, out["opacity_map"], w_color=1.0, w_depth=0.5,
                                           reduction="mean")
            elif args.fused:
                loss = slam.l1_loss(out["render"], out["depth"], obs_c, obs_d, 1.0, 0.5)
            else:
                loss = (out["render"] - obs_c).abs().mean() + 0.5 * (out["depth"] - obs_d).abs().mean()
            loss.backward()
            if not args.graph:  # lazy status mode: every outstanding forward reports before the step (an overflowed one raises here)
                light.check_async_errors()
            opt.step()
            return loss.detach()

        def err():
            with torch.no_grad():
                return float((q / q.norm() - q_true).norm()), float((t - t_true).norm())

        if args.masked:
            print("masked loss (slam.masked_l1_loss):" if masked else "plain L1 loss on the same frame:")
        print(f"start : rotation error {err()[0]:.2e}, translation error {err()[1]:.2e}")
        if args.icp > 0:
            # the model's depth at the start pose, then N ICP iterations of the observed depth against it; the pose the Adam
            # loop starts from is copied into the leaves on the device
            fx, fy, cx, cy = W / (2.0 * tanfovx), H / (2.0 * tanfovy), (W - 1) / 2.0, (H - 1) / 2.0
            with torch.no_grad():
                cam = pose(q, t)
                model = render(cam)
                view0 = cam[0].detach().clone()

                def align():
                    return slam.icp_align(obs_d, model["depth"], None, view0, fx, fy, cx, cy, iterations=args.icp,
                                          opacity_map=model["opacity_map"], depth_range=(1e-3, float("inf")))
                align()  # (kernel loading is not timed)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                aligned = align()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                q.copy_(aligned.quat)
                t.copy_(aligned.trans)
            ok = int(aligned.stats[:, 29].sum())
            print(f"icp   : rotation error {err()[0]:.2e}, translation error {err()[1]:.2e}, {ok} of {args.icp} steps accepted, "
                  f"{int(aligned.stats[-1, 28])} pairs, {dt / args.icp * 1e6:.1f} us per ICP iteration (eager, normals included)")
        if args.rgbd > 0:
            # as above with the hybrid step: the model's colour and depth at the start pose against the observed ones
            fx, fy, cx, cy = W / (2.0 * tanfovx), H / (2.0 * tanfovy), (W - 1) / 2.0, (H - 1) / 2.0
            with torch.no_grad():
                cam = pose(q, t)
                model = render(cam)
                view0 = cam[0].detach().clone()

                def align():
                    return slam.rgbd_align(obs_c, obs_d, model["render"], model["depth"], None, view0, fx, fy, cx, cy,
                                           levels=args.rgbd_levels, iterations=args.rgbd, opacity_map=model["opacity_map"],
                                           depth_range=(1e-3, float("inf")))
                align()  # (kernel loading is not timed)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                aligned = align()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                q.copy_(aligned.quat)
                t.copy_(aligned.trans)
            n = aligned.stats.shape[0]
            print(f"rgbd  : rotation error {err()[0]:.2e}, translation error {err()[1]:.2e}, {int(aligned.stats[:, 31].sum())} of {n} "
                  f"steps accepted, {int(aligned.stats[-1, 28])} geometric and {int(aligned.stats[-1, 30])} photometric pairs, "
                  f"{dt / n * 1e6:.1f} us per iteration (eager, {args.rgbd_levels} level{'s' if args.rgbd_levels > 1 else ''}, maps included)")
        if args.graph:
            step = CapturedStep(iteration, warmup=3)  # (three eager iterations first)
            run = step.replay
        else:
            for _ in range(3):  # the same three iterations, so that one-time costs (kernel loading, optimiser set-up) are not timed
                iteration()
            run = iteration
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reached = None
        for i in range(args.iters):
            loss = run()
            if args.reach and reached is None and err()[0] <= args.reach[0] and err()[1] <= args.reach[1]:
                reached = i + 1
            if args.trace and (i + 1) % args.trace == 0:
                e = err()
                print(f"  iteration {i + 1}: rotation error {e[0]:.2e}, translation error {e[1]:.2e}")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if args.graph:
            step.check()
        print(f"finish: rotation error {err()[0]:.2e}, translation error {err()[1]:.2e}, loss {float(loss):.3e}")
        if args.reach:
            print(f"reach : rotation error {args.reach[0]:.2e} and translation error {args.reach[1]:.2e} "
                  f"{'after ' + str(reached) + ' iterations' if reached else 'not within ' + str(args.iters) + ' iterations'}")
        print(f"{args.iters} iterations in {dt * 1e3:.1f} ms = {dt / args.iters * 1e3:.3f} ms per tracking iteration"
              f" ({'hipGraph replay' if args.graph else 'eager'}{', fused pose and loss' if args.fused else ''}"
              f"{', masked loss' if masked else ''}{', complete pose gradient' if args.complete_pose else ''})")
        return err()

    plain = track(False)
    if args.masked:
        kept = track(True)
        print(f"final pose error, plain L1 -> masked: rotation {plain[0]:.2e} -> {kept[0]:.2e}, "
              f"translation {plain[1]:.2e} -> {kept[1]:.2e}")


if __name__ == "__main__":
    main()
