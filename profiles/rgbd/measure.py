#!/usr/bin/env python3
"""Times the hybrid RGB-D steps at 640 x 480 on the textured room corner of the tests (tests/test_rgbd_model.py: corner_frame),
replayed from a hipGraph, by the method of profiles/icp/measure.py (whose helpers it imports): a graph of --chain chained calls,
--repeats repeats of --replays replays, min / median / max over the repeats.
  intensity_map   slam.intensity_map (one channel) beside slam.depth_normals, one launch per call each
  halve_frame     one pyramid level of (I_model, silhouette, depth), one launch
  rgbd step       dgr_amd.rgbd.rgbd_step at strides 1 and 4 beside dgr_amd.icp.icp_step of the same build on the same frame, in
                  the same process, the two chains timed alternately
  torch step      the hybrid iteration in torch ops (profiles/icp/measure.py's torch_sums with the photometric rows added),
                  the part in front of the solve replayed from a graph
  rgbd_align      the whole call, five levels of six iterations, replayed from a graph
Algorithmic bytes of the hybrid step: 4 (depth) + 4 (intensity) + 16 + 16 (the model's two maps) + 16 (observation normals) per
candidate and iteration.

  python profiles/rgbd/measure.py [--repeats 9] [--out profiles/rgbd/measure.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles", "icp")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import measure as icp_measure  # noqa: E402  (profiles/icp/measure.py)
from dgr_amd import icp, rgbd, slam  # noqa: E402
from test_rgbd_model import corner_frame  # noqa: E402

W, H = 640, 480
captured, timed = icp_measure.captured, icp_measure.timed


def torch_hybrid_sums(depth, vn_obs, vn_model, i_obs, imap, rel, fx, fy, cx, cy, stride, dist_max=0.1, cos_min=0.8):
    """A [6,6] and b [6] of one hybrid iteration in torch ops (both weights 1): the 27 products of either pair in fp32, each
    column summed in float64"""
    d, no, io = depth[::stride, ::stride], vn_obs[::stride, ::stride], i_obs[::stride, ::stride]
    ys, xs = torch.meshgrid(torch.arange(0, H, stride, device=depth.device, dtype=torch.float32),
                            torch.arange(0, W, stride, device=depth.device, dtype=torch.float32), indexing="ij")
    valid = (d > 0) & (no[..., 3] > 0)
    p = torch.stack([(xs - cx) / fx * d, (ys - cy) / fy * d, d], -1)
    q = p @ rel[:3, :3].T + rel[:3, 3]
    uf, vf = fx * q[..., 0] / q[..., 2] + cx, fy * q[..., 1] / q[..., 2] + cy
    u, v = torch.floor(uf + 0.5), torch.floor(vf + 0.5)
    inside = valid & (q[..., 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    ui, vi = u.clamp(0, W - 1).long(), v.clamp(0, H - 1).long()
    m, im = vn_model[vi, ui], imap[vi, ui]
    n, dm = m[..., :3], m[..., 3]
    e = q - torch.stack([(u - cx) / fx * dm, (v - cy) / fy * dm, dm], -1)
    close = inside & (dm > 0) & (e.norm(dim=-1) <= dist_max)
    ok_g = close & (((no[..., :3] @ rel[:3, :3].T) * n).sum(-1) >= cos_min)
    ok_p = close & (im[..., 3] == 1)
    r_g = (n * e).sum(-1)
    r_p = im[..., 0] + im[..., 1] * (uf - u) + im[..., 2] * (vf - v) - io
    g0, g1 = im[..., 1] * fx / q[..., 2], im[..., 2] * fy / q[..., 2]
    g = torch.stack([g0, g1, -(g0 * q[..., 0] + g1 * q[..., 1]) / q[..., 2]], -1)
    iu = torch.triu_indices(6, 6, device=depth.device)
    total = 0
    for ok, vec, r in ((ok_g, n, r_g), (ok_p, g, r_p)):
        J = torch.cat([torch.cross(q, vec, dim=-1), vec], -1)
        J = torch.where(ok[..., None], J, torch.zeros_like(J)).reshape(-1, 6)
        r = torch.where(ok, r, torch.zeros_like(r)).reshape(-1)
        total = total + torch.cat([J[:, iu[0]] * J[:, iu[1]], J * r[:, None]], 1).sum(0, dtype=torch.float64)
    A = torch.zeros((6, 6), dtype=torch.float64, device=depth.device)
    A[iu[0], iu[1]] = total[:21]
    return A + torch.triu(A, 1).T, total[21:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = corner_frame(W, H)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    fx, fy, cx, cy = s["fx"], s["fy"], s["cx"], s["cy"]
    depth_obs, model_depth, model_view = T(s["depth_obs"]), T(s["model_depth"]), T(s["model_view"])
    color_obs, model_color = T(s["color_obs"]), T(s["model_color"])
    vn_model, vn_obs = slam.depth_normals(model_depth, fx, fy, cx, cy), slam.depth_normals(depth_obs, fx, fy, cx, cy)
    imap = slam.intensity_map(model_color)
    res = dict(frame=[W, H], chain=args.chain, replays=args.replays)

    # ---- the per-pixel launches
    out = torch.empty((H, W, 4), device=dev)
    sc = dict(fx=fx, fy=fy, cx=cx, cy=cy, max_jump=0.1, mask_threshold=0.99)
    planes, half_p, half_d = torch.stack([model_color, torch.ones_like(model_color)]), torch.empty((2, H // 2, W // 2), device=dev), \
        torch.empty((H // 2, W // 2), device=dev)

    def chain_of(call):
        def run():
            with rgbd._capi.StepCalls(dev) as abi:
                for _ in range(args.chain):
                    call(abi)
        return run

    for name, call, nbytes in (
            ("depth_normals", lambda abi: icp._normals_into(abi, out, depth_obs, None, sc, 0.0, float("inf")), W * H * 20),
            ("intensity_map", lambda abi: rgbd._intensity_into(abi, model_color[None], None, 0.0, out, None), W * H * 20),
            ("frame_halve", lambda abi: rgbd._halve_into(abi, planes, model_depth, 0.0, float("inf"), 0.1, half_p, half_d), W * H * 15)):
        r = timed(captured(chain_of(call)), args.chain, args.repeats, args.replays)
        r["bytes"], r["GB_per_s"] = nbytes, nbytes / r["median_us"] * 1e-3
        res[name] = r

    # ---- the steps
    for stride in (1, 4):
        S = -(-W // stride) * -(-H // stride)
        pose = model_view.clone()
        scratch = torch.zeros(rgbd._capi.load().dgr_rgbd_scratch_bytes(W, H, stride), dtype=torch.uint8, device=dev)

        def hybrid_chain(n=args.chain):
            pose.copy_(model_view)
            for _ in range(n):
                rgbd.rgbd_step(depth_obs, vn_obs, vn_model, color_obs, imap, model_view, pose, fx, fy, cx, cy, viewmatrix_out=pose,
                               stride=stride, scratch=scratch)

        def icp_chain(n=args.chain):
            pose.copy_(model_view)
            for _ in range(n):
                icp.icp_step(depth_obs, vn_obs, vn_model, model_view, pose, fx, fy, cx, cy, viewmatrix_out=pose, stride=stride,
                             scratch=scratch)

        g_h, g_i = captured(hybrid_chain), captured(icp_chain)
        rows = {"rgbd": [], "icp": []}
        for _ in range(3):  # alternately, so that neither has the machine's better minute
            rows["rgbd"].append(timed(g_h, args.chain, args.repeats, args.replays))
            rows["icp"].append(timed(g_i, args.chain, args.repeats, args.replays))
        best = {k: min(v, key=lambda r: r["median_us"]) for k, v in rows.items()}
        for k, nb in (("rgbd", 56), ("icp", 36)):
            best[k]["bytes"], best[k]["GB_per_s"] = S * nb, S * nb / best[k]["median_us"] * 1e-3
            best[k]["medians_us"] = [r["median_us"] for r in rows[k]]
        best["rgbd"]["single_step_graph"] = timed(captured(lambda: hybrid_chain(1)), 1, args.repeats, args.replays)
        rel0 = torch.eye(4, device=dev)
        t = timed(captured(lambda: torch_hybrid_sums(depth_obs, vn_obs, vn_model, color_obs, imap, rel0, fx, fy, cx, cy, stride)), 1,
                  args.repeats, args.replays)
        res[f"stride{stride}"] = dict(candidates=S, rgbd=best["rgbd"], icp=best["icp"], torch_sums_graph=t,
                                      rgbd_over_icp=best["rgbd"]["median_us"] / best["icp"]["median_us"],
                                      torch_sums_graph_over_rgbd=t["median_us"] / best["rgbd"]["median_us"])

    # ---- the whole call
    def whole():
        slam.rgbd_align(color_obs, depth_obs, model_color, model_depth, None, model_view, fx, fy, cx, cy, levels=5, iterations=6)
    res["rgbd_align_5_levels_x_6"] = timed(captured(whole), 1, args.repeats, args.replays)

    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    fmt = lambda r: f"{r['median_us']:.1f} ({r['min_us']:.1f} .. {r['max_us']:.1f})"  # noqa: E731
    print("| step | us per call, median (min .. max) | algorithmic bytes | GB/s |\n|---|---|---|---|")
    for name in ("depth_normals", "intensity_map", "frame_halve"):
        print(f"| {name} 640 x 480 | {fmt(res[name])} | {res[name]['bytes']} | {res[name]['GB_per_s']:.0f} |")
    for stride in (1, 4):
        r = res[f"stride{stride}"]
        for k in ("rgbd", "icp"):
            print(f"| {k} step, stride {stride} ({r['candidates']} candidates), chained in a graph | {fmt(r[k])} | {r[k]['bytes']} | "
                  f"{r[k]['GB_per_s']:.0f} |")
        print(f"| ... rgbd / icp | {r['rgbd_over_icp']:.2f} | | |")
        print(f"| ... a graph of one rgbd step | {fmt(r['rgbd']['single_step_graph'])} | | |")
        print(f"| torch ops, graph, hybrid sums only | {fmt(r['torch_sums_graph'])} ({r['torch_sums_graph_over_rgbd']:.0f}x) | | |")
    print(f"| rgbd_align, 5 levels x 6 iterations, one graph | {fmt(res['rgbd_align_5_levels_x_6'])} | | |")


if __name__ == "__main__":
    main()
