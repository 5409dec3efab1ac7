#!/usr/bin/env python3
"""Times the two ICP steps at 640 x 480 on the room-corner scene of the tests (tests/icp_model.py), replayed from a hipGraph:
  depth_normals   slam.depth_normals, one launch per call
  icp step        dgr_amd.icp.icp_step at strides 1 and 4, with the observation's normals: one launch per iteration, the
                  iterations chained through one device pose buffer as slam.icp_align chains them
  torch step      the same iteration written in torch ops on the same candidates (gathers, masks as weights instead of a
                  compaction, the 27 products in fp32 and their columns summed in float64 as the fused step forms them,
                  torch.linalg.solve, the update): the yardstick the earlier steps used;
                  the parent commit has no such step.  It is timed eagerly (its solve does not record into a graph here) and, for
                  the part in front of the solve, replayed from a graph as well.
Each graph holds --chain calls; a repeat is --replays replays between two events, and the time per call is the repeat's time over
chain * replays.  --repeats repeats after warm-up; the table gives min / median / max over the repeats.  Achieved bytes/s is on the
algorithmic bytes: 4 (depth) + 16 (model map) + 16 (observation map) per candidate and iteration, 4 + 16 per pixel for the normals.

  python profiles/icp/measure.py [--repeats 9] [--out profiles/icp/measure.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import icp_model as M  # noqa: E402
from dgr_amd import icp, slam  # noqa: E402

W, H = 640, 480


def captured(fn, warmup=3):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def timed(run, calls_per_run, repeats, replays, warmup=5):
    """microseconds per call: min / median / max over `repeats` repeats of `replays` runs each"""
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            run()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / (replays * calls_per_run))
    return dict(min_us=min(us), median_us=statistics.median(us), max_us=max(us), repeats=repeats, calls=replays * calls_per_run)


def torch_sums(depth, vn_obs, vn_model, rel, fx, fy, cx, cy, stride, dist_max=0.1, cos_min=0.8, gemm64=False):
    """A [6,6] and b [6] of one iteration in torch ops, nothing read on the host.  The sums as the fused step forms them: the 27
    products in fp32, each column summed in float64.  gemm64: J^T J and J^T r as float64 matrix products instead (the obvious
    way to write it, and far slower here: kept as a second row)"""
    d = depth[::stride, ::stride]
    no = vn_obs[::stride, ::stride]
    ys, xs = torch.meshgrid(torch.arange(0, H, stride, device=depth.device, dtype=torch.float32),
                            torch.arange(0, W, stride, device=depth.device, dtype=torch.float32), indexing="ij")
    valid = (d > 0) & (no[..., 3] > 0)
    p = torch.stack([(xs - cx) / fx * d, (ys - cy) / fy * d, d], -1)
    q = p @ rel[:3, :3].T + rel[:3, 3]
    u, v = torch.floor(fx * q[..., 0] / q[..., 2] + cx + 0.5), torch.floor(fy * q[..., 1] / q[..., 2] + cy + 0.5)
    inside = valid & (q[..., 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    ui, vi = u.clamp(0, W - 1).long(), v.clamp(0, H - 1).long()
    m = vn_model[vi, ui]
    n, dm = m[..., :3], m[..., 3]
    vm = torch.stack([(u - cx) / fx * dm, (v - cy) / fy * dm, dm], -1)
    e = q - vm
    ok = inside & (dm > 0) & (e.norm(dim=-1) <= dist_max) & (((no[..., :3] @ rel[:3, :3].T) * n).sum(-1) >= cos_min)
    r = (n * e).sum(-1)
    J = torch.cat([torch.cross(q, n, dim=-1), n], -1)
    J = torch.where(ok[..., None], J, torch.zeros_like(J)).reshape(-1, 6)
    r = torch.where(ok, r, torch.zeros_like(r)).reshape(-1)
    if gemm64:
        J, r = J.double(), r.double()
        return J.T @ J, J.T @ r
    iu = torch.triu_indices(6, 6, device=J.device)
    sums = torch.cat([J[:, iu[0]] * J[:, iu[1]], J * r[:, None]], 1).sum(0, dtype=torch.float64)  # [S, 27] fp32 -> 27 doubles
    A = torch.zeros((6, 6), dtype=torch.float64, device=J.device)
    A[iu[0], iu[1]] = sums[:21]
    return A + torch.triu(A, 1).T, sums[21:]


def torch_update(A, b, view_in, model_view):
    """the solve and T_out = T_in T_model^-1 exp(-xi) T_model, float64 torch ops"""
    xi = torch.linalg.solve(A, -b)
    twist = torch.zeros((4, 4), dtype=torch.float64, device=A.device)
    w, v = -xi[:3], -xi[3:]
    twist[0, 1], twist[0, 2], twist[1, 0], twist[1, 2], twist[2, 0], twist[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
    twist[:3, 3] = v
    Tm, Ti = model_view.double().T, view_in.double().T
    return (Ti @ torch.linalg.inv(Tm) @ torch.linalg.matrix_exp(twist) @ Tm).T.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = M.corner_scene(W, H)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    fx, fy, cx, cy = s["fx"], s["fy"], s["cx"], s["cy"]
    depth_obs, model_depth, model_view = T(s["depth_obs"]), T(s["model_depth"]), T(s["model_view"])
    vn_model, vn_obs = slam.depth_normals(model_depth, fx, fy, cx, cy), slam.depth_normals(depth_obs, fx, fy, cx, cy)
    res = dict(frame=[W, H], chain=args.chain, replays=args.replays)

    # ---- the normals
    out = torch.empty((H, W, 4), device=dev)
    sc = dict(fx=fx, fy=fy, cx=cx, cy=cy, max_jump=0.1, mask_threshold=0.99)

    def normals_chain():
        with icp._capi.StepCalls(dev) as abi:  # (the stream that is current now: the one being recorded)
            for _ in range(args.chain):
                icp._normals_into(abi, out, depth_obs, None, sc, 0.0, float("inf"))
    r = timed(captured(normals_chain), args.chain, args.repeats, args.replays)
    r["bytes"] = W * H * 20
    r["GB_per_s"] = r["bytes"] / r["median_us"] * 1e-3
    res["depth_normals"] = r

    # ---- the step, fused and in torch ops
    for stride in (1, 4):
        S = -(-W // stride) * -(-H // stride)
        pose = model_view.clone()
        scratch = torch.zeros(icp._capi.load().dgr_icp_scratch_bytes(W, H, stride), dtype=torch.uint8, device=dev)

        def fused_chain(n=args.chain):
            pose.copy_(model_view)
            for _ in range(n):
                icp.icp_step(depth_obs, vn_obs, vn_model, model_view, pose, fx, fy, cx, cy, viewmatrix_out=pose, stride=stride,
                             scratch=scratch)

        fused_chain()
        torch.cuda.synchronize()
        e_fused = M.pose_error(pose.cpu().numpy(), s["true_view"])
        # (the chain's time includes one 64-byte copy per chain-many steps)
        r = timed(captured(fused_chain), args.chain, args.repeats, args.replays)
        r1 = timed(captured(lambda: fused_chain(1)), 1, args.repeats, args.replays)
        r["bytes"] = S * 36
        r["GB_per_s"] = r["bytes"] / r["median_us"] * 1e-3
        r["single_step_graph"] = r1
        r["pose_error_after_chain"] = e_fused

        tpose = model_view.clone()

        def torch_step():
            rel = (model_view.double().T @ torch.linalg.inv(tpose.double().T)).float()
            A, b = torch_sums(depth_obs, vn_obs, vn_model, rel, fx, fy, cx, cy, stride)
            tpose.copy_(torch_update(A, b, tpose, model_view))

        def torch_chain():
            tpose.copy_(model_view)
            for _ in range(args.chain):
                torch_step()

        torch_chain()
        torch.cuda.synchronize()
        e_torch = M.pose_error(tpose.cpu().numpy(), s["true_view"])
        assert max(abs(a - b) for a, b in zip(e_fused, e_torch)) < 1e-4, (e_fused, e_torch)  # the same iteration, to its pairs
        t = timed(torch_chain, args.chain, args.repeats, max(1, args.replays // 10))
        rel0 = torch.eye(4, device=dev)
        t["sums_only_graph"] = timed(captured(lambda: torch_sums(depth_obs, vn_obs, vn_model, rel0, fx, fy, cx, cy, stride)), 1,
                                     args.repeats, args.replays)
        t["sums_only_graph_gemm64"] = timed(captured(lambda: torch_sums(depth_obs, vn_obs, vn_model, rel0, fx, fy, cx, cy, stride,
                                                                        gemm64=True)), 1, args.repeats, max(1, args.replays // 4))
        t["pose_error_after_chain"] = e_torch
        res[f"stride{stride}"] = dict(candidates=S, fused=r, torch=t, torch_over_fused=t["median_us"] / r["median_us"],
                                      torch_sums_graph_over_fused=t["sums_only_graph"]["median_us"] / r["median_us"])

    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    fmt = lambda r: f"{r['median_us']:.1f} ({r['min_us']:.1f} .. {r['max_us']:.1f})"  # noqa: E731
    print("| step | us per call, median (min .. max) | algorithmic bytes | GB/s |\n|---|---|---|---|")
    n = res["depth_normals"]
    print(f"| depth_normals 640 x 480 | {fmt(n)} | {n['bytes']} | {n['GB_per_s']:.0f} |")
    for stride in (1, 4):
        r = res[f"stride{stride}"]
        print(f"| icp step, stride {stride} ({r['candidates']} candidates), chained in a graph | {fmt(r['fused'])} | {r['fused']['bytes']} | "
              f"{r['fused']['GB_per_s']:.0f} |")
        print(f"| ... a graph of one step | {fmt(r['fused']['single_step_graph'])} | | |")
        print(f"| torch ops, eager, whole iteration | {fmt(r['torch'])} ({r['torch_over_fused']:.0f}x) | | |")
        print(f"| torch ops, graph, sums only | {fmt(r['torch']['sums_only_graph'])} ({r['torch_sums_graph_over_fused']:.0f}x) | | |")
        print(f"| torch ops, graph, sums only, as float64 matrix products | {fmt(r['torch']['sums_only_graph_gemm64'])} | | |")


if __name__ == "__main__":
    main()
