#!/usr/bin/env python3
"""Times the keyframe overlap scores of one 640 x 480 frame (stride 16: 1200 candidates, edge 20) against K = 8, 64 and 512 stored
keyframes, three ways:
  fused       slam.keyframe_overlap: one call, one launch, nothing read on the host
  torch_loop  the step as SplaTAM's keyframe_selection_overlap writes it, in torch ops on the GPU over the same candidates: a
              `where` over the valid depths (a host synchronisation), then a Python loop over the keyframes -- homogeneous
              transform, projection through the intrinsics matrix, the four border tests -- with one host read per keyframe
  torch_batch the same arithmetic vectorised over K (one batched matmul), one host read of all K scores
Wall time of a call including its launches, a host clock around the call and one synchronize at its end; the median of --calls
after warm-up, each variant in a timed run of its own.  The scores of the three are compared first.

  python profiles/keyframe_overlap/measure.py [--calls 30] [--out profiles/keyframe_overlap/measure.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "diff-gaussian-rasterization_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dgr_amd import slam  # noqa: E402

W, H, STRIDE, EDGE = 640, 480, 16, 20.0
FX, FY, CX, CY = 517.3, 516.5, 318.6, 255.3  # TUM RGB-D's freiburg1 intrinsics
KEYFRAMES = (8, 64, 512)


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Km = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Km + (1 - np.cos(angle)) * Km @ Km


def make(K, dev, seed=0):
    """(depth [H,W] with 5 % holes, W2C of the frame [4,4], W2C of the keyframes [K,4,4]): poses up to 0.6 rad and 0.5 units away"""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(1.0, 4.0, (H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.05] = 0.0
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = rotation([0.2, 1.0, 0.1], 0.3), [0.05, -0.02, 0.10]
    kfs = []
    for _ in range(K):
        m = np.eye(4)
        m[:3, :3] = rotation(rng.normal(size=3), rng.uniform(0.0, 0.6)) @ w2c[:3, :3]
        m[:3, 3] = -m[:3, :3] @ (-w2c[:3, :3].T @ w2c[:3, 3] + rng.uniform(-0.5, 0.5, 3))
        kfs.append(m)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    return t(depth), t(w2c), t(np.stack(kfs))


def grid_points(depth, w2c, intrinsics):
    """The valid candidates as world points [n, 3]: a `where` over the valid depths, as SplaTAM compacts its samples (a host
    synchronisation: the result's size)."""
    grid = depth[::STRIDE, ::STRIDE]
    ys, xs = torch.where(grid > 0)
    d = grid[ys, xs]
    x, y = xs.float() * STRIDE, ys.float() * STRIDE
    cam = torch.stack([(x - intrinsics[0, 2]) / intrinsics[0, 0] * d, (y - intrinsics[1, 2]) / intrinsics[1, 1] * d, d,
                       torch.ones_like(d)], dim=1)
    return (torch.inverse(w2c) @ cam.T).T[:, :3]


def inside_mask(points_2d):
    z = points_2d[..., 2:] + 1e-5
    uv = points_2d / z
    return ((uv[..., 0] < W - EDGE) & (uv[..., 0] > EDGE) & (uv[..., 1] < H - EDGE) & (uv[..., 1] > EDGE) & (z[..., 0] > 0))


def torch_loop(depth, w2c, kf_w2c, intrinsics):
    pts = grid_points(depth, w2c, intrinsics)
    pts4 = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)
    scores = []
    for k in range(kf_w2c.shape[0]):
        transformed = (kf_w2c[k] @ pts4.T).T[:, :3]
        mask = inside_mask(torch.matmul(intrinsics, transformed.transpose(0, 1)).transpose(0, 1))
        scores.append(float(mask.sum() / pts.shape[0]))  # (the host read: the scores are sorted on the host)
    return scores


def torch_batch(depth, w2c, kf_w2c, intrinsics):
    pts = grid_points(depth, w2c, intrinsics)
    pts4 = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)
    transformed = (kf_w2c @ pts4.T).transpose(1, 2)[..., :3]  # [K, n, 3]
    mask = inside_mask(transformed @ intrinsics.T)
    return (mask.sum(1) / pts.shape[0]).tolist()  # (the one host read)


def timed(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), calls=calls)


def measure(K, calls, dev):
    depth, w2c, kf_w2c = make(K, dev)
    view, kf_views = w2c.T.contiguous(), kf_w2c.transpose(1, 2).contiguous()
    intrinsics = torch.tensor([[FX, 0.0, CX], [0.0, FY, CY], [0.0, 0.0, 1.0]], device=dev)

    def fused():
        return slam.keyframe_overlap(depth, view, kf_views, FX, FY, CX, CY, stride=STRIDE, edge=EDGE)

    out = fused()
    valid = int(out.valid[0])
    ref_loop, ref_batch = torch_loop(depth, w2c, kf_w2c, intrinsics), torch_batch(depth, w2c, kf_w2c, intrinsics)
    got = out.score.tolist()
    # the three agree up to the pairs that the restatement's z + 1e-5 (0.006 px at the frame's edge) or an fp32 evaluation order
    # moves across a border: a few of the `valid` candidates, where a slip in a convention moves hundreds
    worst = max(max(abs(a - b), abs(a - c)) for a, b, c in zip(got, ref_loop, ref_batch)) * valid
    assert worst <= 0.01 * valid, f"K = {K}: the fused scores and the torch ones differ by {worst:.1f} candidates"
    res = dict(keyframes=K, candidates=-(-W // STRIDE) * -(-H // STRIDE), valid=valid,
               mean_score=sum(got) / K, worst_count_difference=worst)
    res["fused"] = timed(fused, calls)
    res["torch_loop"] = timed(lambda: torch_loop(depth, w2c, kf_w2c, intrinsics), calls)
    res["torch_batch"] = timed(lambda: torch_batch(depth, w2c, kf_w2c, intrinsics), calls)
    res["loop_over_fused"] = res["torch_loop"]["median_ms"] / res["fused"]["median_ms"]
    res["batch_over_fused"] = res["torch_batch"]["median_ms"] / res["fused"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {f"K{K}": measure(K, args.calls, dev) for K in KEYFRAMES}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print("| K | fused, ms | torch loop, ms | torch batched, ms |\n|---|---|---|---|")
    for r in res.values():
        print(f"| {r['keyframes']} | {r['fused']['median_ms']:.3f} | {r['torch_loop']['median_ms']:.3f} ({r['loop_over_fused']:.0f}x) | "
              f"{r['torch_batch']['median_ms']:.3f} ({r['batch_over_fused']:.1f}x) |")


if __name__ == "__main__":
    main()
