#!/usr/bin/env python3
"""Loop edges by generalized ICP, straight into the pose graph (a SLAM back end's registration step in miniature).

K keyframes on a ring look into a synthetic room corner (three planes).  Their depth frames are unprojected into camera-frame
clouds (slam.unproject_depth: unusable pixels become NaN rows, no compaction) and every cloud gets its neighbourhood covariances
(slam.point_covariances: one kNN search and one launch).  The keyframes' pose estimates carry injected drift that grows along the
trajectory, as a tracker's does.  Then
  slam.gicp_align        between consecutive keyframes and across the loop (last against first), each started from the relative
                         pose of the DRIFTED estimates: nearest neighbours in 3-D, plane-to-plane Gauss-Newton steps, a fixed
                         number of them, nothing read on the host
  slam.pose_graph_optimize  takes the results as they are: gicp_align's transform has the layout of an edge's measurement
                         (source = camera j's cloud, target = camera i's: Z_ij), so there is no conversion in between
and the run prints each edge's error to the truth before and after the alignment, and the trajectory's error before and after the
optimisation.  Where examples/mapping.py --pgo takes its loop edge from the true poses, this one measures it.
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd")]

import torch  # noqa: E402

CORNER = (1.6, 1.1, 3.0)  # the planes x = 1.6, y = 1.1, z = 3.0


def look_at(centre, target):
    """W2C^T (float64 [4,4]) of a camera at `centre` whose z axis points at `target`, y roughly down the world's y"""
    z = target - centre
    z = z / z.norm()
    x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), z)
    x = x / x.norm()
    y = torch.linalg.cross(z, x)
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = torch.stack([x, y, z])
    m[:3, 3] = -m[:3, :3] @ centre
    return m.T.contiguous()


def ring_poses(K, radius=0.3):
    """K cameras on a circle of `radius` around (0.2, -0.1, 0.3), in the plane across the view of the corner, all looking at a point
    in front of it"""
    c0, corner = torch.tensor([0.2, -0.1, 0.3], dtype=torch.float64), torch.tensor(CORNER, dtype=torch.float64)
    f = (corner - c0) / (corner - c0).norm()
    u = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), f)
    u = u / u.norm()
    v = torch.linalg.cross(f, u)
    target = c0 + 0.85 * (corner - c0)
    return torch.stack([look_at(c0 + radius * (math.cos(2 * math.pi * k / K) * u + math.sin(2 * math.pi * k / K) * v), target)
                        for k in range(K)])


def corner_depth(view, W, H, fx, fy, cx, cy):
    """the depth image (float32 [H,W]) of the room corner from the pose `view` (W2C^T, float64): ray-plane intersections"""
    m = view.T
    R, t = m[:3, :3], m[:3, 3]
    centre = -R.T @ t
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    rays = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(x)], -1) @ R  # the camera rays in the world
    depth = torch.full((H, W), float("inf"), dtype=torch.float64)
    for axis, value in enumerate(CORNER):
        s = (value - centre[axis]) / rays[..., axis]
        depth = torch.where((s > 0) & (s < depth), s, depth)
    return torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth)).float()


def twist_matrix(w, v):
    """exp of the twist (w, v) as a float64 [4,4] rigid motion (Rodrigues)"""
    th = w.norm()
    K = torch.tensor([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], dtype=torch.float64)
    A, B, C = (torch.sin(th) / th, (1 - torch.cos(th)) / th ** 2, (th - torch.sin(th)) / th ** 3) if th > 1e-9 else (1.0, 0.5, 1.0 / 6.0)
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = torch.eye(3, dtype=torch.float64) + A * K + B * K @ K
    m[:3, 3] = (torch.eye(3, dtype=torch.float64) + B * K + C * K @ K) @ v
    return m


def drifted(views, rot, trans, seed):
    """the estimates of a tracker that drifts: pose k is the true one moved by the product of k random twists of size (rot, trans)"""
    g = torch.Generator().manual_seed(seed)
    out, E = [views[0]], torch.eye(4, dtype=torch.float64)
    for k in range(1, len(views)):
        w, v = torch.randn(3, generator=g, dtype=torch.float64), torch.randn(3, generator=g, dtype=torch.float64)
        E = twist_matrix(rot * w / w.norm(), trans * v / v.norm()) @ E
        out.append((E @ views[k].T).T.contiguous())
    return torch.stack(out)


def motion_error(a, b):
    """(angle in rad, distance of the translations) between two [4,4] transposed motions"""
    a, b = a.double().cpu().T, b.double().cpu().T
    D = a[:3, :3] @ b[:3, :3].T
    sine = 0.5 * torch.stack([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]).norm()
    return float(torch.atan2(sine, 0.5 * (D.trace() - 1.0))), float((a[:3, 3] - b[:3, 3]).norm())


def centres(views):
    m = views.double().cpu().transpose(-1, -2)
    return -(m[:, :3, :3].transpose(-1, -2) @ m[:, :3, 3:])[..., 0]


def run(device, K=6, W=96, H=72, stride=2, iterations=15, k=10, drift_rot=0.008, drift_trans=0.012, max_distance=0.3, seed=0):
    from dgr_amd import slam
    fx = fy = 0.8 * W
    cx, cy = (W - 1) / 2, (H - 1) / 2
    truth = ring_poses(K)
    estimate = drifted(truth, drift_rot, drift_trans, seed)
    clouds, covs = [], []
    for v in truth:
        depth = corner_depth(v, W, H, fx, fy, cx, cy).to(device)
        clouds.append(slam.unproject_depth(depth, fx, fy, cx, cy, stride=stride))
        covs.append(slam.point_covariances(clouds[-1], k=k, viewpoint=(0.0, 0.0, 0.0)))
    truth32, estimate32 = truth.float().to(device), estimate.float().to(device)
    pairs = [(i, i + 1) for i in range(K - 1)] + [(0, K - 1)]  # the trajectory's edges, then the loop
    measured, rows = [], []
    for i, j in pairs:
        start = slam.relative_pose(estimate32[i], estimate32[j])  # Z_ij as the drifted estimates have it
        want = slam.relative_pose(truth32[i], truth32[j])
        # source = camera j's cloud, target = camera i's: the result maps j's coordinates to i's, which is Z_ij
        out = slam.gicp_align(clouds[j], clouds[i], transform=start, source_cov=covs[j], target_cov=covs[i], target_index=covs[i].index,
                              iterations=iterations, max_distance=max_distance)
        measured.append(out.transform)
        rows.append(dict(edge=(i, j), before=motion_error(start, want), after=motion_error(out.transform, want),
                         pairs=int(out.stats[-1, 28]), ok=bool(out.stats[:, 29].all())))
    edges = torch.tensor(pairs, dtype=torch.int32, device=device)
    solved = slam.pose_graph_optimize(estimate32, edges, torch.stack(measured), iterations=20)
    c_true = centres(truth32)
    before = float((centres(estimate32) - c_true).norm(dim=1).mean())
    after = float((centres(solved.viewmatrices) - c_true).norm(dim=1).mean())
    return dict(edges=rows, trajectory_before=before, trajectory_after=after, points=int(clouds[0].shape[0]),
                pgo_ok=bool(solved.stats[2] == 1.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--keyframes", type=int, default=6)
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--height", type=int, default=72)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=15)
    ap.add_argument("--k", type=int, default=10, help="neighbours per covariance")
    ap.add_argument("--drift-rot", type=float, default=0.008, help="drift per keyframe, rad")
    ap.add_argument("--drift-trans", type=float, default=0.012, help="drift per keyframe, m")
    ap.add_argument("--max-distance", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.keyframes < 3:
        ap.error("--keyframes must be at least 3: a loop needs them")
    if not torch.cuda.is_available():
        sys.exit("registration.py needs a GPU (there is no CPU fallback)")
    r = run(torch.device("cuda:0"), a.keyframes, a.width, a.height, a.stride, a.iterations, a.k, a.drift_rot, a.drift_trans,
            a.max_distance, a.seed)
    print(f"{a.keyframes} keyframes, {r['points']} points each, {a.iterations} iterations per edge")
    for e in r["edges"]:
        i, j = e["edge"]
        kind = "loop" if j - i > 1 else "step"
        print(f"edge {i} <- {j} ({kind}): {e['before'][0]:.2e} rad {e['before'][1]:.2e} m -> {e['after'][0]:.2e} rad {e['after'][1]:.2e} m"
              f"  ({e['pairs']} pairs{'' if e['ok'] else ', a step was refused'})")
    print(f"trajectory error {r['trajectory_before']:.3e} m -> {r['trajectory_after']:.3e} m after pose_graph_optimize")
    return r


if __name__ == "__main__":
    main()
