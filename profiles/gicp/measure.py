"""Timing of dgr_point_covariances and dgr_gicp_step from hipGraph replays, beside the same iteration in torch ops on the same GPU,
at S = N = 19 200 (a 640 x 480 depth frame at stride 4) and 76 800 (stride 2): two views of the room corner of
examples/registration.py, unprojected.

Per size: the kNN build and the self search that feed the covariances (k = 10), the covariance launch itself; then per
iteration the whole dgr_gicp_step, the cross-mode search alone (dgr_knn_search on the moved source: the very launches the step
makes), and their difference, which is the transform kernel plus the fused step kernel -- a difference of two medians that each
lie about 10 us above their minimum, so it is good to a few tens of microseconds; the two kernels have no entry point of their
own.  The torch-ops iteration is a chunked cdist + argmin over S x N, a batched 3 x 3 inverse in closed form and the [S,6,6]
einsums, timed eagerly (one warm-up run, then the median of three).  Kernel times are medians of the replays.

  python profiles/gicp/measure.py [--replays 30]
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "..", "diff-gaussian-rasterization_amd"), os.path.join(HERE, "..", "..", "examples")]
from dgr_amd import _capi, gicp, knn  # noqa: E402
from dgr_amd.posegraph import relative_pose  # noqa: E402
import registration as reg  # noqa: E402

KEEP = []  # the graphs stay alive: what a captured call returned lives in their memory pools


def replay_time(fn, replays):
    # what fn reads or uses as scratch was made on the current stream (a zero-fill among it): finished before the side stream starts.
    # A scratch still being filled while the search sorts through it ends in a read at an arbitrary address
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = fn()
    KEEP.append(graph)
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return out, float(np.median(times)), float(np.min(times))


def eager_time(fn, runs=3):
    torch.cuda.synchronize()
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return out, float(np.median(times))


def unpack(rows):
    c = rows[:, :6]
    return torch.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], 1).double()


def torch_iteration(src, tgt, cs, ct, T, chunk=8192):
    """the same Gauss-Newton sums in torch ops: (A [6,6], b [6]) in float64"""
    m = T.T
    R, t = m[:3, :3], m[:3, 3]
    q = src @ R.T + t
    idx = torch.empty(len(q), dtype=torch.long, device=q.device)
    for a in range(0, len(q), chunk):
        idx[a:a + chunk] = torch.cdist(q[a:a + chunk], tgt).argmin(dim=1)
    e = (q - tgt[idx]).double()
    Rd = R.double()
    C = unpack(ct)[idx] + Rd @ unpack(cs) @ Rd.T
    # the batched 3 x 3 inverse in closed form (adjugate over determinant), as elementwise torch ops
    c00, c01, c02, c11, c12, c22 = C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]
    a00, a01, a02 = c11 * c22 - c12 * c12, c02 * c12 - c01 * c22, c01 * c12 - c02 * c11
    a11, a12, a22 = c00 * c22 - c02 * c02, c01 * c02 - c00 * c12, c00 * c11 - c01 * c01
    det = c00 * a00 + c01 * a01 + c02 * a02
    M = torch.stack([torch.stack([a00, a01, a02], 1), torch.stack([a01, a11, a12], 1), torch.stack([a02, a12, a22], 1)], 1) / det[:, None, None]
    qd = q.double()
    zero = torch.zeros_like(qd[:, 0])
    skew = torch.stack([torch.stack([zero, -qd[:, 2], qd[:, 1]], 1), torch.stack([qd[:, 2], zero, -qd[:, 0]], 1),
                        torch.stack([-qd[:, 1], qd[:, 0], zero], 1)], 1)
    J = torch.cat([-skew, torch.eye(3, dtype=torch.float64, device=q.device).expand(len(q), 3, 3)], 2)
    A = torch.einsum("sai,sab,sbj->ij", J, M, J)
    b = torch.einsum("sai,sab,sb->i", J, M, e)
    return A, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H = 640, 480
    fx = fy = 0.8 * W
    cx, cy = (W - 1) / 2, (H - 1) / 2
    poses = reg.ring_poses(6)
    depth = [reg.corner_depth(poses[k], W, H, fx, fy, cx, cy).to(dev) for k in (0, 1)]
    truth = relative_pose(poses[0].float().to(dev), poses[1].float().to(dev))
    drifted = reg.drifted(poses, 0.008, 0.012, 0).float().to(dev)
    start = relative_pose(drifted[0], drifted[1]).contiguous()  # the estimate the iteration is timed at
    print(f"{'S = N':>7} {'build':>8} {'self kNN':>9} {'covs':>8} | {'step':>8} {'(min)':>8} {'search':>8} {'rest':>8} | {'torch ops':>10} {'ratio':>6}"
          "   (us; covs for one cloud, k = 10)")
    for stride in (4, 2):
        tgt = gicp.unproject_depth(depth[0], fx, fy, cx, cy, stride=stride)
        src = gicp.unproject_depth(depth[1], fx, fy, cx, cy, stride=stride)
        S = N = len(src)
        def stage(name):  # one flushed line per finished stage: a run that dies says where
            torch.cuda.synchronize()
            print(f"        [{S}] {name} done", flush=True)
        index, t_build, _ = replay_time(lambda: knn.knn_build(tgt), args.replays)
        stage("build")
        nb, t_self, _ = replay_time(lambda: knn.knn_search(index, None, 10, exclude_self=False), args.replays)
        stage("self search")
        cov_t = torch.empty((N, 8), device=dev)
        params = _capi.CovarianceParams(_capi.COV_PLANE, 1e-3, 4, 1e-4, (_capi._f * 3)(0, 0, 0), 1)

        def covs():
            _capi.call("dgr_point_covariances", dev, N, tgt.data_ptr(), 10, nb.idx.data_ptr(), params, cov_t.data_ptr(), None, None, None, None)
        _, t_cov, _ = replay_time(covs, args.replays)
        stage("covariances")
        cs = gicp.point_covariances(src, k=10, viewpoint=(0, 0, 0)).cov
        scratch = torch.zeros((_capi.load().dgr_gicp_scratch_bytes(N, S),), dtype=torch.uint8, device=dev)
        out, stats = torch.empty((4, 4), device=dev), torch.empty((32,), dtype=torch.float64, device=dev)
        gp = _capi.GicpParams(0.3, float("inf"), 0.0, 1e-8, 6)

        def step():
            _capi.call("dgr_gicp_step", dev, index.index.data_ptr(), N, tgt.data_ptr(), cov_t.data_ptr(), S, src.data_ptr(), cs.data_ptr(),
                       start.data_ptr(), gp, scratch.data_ptr(), out.data_ptr(), None, None, stats.data_ptr(), None, None)
        _, t_step, t_step_min = replay_time(step, args.replays)
        stage("step")
        m = start.T
        q = (src @ m[:3, :3].T + m[:3, 3]).contiguous()
        q = torch.where(torch.isfinite(q), q, torch.full_like(q, float("nan")))
        _, t_search, _ = replay_time(lambda: knn.knn_search(index, q, 1, max_distance=0.3), args.replays)
        stage("cross search")
        (A, b), t_torch = eager_time(lambda: torch_iteration(src, tgt, cs, cov_t, start))
        stage("torch ops")
        # the two agree on what they sum (every pair is within the radius here): A's largest relative difference
        k = 0
        Ak = torch.zeros((6, 6), dtype=torch.float64, device=dev)
        for i in range(6):
            for j in range(i, 6):
                Ak[i, j] = Ak[j, i] = stats[k]
                k += 1
        agree = float((Ak - A).abs().max() / A.abs().max())
        print(f"{S:>7} {t_build:>8.1f} {t_self:>9.1f} {t_cov:>8.1f} | {t_step:>8.1f} {t_step_min:>8.1f} {t_search:>8.1f} {t_step - t_search:>8.1f} | "
              f"{t_torch:>10.1f} {t_torch / t_step:>6.1f}   pairs {int(stats[28])}, ok {int(stats[29])}, A agrees to {agree:.1e}", flush=True)
        full = gicp.gicp_align(src, tgt, transform=start, source_cov=cs, target_cov=cov_t, target_index=index, iterations=15, max_distance=0.3)
        _, t_align, _ = replay_time(lambda: gicp.gicp_align(src, tgt, transform=start, source_cov=cs, target_cov=cov_t, target_index=index,
                                                            iterations=15, max_distance=0.3), max(args.replays // 3, 5))
        print(f"        gicp_align, 15 iterations in one graph: {t_align:.1f} us; error to the truth "
              f"{reg.motion_error(start, truth)} -> {reg.motion_error(full.transform, truth)}", flush=True)


if __name__ == "__main__":
    main()
