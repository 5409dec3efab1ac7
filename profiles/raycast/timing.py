"""Time per call of slam.tsdf_raycast (with the brick map, without it, and "build" = map + march) and of slam.tsdf_bricks alone,
replayed from a hipGraph, beside a march of the same samples in float32 torch ops (grid_sample over chunks of samples):
    python profiles/raycast/timing.py [N:W:H ...]          (default 256:640:480: a 256^3 lattice, 640 x 480 views)
Every measurement runs in a child process of its own under a time limit; the first one that fails ends the run.
The volume is the scene of profiles/tsdf/timing.py (the tests' sphere in front of a wall) fused from its eight poses; it is ray-cast
from the first V of them.  Each ray-cast child also checks that the results with and without the map are the same bits."""
import importlib.util
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
_spec = importlib.util.spec_from_file_location("tsdf_timing", os.path.join(ROOT, "profiles", "tsdf", "timing.py"))
tsdf_timing = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tsdf_timing)

STEP_LIMIT = 240  # seconds per child


def torch_march(tsdf5, valid5, views, fx, fy, cx, cy, H, W, origin, voxel, dims, lo, step, K, chunk=32):
    """the first sample with a valid F <= 0 per ray, in float32 torch ops: grid_sample of the tsdf and of the cells' validity over
    chunks of `chunk` samples of every ray (what materialising the samples costs; no predecessor test, no normals, no colour)"""
    import torch
    dev = tsdf5.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    dc = torch.stack([(xs - cx) / fx, (ys - cy) / fy, torch.ones_like(xs)], dim=-1)
    R, t = views[0, :3, :3].T, views[0, 3, :3]
    q0 = (-(R.T @ t) - torch.tensor(origin, device=dev)) / voxel
    dq = (dc @ R) / voxel
    scale = 2.0 / (torch.tensor(dims, device=dev, dtype=torch.float32) - 1.0)
    first = torch.full((H, W), K, dtype=torch.int64, device=dev)
    for k0 in range(0, K, chunk):
        k = torch.arange(k0, min(k0 + chunk, K), device=dev, dtype=torch.float32)
        z = lo + k * step
        q = q0 + z[:, None, None, None] * dq[None]                 # [chunk, H, W, 3]
        grid = (q * scale - 1.0)[None]                              # [1, chunk, H, W, 3] in (x, y, z) order
        F = torch.nn.functional.grid_sample(tsdf5, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0]
        ok = torch.nn.functional.grid_sample(valid5, grid, mode="nearest", padding_mode="zeros", align_corners=True)[0, 0] > 0.5
        dec = ok & (F <= 0)
        idx = torch.where(dec.any(dim=0), dec.float().argmax(dim=0) + k0, torch.full_like(first, K))
        first = torch.minimum(first, idx)
    return first


def child(what, N, W, H, V):
    import torch
    from dgr_amd import slam
    dev = torch.device("cuda:0")
    s = tsdf_timing.scene(N, W, H, 8)
    T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    vol = slam.TsdfVolume(s["origin"], s["voxel"], s["dims"], device=dev)
    args = (s["fx"], s["fy"], s["cx"], s["cy"])
    slam.tsdf_integrate(vol, T(s["depth"]), T(s["views"]), *args, color=T(s["color"]))
    views = T(s["views"][:V])
    tag = f"{N}^3 {W}x{H} V={V}"
    bricks = slam.tsdf_bricks(vol)
    live = float(bricks.float().mean())
    if what == "bricks":
        ms, lo, hi = tsdf_timing.replay_time(lambda: slam.tsdf_bricks(vol))
        nbytes = N ** 3 * 8
        print(f"bricks {N}^3: {ms * 1e3:.1f} us per call ({lo * 1e3:.1f} .. {hi * 1e3:.1f}); {bricks.numel()} bricks, {live:.3f} live; the volume "
              f"once = {nbytes / 1e6:.1f} MB -> {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s (each brick reads 9^3 samples for its 8^3 cells: 1.42 x that)")
    elif what in ("map", "march", "build", "depth-only"):
        kw = dict(bricks={"map": bricks, "march": None, "build": "build", "depth-only": bricks}[what], return_flags=True)
        if what == "depth-only":
            kw.update(normals=False, color=False, return_flags=False)
        fn = lambda: slam.tsdf_raycast(vol, views, *args, H, W, **kw)  # noqa: E731
        a, b = fn(), slam.tsdf_raycast(vol, views, *args, H, W, bricks=None, return_flags=True)
        same = all(x is None or torch.equal(x, y) for x, y in zip(a, b))
        hits = float((b.flags & 1).float().mean())
        ms, lo, hi = tsdf_timing.replay_time(fn)
        rays = V * W * H
        print(f"raycast {tag} {what}: {ms * 1e3:.1f} us per call ({lo * 1e3:.1f} .. {hi * 1e3:.1f}), {ms * 1e3 / V:.1f} us per view, "
              f"{ms * 1e6 / rays:.2f} ns per ray; hits {hits:.3f}, live bricks {live:.3f}, same bits as the full march: {same}")
        assert same
    else:  # torch
        K = int((1.0 + N * s["voxel"] * 1.75 - 0.05) / (0.5 * s["voxel"]))  # to the far corner of the box
        tsdf5 = vol.volume[..., 0][None, None].contiguous()
        w = (vol.volume[..., 1] >= 1.0).float()[None, None]
        valid5 = (-torch.nn.functional.max_pool3d(-torch.nn.functional.pad(w, (0, 1, 0, 1, 0, 1)), 2, stride=1)).contiguous()  # a cell's 8 corners
        one = lambda: torch_march(tsdf5, valid5, views, *args, H, W, s["origin"], s["voxel"], s["dims"], 0.05, 0.5 * s["voxel"], K)  # noqa: E731
        first = one()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(3):
            one()
        stop.record()
        torch.cuda.synchronize()
        print(f"torch ops {N}^3 {W}x{H} one view: {start.elapsed_time(stop) / 3 * 1e3:.1f} us per view (float32, eager, grid_sample over {K} samples "
              f"per ray in chunks of 32, 3 calls); rays that end {float((first < K).float().mean()):.3f}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        what, N, W, H, V = sys.argv[2:7]
        child(what, int(N), int(W), int(H), int(V))
        sys.exit(0)
    for spec in sys.argv[1:] or ["256:640:480"]:
        N, W, H = (int(f) for f in spec.split(":"))
        steps = [("map", 1), ("march", 1), ("build", 1), ("depth-only", 1), ("map", 4), ("march", 4), ("bricks", 1), ("torch", 1)]
        for what, V in steps:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(N), str(W), str(H), str(V)], timeout=STEP_LIMIT)
            if r.returncode != 0:
                sys.exit(f"{what} V={V} ended with status {r.returncode}: stopping")
