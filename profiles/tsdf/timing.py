"""Time per call of slam.tsdf_integrate and of the two halves of slam.extract_mesh (plan = count + scan, emit), replayed from a
hipGraph, beside the same fusion in float32 torch ops one view at a time, and a call whose views all look away (the brick culling alone):
    python profiles/tsdf/timing.py [N:W:H ...]          (default 256:640:480: a 256^3 lattice, 640 x 480 views)
Every measurement runs in a child process of its own under a time limit; the first one that fails ends the run.
The scene is the tests' sphere in front of a wall (tests/tsdf_model.py), seen from eight poses.
Algorithmic bytes of an integrate call: the volume read and written once (16 bytes per sample, 48 with colour), the images once
per view (4 bytes per pixel, 16 with colour); the fraction quoted is of 8 TB/s."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

PEAK = 8.0e12
STEP_LIMIT = 240  # seconds per child


def scene(N, W, H, V):
    import numpy as np
    import tsdf_model as M
    poses = M.MAIN_POSES + [M.pose(0.1, 0.3, -0.1, [-0.4, 0.1, 0.0]), M.pose(-0.2, -0.25, 0.05, [0.4, -0.15, 0.1]),
                            M.pose(0.15, 0.0, 0.2, [0.0, 0.25, -0.1])]
    fx = 0.9375 * W
    frames = [M.render_scene(p, H, W, fx, fx, (W - 1) / 2.0, (H - 1) / 2.0) for p in poses[:V]]
    voxel = 2.56 / N
    return dict(origin=(-1.28, -1.28, 1.0), voxel=voxel, dims=(N, N, N), fx=fx, fy=fx, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0,
                depth=np.stack([f[0] for f in frames]), color=np.stack([f[1] for f in frames]), views=np.stack(poses[:V]))


def replay_time(fn, replays=20, windows=5):
    """ms per call of fn() from a hipGraph: (mean, min, max) over `windows` windows of `replays` replays"""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(replays):
            graph.replay()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / replays)
    return sum(times) / len(times), min(times), max(times)


def torch_fuse_one(vol, col, X, Y, Z, depth, color, view, fx, fy, cx, cy, trunc, near=0.05):
    """the same rule for one view in float32 torch ops (eager), in place"""
    import torch
    H, W = depth.shape
    pc = [view[0, j] * X + view[1, j] * Y + view[2, j] * Z + view[3, j] for j in range(3)]
    z = pc[2]
    fu, fv = torch.floor(fx * pc[0] / z + cx + 0.5), torch.floor(fy * pc[1] / z + cy + 0.5)
    ok = (z > near) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    q = torch.where(ok, fv * W + fu, torch.zeros_like(fu)).long()
    d = depth.reshape(-1)[q]
    sdf = d - z
    ok &= (d > 0) & ~(sdf < -trunc)
    t = torch.clamp(sdf / trunc, max=1.0)
    w = vol[..., 1]
    wn = w + 1.0
    vol[..., 0] = torch.where(ok, (vol[..., 0] * w + t) / wn, vol[..., 0])
    if col is not None:
        for c in range(3):
            col[..., c] = torch.where(ok, (col[..., c] * w + color[c].reshape(-1)[q]) / wn, col[..., c])
    vol[..., 1] = torch.where(ok, wn, w)


def child(what, N, W, H, V, with_color):
    import torch
    from dgr_amd import slam
    dev = torch.device("cuda:0")
    s = scene(N, W, H, max(V, 1))
    T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    depth, color, views = T(s["depth"]), T(s["color"]), T(s["views"])
    vol = slam.TsdfVolume(s["origin"], s["voxel"], s["dims"], color=with_color, device=dev)
    args = (s["fx"], s["fy"], s["cx"], s["cy"])
    samples, pixels = N ** 3, W * H
    tag = f"{N}^3 {W}x{H} V={V} {'colour' if with_color else 'no colour'}"
    if what == "away":  # every view turned away from the lattice: each brick tests the views and leaves before it loads anything
        import numpy as np
        import tsdf_model as M
        views = T(np.stack([M.pose(0.0, np.pi, 0.0, [0.0, 0.0, 0.0])] * V))
        ms, lo, hi = replay_time(lambda: slam.tsdf_integrate(vol, depth, views, *args, color=color if with_color else None))
        assert not bool(vol.volume.any())
        print(f"integrate {tag}, every view turned away: {ms * 1e3:.1f} us per call ({lo * 1e3:.1f} .. {hi * 1e3:.1f}): what a call costs that culls "
              f"every brick ({samples // 256} workgroups, {V} pose tests each, nothing loaded)")
    elif what == "integrate":
        fn = lambda: slam.tsdf_integrate(vol, depth, views, *args, color=color if with_color else None)  # noqa: E731
        ms, lo, hi = replay_time(fn)
        nbytes = samples * (48 if with_color else 16) + V * pixels * (16 if with_color else 4)
        touched = float((vol.volume[..., 1] > 0).float().mean())
        print(f"integrate {tag}: {ms * 1e3:.1f} us per call ({lo * 1e3:.1f} .. {hi * 1e3:.1f}), {ms * 1e3 / V:.1f} us per view; algorithmic bytes "
              f"{nbytes / 1e6:.1f} MB -> {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (ms * 1e-3) / PEAK:.1f} % of 8 TB/s; samples touched {touched:.3f}")
    elif what == "torch":
        X, Y, Z = (T(a.astype("float32").copy()) for a in __import__("tsdf_model").lattice(s["origin"], s["voxel"], s["dims"]))
        one = lambda: torch_fuse_one(vol.volume, vol.color, X, Y, Z, depth[0], color[0], views[0], *args, vol.truncation)  # noqa: E731
        for _ in range(2):
            one()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(5):
            one()
        stop.record()
        torch.cuda.synchronize()
        print(f"torch ops {tag.replace(f'V={V}', 'one view')}: {start.elapsed_time(stop) / 5 * 1e3:.1f} us per view (float32, eager, 5 calls)")
    else:  # mesh
        slam.tsdf_integrate(vol, depth, views, *args, color=color if with_color else None)
        need = int(slam.extract_mesh(vol).count.item())
        from dgr_amd import _capi
        grid = vol.grid()
        scratch = torch.empty((_capi.load().dgr_mesh_scratch_bytes(grid),), dtype=torch.uint8, device=dev)
        words = torch.zeros((2,), dtype=torch.int32, device=dev)
        vertices, colors = torch.empty((3 * need, 3), device=dev), torch.empty((3 * need, 3), device=dev) if with_color else None
        p = _capi.ptr
        plan = lambda: _capi.call("dgr_mesh_plan", dev, grid, p(vol.volume), 1.0, need, p(scratch), words.data_ptr(), words.data_ptr() + 4)  # noqa: E731
        emit = lambda: _capi.call("dgr_mesh_emit", dev, grid, p(vol.volume), p(vol.color), 1.0, need, p(scratch), p(vertices), p(colors))  # noqa: E731
        pm, plo, phi = replay_time(plan)
        em, elo, ehi = replay_time(emit)
        cells = (N - 1) ** 3
        print(f"mesh {tag}: {need} triangles of {cells} cells ({(cells + 255) // 256} blocks); plan (count + scan) {pm * 1e3:.1f} us ({plo * 1e3:.1f} .. "
              f"{phi * 1e3:.1f}): the volume once = {samples * 8 / 1e6:.1f} MB -> {samples * 8 / (pm * 1e-3) / 1e12:.2f} TB/s; emit {em * 1e3:.1f} us "
              f"({elo * 1e3:.1f} .. {ehi * 1e3:.1f}): the volume once more and {need * (72 if with_color else 36) / 1e6:.1f} MB of triangles")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        what, N, W, H, V, c = sys.argv[2:8]
        child(what, int(N), int(W), int(H), int(V), c == "1")
        sys.exit(0)
    for spec in sys.argv[1:] or ["256:640:480"]:
        N, W, H = (int(f) for f in spec.split(":"))
        steps = [("integrate", V, c) for c in (1, 0) for V in (1, 4, 8)] + [("away", 8, 1), ("torch", 1, 1), ("torch", 1, 0), ("mesh", 8, 1)]
        for what, V, c in steps:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(N), str(W), str(H), str(V), str(c)],
                               timeout=STEP_LIMIT)
            if r.returncode != 0:
                sys.exit(f"{what} V={V} colour={c} ended with status {r.returncode}: stopping")
