"""slam.tsdf_bricks and slam.tsdf_raycast on the GPU against the float64 numpy model (tests/raycast_model.py).

Decisions.  Outside the model's `ambiguous` mask (at most 3 % of a case's pixels, tests/test_raycast_model.py) `flags` equal the
model's exactly, and the brick map equals the model's everywhere.
Values.  On the pixels both call a hit, depth, normal and colour stand within max(2 e32, floor) of the float64 model: e32 = the
largest |raycast32 - raycast| of the case (what float32 costs in numpy's operation order; the factor 2 covers another equally
valid order and the kernel's fused multiply-adds).  The floors come from the position's rounding: a lattice coordinate
q = q0 + z dq of size up to Q = 64 is the result of about six roundings of terms of that size (the pose's three products and their
sum, the division by the voxel, the product with z, the sum), dq = 6 Q eps = 4.6e-5 cells at the worst.
 * depth: the interpolant falls by at most 1 / 4 per cell (truncation 4 voxels), so F is off by dq / 4 = 1.2e-5; along the ray it
   changes by step / truncation = 1 / 8 per sample of 0.025 m: 2.3e-6 m, and four roundings of a depth of up to 4 m: 32 eps = 3.8e-6.
 * normal: each of the six values is off by dq / 4 against a gradient of length 1 / 2 (two cells apart): 4 x 1.2e-5 = 4.6e-5,
   and the normalisation's and rotation's few eps: 512 eps = 6.1e-5.
 * colour: random colours in (0, 1) change by up to 0.9 per cell along each of three axes: 2.7 dq = 1.2e-4 = 1024 eps.
Figures measured on the MI355X: profiles/raycast/measured.txt.

The march's invariants are bit-for-bit: with and without the brick map, two runs, V views in one call against V calls, every
combination of absent outputs, a replayed graph against eager."""
import numpy as np
import pytest
import torch

import icp_model as I
import raycast_model as M
import tsdf_model as TM
from dgr_amd import _capi, fusion, icp, slam

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
FLOOR_DEPTH, FLOOR_NORMAL, FLOOR_COLOR = 32 * EPS, 512 * EPS, 1024 * EPS
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def all_cases():
    return {**M.cases(), **M.extra_cases()}


def make_volume(case, with_color=True):
    nz, ny, nx = case["volume"].shape[:3]
    vol = slam.TsdfVolume(case["origin"], case["voxel"], (nx, ny, nz), color=with_color, device=DEV)
    vol.volume.copy_(T(case["volume"]))
    if with_color:
        vol.color.copy_(T(case["color"]))
    return vol


def cast(vol, case, views=None, **kw):
    opts = dict(case.get("opts", {}))
    opts.update(kw)
    opts.setdefault("return_flags", True)
    views = case["views"] if views is None else views
    return slam.tsdf_raycast(vol, T(views), case["fx"], case["fy"], case["cx"], case["cy"], case["H"], case["W"], **opts)


def host(r):
    torch.cuda.synchronize()
    return {k: None if t is None else t.cpu().numpy() for k, t in r._asdict().items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(bits(a[k]), bits(b[k])) for k in a)


def check_against_model(name, got):
    """the comparison of the module's docstring; returns the line of figures"""
    r, r32 = M.reference(name), M.reference32(name)
    keep = ~r["ambiguous"]
    assert r["ambiguous"].mean() <= 0.03
    assert np.array_equal(got["flags"][keep], r["flags"][keep]), (name, int((got["flags"] != r["flags"])[keep].sum()))
    hit = keep & ((r["flags"] & M.HIT) > 0)
    normal = hit & ((r["flags"] & M.NO_NORMAL) == 0)
    line = (f"raycast-measured {name}: pixels {keep.size} ambiguous {r['ambiguous'].mean():.4f} hits {hit.mean():.3f} unseen "
            f"{((r['flags'] & M.UNSEEN) > 0).mean():.3f} without normal {((r['flags'] & M.NO_NORMAL) > 0).mean():.3f}")
    # what is no hit is zero, exactly
    assert not got["depth"][keep & ~hit].any() and not got["vnmap"][keep & ~normal].any()
    for key, floor, mask, pick in (("depth", FLOOR_DEPTH, hit, lambda a: a), ("vnmap", FLOOR_NORMAL, normal, lambda a: a[..., :3]),
                                   ("color", FLOOR_COLOR, hit, lambda a: np.moveaxis(a, 1, -1))):
        if got[key] is None:
            continue
        e32 = float(np.abs(pick(r32[key]).astype(np.float64) - pick(r[key]))[mask].max(initial=0.0))
        err = float(np.abs(pick(got[key]).astype(np.float64) - pick(r[key]))[mask].max(initial=0.0))
        line += f" | {key} e32 {e32:.3e} kernel-vs-model {err:.3e}"
        assert err <= max(2 * e32, floor), (name, key, err, e32)
    if got["vnmap"] is not None:  # the map's fourth entry is the depth's bits where there is a normal
        assert np.array_equal(bits(got["vnmap"][..., 3][normal]), bits(got["depth"][normal]))
    if got["color"] is not None:
        assert not np.moveaxis(got["color"], 1, -1)[keep & ~hit].any()
    print(line)
    return line


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_raycast_equals_the_model_with_and_without_the_brick_map(name):
    case = all_cases()[name]
    vol = make_volume(case)
    built = host(cast(vol, case))
    check_against_model(name, built)
    marched = host(cast(vol, case, bricks=None))
    assert same_bits(built, marched), name
    again = host(cast(vol, case, bricks=slam.tsdf_bricks(vol, min_weight=case.get("opts", {}).get("min_weight", 1.0))))
    assert same_bits(built, again), name
    V, H, W = case["views"].shape[0], case["H"], case["W"]
    assert built["depth"].shape == (V, H, W) and built["vnmap"].shape == (V, H, W, 4) and built["color"].shape == (V, 3, H, W)
    assert built["flags"].shape == (V, H, W) and built["flags"].dtype == np.uint8
    if name in ("away", "lattice-1x1x1", "max-in-front", "weight-10"):
        assert not built["flags"].any() and not built["depth"].any() and not built["vnmap"].any() and not built["color"].any()
    if name == "min-beyond":
        assert ((built["flags"] & M.UNSEEN) > 0).mean() > 0.05
    if name == "inside":
        assert ((built["flags"][1] & M.HIT) > 0).mean() > 0.05 and not (built["flags"][0] & M.HIT).any()


def last_plane_volume():
    """17 x 10 x 9 samples, all positive, the only negative one on the last lattice plane of x (and of z)"""
    v = np.stack([np.full((9, 10, 17), 0.5, dtype=np.float32), np.ones((9, 10, 17), dtype=np.float32)], axis=-1)
    v[8, 4, 16, 0] = -0.5
    return v


@pytest.mark.parametrize("name", sorted(M.cases()) + ["graze", "last-plane"])
def test_bricks_equal_the_model(name):
    if name == "last-plane":
        case = dict(volume=last_plane_volume(), color=None, origin=(0.0, 0.0, 0.0), voxel=0.05)
    else:
        case = all_cases()[name]
    vol = make_volume(case, with_color=False)
    weights = (1.0, 0.5, 2.0, 3.5) if name.startswith("main") else (1.0, 1.5)
    for mw in weights:
        got = slam.tsdf_bricks(vol, min_weight=mw).cpu().numpy()
        want = M.bricks(case["volume"], min_weight=mw)
        assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want), (name, mw)
    if name == "last-plane":
        want = np.zeros((1, 2, 2), dtype=np.uint8)
        want[0, 0, 1] = 1
        assert np.array_equal(slam.tsdf_bricks(vol).cpu().numpy(), want)
        assert not slam.tsdf_bricks(vol, min_weight=1.5).any()  # a min_weight that kills it
        low = case["volume"].copy()
        low[7, 4, 15, 1] = 0.5                                    # a corner of both cells around it
        vol.volume.copy_(T(low))
        assert not slam.tsdf_bricks(vol).any() and slam.tsdf_bricks(vol, min_weight=0.5).sum().item() == 1
    if name.startswith("main"):
        assert 0.05 < slam.tsdf_bricks(vol).float().mean().item() < 0.6


def test_views_in_one_call_equal_the_same_views_in_several_calls_and_two_runs_are_equal():
    case = all_cases()["main-64x48-v3"]
    vol = make_volume(case)
    whole = host(cast(vol, case))
    assert same_bits(whole, host(cast(vol, case)))
    for v in range(3):
        one = host(cast(vol, case, views=case["views"][v:v + 1]))
        assert all(np.array_equal(bits(one[k][0]), bits(whole[k][v])) for k in one), v
        single = host(cast(vol, case, views=case["views"][v]))  # a [4, 4] pose: [H, W]-shaped results
        assert single["depth"].shape == (48, 64) and single["vnmap"].shape == (48, 64, 4) and single["color"].shape == (3, 48, 64)
        assert all(np.array_equal(bits(single[k]), bits(whole[k][v])) for k in single), v


def raw_raycast(vol, case, bricks, outputs):
    """dgr_tsdf_raycast itself, with any of the four outputs absent"""
    o = dict(case.get("opts", {}))
    lo, hi = o.get("depth_range", (0.05, M.INF))
    params = _capi.RaycastParams(case["fx"], case["fy"], case["cx"], case["cy"], lo, hi, o.get("step", 0.5 * case["voxel"]), o.get("min_weight", 1.0))
    views = T(case["views"])
    p = _capi.ptr
    _capi.call("dgr_tsdf_raycast", vol.device, vol.grid(), p(vol.volume), p(vol.color), p(bricks), views.shape[0], case["W"], case["H"],
               p(views), params, p(outputs.get("depth")), p(outputs.get("vnmap")), p(outputs.get("color")), p(outputs.get("flags")))
    torch.cuda.synchronize()


def test_every_combination_of_absent_outputs_leaves_the_others_unchanged_and_nothing_is_written_outside():
    from test_hip_guarded_buffers import GuardedTorch
    case = all_cases()["main-37x29-v3"]
    vol = make_volume(case)
    V, H, W = 3, case["H"], case["W"]
    shapes = dict(depth=((V, H, W), torch.float32), vnmap=((V, H, W, 4), torch.float32), color=((V, 3, H, W), torch.float32),
                  flags=((V, H, W), torch.uint8))
    full = host(cast(vol, case))
    bricks = slam.tsdf_bricks(vol)
    for mask in range(1, 16):
        guarded = GuardedTorch()
        keys = [k for i, k in enumerate(shapes) if mask >> i & 1]
        outs = {k: guarded.empty(shapes[k][0], dtype=shapes[k][1], device=DEV) for k in keys}
        raw_raycast(vol, case, bricks if mask & 1 else None, outs)
        assert guarded.check() == len(keys)
        for k in keys:
            assert np.array_equal(bits(outs[k].cpu().numpy()), bits(full[k])), (mask, k)


def test_the_python_surface_allocates_what_was_asked_for_and_stays_inside(monkeypatch):
    from test_hip_guarded_buffers import GuardedTorch
    case = all_cases()["main-17x15-v1"]
    vol = make_volume(case)
    full = host(cast(vol, case))
    guarded = GuardedTorch()
    monkeypatch.setattr(fusion, "torch", guarded)
    r = cast(vol, case, normals=False, color=False, return_flags=False)
    assert guarded.check() == 2 and r.vnmap is None and r.color is None and r.flags is None  # (the brick map and the depth)
    assert np.array_equal(bits(r.depth.cpu().numpy()), bits(full["depth"]))
    r = cast(vol, case)
    assert guarded.check() == 5 and same_bits(host(r), full)
    no_color = make_volume(case, with_color=False)
    r = cast(no_color, case)
    assert r.color is None and np.array_equal(bits(r.vnmap.cpu().numpy()), bits(full["vnmap"]))


def test_nan_and_inf_in_the_pose_and_the_volume_complete():
    """ordinary inputs that happen to hold such values: the views and samples without them keep their bits"""
    case = dict(all_cases()["main-64x48-v3"])
    vol = make_volume(case)
    clean = host(cast(vol, case))
    views = np.concatenate([case["views"], case["views"][:1], case["views"][:1], case["views"][:1]]).copy()
    views[3] = np.nan
    views[4][3, 2] = np.inf
    views[5][1, 1] = np.nan
    for bricks in ("build", None):
        got = host(cast(vol, case, views=views, bricks=bricks))
        assert all(np.array_equal(bits(got[k][:3]), bits(clean[k])) for k in got)
        assert not got["flags"][3].any() and not got["depth"][3].any() and not got["flags"][4].any()  # a NaN pose: all misses
    # NaN and Inf samples in the volume: a miss, an unseen end or a garbage value, and the same bits with and without the map
    dirty = case["volume"].copy()
    rng = np.random.default_rng(4)
    idx = rng.integers(0, dirty[..., 0].size, 400)
    dirty[..., 0].reshape(-1)[idx[:100]] = np.nan
    dirty[..., 0].reshape(-1)[idx[100:200]] = np.inf
    dirty[..., 0].reshape(-1)[idx[200:250]] = -np.inf
    dirty[..., 1].reshape(-1)[idx[250:350]] = np.nan
    dirty[..., 1].reshape(-1)[idx[350:]] = np.inf
    vol.volume.copy_(T(dirty))
    a, b = host(cast(vol, case)), host(cast(vol, case, bricks=None))
    assert np.array_equal(a["flags"], b["flags"]) and np.array_equal(bits(a["depth"]), bits(b["depth"]))
    assert np.array_equal(bits(a["vnmap"]), bits(b["vnmap"])) and np.array_equal(bits(a["color"]), bits(b["color"]))
    assert np.array_equal(slam.tsdf_bricks(vol).cpu().numpy(), M.bricks(dirty))
    assert ((a["flags"] & M.HIT) > 0).mean() > 0.2


def test_a_replayed_graph_of_bricks_and_raycast_follows_the_volume():
    s = TM.main_scene(3)
    vol = slam.TsdfVolume(s["origin"], s["voxel"], s["dims"], device=DEV)
    cam = M.IMAGES["64x48"]
    views = T(M.VIEWS3)
    depth, color, poses = T(s["depth"]), T(s["color"]), T(s["views"])
    fuse = lambda v: slam.tsdf_integrate(vol, depth[v:v + 1], poses[v:v + 1], s["fx"], s["fy"], s["cx"], s["cy"], color=color[v:v + 1])  # noqa: E731
    step = lambda: slam.tsdf_raycast(vol, views, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["H"], cam["W"], return_flags=True)  # noqa: E731
    fuse(0)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = step()
    seen = []
    for v in (None, 1, 2):
        if v is not None:
            fuse(v)  # the volume integrated between the replays
        graph.replay()
        got = host(out)
        assert same_bits(got, host(step())), v
        seen.append(got)
    assert not np.array_equal(seen[0]["flags"], seen[1]["flags"]) and not np.array_equal(bits(seen[1]["depth"]), bits(seen[2]["depth"]))


# ---- end to end: the ray-cast as the model frame of the ICP

E2E = dict(dims=(80, 64, 46), voxel=0.05, origin=(-2.0, -1.6, 1.2))  # the sphere AND the wall behind it (z = 3.2) inside
TRUE_POSE = TM.pose(0.02, -0.05, 0.0, [0.1, 0.02, 0.03])
START_POSE = TM.pose(0.05, -0.07, 0.0, [0.16, -0.02, 0.08])


def alignment_error(view, depth_obs, cam):
    """the pose error as the scene sees it: the mean distance of the observed points, placed in the world by `view`, from the
    analytic sphere and wall.  (The scene is symmetric about the axis through the sphere's centre along z: a rotation about it is
    no error, no route can recover it, and the raw pose error of either route wanders along it.)"""
    m = np.asarray(view, dtype=np.float64).T
    R, t = m[:3, :3], m[:3, 3]
    ys, xs = np.mgrid[0:cam["H"], 0:cam["W"]].astype(np.float64)
    d = depth_obs.astype(np.float64)
    pc = np.stack([(xs - cam["cx"]) / cam["fx"] * d, (ys - cam["cy"]) / cam["fy"] * d, d], axis=-1)
    pw = (pc - t) @ R
    dist = np.minimum(np.abs(np.linalg.norm(pw - TM.SPHERE_C, axis=-1) - TM.SPHERE_R), np.abs(pw[..., 2] - TM.WALL_Z))
    return float(dist[d > 0].mean())


def test_end_to_end_the_raycast_serves_icp_as_the_model_frame():
    """The existing route -- icp_align on render_scene's analytic depth at the start pose -- is the reference; the ray-cast of the
    volume fused from three views replaces that depth (icp_align) and its vnmap the model map (icp_step, chained).  The analytic
    depth has no discretisation; the fused surface lies up to a voxel from the true one (a projective TSDF fed from the nearest
    pixel: half a pixel's footprint, 0.017 m at 2 m, times the surface's slope), and a rigid alignment to a surface displaced by
    at most a voxel ends at most a voxel from the true one: the ray-cast routes may be worse than the reference by one voxel,
    0.05 m.  The start is 0.054 m off by the same measure, so a route that did not align would fail."""
    cam = M.IMAGES["64x48"]
    intr = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    s = TM.scene(V=3, **E2E)
    vol = slam.TsdfVolume(s["origin"], s["voxel"], s["dims"], device=DEV)
    slam.tsdf_integrate(vol, T(s["depth"]), T(s["views"]), s["fx"], s["fy"], s["cx"], s["cy"], color=T(s["color"]))
    obs = TM.render_scene(TRUE_POSE, cam["H"], cam["W"], *intr, holes=False)[0]
    analytic = TM.render_scene(START_POSE, cam["H"], cam["W"], *intr, holes=False)[0]
    start = T(START_POSE)
    rc = slam.tsdf_raycast(vol, start, *intr, cam["H"], cam["W"], return_flags=True)
    hit_share = float((rc.flags & 1).float().mean())
    both = (rc.depth > 0) & (T(analytic) > 0)
    depth_gap = float((rc.depth - T(analytic)).abs()[both].mean())
    ref = slam.icp_align(T(obs), T(analytic), None, start, *intr, iterations=10)
    by_depth = slam.icp_align(T(obs), rc.depth, None, start, *intr, iterations=10)
    vn_obs = slam.depth_normals(T(obs), *intr)
    view = start.clone()
    for _ in range(10):
        view = icp.icp_step(T(obs), vn_obs, rc.vnmap.contiguous(), start, view, *intr).viewmatrix
    torch.cuda.synchronize()
    err = {k: alignment_error(v.cpu().numpy(), obs, cam) for k, v in (("reference", ref.viewmatrix), ("raycast depth", by_depth.viewmatrix),
                                                                      ("raycast vnmap", view))}
    err["start"] = alignment_error(START_POSE, obs, cam)
    raw = {k: I.pose_error(v.cpu().numpy(), TRUE_POSE) for k, v in (("reference", ref.viewmatrix), ("raycast depth", by_depth.viewmatrix),
                                                                    ("raycast vnmap", view))}
    margin = E2E["voxel"]
    print(f"raycast-measured end-to-end: hits {hit_share:.3f}, mean |ray-cast - analytic depth| {depth_gap:.4f} m; alignment error (m) "
          + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"; margin {margin}; raw pose error (rad, m) "
          + ", ".join(f"{k} ({a:.4f}, {d:.4f})" for k, (a, d) in raw.items()))
    assert hit_share > 0.9 and depth_gap < E2E["voxel"]
    assert err["start"] > err["reference"] + margin
    assert err["raycast depth"] <= err["reference"] + margin and err["raycast vnmap"] <= err["reference"] + margin
