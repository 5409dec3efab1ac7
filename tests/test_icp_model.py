"""The float64 model of the ICP steps (tests/icp_model.py) on its own, without a GPU: closed forms, the cap on its ambiguity
marks on every frame the GPU tests use, and that its error bounds for the sums cannot hide a wrong kernel -- each of four
deliberately wrong models breaks them on every frame."""
import functools

import numpy as np
import pytest

import icp_model as M

INF = float("inf")
# (W, H, stride) of every frame the GPU tests of the step use; the 67 x 5 frame is for sums only, not for convergence
FRAMES = [(3, 3, 1), (67, 5, 1), (67, 5, 3), (24, 18, 1), (96, 80, 1), (640, 480, 4), (640, 480, 1)]
IDS = [f"{w}x{h}-stride{s}" for w, h, s in FRAMES]
MARK_CAP = 0.01  # at most 1 % of the valid pixels of any test frame may be marked


def max_jump_of(W):
    """0.1, the default, where the scene's depth steps between neighbouring pixels stay below it; on the two frames a few pixels
    wide, whose neighbouring rays are degrees apart, no jump test (the frames are there for the sums' edges)"""
    return 0.1 if W >= 24 else 1e3


@functools.lru_cache(maxsize=None)
def frame(W, H):
    """the corner scene with both normal maps of the model (fp32, as the kernel's are)"""
    s = M.corner_scene(W, H)
    kw = dict(max_jump=max_jump_of(W))
    s["normals_model"] = M.depth_normals_model(s["model_depth"], s["fx"], s["fy"], s["cx"], s["cy"], **kw)
    s["normals_obs"] = M.depth_normals_model(s["depth_obs"], s["fx"], s["fy"], s["cx"], s["cy"], **kw)
    s["vn_model"], s["vn_obs"] = (s[k]["vnmap"].astype(np.float32) for k in ("normals_model", "normals_obs"))
    s["view_in"] = partial_pose(s)
    return s


def partial_pose(s):
    """the estimate a step starts from: the model pose moved by half the scene's twist (rel is then no identity, and a rotation
    applied transposed shows)"""
    Rm, tm = M.pose_of(s["model_view"])
    Re, te = M.se3_exp(0.5 * M.TWIST)
    return M.w2ct(Re @ Rm, Re @ tm + te)


@functools.lru_cache(maxsize=None)
def right_step(W, H, stride, huber_delta=INF):
    """the right model's step on a frame, shared by the tests that compare against it"""
    return step(frame(W, H), stride, huber_delta=huber_delta)


def step(s, stride, with_obs=True, **kw):
    return M.icp_step_model(s["depth_obs"], s["vn_obs"] if with_obs else None, s["vn_model"], s["model_view"], s["view_in"],
                            s["fx"], s["fy"], s["cx"], s["cy"], stride=stride, **kw)


def exact_depth(s):
    """(the scene's model depth before its rounding to fp32, the plane each pixel's ray meets first: 0, 1, 2 = x, y, z)"""
    R, t = M.pose_of(s["model_view"])
    centre = -R.T @ t
    fx, fy, cx, cy = (M.f32(s[k]) for k in ("fx", "fy", "cx", "cy"))
    y, x = np.mgrid[0:s["H"], 0:s["W"]]
    rays = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x, float)], -1) @ R
    depth, plane = np.full(x.shape, np.inf), np.full(x.shape, -1)
    for axis, value in ((0, 1.6), (1, 1.1), (2, 3.0)):
        with np.errstate(divide="ignore"):
            d = (value - centre[axis]) / rays[..., axis]
        nearer = (d > 0) & (d < depth)
        depth, plane = np.where(nearer, d, depth), np.where(nearer, axis, plane)
    return depth, plane


def away_from_creases_and_borders(plane, axis, margin=2):
    """pixels of `plane == axis` whose whole (2 margin + 1)^2 neighbourhood lies in the image and on the same plane: chosen by
    the scene's geometry, not by what the model returns"""
    H, W = plane.shape
    core = np.zeros((H, W), bool)
    inner = (slice(margin, H - margin), slice(margin, W - margin))
    core[inner] = True
    for dy in range(-margin, margin + 1):
        for dx in range(-margin, margin + 1):
            core[inner] &= plane[margin + dy:H - margin + dy, margin + dx:W - margin + dx] == axis
    return core


def test_normals_of_the_three_planes_are_exact_away_from_creases_and_borders():
    """The closed form: on a plane the central differences lie in the plane, so the model's normal IS the plane's.  The model on
    the scene's float64 depths (its float64 path) gives it to 1e-12 at every pixel two or more away from a crease or the border;
    on the fp32 depths the kernel gets, the depths' rounding (2^-24 relative) is amplified by |V| / |V(x+1) - V(x-1)|, about the
    distance from the principal point in pixels (at most 60 here): below 1e-4."""
    s = frame(96, 80)
    R, _ = M.pose_of(s["model_view"])
    depth64, plane = exact_depth(s)
    assert np.array_equal(depth64.astype(np.float32), s["model_depth"])
    exact = M.depth_normals_model(depth64, s["fx"], s["fy"], s["cx"], s["cy"])
    rounded = s["normals_model"]
    seen = 0
    for axis in range(3):
        want = -R[:, axis] / np.linalg.norm(R[:, axis])  # the normal towards the camera, in camera coordinates (R is an fp32 pose)
        core = away_from_creases_and_borders(plane, axis)
        seen += int(core.sum())
        assert core.sum() > 500 and exact["usable"][core].all() and rounded["usable"][core].all()
        worst = np.abs(exact["vnmap"][core][:, :3] - want).max()
        print(f"plane {axis}: {int(core.sum())} pixels, float64 depths |n - plane's| at most {worst:.2e}, fp32 depths "
              f"{np.abs(rounded['vnmap'][core][:, :3] - want).max():.2e}")
        assert worst < 1e-12
        assert np.array_equal(exact["vnmap"][core][:, 3], depth64[core])
        assert np.abs(rounded["vnmap"][core][:, :3] - want).max() < 1e-4
    assert seen > 0.75 * 96 * 80


def test_a_constant_depth_image_gives_exact_normals():
    out = M.depth_normals_model(np.full((7, 9), 2.5, np.float32), 7.2, 6.75, 4.63, 2.65)
    vn = out["vnmap"]
    assert out["usable"][1:-1, 1:-1].all() and not out["usable"][0].any() and not out["usable"][:, -1].any()
    assert np.all(vn[1:-1, 1:-1, 0] == 0.0) and np.all(vn[1:-1, 1:-1, 1] == 0.0) and np.all(vn[1:-1, 1:-1, 2] == -1.0)
    assert np.all(vn[1:-1, 1:-1, 3] == 2.5) and not vn[0].any() and not vn[:, 0].any() and not out["ambiguous"].any()


def test_unusable_pixels_of_the_normal_map():
    depth = np.full((6, 8), 2.0, np.float32)
    depth[2, 3] = np.nan
    depth[4, 6] = 2.3  # a step of 15 %
    mask = np.ones((6, 8), np.float32)
    mask[3, 5] = 0.5
    out = M.depth_normals_model(depth, 6.4, 6.0, 4.0, 2.2, mask_image=mask)
    u = out["usable"]
    assert not u[2, 3] and not u[2, 2] and not u[2, 4] and not u[1, 3] and not u[3, 3]  # the hole and its four neighbours
    assert not u[3, 5] and u[3, 4]                                                     # the mask is the pixel's own
    assert not u[4, 6] and not u[4, 5] and not u[3, 6]                                 # the step, from either side
    assert u[1, 1] and u[4, 1] and u.sum() == 24 - 5 - 1 - 3
    out = M.depth_normals_model(depth, 6.4, 6.0, 4.0, 2.2, max_jump=0.2)
    assert out["usable"][4, 6] and out["usable"][4, 5]
    out = M.depth_normals_model(depth, 6.4, 6.0, 4.0, 2.2, depth_range=(2.1, INF))
    assert not out["usable"].any()


@pytest.mark.parametrize("W,H,stride", FRAMES, ids=IDS)
def test_the_marks_stay_within_the_cap(W, H, stride):
    s = frame(W, H)
    for key, depth in (("normals_model", "model_depth"), ("normals_obs", "depth_obs")):
        marked, valid = int(s[key]["ambiguous"].sum()), int((s[depth] > 0).sum())
        print(f"{W}x{H} {key}: {marked} of {valid} marked")
        assert marked <= MARK_CAP * valid
    for with_obs in (True, False):
        m = step(s, stride, with_obs)
        marked = int(m["ambiguous"].sum())
        print(f"{W}x{H}/{stride} step, vn_obs {with_obs}: valid {m['valid']} associated {int(m['associated'].sum())} marked {marked}")
        assert marked <= MARK_CAP * m["valid"] and m["valid"] > 0 and m["associated"].sum() > 0


@pytest.mark.parametrize("mutate,kw", [("cross_sign", {}), ("drop_block", {}), ("transpose_rotation", {}),
                                        ("ignore_w", dict(huber_delta=1e-3))])
@pytest.mark.parametrize("W,H,stride", FRAMES, ids=IDS)
def test_a_wrong_model_breaks_the_bound(W, H, stride, mutate, kw):
    """|S_wrong - S| exceeds B + 2^-50 sum |term| in at least one of the 28 sums, both over the right model's associated set"""
    s = frame(W, H)
    right, wrong = right_step(W, H, stride, **kw), step(s, stride, mutate=mutate, **kw)
    sel = right["associated"]
    (S, B, mag), (S_wrong, _, _) = right["sums"](sel), wrong["sums"](sel)
    excess = np.abs(S_wrong[:28] - S[:28]) / (B + 2.0 ** -50 * mag + 1e-300)
    print(f"{W}x{H}/{stride} {mutate}: largest |S_wrong - S| / bound {excess.max():.3g}; B / sum |term| at most "
          f"{(B / (mag + 1e-300)).max():.3g}")
    assert excess.max() > 1.0
    assert (B <= 1e-3 * mag + 1e-12).all()  # and the bound is a rounding bound: far below the sums' own size


def test_equal_poses_give_a_zero_step():
    """(the identity as both poses: an fp32 pose is orthonormal to 1e-8 only, and rel = T T^-1 formed from it carries that)"""
    s = M.corner_scene(24, 18)
    eye = np.eye(4, dtype=np.float32)
    vn = M.depth_normals_model(s["model_depth"], s["fx"], s["fy"], s["cx"], s["cy"])["vnmap"].astype(np.float32)
    m = M.icp_step_model(s["model_depth"], vn, vn, eye, eye, s["fx"], s["fy"], s["cx"], s["cy"])
    S29, _, _ = m["sums"]()
    assert S29[28] > 100 and not S29[21:28].any()  # every residual is zero: q is the model's own point
    out = M.solve_update(S29, eye, eye)
    assert out["ok"] and not out["xi"].any() and out["cond"] < 1e3
    assert np.array_equal(out["viewmatrix"], eye) and out["quat"].tolist() == [1.0, 0.0, 0.0, 0.0] and not out["trans"].any()


def test_one_step_recovers_a_small_twist_to_second_order():
    """On planes the point-to-plane residual does not depend on which pixel of the plane a point is paired with, so with the
    pixels next to a crease left out of the model's map (their normals blend two planes) one Gauss-Newton step from a twist of
    1e-4 leaves an error of second order -- about 1e-4 of the twist, beside the fp32 depths' rounding averaged over
    thousands of pairs -- which 1 % of the twist bounds with room, while a first-order slip (a mis-scaled column of J) leaves far more."""
    twist = 1e-4 * np.array([0.7, -0.5, 0.4, 0.6, -0.8, 0.3])
    s = M.corner_scene(96, 80, twist)
    vn = M.depth_normals_model(s["model_depth"], s["fx"], s["fy"], s["cx"], s["cy"])["vnmap"]
    n = vn[..., :3]
    core = np.zeros(n.shape[:2], bool)
    core[2:-2, 2:-2] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            core[2:-2, 2:-2] &= np.abs(n[2 + dy:78 + dy, 2 + dx:94 + dx] - n[2:-2, 2:-2]).max(-1) < 1e-3
    vn = np.where(core[..., None], vn, 0.0).astype(np.float32)
    m = M.icp_step_model(s["depth_obs"], None, vn, s["model_view"], s["model_view"], s["fx"], s["fy"], s["cx"], s["cy"])
    S29, _, _ = m["sums"]()
    out = M.solve_update(S29, s["model_view"], s["model_view"])
    e0, e1 = M.pose_error(s["model_view"], s["true_view"]), M.pose_error(out["viewmatrix"], s["true_view"])
    print("pairs", S29[28], "pose error before", e0, "after one step", e1)
    assert out["ok"] and S29[28] > 5000 and e1[0] < 1e-2 * e0[0] and e1[1] < 1e-2 * e0[1]


def test_the_fronto_parallel_plane_is_refused_and_solves_under_damping():
    s = M.fronto_parallel_scene(24, 18)
    vn = M.depth_normals_model(s["model_depth"], s["fx"], s["fy"], s["cx"], s["cy"])["vnmap"].astype(np.float32)
    assert np.all(vn[1:-1, 1:-1, :3] == np.array([0.0, 0.0, -1.0], np.float32))
    m = M.icp_step_model(s["depth_obs"], vn, vn, s["model_view"], s["model_view"], s["fx"], s["fy"], s["cx"], s["cy"])
    S29, _, _ = m["sums"]()
    A, b, _, count = M.unpack(S29)
    assert count == 22 * 16
    for k in (2, 3, 4):  # omega_z, v_x, v_y
        assert not A[k].any() and not A[:, k].any() and b[k] == 0.0
    out = M.solve_update(S29, s["model_view"], s["model_view"])
    assert not out["ok"] and np.array_equal(out["viewmatrix"], s["model_view"]) and out["omega"] == 0.0
    # the plane moved by 1 cm along the axis and tilted: damping solves, and only omega_x, omega_y, v_z move
    S29[21:27] = A @ np.array([1e-3, -2e-3, 0.0, 0.0, 0.0, 1e-2])
    out = M.solve_update(S29, s["model_view"], s["model_view"], damping=1e-3)
    assert out["ok"] and np.all(out["xi"][[2, 3, 4]] == 0.0) and np.all(out["xi"][[0, 1, 5]] != 0.0)
    assert np.allclose(out["xi"][[0, 1, 5]], [-1e-3, 2e-3, -1e-2], rtol=0.02)


def test_refusals_of_the_solve():
    s = frame(24, 18)
    S29, _, _ = step(s, 1)["sums"]()
    ok = M.solve_update(S29, s["model_view"], s["model_view"])
    assert ok["ok"] and ok["cond"] < 1e3 and ok["quat"][0] > 0 and abs(np.linalg.norm(ok["quat"].astype(np.float64)) - 1) < 2e-7
    assert not M.solve_update(S29, s["model_view"], s["model_view"], min_points=int(S29[28]) + 1)["ok"]
    assert not M.solve_update(S29, s["model_view"], s["model_view"], rcond=0.5)["ok"]
    bad = S29.copy()
    bad[5] = np.nan
    out = M.solve_update(bad, s["model_view"], s["true_view"])
    assert not out["ok"] and np.array_equal(out["viewmatrix"], s["true_view"]) and np.array_equal(out["trans"], s["true_view"][3, :3])
    R, _ = M.pose_of(s["true_view"])
    assert np.abs(M.quat_to_rotation(out["quat"].astype(np.float64)) - R).max() < 1e-6


def test_convergence_on_the_scene():
    """the issue's table: 96 x 80 at stride 1 ends near 3.6e-4 rad / 5.6e-4 m, bounded by the pixel size, not by the solver"""
    s = frame(96, 80)
    out = M.icp_align_model(s["depth_obs"], s["model_depth"], None, s["model_view"], s["fx"], s["fy"], s["cx"], s["cy"])
    e = M.pose_error(out["viewmatrix"], s["true_view"])
    print("96 x 80, 10 iterations:", e, out["count"])
    assert all(out["ok"]) and e[0] < 1e-3 and e[1] < 1e-3 and 6500 < out["count"][-1] < 7332
