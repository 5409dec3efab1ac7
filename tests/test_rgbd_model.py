"""The float64 model of the hybrid RGB-D steps (tests/rgbd_model.py) on its own, without a GPU: closed forms of the intensity map,
the photometric residual and its Jacobian, the halving on a hand-made frame, the cap on the ambiguity marks on every frame the GPU
tests use, the model's convergence on the textured fronto-parallel plane where ICP refuses, the recorded pyramid case, and that
the error bounds cannot hide a wrong kernel: each deliberately wrong model breaks them by orders of magnitude."""
import functools

import numpy as np
import pytest

import icp_model as M
import rgbd_model as R
from test_icp_model import frame

INF = float("inf")
# (W, H, stride) of every frame the GPU tests of the step use
FRAMES = [(3, 3, 1), (67, 5, 1), (67, 5, 3), (96, 80, 1), (640, 480, 4)]
IDS = [f"{w}x{h}-stride{s}" for w, h, s in FRAMES]
MAP_FRAMES = [(3, 3), (67, 5), (24, 18), (96, 80)]
MARK_CAP = 0.01
# (geo_weight, photo_weight) and (huber_delta, photo_huber) of the GPU tests of the step
WEIGHTS = [(1.0, 1.0), (0.0, 0.6)]
HUBERS = [(INF, INF), (0.01, 0.02)]


def corner_albedo(P):
    """the texture of the room corner's three planes, a smooth function of the world point; its last term has a period of some
    six pixels on the small frames and some fifty at 640 x 480, where the sub-pixel correction still has to show in the sums"""
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    return (0.5 + 0.2 * np.sin(1.7 * X + 0.3) * np.cos(1.3 * Y - 0.2) + 0.15 * np.sin(0.9 * X - 1.1 * Z) +
            0.1 * np.sin(25.0 * X + 0.4) * np.sin(21.0 * Y - 23.0 * Z + 1.0))


def color_of(s, view, depth):
    """the intensity image [H,W] float32 of the textured scene seen at `view` with the depths `depth` (0.5 where there is none)"""
    Rv, t = M.pose_of(view)
    fx, fy, cx, cy = (M.f32(s[k]) for k in ("fx", "fy", "cx", "cy"))
    y, x = np.mgrid[0:s["H"], 0:s["W"]]
    d = depth.astype(np.float64)
    cam = np.stack([(x - cx) / fx * d, (y - cy) / fy * d, d], -1)
    world = (cam - t) @ Rv  # R^T (p - t)
    return np.where(depth > 0, corner_albedo(world), 0.5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def corner_frame(W, H):
    """test_icp_model's frame of the room corner, textured: the intensities of both views and the model's intensity map"""
    s = dict(frame(W, H))
    s["model_color"], s["color_obs"] = color_of(s, s["model_view"], s["model_depth"]), color_of(s, s["true_view"], s["depth_obs"])
    s["imap"] = R.intensity_map_model(s["model_color"])
    s["imap_model"] = s["imap"]["imap"].astype(np.float32)
    return s


def step(s, stride, with_obs=True, **kw):
    return R.rgbd_step_model(s["depth_obs"], s["vn_obs"] if with_obs else None, s["vn_model"], s["color_obs"], s["imap_model"],
                             s["model_view"], s["view_in"], s["fx"], s["fy"], s["cx"], s["cy"], stride=stride, **kw)


@functools.lru_cache(maxsize=None)
def right_step(W, H, stride, weights=(1.0, 1.0), hubers=(INF, INF)):
    return step(corner_frame(W, H), stride, geo_weight=weights[0], photo_weight=weights[1], huber_delta=hubers[0], photo_huber=hubers[1])


def map_frame(W, H, masked, seed=0):
    """(image [3,H,W] or [1,H,W], mask or None) of the map tests: a smooth colour image with noise; 3 channels on the odd seeds"""
    rng = np.random.default_rng(1000 + 7 * W + seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.3 * np.sin(0.4 * x + 0.1 * seed) * np.cos(0.3 * y)
    channels = 3 if (W + seed) % 2 else 1
    image = np.stack([base + 0.1 * rng.standard_normal((H, W)) for _ in range(channels)]).astype(np.float32)
    mask = rng.uniform(0.985, 1.0, (H, W)).astype(np.float32) if masked else None  # a third below the threshold
    return image, mask


# ------------------------------------------------------------------------------------------------------------- closed forms
def test_a_ramp_has_its_own_gradient_and_an_exact_residual_under_any_sub_pixel_shift():
    a, b = 0.25, -0.5
    y, x = np.mgrid[0:18, 0:24]
    ramp = (a * x + b * y + 3.0).astype(np.float32)  # (exact in fp32: multiples of 1/4)
    out = R.intensity_map_model(ramp)
    assert np.all(out["imap"][1:-1, 1:-1, 1] == a) and np.all(out["imap"][1:-1, 1:-1, 2] == b) and out["usable"][1:-1, 1:-1].all()
    assert np.array_equal(out["imap"][1:-1, 1:-1, 0], ramp[1:-1, 1:-1]) and not out["imap"][0].any() and not out["usable"][:, 0].any()
    # the plane moved in itself by a fraction of a pixel: the observation sees the ramp at the landing position
    p = M.fronto_parallel_scene(24, 18)
    vn = M.depth_normals_model(p["model_depth"], p["fx"], p["fy"], p["cx"], p["cy"])["vnmap"].astype(np.float32)
    for shift in ((0.3, -0.2), (-0.45, 0.49), (0.0, 0.125)):
        fx, fy = M.f32(p["fx"]), M.f32(p["fy"])
        view_in = M.w2ct(np.eye(3), np.array([-shift[0] * 2.0 / fx, -shift[1] * 2.0 / fy, 0.0]))
        m = R.rgbd_step_model(p["depth_obs"], None, vn, np.zeros((18, 24), np.float32), out["imap"].astype(np.float32),
                              p["model_view"], view_in, p["fx"], p["fy"], p["cx"], p["cy"])
        lit = m["photometric"]
        want = a * m["u"] + b * m["v"] + 3.0  # the ramp at the landing position, against I_obs = 0
        assert lit.sum() >= 20 * 14 and np.abs(m["u"] - np.tile(np.arange(24), 18) - shift[0])[lit].max() < 1e-5
        assert np.abs(m["r_p"] - want)[lit].max() < 1e-12


def test_the_jacobian_is_the_finite_difference_of_the_residual():
    """r_p(eps) = I(pi(exp(eps xi) q)) on a smooth image, J_p . xi its derivative at 0, in float64"""
    fx, fy, cx, cy = 70.0, 64.0, 47.0, 36.0
    image = lambda u, v: 0.5 + 0.2 * np.sin(0.11 * u + 0.3) * np.cos(0.07 * v) + 0.1 * np.sin(0.05 * u - 0.09 * v)  # noqa: E731
    du = lambda u, v: 0.2 * 0.11 * np.cos(0.11 * u + 0.3) * np.cos(0.07 * v) + 0.1 * 0.05 * np.cos(0.05 * u - 0.09 * v)  # noqa: E731
    dv = lambda u, v: -0.2 * 0.07 * np.sin(0.11 * u + 0.3) * np.sin(0.07 * v) - 0.1 * 0.09 * np.cos(0.05 * u - 0.09 * v)  # noqa: E731
    project = lambda q: (fx * q[0] / q[2] + cx, fy * q[1] / q[2] + cy)  # noqa: E731
    rng = np.random.default_rng(3)
    for _ in range(20):
        q = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(1.5, 3.0)])
        xi = rng.standard_normal(6)
        J = R.photo_jacobian(du(*project(q)), dv(*project(q)), fx, fy, q)
        eps = 1e-6
        moved = []
        for sign in (1.0, -1.0):
            Re, te = M.se3_exp(sign * eps * xi)
            moved.append(image(*project(Re @ q + te)))
        numeric = (moved[0] - moved[1]) / (2 * eps)
        assert abs(J @ xi - numeric) <= 1e-8 * max(1.0, abs(numeric)), (J @ xi, numeric)


def test_halving_a_hand_made_frame_with_a_hole_and_a_step():
    planes = np.arange(15, dtype=np.float32).reshape(1, 3, 5)
    depth = np.array([[1.0, 1.05, 0.0, 2.0, 9.0],
                      [1.0, np.nan, 0.0, 3.0, 9.0],
                      [7.0, 7.0, 7.0, 7.0, 7.0]], np.float32)
    out = R.halve_model(planes, depth)
    assert out["planes"].shape == (1, 1, 2) and out["planes"].tolist() == [[[3.0, 5.0]]]  # (0 + 1 + 5 + 6) / 4, (2 + 3 + 7 + 8) / 4
    want = np.float32(np.float32(np.float32(1.0) + np.float32(1.05)) + np.float32(1.0)) / np.float32(3.0)  # the hole is left out
    assert out["depth"].shape == (1, 2) and out["depth"][0, 0] == want and out["depth"][0, 1] == 0.0  # a step of 50 %: refused
    assert R.halve_model(None, depth, max_jump=0.5)["depth"][0, 1] == np.float32(2.5)
    assert R.halve_model(None, depth, depth_range=(1.02, INF))["depth"][0, 0] == np.float32(1.05)
    assert R.halve_model(None, np.zeros((2, 2), np.float32))["depth"].tolist() == [[0.0]]
    assert R.level_intrinsics(525.0, 520.0, 319.5, 239.5) == (262.5, 260.0, 159.5, 119.5)
    # pixel (x, y) of the level covers pixels 2x, 2x + 1 of the level below: its centre is at 2x + 0.5 there
    fx, _, cx, _ = R.level_intrinsics(525.0, 520.0, 319.5, 239.5)
    assert (7 - cx) / fx == (2 * 7 + 0.5 - 319.5) / 525.0


def test_unusable_pixels_of_the_intensity_map():
    image = np.full((1, 6, 8), 0.5, np.float32)
    image[0, 2, 3] = np.nan
    mask = np.ones((6, 8), np.float32)
    mask[4, 6] = 0.5
    u = R.intensity_map_model(image)["usable"]
    assert not u[1:4, 2:5].any() and u[1:5, 1].all() and u[4, 2:7].all() and u.sum() == 24 - 9
    u = R.intensity_map_model(image, mask_image=mask)["usable"]
    assert not u[3:5, 5:7].any() and u[4, 4] and u.sum() == 24 - 9 - 4  # (the mask's 3 x 3 reaches four interior pixels)
    rgb = np.full((3, 6, 8), 0.5, np.float32)
    rgb[1, 0, 0] = np.inf  # a corner: poisons the one interior pixel next to it
    out = R.intensity_map_model(rgb)
    assert not out["usable"][1, 1] and out["usable"].sum() == 23
    assert abs(out["imap"][2, 2, 0] - 0.5) < 1e-7 and out["bound"][2, 2, 0] > 0 and not out["imap"][2, 2, 1:3].any()


# -------------------------------------------------------------------------------------------------- marks, bounds, mutants
@pytest.mark.parametrize("W,H,stride", FRAMES, ids=IDS)
def test_the_marks_stay_within_the_cap(W, H, stride):
    s = corner_frame(W, H)
    for weights in WEIGHTS:
        for hubers in HUBERS:
            m = right_step(W, H, stride, weights, hubers)
            marked = int(m["ambiguous"].sum())
            print(f"{W}x{H}/{stride} {weights} {hubers}: valid {m['valid']} geometric {int(m['geometric'].sum())} photometric "
                  f"{int(m['photometric'].sum())} marked {marked}")
            assert marked <= MARK_CAP * m["valid"] and m["geometric"].sum() > 0
            assert m["photometric"].sum() > 0
    assert not s["imap"]["ambiguous"].any()
    t = R.textured_plane_scene(96, 80)
    for key in ("model_depth", "depth_obs"):
        assert not M.depth_normals_model(t[key], t["fx"], t["fy"], t["cx"], t["cy"])["ambiguous"].any()


MUTANT_FRAMES = [f for f in FRAMES if f[0] > 3]  # (3 x 3 has one usable map pixel: a handful of pairs, there for the edges)


@pytest.mark.parametrize("mutate", ["gz_sign", "no_subpixel", "weight_on_A_only", "swap_axes"])
@pytest.mark.parametrize("W,H,stride", MUTANT_FRAMES, ids=IDS[1:])
def test_a_wrong_model_breaks_the_bound_by_orders_of_magnitude(W, H, stride, mutate):
    s = corner_frame(W, H)
    kw = dict(geo_weight=1.0, photo_weight=0.6)
    right, wrong = step(s, stride, **kw), step(s, stride, mutate=mutate, **kw)
    sets = (right["geometric"], right["photometric"])
    (S, B, mag), (S_wrong, _, _) = right["sums"](*sets), wrong["sums"](*sets)
    excess = np.abs(S_wrong - S) / (B + 2.0 ** -50 * mag + 1e-300)
    print(f"{W}x{H}/{stride} {mutate}: largest |S_wrong - S| / bound {excess.max():.3g}; B / sum |term| at most "
          f"{(B / (mag + 1e-300)).max():.3g}")
    # two orders of magnitude, and one at 640 x 480: there the bound of the sums is no longer the roundings' but that of the 25
    # candidates at a landing pixel's edge, each of which covers the change to the neighbouring pixel (no_subpixel: 27)
    assert excess.max() > (100.0 if W <= 96 else 10.0)
    assert (B <= 1e-3 * mag + 1e-12).all()  # the bound stays far below the sums' own size


@pytest.mark.parametrize("W,H", MAP_FRAMES[1:], ids=[f"{w}x{h}" for w, h in MAP_FRAMES[1:]])
def test_swapped_sobel_axes_break_the_map_bound(W, H):
    image, _ = map_frame(W, H, False)
    right, wrong = R.intensity_map_model(image), R.intensity_map_model(image, mutate="swap_axes")
    u = right["usable"]
    excess = np.abs(wrong["imap"][u][:, 1:3] - right["imap"][u][:, 1:3]) / (right["bound"][u][:, 1:3] + 1e-300)
    print(f"{W}x{H}: median excess {np.median(excess):.3g}")
    assert np.median(excess) > 100.0


def test_photo_weight_zero_is_the_icp_model():
    s = corner_frame(96, 80)
    m = step(s, 1, photo_weight=0.0)
    icp = M.icp_step_model(s["depth_obs"], s["vn_obs"], s["vn_model"], s["model_view"], s["view_in"], s["fx"], s["fy"], s["cx"], s["cy"])
    S31, _, _ = m["sums"]()
    S29, _, _ = icp["sums"]()
    assert np.array_equal(S31[:29], S29) and S31[29] == 0.0 and S31[30] == 0.0 and m["photometric"].sum() > 0
    assert np.array_equal(m["flags"] & 7, icp["flags"])


# -------------------------------------------------------------------------------------------------------------- convergence
def test_the_textured_fronto_parallel_plane_converges_where_icp_refuses():
    s = R.textured_plane_scene(96, 80)
    intr = (s["fx"], s["fy"], s["cx"], s["cy"])
    icp = M.icp_align_model(s["depth_obs"], s["model_depth"], None, s["model_view"], *intr, iterations=1)
    assert icp["ok"] == [False] and icp["count"][0] > 5000
    out = R.rgbd_align_model(s["color_obs"], s["depth_obs"], s["model_color"], s["model_depth"], None, s["model_view"], *intr, iterations=3)
    e0, e = M.pose_error(s["model_view"], s["true_view"]), M.pose_error(out["viewmatrix"], s["true_view"])
    print("textured plane 96 x 80: start", e0, "after three iterations", e, out["rows"])
    assert all(r["ok"] for r in out["rows"]) and e0[0] > 2e-2 and e0[1] > 2.5e-2 and e[0] < 1e-4 and e[1] < 1e-4
    assert all(r["marked"] <= MARK_CAP * 96 * 80 for r in out["rows"])
    # the hybrid system is well conditioned where the geometric one is singular
    vn = M.depth_normals_model(s["model_depth"], *intr)["vnmap"].astype(np.float32)
    imap = R.intensity_map_model(s["model_color"])["imap"].astype(np.float32)
    m = R.rgbd_step_model(s["depth_obs"], None, vn, s["color_obs"], imap, s["model_view"], s["model_view"], *intr)
    sol = R.solve_update(m["sums"]()[0], s["model_view"], s["model_view"])
    print("cond(A)", sol["cond"])
    assert sol["ok"] and sol["cond"] < 1e3


def test_the_recorded_pyramid_case():
    """tests/golden/rgbd_pyramid_640x480.json is what `python tests/rgbd_model.py` wrote: one level stays stuck in the fine
    texture's basin, five levels converge.  The first three (cheap) levels of the five are run again here."""
    g = R.golden()
    one, five = g["one_level"], g["five_levels"]
    print("one level", one["pose_error"], "five levels", five["pose_error"])
    assert one["pose_error"][0] > 1e-2 and one["pose_error"][1] > 1e-2
    assert five["pose_error"][0] < 1e-5 and five["pose_error"][1] < 1e-5
    assert len(five["rows"]) == 30 and [r["level"] for r in five["rows"]] == [lv for lv in (4, 3, 2, 1, 0) for _ in range(6)]
    _, again = R.pyramid_model("five_levels", stop_after=18)
    assert again["rows"] == five["rows"][:18]
    assert all(r["marked"] <= MARK_CAP * (640 >> r["level"]) * (480 >> r["level"]) for r in one["rows"] + five["rows"])
