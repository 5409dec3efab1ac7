"""The float64 model of generalized ICP (tests/gicp_model.py) against closed forms, its own convergence on the room corner, and
deliberately wrong models: none of it needs a GPU.  The GPU tests hold the kernels to this model."""
import numpy as np
import pytest

import gicp_model as gm
import icp_model as im


def _rotation(seed):
    q = np.random.default_rng(seed).standard_normal(4)
    return im.quat_to_rotation(q / np.linalg.norm(q))


def _lattice_patch(h, G=None, c=None):
    """the 3 x 3 lattice patch of the plane z = 0 with spacing h, moved by X -> G X + c; every row's neighbourhood is all nine"""
    g = np.array([-1.0, 0.0, 1.0]) * h
    y, x = np.meshgrid(g, g, indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), np.zeros(9)], 1)
    if G is not None:
        p = p @ G.T + c
    return p.astype(np.float32), np.tile(np.arange(9), (9, 1))


# --------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("h", [0.25, 1.0, 2.0 ** -6])
def test_lattice_patch_of_a_plane_gives_the_closed_form(h):
    """spacing h (a power of two: the coordinates are exact): C = diag(2/3 h^2, 2/3 h^2, 0), the normal is exactly z, sigma = 0,
    PLANE = I - (1 - epsilon) n n^T"""
    p, idx = _lattice_patch(h)
    m = gm.covariances_model(p, idx, mode=gm.RAW, min_neighbours=3)
    assert m["valid"].all() and (m["n"] == 9).all()
    want = np.diag([2.0 / 3.0 * h * h, 2.0 / 3.0 * h * h, 0.0])
    assert np.abs(m["C"] - want).max() <= 4 * gm.U64 * h * h
    assert np.array_equal(m["normals"][:, :3], np.tile([0.0, 0.0, 1.0], (9, 1))) and np.all(m["sigma"] == 0.0)
    assert np.array_equal(m["lam"][:, 0], np.zeros(9))
    eps = 1e-3
    pl = gm.covariances_model(p, idx, mode=gm.PLANE, epsilon=eps, min_neighbours=3)
    want6 = np.array([1.0, 0.0, 0.0, 1.0, 0.0, gm.f32(eps)])
    assert np.abs(pl["cov"][:, :6] - want6).max() <= 2 * gm.U64
    assert np.array_equal(pl["cov"][:, 7], np.full(9, 9.0))
    # the Gaussian: two scales of sqrt(2/3) h, the third at the floor, a frame with det +1 whose third axis is the normal
    assert np.abs(m["log_scales"][:, :2] - 0.5 * np.log(2.0 / 3.0 * h * h)).max() <= 1e-14
    assert np.all(m["log_scales"][:, 2] == 0.5 * np.log(gm.f32(1e-4) ** 2))
    assert np.abs(np.linalg.det(m["frame"]) - 1.0).max() <= 1e-14 and np.array_equal(m["frame"][:, :, 2], m["normals"][:, :3])


@pytest.mark.parametrize("seed", range(4))
def test_covariance_transforms_as_G_C_Gt_under_a_rigid_motion(seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    idx = gm.self_neighbours(p, 10)
    G, c = _rotation(seed), rng.uniform(-2, 2, 3)
    moved = (p.astype(np.float64) @ G.T + c)
    a = gm.covariances_model(p, idx, mode=gm.RAW)
    b = gm.covariances_model(moved.astype(np.float32), idx, mode=gm.RAW)
    want = G[None] @ a["C"] @ G.T[None]
    # (the moved cloud is rounded to fp32: 2^-24 of |p| <= 4 on each coordinate, against deviations of order 1)
    assert np.abs(b["C"] - want).max() <= 64 * gm.U32
    assert np.abs(b["lam"] - a["lam"]).max() <= 64 * gm.U32
    n_a, n_b = a["normals"][:, :3] @ G.T, b["normals"][:, :3]
    keep = a["gap"] > 1e-2
    assert keep.sum() >= 30
    assert (np.abs(np.abs(np.sum(n_a * n_b, 1)) - 1.0)[keep] <= 1e-4).all()


def test_jacobi_agrees_with_lapack_and_ends_with_exact_zeros():
    rng = np.random.default_rng(5)
    B = rng.standard_normal((500, 3, 3)) * rng.uniform(1e-3, 10, (500, 1, 1))
    C = B @ B.transpose(0, 2, 1)
    C[:50] = np.diag([1.0, 1.0, 2.0])  # degenerate and already diagonal
    C[50:100, 2] = C[50:100, :, 2] = 0.0  # rank 2
    lam, V = gm.jacobi_eigen(C)
    want = np.linalg.eigvalsh(C)
    assert np.abs(np.sort(lam, 1) - want).max() <= 1e-15 * np.abs(want).max(1).max() * 50
    assert (np.abs(np.sort(lam, 1) - want) <= 1e-15 * 8 * np.abs(want).max(1)[:, None]).all()
    assert np.abs(V.transpose(0, 2, 1) @ V - np.eye(3)).max() <= 1e-14
    recon = (V * lam[:, None, :]) @ V.transpose(0, 2, 1)
    assert (np.abs(recon - C).max((1, 2)) <= 1e-14 * np.abs(C).max((1, 2))).all()


def test_orientation_rules_and_invalid_rows():
    p, idx = _lattice_patch(0.5, _rotation(3), np.array([0.3, -0.2, 2.0]))
    toward = gm.covariances_model(p, idx, viewpoint=(0.0, 0.0, 0.0), min_neighbours=3)
    n = toward["normals"][:, :3]
    assert (np.sum(n * (0.0 - p.astype(np.float64)), 1) >= 0).all()
    away = gm.covariances_model(p, idx, viewpoint=(0.6, -0.4, 4.0), min_neighbours=3)
    assert np.abs(away["normals"][:, :3] + n).max() <= 1e-12
    plain = gm.covariances_model(p, idx, min_neighbours=3)["normals"][:, :3]
    lead = np.take_along_axis(plain, np.abs(plain).argmax(1)[:, None], 1)
    assert (lead > 0).all()
    # -1 ends a list; an out-of-range entry ends it too; too few neighbours, a NaN neighbour, coincident points: invalid
    bad = idx.copy()
    bad[0, 5:] = -1
    bad[1, 2] = 9
    bad[2, 3] = -7
    q = p.copy()
    q[8] = np.nan
    m = gm.covariances_model(q, bad, min_neighbours=4)
    assert list(m["n"][:3]) == [5, 2, 3] and m["valid"][0] and not m["valid"][1] and not m["valid"][2]
    assert not m["valid"][3:].any()  # every other row lists the NaN point 8
    for key in ("cov", "normals", "log_scales", "quats"):
        assert not m[key][~m["valid"]].any(), key
    same = np.zeros((6, 3), np.float32) + np.float32(0.7)
    assert not gm.covariances_model(same, np.tile(np.arange(6), (6, 1)))["valid"].any()


# ---------------------------------------------------------------------------------------------------------------------- step
def test_point_to_point_with_known_pairs_recovers_a_small_twist_to_second_order():
    rng = np.random.default_rng(11)
    target = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    for scale in (1e-2, 1e-3):
        xi = scale * np.array([0.5, -0.8, 0.3, 0.6, 0.2, -0.7])
        R, t = im.se3_exp(xi)
        source = ((target.astype(np.float64) - t) @ R).astype(np.float32)  # R^T (b - t): the motion (R, t) takes it back
        m = gm.gicp_step_model(target, None, source, None, np.eye(4, dtype=np.float32), idx=np.arange(300))
        out = gm.solve_update(m["sums"]()[0], np.eye(4, dtype=np.float32))
        assert out["ok"] and m["sums"]()[0][28] == 300
        err = np.abs(out["xi"] - xi).max()
        assert err <= 4 * scale * scale + 1e-6, (scale, err)  # one Gauss-Newton step: second order in the twist (+ fp32 clouds)


def test_a_single_plane_is_refused_undamped_and_solved_damped_without_motion_in_the_free_directions():
    g = np.linspace(-1, 1, 12)
    y, x = np.meshgrid(g, g, indexing="ij")
    target = np.stack([x.ravel(), y.ravel(), np.full(144, 2.0)], 1).astype(np.float32)
    source = target + np.float32([0.0, 0.0, 0.05])
    n = np.zeros((144, 3, 3))
    n[:, 2, 2] = 1.0
    eye = np.eye(4, dtype=np.float32)
    # the plane's own degenerate covariance diag(1, 1, 0) has no inverse: every pair is singular and dropped
    flat = gm.pack_cov(n * 0 + np.diag([1.0, 1.0, 0.0])[None])
    assert gm.gicp_step_model(target, flat, source, None, eye, idx=np.arange(144))["flags"].tolist() == [7] * 144
    # the point-to-plane limit: M = z z^T (to 1e-30) handed in as C = diag(big, big, 1)
    big = gm.pack_cov(np.diag([1e30, 1e30, 1.0])[None].repeat(144, 0))
    m = gm.gicp_step_model(target, big, source, None, eye, idx=np.arange(144))
    s29 = m["sums"]()[0]
    refused = gm.solve_update(s29, eye, damping=0.0)
    assert not refused["ok"] and np.array_equal(refused["viewmatrix"], eye) and refused["omega"] == 0.0
    solved = gm.solve_update(s29, eye, damping=1e-3)
    assert solved["ok"]
    xi = solved["xi"]
    assert abs(xi[5] + 0.05) <= 1e-3 * 0.05 * 2  # v_z closes the gap (shrunk by the damping)
    assert np.abs(xi[[2, 3, 4]]).max() <= 1e-12  # omega_z, v_x, v_y: free, and not moved


def test_convergence_on_the_room_corner():
    """24 x 18: from the identity, (2.1e-2 rad, 3.1e-2 m) from the truth.  Recorded here (float64 model, k = 10, PLANE both sides):
    iteration 3 is below 1e-3 in both, every valid source is associated, cond(A) is of order 10^2."""
    c = gm.corner_clouds(24, 18)
    cs = gm.covariances_model(c["source"], gm.self_neighbours(c["source"], 10))
    ct = gm.covariances_model(c["target"], gm.self_neighbours(c["target"], 10))
    assert not (cs["gap"][cs["valid"]] < 1e-2).any() and not (ct["gap"][ct["valid"]] < 1e-2).any()
    a0, t0 = gm.transform_error(np.eye(4, dtype=np.float32), c["truth"])
    assert abs(a0 - np.linalg.norm(im.TWIST[:3])) <= 1e-6 and 2e-2 <= t0 <= 4e-2
    errs = []
    for it in (1, 2, 3, 6):
        out = gm.gicp_align_model(c["source"], c["target"], source_cov=cs["cov"].astype(np.float32),
                                  target_cov=ct["cov"].astype(np.float32), iterations=it)
        errs.append(gm.transform_error(out["transform"], c["truth"]))
        assert all(out["ok"]) and out["count"][-1] == 432
    print("gicp model, corner 24x18: errors after 1, 2, 3, 6 iterations", errs, "cond", out["cond"])
    assert errs[2][0] <= 1e-3 and errs[2][1] <= 1e-3
    assert errs[0][0] < a0 and errs[0][1] < t0
    assert max(out["cond"]) <= 1e3


@pytest.mark.parametrize("shape", [(24, 18, 1), (96, 80, 2), (160, 120, 4)])
def test_the_corner_clouds_mark_no_row(shape):
    W, H, stride = shape
    c = gm.corner_clouds(W, H, stride)
    for name in ("source", "target"):
        m = gm.covariances_model(c[name], gm.self_neighbours(c[name], 10))
        assert m["valid"].all() and not m["ambiguous"].any()
        assert m["gap"].min() >= 1e-2, (name, m["gap"].min())


# ---------------------------------------------------------------------------------------------------------------- wrong models
@pytest.fixture(scope="module", params=[(24, 18, 1), (96, 80, 2), (160, 120, 4)], ids=["24x18", "96x80s2", "160x120s4"])
def corner(request):
    c = gm.corner_clouds(*request.param)
    R, t = im.se3_exp(0.5 * im.TWIST + 0.01)
    c["T"] = gm.as_transform(R, t)
    c["cs"] = gm.covariances_model(c["source"], gm.self_neighbours(c["source"], 10))["cov"].astype(np.float32)
    c["ct"] = gm.covariances_model(c["target"], gm.self_neighbours(c["target"], 10))["cov"].astype(np.float32)
    return c


@pytest.mark.parametrize("mutate", gm.STEP_MUTANTS)
def test_wrong_step_models_break_the_bound_by_orders_of_magnitude(corner, mutate):
    c = corner
    right = gm.gicp_step_model(c["target"], c["ct"], c["source"], c["cs"], c["T"])
    wrong = gm.gicp_step_model(c["target"], c["ct"], c["source"], c["cs"], c["T"], mutate=mutate)
    (s, bound), (sw, _) = right["sums"](), wrong["sums"]()
    excess = np.abs(sw[:28] - s[:28]) / np.maximum(bound, 1e-300)
    assert excess.max() >= 1e6, (mutate, excess.max())


def test_a_right_update_breaks_the_pose_figures(corner):
    c = corner
    s29 = gm.gicp_step_model(c["target"], c["ct"], c["source"], c["cs"], c["T"])["sums"]()[0]
    want = gm.solve_update(s29, c["T"])
    wrong = gm.solve_update(s29, c["T"], mutate="right_update")
    assert want["ok"] and wrong["ok"]
    fig = im.pose_figures(wrong["viewmatrix"], wrong["quat"], wrong["trans"], want)
    assert not im.pose_holds(fig) and fig["ulps"].max() >= 1e2
    assert im.pose_holds(im.pose_figures(want["viewmatrix"], want["quat"], want["trans"], want))


def test_the_sample_covariance_breaks_the_raw_bound(corner):
    p = corner["source"]
    idx = gm.self_neighbours(p, 10)
    right = gm.covariances_model(p, idx, mode=gm.RAW)
    wrong = gm.covariances_model(p, idx, mode=gm.RAW, mutate="n_minus_1")
    excess = np.abs(wrong["cov"][:, :6] - right["cov"][:, :6]).max(1) / right["cov_bound"].max(1)
    assert excess.min() >= 1e4, excess.min()


def test_the_transform_twin_rounds_every_operation_once():
    rng = np.random.default_rng(2)
    a = rng.uniform(-3, 3, (1000, 3)).astype(np.float32)
    a[7] = [np.nan, 1.0, 2.0]
    a[9] = [1.0, np.inf, 2.0]
    R, t = im.se3_exp(im.TWIST * 3)
    T = gm.as_transform(R, t)
    q = gm.transform32(T, a)
    exact = a.astype(np.float64) @ im.pose_of(T)[0].T + im.pose_of(T)[1]
    ok = np.isfinite(a).all(1)
    assert np.abs(q[ok] - exact[ok]).max() <= 4 * gm.U32 * 12 and not np.isfinite(q[7]).all() and not np.isfinite(q[9]).all()
    # against a fused evaluation (float64 then one rounding) some values differ in the last bit: the twin is not that
    assert (q[ok] != exact[ok].astype(np.float32)).any()
    assert gm.max_dist2(0.1) == np.float32(0.1) * np.float32(0.1) and gm.max_dist2(gm.INF) == np.inf
