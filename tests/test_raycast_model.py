"""The numpy model of the ray-cast (tests/raycast_model.py) against surfaces whose answer is known, on the CPU: a plane (the
trilinear interpolant reproduces a linear field, so depth and normal are analytic to rounding), a sphere (inside a second-order
bound derived below), the brick rule on hand-built volumes, and the share of ambiguous pixels of every case the GPU tests use."""
import numpy as np
import pytest

import raycast_model as M
import tsdf_model as T

DIMS, ORIGIN, VOXEL = (30, 26, 24), (-0.75, -0.65, 1.0), 0.05
CAM = dict(H=24, W=32, fx=34.0, fy=36.0, cx=15.3, cy=11.8)


def _plane_volume(normal, offset, scale):
    """float64 [Nz, Ny, Nx, 2]: the UNCLIPPED linear field (offset - normal . p) / scale with weight 2 (float64 storage: the
    model converts the volume to its own type, so nothing is rounded to float32 on the way)"""
    X, Y, Z = T.lattice(ORIGIN, VOXEL, DIMS)
    v = (offset - (normal[0] * X + normal[1] * Y + normal[2] * Z)) / scale
    return np.stack([v, np.full(v.shape, 2.0)], axis=-1)


@pytest.mark.parametrize("name, pose, normal, offset", [
    ("frontal", T.pose(0.0, 0.0, 0.0, [0.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), 1.6),
    ("tilted", T.pose(0.07, -0.15, 0.04, [0.1, -0.03, 0.02]), np.array([0.31, -0.22, 1.0]) / np.linalg.norm([0.31, -0.22, 1.0]), 1.62),
])
def test_a_plane_gives_the_analytic_depth_and_normal(name, pose, normal, offset):
    """the field is positive on the camera's side of the plane normal . p = offset"""
    vol = _plane_volume(normal, offset, 2.0)
    r = M.raycast(vol, None, ORIGIN, VOXEL, pose, **CAM)
    m = pose.astype(np.float64).T
    R, t = m[:3, :3], m[:3, 3]
    ys, xs = np.mgrid[0:CAM["H"], 0:CAM["W"]].astype(np.float64)
    dc = np.stack([(xs - np.float32(CAM["cx"])) / np.float32(CAM["fx"]), (ys - np.float32(CAM["cy"])) / np.float32(CAM["fy"]), np.ones_like(xs)], -1)
    o_w, d_w = -R.T @ t, dc @ R
    z = (offset - normal @ o_w) / (d_w @ normal)
    hit = (r["flags"][0] & M.HIT) > 0
    assert hit.mean() > 0.5 and not (r["flags"][0] & M.UNSEEN).any()
    assert np.abs(r["depth"][0] - z)[hit].max() < 1e-9
    with_normal = hit & ((r["flags"][0] & M.NO_NORMAL) == 0)
    assert with_normal.mean() > 0.4
    n_c = R @ -normal  # the field's gradient is -normal: towards the camera
    assert (n_c * dc[with_normal] ).sum(-1).max() < 0  # facing the camera
    assert np.abs(r["vnmap"][0][with_normal][:, :3] - n_c).max() < 1e-9
    assert np.abs(r["vnmap"][0][with_normal][:, 3] - z[with_normal]).max() < 1e-9
    assert not r["vnmap"][0][~with_normal].any() and not r["depth"][0][~hit].any()


def test_a_sphere_lies_inside_the_second_order_bound():
    """phi(p) = |p - c| - r has the Hessian (I - n n^T) / rho, rho = |p - c|: positive semi-definite with trace 2 / rho.
    Trilinear interpolation over a cell of size h errs by at most sum_a h^2 / 8 max |d_aa phi| = h^2 / (4 rho) =: E1.  Along a ray
    phi'' <= 1 / rho, so the chord between two samples a length L apart errs by at most L^2 / (8 rho) =: E2.  The secant's root
    z* therefore has |phi(p*)| <= E1 + E2, and with the incidence cosine c the depth is off by at most (E1 + E2) / (c |d_c|), to
    first order; 1.2 covers the change of c over that distance (error << r), pixels with c >= 0.5 are judged.
    Normal: each central difference over +- h errs by E1 / h (two values E1 off, 2 h apart) plus h^2 / 6 |phi'''| <= h^2 / (2 rho^2):
    eps = h / (4 rho) + h^2 / (2 rho^2) per axis, the angle at most sqrt(3) eps / (1 - sqrt(3) eps).
    rho >= r - 3 h in every cell and stencil point involved."""
    c, r0, h = np.array([0.013, -0.021, 1.62]), 0.45, VOXEL
    vol = T.sdf_volume(DIMS, ORIGIN, VOXEL, 4.0 * VOXEL, T.sphere_sdf(c, r0), weight=2.0)
    pose = T.pose(0.03, -0.05, 0.02, [0.04, -0.02, 0.01])
    r = M.raycast(vol, None, ORIGIN, VOXEL, pose, **CAM)
    m = pose.astype(np.float64).T
    R, t = m[:3, :3], m[:3, 3]
    ys, xs = np.mgrid[0:CAM["H"], 0:CAM["W"]].astype(np.float64)
    dc = np.stack([(xs - np.float32(CAM["cx"])) / np.float32(CAM["fx"]), (ys - np.float32(CAM["cy"])) / np.float32(CAM["fy"]), np.ones_like(xs)], -1)
    o_w, d_w = -R.T @ t, dc @ R
    oc = o_w - c
    A, B, C = (d_w * d_w).sum(-1), 2.0 * (d_w @ oc), oc @ oc - r0 ** 2
    disc = B * B - 4 * A * C
    z = (-B - np.sqrt(np.maximum(disc, 0.0))) / (2 * A)
    p = o_w + z[..., None] * d_w
    n_w = (p - c) / r0
    dlen = np.sqrt(A)
    cos = -(n_w * d_w).sum(-1) / dlen
    judged = (disc > 0) & (cos >= 0.5)
    hit = (r["flags"][0] & M.HIT) > 0
    assert judged.sum() > 100 and hit[judged].all()
    rho = r0 - 3 * h
    L = 0.5 * h * dlen
    bound = 1.2 * (h * h / (4 * rho) + L * L / (8 * rho)) / (cos * dlen)
    err = np.abs(r["depth"][0] - z)
    assert (err[judged] <= bound[judged]).all(), (err[judged] / bound[judged]).max()
    eps = h / (4 * rho) + h * h / (2 * rho * rho)
    angle_max = np.sqrt(3) * eps / (1 - np.sqrt(3) * eps)
    with_normal = judged & ((r["flags"][0] & M.NO_NORMAL) == 0)
    assert with_normal.sum() > 100
    n_c = n_w @ R.T
    angle = np.arccos(np.clip((r["vnmap"][0][..., :3] * n_c).sum(-1), -1, 1))
    assert angle[with_normal].max() <= angle_max, (angle[with_normal].max(), angle_max)
    print(f"sphere: depth error at most {err[judged].max():.2e} ({(err[judged] / bound[judged]).max():.2f} of the bound), "
          f"angle at most {angle[with_normal].max():.4f} rad (bound {angle_max:.4f})")


def _positive(n=17):
    return np.stack([np.full((n, n, n), 0.5, dtype=np.float32), np.ones((n, n, n), dtype=np.float32)], axis=-1)


def test_the_brick_rule_on_hand_built_volumes():
    """17^3 samples = 16^3 cells = 2 x 2 x 2 bricks; volume[z, y, x]"""
    none = np.zeros((2, 2, 2), dtype=np.uint8)
    assert np.array_equal(M.bricks(_positive()), none)
    # one negative corner inside a brick: its 8 cells (2..3 on every axis) lie in brick (0, 0, 0)
    v = _positive()
    v[3, 3, 3, 0] = -0.25
    want = none.copy()
    want[0, 0, 0] = 1
    assert np.array_equal(M.bricks(v), want)
    # an exact zero counts (tsdf <= 0), a NaN does not
    v[3, 3, 3, 0] = 0.0
    assert np.array_equal(M.bricks(v), want)
    v[3, 3, 3, 0] = np.nan
    assert np.array_equal(M.bricks(v), none)
    v[3, 3, 3, 0] = -0.25
    # a neighbour below min_weight kills the four cells that hold both (x = 3 .. 4); the four at x = 2 .. 3 keep the brick alive
    v[3, 3, 4, 1] = 0.5
    assert np.array_equal(M.bricks(v), want)
    # the neighbour on the other side too: every cell around the corner is invalid now
    v[3, 3, 2, 1] = 0.5
    assert np.array_equal(M.bricks(v), none)
    assert np.array_equal(M.bricks(v, min_weight=0.5), want)  # (>=: a weight AT min_weight counts)
    # the corner's own weight
    v = _positive()
    v[3, 3, 3] = (-0.25, 0.0)
    assert np.array_equal(M.bricks(v), none)
    # a negative corner on a brick boundary plane belongs to the cells on both sides of it
    v = _positive()
    v[3, 3, 8, 0] = -0.25
    want = none.copy()
    want[0, 0, :] = 1
    assert np.array_equal(M.bricks(v), want)
    v = _positive()
    v[8, 8, 8, 0] = -0.25
    assert np.array_equal(M.bricks(v), np.ones((2, 2, 2), dtype=np.uint8))
    # the last lattice plane: only the cells in front of it
    v = _positive()
    v[5, 16, 5, 0] = -0.25
    want = none.copy()
    want[0, 1, 0] = 1
    assert np.array_equal(M.bricks(v), want)
    # shapes: a lattice without a cell has no brick, 9 samples make one brick, 10 make two
    assert M.bricks(_positive(1)).shape == (0, 0, 0) and M.bricks(_positive(9)).shape == (1, 1, 1)
    assert M.bricks(np.zeros((9, 10, 17, 2), dtype=np.float32)).shape == (1, 2, 2)


def test_a_dead_brick_holds_no_decisive_sample():
    """the reason the skipping is allowed: in the fused volume no sample in a cell of a dead brick is valid with F <= 0"""
    vol, _ = M.fused_main()
    b = M.bricks(vol)
    assert 0.05 < b.mean() < 0.6
    rng = np.random.default_rng(0)
    nz, ny, nx = vol.shape[:3]
    q = rng.uniform(0, 1, (200000, 3)) * (np.array([nx, ny, nz]) - 1)
    valid, F = M._sample(np.float64, vol, q, 1.0)
    i = np.floor(q).astype(int) // 8
    dead = b[i[:, 2], i[:, 1], i[:, 0]] == 0
    assert dead.sum() > 10000 and not (valid & (F <= 0) & dead).any()
    assert (valid & (F <= 0) & ~dead).sum() > 1000


@pytest.mark.parametrize("name", sorted(M.cases()) + sorted(M.extra_cases()))
def test_the_ambiguous_share_of_every_gpu_case_stays_under_the_cap(name):
    case = {**M.cases(), **M.extra_cases()}[name]
    r = M.reference(name)
    assert r["ambiguous"].mean() <= 0.03, r["ambiguous"].mean()
    # the float32 twin takes the same decisions wherever the model calls the pixel decided
    r32 = M.reference32(name)
    keep = ~r["ambiguous"]
    assert np.array_equal(r["flags"][keep], r32["flags"][keep])
    assert case["views"].shape[0] == r["flags"].shape[0]
