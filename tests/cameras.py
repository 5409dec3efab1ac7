"""Pinhole cameras beyond synth's one symmetric frustum, and scene placements that reach the camera arithmetic's edges.

`dgr_amd.synth.camera()` always builds a centred frustum with focal_x == focal_y: Proj[0][2] = Proj[1][2] = 0, so a swapped
focal / limit pair or a dropped off-diagonal perspec entry renders and differentiates the same there.  `Camera` is a general
pinhole camera -- (W, H, fx, fy, cx, cy), a world-to-camera pose and znear / zfar -- and `scene()` builds a synth `Scene` for it
with synth's draws (in the camera's own frustum).  The matrices follow synth's conventions: `view`, `proj` and `persp` hold
W2C^T, (Proj W2C)^T and Proj^T, `campos` = -R^T t, and

    tanfovx = W / (2 fx), tanfovy = H / (2 fy), Proj[0][0] = 2 fx / W, Proj[1][1] = 2 fy / H,
    Proj[0][2] = (2 cx + 1) / W - 1, Proj[1][2] = (2 cy + 1) / H - 1,

so that a point on the optical axis lands on pixel (cx, cy) under the reference's ndc2Pix(v, S) = ((v + 1) S - 1) / 2.

Placements (like synth.heavy_tail_scene) return (scene, info) and each has an `assert_*` that checks the edge it is meant to
reach against the oracle:
  clamp -- a band of Gaussians with |t.x/t.z| or |t.y/t.z| in 1.3 .. 2 tanfov on all four sides (where forward.cu clamps the
           Jacobian's t.x/t.z and the backward zeroes x_grad_mul / y_grad_mul), on-screen sigma 20 .. 150 px so that the
           footprint still enters the frame: at least 50 of them rendered;
  near  -- Gaussians at camera z in (0.2, 0.4] with large footprints, and an "ulp group" whose float32 camera-space z (the
           kernels' and the oracle's evaluation order, no fused multiply-add) is 0.2f and its neighbours up to 4 ulp away: the
           in_frustum test z <= 0.2f decides by the float32 rounding.
"""
from typing import NamedTuple

import numpy as np

from dgr_amd.synth import Scene

NEAR = np.float32(0.2)  # in_frustum's z <= 0.2 (cuda_rasterizer/auxiliary.h:152)


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


class Camera(NamedTuple):
    id: str
    W: int
    H: int
    fx: float
    fy: float
    cx: float
    cy: float
    R: np.ndarray        # [3,3] world -> camera rotation
    t: np.ndarray        # [3]   world -> camera translation
    znear: float = 0.01
    zfar: float = 100.0

    @property
    def tanfovx(self):
        return self.W / (2.0 * self.fx)

    @property
    def tanfovy(self):
        return self.H / (2.0 * self.fy)

    def at(self, W):
        """The same camera at width W (height in proportion): intrinsics scaled about the pixel-centre convention."""
        k = W / self.W
        H = max(1, int(round(self.H * k)))
        return self._replace(W=int(W), H=H, fx=self.fx * k, fy=self.fy * H / self.H, cx=(self.cx + 0.5) * k - 0.5,
                             cy=(self.cy + 0.5) * H / self.H - 0.5)

    def with_pp(self, cx, cy):
        return self._replace(cx=float(cx), cy=float(cy))

    def projection(self):
        """Proj (row-major math, z forward) in float64."""
        Pm = np.zeros((4, 4))
        Pm[0, 0] = 2 * self.fx / self.W
        Pm[1, 1] = 2 * self.fy / self.H
        Pm[0, 2] = (2 * self.cx + 1) / self.W - 1
        Pm[1, 2] = (2 * self.cy + 1) / self.H - 1
        Pm[2, 2] = self.zfar / (self.zfar - self.znear)
        Pm[2, 3] = -(self.zfar * self.znear) / (self.zfar - self.znear)
        Pm[3, 2] = 1
        return Pm

    def matrices(self):
        """(view, proj, persp, campos) as float32, stored as synth stores them."""
        W2C = np.eye(4)
        W2C[:3, :3] = self.R
        W2C[:3, 3] = self.t
        Pm = self.projection()
        return (W2C.T.astype(np.float32), (W2C.T @ Pm.T).astype(np.float32), Pm.T.astype(np.float32),
                (-self.R.T @ self.t).astype(np.float32))

    def to_camera(self, world):
        return np.asarray(world, np.float64) @ self.R.T + self.t

    def to_world(self, cam_pts):
        return (np.asarray(cam_pts, np.float64) - self.t) @ self.R


def _synth_pose(angle=0.05):
    return rotation([0.2, 1.0, 0.1], angle), np.array([0.05, -0.02, 0.10])


def _far_pose():
    R = rotation([1.0, 0.4, 0.3], 2.1)            # > 1 rad about an axis far from z
    campos = np.array([18.0, -24.0, 21.0])        # |campos| = 36.6 units from the world origin
    return R, -R @ campos


def _cameras():
    R0, t0 = _synth_pose()
    R1, t1 = _synth_pose(0.3)
    Rf, tf = _far_pose()
    W, H = 640, 480
    return {
        "tum": Camera("tum", 640, 480, 517.3, 516.5, 318.6, 255.3, R0, t0),
        "replica": Camera("replica", 1200, 680, 600.0, 600.0, 599.5, 339.5, R1, t1),
        # principal point 20 % of W / H off centre, fx / fy = 1.3
        "skewed_pp": Camera("skewed_pp", W, H, 520.0, 400.0, (W - 1) / 2 + 0.2 * W, (H - 1) / 2 - 0.2 * H, R1, t1),
        "wide": Camera("wide", W, H, W / 3.0, W / 3.0 * 0.95, 331.0, 236.0, R0, t0),          # tanfovx 1.5
        "narrow": Camera("narrow", W, H, W / 0.3, W / 0.3 * 1.02, 309.0, 247.0, R0, t0),      # tanfovx 0.15
        "far": Camera("far", W, H, 500.0, 505.0, 324.0, 236.5, Rf, tf),
    }


CAMERAS = _cameras()
CAMERA_IDS = list(CAMERAS)


def scene(cam: Camera, P, seed=0):
    """synth.make_scene's draws (same order and distributions) in `cam`'s frustum: camera z in [1, 6], pixel positions
    uniform over the frame widened by 10 % on each side, on-screen sigma 0.7 .. 4 px."""
    rng = np.random.default_rng(seed)
    view, proj, persp, campos = cam.matrices()
    W, H = cam.W, cam.H
    z = rng.uniform(1.0, 6.0, P)
    u = rng.uniform(-0.1, 1.1, P) * W - 0.5
    v = rng.uniform(-0.1, 1.1, P) * H - 0.5
    xc, yc = (u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z
    means = cam.to_world(np.stack([xc, yc, z], 1)).astype(np.float32)
    sig_px = np.exp(rng.uniform(np.log(0.7), np.log(4.0), (P, 3)))
    scales = (sig_px / cam.fx * z[:, None]).astype(np.float32)
    q = rng.normal(size=(P, 4))
    rots = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    opac = rng.uniform(0.05, 1.0, (P, 1)).astype(np.float32)
    shs = rng.normal(size=(P, 16, 3))
    shs[:, 0, :] *= 0.5
    shs[:, 1:, :] *= 0.1
    shs = shs.astype(np.float32)
    gt = rng.uniform(1.0, 6.0, (H, W)).astype(np.float32)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    gC = (rng.normal(size=(3, H, W)) / (H * W)).astype(np.float32)
    gD = (rng.normal(size=(H, W)) / (H * W)).astype(np.float32)
    gM = (rng.normal(size=(H, W)) / (H * W)).astype(np.float32)
    gV = (rng.normal(size=(H, W)) / (H * W)).astype(np.float32)
    return Scene(P, W, H, cam.tanfovx, cam.tanfovy, view, proj, persp, campos, means, scales, rots, opac, shs, gt, bg,
                 gC, gD, gM, gV)


def camera_z32(s, means=None):
    """Camera-space z as the kernels and the oracle evaluate it: float32, v2 x + v6 y + v10 z + v14 left to right, no FMA."""
    m = np.asarray(s.means if means is None else means, np.float32)
    v = np.asarray(s.view, np.float32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((v[2] * m[:, 0] + v[6] * m[:, 1]) + v[10] * m[:, 2]) + v[14]


def camera_t64(s, means=None):
    m = np.asarray(s.means if means is None else means, np.float64)
    v = np.asarray(s.view, np.float64)
    return np.concatenate([m, np.ones((len(m), 1))], 1) @ v


# ------------------------------------------------------------------------------------------ placements
def _band_opacity(s: Scene, idx, opacity, rng):
    """`opacity` None: as drawn; (lo, hi): the band's opacities uniform in it (a translucent band keeps the pixels behind it from
    terminating, which the small frames of the float64 models need)."""
    if opacity is None:
        return s.opac
    o = s.opac.copy()
    o[idx, 0] = rng.uniform(opacity[0], opacity[1], len(idx)).astype(np.float32)
    return o


def clamp_scene(s: Scene, cam: Camera, n=None, sigma_px=(20.0, 150.0), seed=3, opacity=None):
    """`n` Gaussians (default max(100, P / 10)) moved into the clamp band: |t.x/t.z| (sides 0, 1) or |t.y/t.z| (sides 2, 3)
    drawn in 1.3 .. 2 tanfov, the other ratio inside the frame, camera z in 1 .. 6, isotropic on-screen sigma log-uniform in
    `sigma_px`.  info["band"]: their indices."""
    rng = np.random.default_rng(seed)
    n = max(100, s.P // 10) if n is None else n
    idx = np.sort(rng.choice(s.P, n, replace=False))
    side = np.arange(n) % 4
    z = rng.uniform(1.0, 6.0, n)
    ratio = rng.uniform(1.3, 2.0, n)
    sign = np.where(side % 2 == 0, 1.0, -1.0)
    u = rng.uniform(0.0, 1.0, n) * cam.W - 0.5
    v = rng.uniform(0.0, 1.0, n) * cam.H - 0.5
    rx = np.where(side < 2, sign * ratio * cam.tanfovx, (u - cam.cx) / cam.fx)
    ry = np.where(side >= 2, sign * ratio * cam.tanfovy, (v - cam.cy) / cam.fy)
    means = s.means.copy()
    means[idx] = cam.to_world(np.stack([rx * z, ry * z, z], 1)).astype(np.float32)
    sig = np.exp(rng.uniform(np.log(sigma_px[0]), np.log(sigma_px[1]), n))
    scales = s.scales.copy()
    scales[idx] = (sig[:, None] * rng.uniform(0.9, 1.1, (n, 3)) / cam.fx * z[:, None]).astype(np.float32)
    return s._replace(means=means, scales=scales, opac=_band_opacity(s, idx, opacity, rng)), dict(band=idx)


def assert_clamp_edge(s: Scene, info, radii, least=50):
    """The band lies where the Jacobian clamp acts (in float32 and in float64) and at least `least` of it is rendered."""
    t = camera_t64(s)[info["band"]]
    rx, ry = np.abs(t[:, 0] / t[:, 2]), np.abs(t[:, 1] / t[:, 2])
    clamped = (rx > 1.3 * s.tanfovx * (1 + 1e-5)) | (ry > 1.3 * s.tanfovy * (1 + 1e-5))
    assert clamped.all(), f"{int((~clamped).sum())} band Gaussians are not beyond the clamp"
    shown = np.asarray(radii).reshape(-1)[info["band"]] > 0
    sides = [(rx > 1.3 * s.tanfovx) & (t[:, 0] > 0), (rx > 1.3 * s.tanfovx) & (t[:, 0] < 0),
             (ry > 1.3 * s.tanfovy) & (t[:, 1] > 0), (ry > 1.3 * s.tanfovy) & (t[:, 1] < 0)]
    assert int(shown.sum()) >= least, f"only {int(shown.sum())} clamped Gaussians rendered"
    assert all(int((shown & sd).sum()) >= 1 for sd in sides), [int((shown & sd).sum()) for sd in sides]
    return int(shown.sum())


def _ulp_group(cam: Camera, s: Scene, rng, per_value=3, span=4, positions=24):
    """World positions whose float32 camera z (camera_z32) takes the 2 span + 1 values the float32 sum reaches closest to
    0.2f -- 0.2f and its neighbours up to `span` ulp away where the camera's grid reaches them -- `per_value` positions each,
    at pixel positions spread over the frame.  Found by walking two float32 world coordinates a few dozen ulps about the
    float64 solution.  Returns (points [n, 3], z32 [n])."""
    steps = np.arange(-24, 25).astype(np.float32)
    ax = np.argsort(-np.abs(np.asarray(s.view, np.float64)[:3, 2]))[:2]
    pts, zs = [], []
    for _ in range(positions):
        u = rng.uniform(0.1, 0.9) * cam.W - 0.5
        v = rng.uniform(0.1, 0.9) * cam.H - 0.5
        zc = float(NEAR)
        w0 = cam.to_world([[(u - cam.cx) / cam.fx * zc, (v - cam.cy) / cam.fy * zc, zc]])[0].astype(np.float32)
        A, B = np.meshgrid(w0[ax[0]] + steps * np.spacing(w0[ax[0]]), w0[ax[1]] + steps * np.spacing(w0[ax[1]]), indexing="ij")
        cand = np.repeat(w0[None], A.size, 0)
        cand[:, ax[0]] = A.reshape(-1)
        cand[:, ax[1]] = B.reshape(-1)
        z = camera_z32(s, cand)
        pts.append(cand)
        zs.append(z)
    pts, zs = np.concatenate(pts), np.concatenate(zs)
    vals = np.unique(zs)
    below, above = vals[vals <= NEAR][-(span + 1):], vals[vals > NEAR][:span]
    out_p, out_z = [], []
    for zv in np.concatenate([below, above]):
        hit = np.nonzero(zs == zv)[0]
        pick = rng.choice(hit, min(per_value, len(hit)), replace=False)
        out_p.append(pts[pick])
        out_z.append(zs[pick])
    return np.concatenate(out_p).astype(np.float32), np.concatenate(out_z)


def near_scene(s: Scene, cam: Camera, n=None, sigma_px=(10.0, 80.0), seed=4, opacity=None):
    """`n` Gaussians (default max(60, P / 20)) at camera z in (0.2, 0.4] over the frame with on-screen sigma in `sigma_px`,
    then the ulp group (see _ulp_group) with small extents.  info: "band" (the first), "ulp" (the second), "ulp_k" (each one's
    offset in ulps from 0.2f)."""
    rng = np.random.default_rng(seed)
    n = max(60, s.P // 20) if n is None else n
    ulp_pts, ulp_z = _ulp_group(cam, s, rng)
    ulp_k = np.rint((ulp_z.astype(np.float64) - float(NEAR)) / float(np.spacing(NEAR))).astype(np.int64)
    m = len(ulp_pts)
    idx = np.sort(rng.choice(s.P, n + m, replace=False))
    perm = rng.permutation(n + m)
    band, ulp = np.sort(idx[perm[:n]]), idx[perm[n:]]
    z = 0.2 + rng.uniform(0.0, 0.2, n) + 1e-4    # (0.2, 0.4]
    u = rng.uniform(0.0, 1.0, n) * cam.W - 0.5
    v = rng.uniform(0.0, 1.0, n) * cam.H - 0.5
    means = s.means.copy()
    means[band] = cam.to_world(np.stack([(u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z], 1)).astype(np.float32)
    means[ulp] = ulp_pts
    sig = np.exp(rng.uniform(np.log(sigma_px[0]), np.log(sigma_px[1]), n))
    scales = s.scales.copy()
    scales[band] = (sig[:, None] * rng.uniform(0.9, 1.1, (n, 3)) / cam.fx * z[:, None]).astype(np.float32)
    scales[ulp] = (rng.uniform(2.0, 6.0, (m, 3)) / cam.fx * float(NEAR)).astype(np.float32)
    return s._replace(means=means, scales=scales, opac=_band_opacity(s, band, opacity, rng)), dict(band=band, ulp=ulp, ulp_k=ulp_k)


def assert_near_edge(s: Scene, info, visible, radii=None, least=20):
    """The band sits in (0.2, 0.4] in float32; the ulp group's float32 z straddles 0.2f (0.2f itself and both neighbours
    where the float32 grid of the sum reaches them: everywhere but at the `far` camera, whose world coordinates of ~30 leave
    a coarser grid) and `visible` ([P] bool, the oracle's mark_visible) is exactly z32 > 0.2f on it -- the float32 order of
    evaluation, not the float64 position, decides.  `radii` (the oracle's): at least `least` of the band rendered."""
    z32 = camera_z32(s)
    zb = z32[info["band"]]
    assert np.all((zb > NEAR) & (zb <= np.float32(0.4) + np.float32(1e-3))), (zb.min(), zb.max())
    zu = z32[info["ulp"]]
    assert (zu <= NEAR).any() and (zu > NEAR).any(), "the ulp group does not straddle the near plane"
    ks = set(int(k) for k in info["ulp_k"])
    near_origin = float(np.abs(camera_t64(s)[info["ulp"], :3]).max()) < 2.0 and float(np.abs(s.campos).max()) < 2.0
    if near_origin:  # (the float32 grid of the sum is as fine as 0.2f's own)
        assert ks == set(range(-4, 5)), ks
    vis = np.asarray(visible).reshape(-1)
    assert np.array_equal(vis[info["ulp"]], zu > NEAR)
    if radii is not None:
        shown = int((np.asarray(radii).reshape(-1)[info["band"]] > 0).sum())
        assert shown >= least, f"only {shown} near-plane Gaussians rendered"
    return ks


PLACEMENTS = ("plain", "clamp", "near")


def placed(cam: Camera, P, placement, seed=0, **kw):
    """(scene, info) of `cam` with `placement` applied ("plain": none); `kw` goes to the placement."""
    s = scene(cam, P, seed)
    if placement == "clamp":
        return clamp_scene(s, cam, **kw)
    if placement == "near":
        return near_scene(s, cam, **kw)
    return s, {}


# ------------------------------------------------------------------------------------------ cases of the float64 model's tests
# (camera, placement, P, W, SH degree, seed): off-centre principal points, fx != fy, the Jacobian clamp and the near plane, where
# the reference's shortened pose Jacobian and the exact one part.  (The placements' bands are sized to these small frames: a
# hundred Gaussians of sigma 20 .. 150 px stacked on every pixel of a 64 x 48 frame leave the float32 backward's transmittance,
# re-derived by division, at 5e-4 of scale from float64 -- in dL_dopacity as much as anywhere, a property of the reference's
# algorithm, not of the camera.)
CAMERA_CASES = [("tum", "plain", 400, 64, 3, 21), ("skewed_pp", "plain", 400, 64, 2, 22),
                ("skewed_pp", "clamp", 500, 96, 3, 23, dict(n=70, sigma_px=(12.0, 40.0), opacity=(0.05, 0.25))),
                ("tum", "near", 300, 48, 1, 24, dict(n=30, sigma_px=(4.0, 16.0), opacity=(0.05, 0.25)))]


def camera_case_id(case):
    return f"{case[0]}-{case[1]}"


def camera_case_scene(case):
    """(scene, SH degree, placement info) of a CAMERA_CASES entry; the placement's edge is asserted by the caller."""
    cid, placement, P, W, deg, seed = case[:6]
    s, info = placed(CAMERAS[cid].at(W), P, placement, seed, **(case[6] if len(case) > 6 else {}))
    return s, deg, info


def assert_placement_edge(oracle, placement, s, info, radii):
    if placement == "clamp":
        assert_clamp_edge(s, info, radii)
    elif placement == "near":
        assert_near_edge(s, info, oracle.mark_visible(s.means, s.view, s.proj), radii, least=10)
