"""Hybrid RGB-D alignment as include/dgr_hip.h defines it (dgr_intensity_map, dgr_frame_halve, dgr_rgbd_step) and slam.rgbd_align,
restated in float64 numpy on the CPU.  Written from that text, on top of the ICP model (tests/icp_model.py), whose geometric pair
the hybrid step takes over unchanged.  Beside each result it returns what a comparison with an fp32 kernel needs, in icp_model's
style: ambiguity marks and per-term rounding bounds, u = 2^-24 per rounding, counted on csrc/icp.hip as if no multiply-add were
fused (fusing removes roundings):
  I      = (c_r R + c_g G) + c_b B           3 products, 2 additions: 3 u (|c_r R| + |c_g G| + |c_b B|); the constants are the fp32
                                             ones in kernel and model alike; a single channel is exact
  I_x    = (((a - b) + (c - d)) + 2 (e - f)) / 8   the six intensities' own errors (weights 1, 1, 1, 1, 2, 2), one rounding per
                                             difference and two for the additions: 3 u (|a - b| + |c - d| + 2 |e - f|); the
                                             doubling and the division by 8 are exact.  I_y alike
  u - px = the landing position against its pixel: icp_model's error of u (du) + u |u - px| for the subtraction
  r_p    = ((I_m + I_x dx) + I_y dy) - I_obs  |I_x| ddx + |I_y| ddy + 4 u (|I_m| + |I_x dx| + |I_y dy| + |I_obs|): the
                                             cancellation in I_m - I_obs is bounded on the intensities, not on |r_p|
  g_x    = (I_x fx) / q_z                    2 roundings and q_z's error: |g_x| (dq_z / |q_z| + 2 u); g_y alike
  g_z    = -((g_x q_x + g_y q_y) / q_z)      dg_x |q_x| + |g_x| dq_x + (y alike) + 3 u (|g_x q_x| + |g_y q_y|), over |q_z|, and
                                             |g_z| (dq_z / |q_z| + u)
  J_rot  = q x g                             per entry |g_b| dq_a + |q_a| dg_b + |g_a| dq_b + |q_b| dg_a + 2 u (|q_a g_b| + |q_b g_a|);
                                             J_trans = g carries dg
  w_p    = Huber's weight: icp_model's rule
  s      = class weight * w                  one more rounding on every term of A and b unless the class weight is 1
The landing-pixel-edge case is icp_model's: a candidate within its error of a pixel's edge may read the neighbouring model pixel,
and its bound covers the change of every term among the neighbours in question.  The intensity map's usable flag is decided by
raw comparisons (finite, mask > threshold) and is never ambiguous."""
import json
import os

import numpy as np

import icp_model as M

U, INF = M.U, M.INF
PHOTOMETRIC = 8
C_R, C_G, C_B = (float(np.float32(c)) for c in (0.299, 0.587, 0.114))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rgbd_pyramid_640x480.json")


# -------------------------------------------------------------------------------------------------------------------- scenes
def smooth_albedo(X, Y):
    """the textured plane of the 96 x 80 case: periods of many pixels at every size the tests use"""
    return 0.5 + 0.2 * np.sin(1.7 * X + 0.3) * np.cos(1.3 * Y - 0.2) + 0.15 * np.sin(0.9 * X - 1.1 * Y)


def pyramid_albedo(X, Y):
    """the pyramid case's: smooth terms and a fine one whose period is a few pixels at 640 x 480"""
    return (0.5 + 0.1 * np.sin(5 * X + 0.3) * np.cos(4 * Y - 0.2) + 0.08 * np.sin(2.3 * X - 3.1 * Y) +
            0.25 * np.sin(60 * X + 0.4) * np.sin(52 * Y + 1.0))


TEXTURED_TWIST = np.array([0.004, -0.003, 0.02, 0.02, -0.015, 0.01])
PYRAMID_TWIST = np.array([0.004, -0.003, 0.03, 0.03, -0.02, 0.01])


def render_plane(W, H, fx, fy, cx, cy, view, albedo, depth=2.0):
    """(depth [H,W], intensity [H,W], both float32) of the world plane z = `depth` textured by albedo(X, Y), seen from `view`
    (W2C^T, fp32): ray-plane intersection in float64"""
    R, t = M.pose_of(view)
    centre = -R.T @ t
    fx, fy, cx, cy = (M.f32(v) for v in (fx, fy, cx, cy))
    y, x = np.mgrid[0:H, 0:W]
    rays = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones((H, W))], -1) @ R
    s = (depth - centre[2]) / rays[..., 2]
    P = centre + s[..., None] * rays
    return s.astype(np.float32), albedo(P[..., 0], P[..., 1]).astype(np.float32)


def textured_plane_scene(W, H, twist=TEXTURED_TWIST, albedo=smooth_albedo, depth=2.0, intrinsics=None):
    """icp_model's fronto-parallel plane with a texture: the model camera is the identity, the current frame's true pose is the
    model's moved by `twist`.  Point-to-plane ICP has exactly zero rows for omega_z, v_x, v_y here."""
    fx, fy, cx, cy = M.intrinsics(W, H) if intrinsics is None else intrinsics
    eye = np.eye(4, dtype=np.float32)
    Re, te = M.se3_exp(twist)
    true_view = M.w2ct(Re, te)
    md, mi = render_plane(W, H, fx, fy, cx, cy, eye, albedo, depth)
    od, oi = render_plane(W, H, fx, fy, cx, cy, true_view, albedo, depth)
    return dict(W=W, H=H, fx=fx, fy=fy, cx=cx, cy=cy, model_view=eye, true_view=true_view, model_depth=md, depth_obs=od,
                model_color=mi[None], color_obs=oi[None])


def pyramid_scene():
    """the issue's pyramid case: 640 x 480, fx = fy = 525, the principal point at the image centre"""
    return textured_plane_scene(640, 480, PYRAMID_TWIST, pyramid_albedo, intrinsics=(525.0, 525.0, 319.5, 239.5))


def level_intrinsics(fx, fy, cx, cy, level=1):
    """pixel centres sit at integers: fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2 per level (float64; rounded once on use)"""
    for _ in range(level):
        fx, fy, cx, cy = 0.5 * fx, 0.5 * fy, 0.5 * (cx - 0.5), 0.5 * (cy - 0.5)
    return float(fx), float(fy), float(cx), float(cy)


# ------------------------------------------------------------------------------------------------------------ intensity map
def intensity_of(image):
    """image [C,H,W] or [H,W] float32 -> (I float64 [H,W], its bound)"""
    image = np.asarray(image, np.float32).astype(np.float64)
    if image.ndim == 2:
        image = image[None]
    if image.shape[0] == 1:
        return image[0], np.zeros(image.shape[1:])
    with np.errstate(invalid="ignore", over="ignore"):
        parts = [C_R * image[0], C_G * image[1], C_B * image[2]]
        return (parts[0] + parts[1]) + parts[2], 3 * U * (np.abs(parts[0]) + np.abs(parts[1]) + np.abs(parts[2]))


def intensity_map_model(image, *, mask_image=None, mask_threshold=0.99, mutate=None):
    """Returns a dict: imap float64 [H,W,4] (zeros where unusable), usable bool [H,W], ambiguous bool [H,W] (never set: see the
    module's text), bound float64 [H,W,3] on (I, I_x, I_y) at a usable pixel, intensity float64 [H,W] with its bound dI.
    `mutate`: "swap_axes" (the Sobel axes exchanged)."""
    I, dI = intensity_of(image)
    H, W = I.shape
    imap, bound = np.zeros((H, W, 4)), np.zeros((H, W, 3))
    usable = np.zeros((H, W), bool)
    out = dict(imap=imap, usable=usable, ambiguous=np.zeros((H, W), bool), bound=bound, intensity=I, dI=dI)
    if H < 3 or W < 3:
        return out
    fin = np.isfinite(I)
    good = fin.copy()
    if mask_image is not None:
        with np.errstate(invalid="ignore"):
            good &= np.asarray(mask_image, np.float32).reshape(H, W) > np.float32(mask_threshold)
    ok = np.ones((H - 2, W - 2), bool)
    sh = lambda a, dy, dx: a[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]  # noqa: E731
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ok &= sh(good, dy, dx)
    Z, dZ = np.where(fin, I, 0.0), np.where(fin, dI, 0.0)

    def sobel(step):  # step = (dy, dx) of the axis differentiated along; the other axis carries the weights 1, 2, 1
        ay, ax = step
        py, px = ax, ay  # the perpendicular axis
        d = [sh(Z, ay + k * py, ax + k * px) - sh(Z, -ay + k * py, -ax + k * px) for k in (-1, 1, 0)]
        e = [sh(dZ, ay + k * py, ax + k * px) + sh(dZ, -ay + k * py, -ax + k * px) for k in (-1, 1, 0)]
        mags = np.abs(d[0]) + np.abs(d[1]) + 2 * np.abs(d[2])
        return ((d[0] + d[1]) + 2 * d[2]) * 0.125, 0.125 * (e[0] + e[1] + 2 * e[2] + 3 * U * mags)

    gx, dgx = sobel((0, 1))
    gy, dgy = sobel((1, 0))
    if mutate == "swap_axes":
        gx, gy = gy, gx
    c = (slice(1, -1), slice(1, -1))
    usable[c] = ok
    imap[c] = np.where(ok[..., None], np.stack([sh(Z, 0, 0), gx, gy, np.ones_like(gx)], -1), 0.0)
    bound[c] = np.where(ok[..., None], np.stack([sh(dZ, 0, 0), dgx, dgy], -1), 0.0)
    return out


# -------------------------------------------------------------------------------------------------------------------- halve
def halve_model(planes=None, depth=None, *, depth_range=(0.0, INF), max_jump=0.1):
    """planes [N,H,W], depth [H,W] float32.  Returns a dict: planes float32 [N,H//2,W//2] (every operation in fp32, in the
    header's association: the kernel's bits), depth float32 [H//2,W//2], ambiguous bool [H//2,W//2] (the jump test decided
    within its rounding)."""
    out = dict(planes=None, depth=None, ambiguous=None)

    def blocks_of(a):  # the four pixels of every 2 x 2 block; an odd last row or column is dropped
        H2, W2 = a.shape[-2] // 2, a.shape[-1] // 2
        a = a[..., :2 * H2, :2 * W2]
        return a[..., 0::2, 0::2], a[..., 0::2, 1::2], a[..., 1::2, 0::2], a[..., 1::2, 1::2]

    if planes is not None:
        a, b, c, d = blocks_of(np.asarray(planes, np.float32))
        with np.errstate(invalid="ignore", over="ignore"):
            out["planes"] = ((a + b) + (c + d)) * np.float32(0.25)
    if depth is not None:
        ds = blocks_of(np.asarray(depth, np.float32))
        lo, hi, mj = np.float32(depth_range[0]), np.float32(depth_range[1]), np.float32(max_jump)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            oks = [(d > lo) & (d < hi) for d in ds]
            v = [np.where(ok, d, np.float32(0.0)) for ok, d in zip(oks, ds)]
            n = sum(ok.astype(np.float32) for ok in oks)
            small = np.minimum.reduce([np.where(ok, d, np.float32(np.inf)) for ok, d in zip(oks, ds)])
            large = np.maximum.reduce([np.where(ok, d, np.float32(-np.inf)) for ok, d in zip(oks, ds)])
            spread, lim = (large - small).astype(np.float64), mj.astype(np.float64) * small.astype(np.float64)
            keep = (n > 0) & ((large - small) <= mj * small)
            mean = ((v[0] + v[1]) + (v[2] + v[3])) / np.maximum(n, np.float32(1.0))
            out["depth"] = np.where(keep, mean, np.float32(0.0)).astype(np.float32)
            out["ambiguous"] = (n > 0) & (np.abs(spread - lim) <= 2 * U * (np.abs(large) + np.abs(small) + np.abs(lim)))
    return out


# --------------------------------------------------------------------------------------------------------------------- step
def photo_gradient(Ix, Iy, fx, fy, qx, qy, qz):
    """g, the gradient of the model's intensity at the landing position with respect to the camera point q"""
    g0, g1 = Ix * fx / qz, Iy * fy / qz
    return g0, g1, -((g0 * qx + g1 * qy) / qz)


def photo_jacobian(Ix, Iy, fx, fy, q):
    """J_p = (q x g, g) [.., 6] of the photometric residual under q' = exp(xi) q"""
    g = np.stack(photo_gradient(Ix, Iy, fx, fy, q[..., 0], q[..., 1], q[..., 2]), -1)
    return np.concatenate([np.cross(q, g), g], -1)


def rgbd_step_model(depth_obs, vn_obs, vn_model, intensity_obs, imap_model, model_view, view_in, fx, fy, cx, cy, *, stride=1,
                    depth_range=(0.0, INF), dist_max=0.1, normal_cos_min=0.8, huber_delta=INF, geo_weight=1.0, photo_weight=1.0,
                    photo_max=INF, photo_huber=INF, mutate=None):
    """The arrays the kernel is given (float32).  Returns a dict: flags uint8 [S] (icp_model's bits and PHOTOMETRIC), ambiguous
    bool [S], geometric and photometric bool [S] (the model's own pairs), valid, S, and `sums(geometric, photometric)`: the 31
    sums of the header's stats, their bounds B [31] and sum |term| [31] over any two sets of pairs (None: the model's own).
    `mutate`: "gz_sign", "no_subpixel", "weight_on_A_only", "swap_axes" -- deliberately wrong models."""
    geo = M.icp_step_model(depth_obs, vn_obs, vn_model, model_view, view_in, fx, fy, cx, cy, stride=stride, depth_range=depth_range,
                           dist_max=dist_max, normal_cos_min=normal_cos_min, huber_delta=huber_delta)
    depth_obs, vn_model = np.asarray(depth_obs, np.float32), np.asarray(vn_model, np.float32)
    imap_model, intensity_obs = np.asarray(imap_model, np.float32), np.asarray(intensity_obs, np.float32)
    H, W = depth_obs.shape
    intensity_obs = intensity_obs.reshape(H, W)
    gw, pw, pmax, pdelta = (M.f32(v) for v in (geo_weight, photo_weight, photo_max, photo_huber))
    fx, fy, cx, cy, dmax = (M.f32(v) for v in (fx, fy, cx, cy, dist_max))
    ifx, ify = M.f32(1.0 / fx), M.f32(1.0 / fy)
    x, y = M.candidates(W, H, stride)
    S = len(x)
    valid = (geo["flags"] & M.VALID) != 0
    d = np.where(valid, depth_obs[y, x], 1.0).astype(np.float64)
    io32 = intensity_obs[y, x]
    io_ok = np.isfinite(io32)
    io = np.where(io_ok, io32, 0.0).astype(np.float64)
    # the geometry of icp_model's step, restated: q, the landing position and the pixels in question
    R, t = M.relative_transform(model_view, view_in)
    p = np.stack([(x - cx) * ifx * d, (y - cy) * ify * d, d], 1)
    q = p @ R.T + t
    dq = 8 * U * (np.abs(p) @ np.abs(R).T + np.abs(t))
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = fx * q[:, 0] / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy
        du = fx / np.abs(q[:, 2]) * (dq[:, 0] + np.abs(q[:, 0] / q[:, 2]) * dq[:, 2]) + 4 * U * (np.abs(u - cx) + abs(cx) + 0.5)
        dv = fy / np.abs(q[:, 2]) * (dq[:, 1] + np.abs(q[:, 1] / q[:, 2]) * dq[:, 2]) + 4 * U * (np.abs(v - cy) + abs(cy) + 0.5)
    ok_uv = valid & (q[:, 2] > 0.0) & np.isfinite(u) & np.isfinite(v)
    u, v = np.where(ok_uv, u, 0.0), np.where(ok_uv, v, 0.0)
    du, dv = np.where(ok_uv, du, 0.0), np.where(ok_uv, dv, 0.0)
    qz = np.where(ok_uv, q[:, 2], 1.0)
    uh, vh = u + 0.5, v + 0.5
    px, py = np.floor(uh), np.floor(vh)
    near_x, near_y = ok_uv & (np.abs(uh - np.rint(uh)) <= du), ok_uv & (np.abs(vh - np.rint(vh)) <= dv)
    px_alt, py_alt = np.where(uh - px < 0.5, px - 1, px + 1), np.where(vh - py < 0.5, py - 1, py + 1)

    def pair(px, py):
        in_image = ok_uv & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        iy, ix = np.clip(py, 0, H - 1).astype(np.int64), np.clip(px, 0, W - 1).astype(np.int64)
        m32, im32 = vn_model[iy, ix], imap_model[iy, ix]
        with np.errstate(invalid="ignore"):
            inside = in_image & (m32[:, 3] > 0)
        dm = np.where(inside, m32[:, 3], 0.0).astype(np.float64)
        vm = np.stack([(px - cx) * ifx * dm, (py - cy) * ify * dm, dm], 1)
        e = q - vm
        de = dq + 4 * U * np.abs(vm) * np.array([1.0, 1.0, 0.0]) + U * np.abs(e)
        dist = np.linalg.norm(e, axis=1)
        close = inside & (dist <= dmax)
        amb = inside & (np.abs(dist - dmax) <= np.linalg.norm(de, axis=1) + 3 * U * dist)
        have = inside & (im32[:, 3] == 1) & io_ok  # (wider than the pair: a distance decided the other way still has its terms)
        lit = have & close
        im = np.where(have[:, None], im32, 0.0).astype(np.float64)
        Im, Ix, Iy = im[:, 0], im[:, 1], im[:, 2]
        if mutate == "swap_axes":
            Ix, Iy = Iy, Ix
        dx, dy = u - px, v - py
        ddx, ddy = du + U * np.abs(dx), dv + U * np.abs(dy)
        if mutate == "no_subpixel":
            dx, dy = np.zeros(S), np.zeros(S)
        r = ((Im + Ix * dx) + Iy * dy) - io
        dr = np.abs(Ix) * ddx + np.abs(Iy) * ddy + 4 * U * (np.abs(Im) + np.abs(Ix * dx) + np.abs(Iy * dy) + np.abs(io))
        ar = np.abs(r)
        photometric = lit & (ar <= pmax)
        amb |= lit & (np.abs(ar - pmax) <= dr)
        g0, g1, g2 = photo_gradient(Ix, Iy, fx, fy, q[:, 0], q[:, 1], qz)
        dg0, dg1 = np.abs(g0) * (dq[:, 2] / np.abs(qz) + 2 * U), np.abs(g1) * (dq[:, 2] / np.abs(qz) + 2 * U)
        aq = np.abs(q)
        dg2 = ((dg0 * aq[:, 0] + np.abs(g0) * dq[:, 0] + dg1 * aq[:, 1] + np.abs(g1) * dq[:, 1] +
                3 * U * (np.abs(g0 * q[:, 0]) + np.abs(g1 * q[:, 1]))) / np.abs(qz) + np.abs(g2) * (dq[:, 2] / np.abs(qz) + U))
        if mutate == "gz_sign":
            g2 = -g2
        g, dg = np.stack([g0, g1, g2], 1), np.stack([dg0, dg1, dg2], 1)
        ag = np.abs(g)
        Jr = np.cross(q, g)

        def cross_bound(a, b):  # entry q_a g_b - q_b g_a
            return (ag[:, b] * dq[:, a] + aq[:, a] * dg[:, b] + ag[:, a] * dq[:, b] + aq[:, b] * dg[:, a] +
                    2 * U * (aq[:, a] * ag[:, b] + aq[:, b] * ag[:, a]))

        dJr = np.stack([cross_bound(1, 2), cross_bound(2, 0), cross_bound(0, 1)], 1)
        J, dJ = np.concatenate([Jr, g], 1), np.concatenate([dJr, dg], 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(ar <= pdelta, 1.0, pdelta / ar)
            dw = np.where((ar >= pdelta - dr) & (ar > 0), np.minimum(w, 1.0) * (dr / ar + U), 0.0)
        terms, bounds = M._terms(J, dJ, r, dr, w, dw)
        keep = have[:, None]
        residual.setdefault("r_p", np.where(have, r, 0.0))  # (the first call's: the model's own pixel)
        return have, photometric, amb, np.where(keep, terms, 0.0), np.where(keep, bounds, 0.0)

    residual = {}
    lit, photometric, amb, terms, bounds = pair(px, py)
    for near, ax, ay in ((near_x, px_alt, py), (near_y, px, py_alt), (near_x & near_y, px_alt, py_alt)):
        if near.any():
            lit2, _, _, t2, b2 = pair(np.where(near, ax, px), np.where(near, ay, py))
            use = near & lit2
            swap = use & ~lit
            change = np.where((use & lit)[:, None], np.abs(t2 - terms) + b2, 0.0)
            terms = np.where(swap[:, None], t2, terms)
            bounds = np.where(swap[:, None], b2, np.maximum(bounds, change + np.where(use[:, None], bounds, 0.0)))
    ambiguous = geo["ambiguous"] | (valid & (near_x | near_y | amb))
    flags = (geo["flags"] + photometric * PHOTOMETRIC).astype(np.uint8)
    geometric = geo["associated"]
    scale_g = np.full(28, gw)
    scale_p = np.full(28, pw)
    scale_g[27] = scale_p[27] = 1.0  # sum w r^2 is kept unscaled
    if mutate == "weight_on_A_only":
        scale_p[21:27] = 1.0
    extra_g, extra_p = (0.0 if gw == 1.0 else U), (0.0 if pw == 1.0 else U)  # s = class weight * w: one more rounding

    def sums(geometric_set=None, photometric_set=None):
        """(the 31 sums, B [31], sum |term| [31])"""
        sg = (geometric if geometric_set is None else np.asarray(geometric_set, bool)) & (gw > 0)
        sp = (photometric if photometric_set is None else np.asarray(photometric_set, bool)) & (pw > 0)
        tg, tp = geo["terms"][sg] * scale_g, terms[sp] * scale_p
        bg = (geo["bounds"][sg] + extra_g * np.abs(geo["terms"][sg])) * scale_g
        bp = (bounds[sp] + extra_p * np.abs(terms[sp])) * scale_p
        S31, B, mag = np.zeros(31), np.zeros(31), np.zeros(31)
        S31[:27], B[:27], mag[:27] = (tg.sum(0) + tp.sum(0))[:27], (bg.sum(0) + bp.sum(0))[:27], (np.abs(tg).sum(0) + np.abs(tp).sum(0))[:27]
        S31[27], B[27], mag[27] = tg.sum(0)[27], bg.sum(0)[27], np.abs(tg).sum(0)[27]
        S31[29], B[29], mag[29] = tp.sum(0)[27], bp.sum(0)[27], np.abs(tp).sum(0)[27]
        S31[28], S31[30] = float(sg.sum()), float(sp.sum())
        return S31, B, mag

    return dict(flags=flags, ambiguous=ambiguous, geometric=geometric, photometric=photometric, S=S, valid=int(valid.sum()),
                sums=sums, photo_terms=terms, r_p=residual["r_p"], u=u, v=v)


def as_icp_sums(sums31):
    """the 29 sums icp_model.solve_update takes, of the hybrid step's 31: A, b, the two residual sums together (all that the
    solve asks of them is that they are finite), count_g + count_p"""
    s = np.asarray(sums31, np.float64)
    return np.concatenate([s[:27], [s[27] + s[29], s[28] + s[30]]])


def solve_update(sums31, model_view, view_in, **kw):
    return M.solve_update(as_icp_sums(sums31), model_view, view_in, **kw)


# -------------------------------------------------------------------------------------------------------------------- align
def rgbd_align_model(color_obs, depth_obs, model_color, model_depth, viewmatrix, model_viewmatrix, fx, fy, cx, cy, *, levels=1,
                     iterations=10, strides=None, opacity_map=None, silhouette_threshold=0.99, geo_weight=1.0, photo_weight=1.0,
                     photo_max=INF, photo_huber=INF, depth_range=(0.0, INF), max_jump=0.1, dist_max=0.1, normal_cos_min=0.8,
                     use_obs_normals=True, huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6, stop_after=None):
    """slam.rgbd_align in float64 (every image and map rounded to fp32 where the kernels store one).  Returns a dict: viewmatrix,
    quat, trans, and per iteration in the order they run: level, ok, count_g, count_p, marked.  `stop_after`: run only the first
    so many iterations."""
    per_level = (iterations,) * levels if isinstance(iterations, int) else tuple(iterations)
    order = [level for level, k in zip(range(levels - 1, -1, -1), per_level) for _ in range(k)]
    strides = (1,) * len(order) if strides is None else tuple(strides)
    f32 = lambda a: None if a is None else np.asarray(a, np.float32)  # noqa: E731
    frames = [dict(obs=intensity_of(color_obs)[0].astype(np.float32), model=intensity_of(model_color)[0].astype(np.float32),
                   depth_obs=f32(depth_obs).reshape(np.shape(depth_obs)[-2:]), depth_model=f32(model_depth).reshape(np.shape(model_depth)[-2:]),
                   mask=None if opacity_map is None else f32(opacity_map).reshape(np.shape(opacity_map)[-2:]))]
    frames[0]["imap"] = intensity_map_model(model_color, mask_image=frames[0]["mask"], mask_threshold=silhouette_threshold)["imap"]
    for level in range(1, levels):
        b = frames[-1]
        ho = halve_model(b["obs"][None], b["depth_obs"], depth_range=depth_range, max_jump=max_jump)
        planes = np.stack([b["model"]] + ([b["mask"]] if b["mask"] is not None else []))
        hm = halve_model(planes, b["depth_model"], depth_range=depth_range, max_jump=max_jump)
        f = dict(obs=ho["planes"][0], depth_obs=ho["depth"], model=hm["planes"][0], depth_model=hm["depth"],
                 mask=hm["planes"][1] if b["mask"] is not None else None)
        f["imap"] = intensity_map_model(f["model"], mask_image=f["mask"], mask_threshold=silhouette_threshold)["imap"]
        frames.append(f)
    view = np.asarray(model_viewmatrix if viewmatrix is None else viewmatrix, np.float32).reshape(4, 4)
    rows, out, maps_of = [], None, {}
    for k, (level, stride) in enumerate(zip(order, strides)):
        if stop_after is not None and k >= stop_after:
            break
        f, intr = frames[level], level_intrinsics(float(fx), float(fy), float(cx), float(cy), level)
        if level not in maps_of:
            kw = dict(depth_range=depth_range, max_jump=max_jump)
            vm = M.depth_normals_model(f["depth_model"], *intr, mask_image=f["mask"], mask_threshold=silhouette_threshold, **kw)
            vo = M.depth_normals_model(f["depth_obs"], *intr, **kw)["vnmap"].astype(np.float32) if use_obs_normals else None
            maps_of[level] = (vm["vnmap"].astype(np.float32), vo, f["imap"].astype(np.float32))
        vn_model, vn_obs, imap = maps_of[level]
        m = rgbd_step_model(f["depth_obs"], vn_obs, vn_model, f["obs"], imap, model_viewmatrix, view, *intr, stride=stride,
                            depth_range=depth_range, dist_max=dist_max, normal_cos_min=normal_cos_min, huber_delta=huber_delta,
                            geo_weight=geo_weight, photo_weight=photo_weight, photo_max=photo_max, photo_huber=photo_huber)
        s31, _, _ = m["sums"]()
        out = solve_update(s31, model_viewmatrix, view, damping=damping, rcond=rcond, min_points=min_points)
        view = out["viewmatrix"]
        rows.append(dict(level=level, ok=bool(out["ok"]), count_g=int(s31[28]), count_p=int(s31[30]), marked=int(m["ambiguous"].sum())))
    return dict(viewmatrix=view, quat=out["quat"], trans=out["trans"], rows=rows, frames=frames)


# ------------------------------------------------------------------------------------------------------------------- golden
PYRAMID_RUNS = {"one_level": dict(levels=1, iterations=6), "five_levels": dict(levels=5, iterations=6)}


def pyramid_model(run, stop_after=None):
    s = pyramid_scene()
    return s, rgbd_align_model(s["color_obs"], s["depth_obs"], s["model_color"], s["model_depth"], None, s["model_view"], s["fx"],
                               s["fy"], s["cx"], s["cy"], stop_after=stop_after, **PYRAMID_RUNS[run])


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":  # records what the model gives on the pyramid case (a minute of numpy): python tests/rgbd_model.py
    record = {}
    for run in PYRAMID_RUNS:
        s, out = pyramid_model(run)
        err = M.pose_error(out["viewmatrix"], s["true_view"])
        record[run] = dict(pose_error=list(err), viewmatrix=[float(v) for v in out["viewmatrix"].reshape(-1)], rows=out["rows"])
        print(run, err)
    with open(GOLDEN, "w") as f:
        json.dump(record, f, indent=1)
