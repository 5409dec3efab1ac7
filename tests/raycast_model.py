"""A numpy model of the ray-cast of the TSDF volume (include/dgr_hip.h: dgr_tsdf_bricks, dgr_tsdf_raycast) that shares no code with
the kernels: `raycast` is the header's rule in float64 from the same float32 inputs, vectorised over rays, EVERY sample of a ray
evaluated (no box clipping beyond "outside the lattice is invalid", no skipping), with the mask of the pixels that sit next to a
decision; `raycast32` the same arithmetic in float32 (it only sizes the tolerance); `bricks` the brick rule, cell by cell.
Scenes, poses and volumes come from tests/tsdf_model.py.

`ambiguous` (a pixel float32 cannot be held to): every sample up to the decisive one is evaluated at its position and at the
eight positions EPS_Q lattice units away along the diagonals (which reach every neighbouring cell a rounding of the position can
reach).  A pixel is ambiguous when
 * a sample before k* could be decisive at one of the nine positions (valid, F <= EPS_F), or any sample of a miss could;
 * sample k* is not decisive at all nine (valid, F <= -EPS_F): |F| within EPS_F of 0, or a cell face within EPS_Q across which
   validity differs;
 * sample k* - 1 of a hit is not valid with F >= EPS_F at all nine, or that of an unseen end could be valid with F > -EPS_F at one;
 * a sample within EPS_Z of depth_max could be decisive;
 * one of the six evaluations of a hit's normal changes its validity among the nine positions, or the gradient is below EPS_G.
A weight within EPS_W of min_weight would make a pixel ambiguous too, but EPS_W is 0: the weights are inputs, not results -- the
kernel and the model compare the same float32 numbers, so that test is exact and no pixel is excused for it."""
import numpy as np

import tsdf_model as T

EPS_Q, EPS_F, EPS_W, EPS_Z, EPS_G = 1e-4, 2e-5, 0.0, 1e-5, 1e-4
INF = float("inf")
HIT, UNSEEN, NO_NORMAL = 1, 2, 4
SHIFTS = np.array([[0, 0, 0]] + [[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64) * EPS_Q


def _sample(dtype, volume, q, min_weight, slack=0.0):
    """the validity-checked trilinear interpolant at lattice coordinates q [..., 3] -> (valid, F); `slack` loosens (> 0) or
    tightens (< 0) the weight test"""
    nz, ny, nx = volume.shape[:3]
    n = np.array([nx, ny, nz])
    with np.errstate(all="ignore"):
        fl = np.floor(q)
        inside = np.all((fl >= 0) & (fl <= n - 2), axis=-1)
        i = np.where(inside[..., None], fl, 0).astype(np.int64)
        f = (q - fl).astype(dtype)
        valid = inside.copy()
        c = {}
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    ix, iy, iz = np.minimum(i[..., 0] + dx, nx - 1), np.minimum(i[..., 1] + dy, ny - 1), np.minimum(i[..., 2] + dz, nz - 1)
                    tw = volume[iz, iy, ix]
                    valid &= tw[..., 1].astype(np.float64) >= np.float64(np.float32(min_weight)) - slack
                    c[dx, dy, dz] = tw[..., 0].astype(dtype)
        lerp = lambda t, a, b: a + t * (b - a)
        x = {(dy, dz): lerp(f[..., 0], c[0, dy, dz], c[1, dy, dz]) for dy in (0, 1) for dz in (0, 1)}
        F = lerp(f[..., 2], lerp(f[..., 1], x[0, 0], x[1, 0]), lerp(f[..., 1], x[0, 1], x[1, 1]))
    return valid, F


def _color(dtype, color_volume, q):
    nz, ny, nx = color_volume.shape[:3]
    n = np.array([nx, ny, nz])
    with np.errstate(all="ignore"):
        fl = np.clip(np.nan_to_num(np.floor(q), nan=0.0), 0, np.maximum(n - 2, 0))
        i, f = fl.astype(np.int64), (q - fl).astype(dtype)
        lerp = lambda t, a, b: a + t * (b - a)
        c = {(dx, dy, dz): color_volume[np.minimum(i[..., 2] + dz, nz - 1), np.minimum(i[..., 1] + dy, ny - 1),
                                        np.minimum(i[..., 0] + dx, nx - 1), :3].astype(dtype)
             for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
        x = {(dy, dz): lerp(f[..., 0:1], c[0, dy, dz], c[1, dy, dz]) for dy in (0, 1) for dz in (0, 1)}
        return lerp(f[..., 2:3], lerp(f[..., 1:2], x[0, 0], x[1, 0]), lerp(f[..., 1:2], x[0, 1], x[1, 1]))


def _raycast(dtype, volume, color_volume, origin, voxel, views, fx, fy, cx, cy, H, W, depth_range, step, min_weight, with_ambiguous):
    f = dtype
    nz, ny, nx = volume.shape[:3]
    n = np.array([nx, ny, nz])
    views = np.asarray(views, dtype=np.float32).reshape(-1, 4, 4)
    V = views.shape[0]
    o, h = np.array([f(np.float32(v)) for v in origin], dtype=f), f(np.float32(voxel))
    fx, fy, cx, cy, step = (f(np.float32(v)) for v in (fx, fy, cx, cy, voxel / 2 if step is None else step))
    dmin, dmax = f(np.float32(depth_range[0])), f(np.float32(depth_range[1]))
    ys, xs = np.mgrid[0:H, 0:W]
    dc = np.stack([(xs.astype(f) - cx) / fx, (ys.astype(f) - cy) / fy, np.ones((H, W), dtype=f)], axis=-1)  # [H, W, 3]
    depth, vnmap = np.zeros((V, H, W), dtype=f), np.zeros((V, H, W, 4), dtype=f)
    color = None if color_volume is None else np.zeros((V, 3, H, W), dtype=f)
    flags, ambiguous = np.zeros((V, H, W), dtype=np.uint8), np.zeros((V, H, W), dtype=bool)
    for v in range(V):
        with np.errstate(all="ignore"):
            m = views[v].astype(f)  # W2C^T: R[j][i] at [i, j], t[j] at [3, j]
            R, t = m[:3, :3].T, m[3, :3]
            dirw = dc @ R                      # R^T d_c per pixel
            ow = -(R.T @ t)
            q0, dq = (ow - o) / h, dirw / h    # lattice coordinates of depth z: q0 + z dq
            # every sample that can lie in the lattice: z-depth <= the distance to the farthest corner of the box
            corners = np.array([[a, b, c] for a in (0, nx - 1) for b in (0, ny - 1) for c in (0, nz - 1)], dtype=np.float64)
            far = np.max(np.linalg.norm(corners - q0.astype(np.float64), axis=1)) * float(h) + 2 * float(step)
            if not np.isfinite(far) or not np.all(np.isfinite(dq)):
                continue  # NaN or infinite coordinates: every sample invalid, all misses
            K = int(np.clip(np.ceil((min(float(dmax) + EPS_Z, far) - float(dmin)) / float(step)) + 1, 0, 1 << 20))
            if K == 0:
                continue
            k = np.arange(K, dtype=f)
            z = k * step + dmin                                        # [K] (float64: exact to rounding; float32: like one fma)
            q = q0 + z[None, None, :, None] * dq[:, :, None, :]        # [H, W, K, 3]
            live = z < dmax
            valid, F = _sample(dtype, volume, q, min_weight)
            dec = valid & (F <= 0) & live[None, None, :]
            found = dec.any(axis=-1)
            ks = np.where(found, dec.argmax(axis=-1), 0)
            yy, xx = np.mgrid[0:H, 0:W]
            Fs = F[yy, xx, ks]
            kp = np.maximum(ks - 1, 0)
            pv, pF = valid[yy, xx, kp] & (ks >= 1), F[yy, xx, kp]
            hit = found & pv & (pF > 0)
            fl = np.where(hit, HIT, np.where(found, UNSEEN, 0)).astype(np.uint8)
            zp = kp.astype(f) * step + dmin
            zs = zp + step * pF / (pF - Fs)
            qs = q0 + zs[..., None] * dq
            # the normal: central differences of the interpolant one voxel either side, along the world axes
            g = np.zeros((H, W, 3), dtype=f)
            nok = np.ones((H, W), dtype=bool)
            for ax in range(3):
                e = np.zeros(3, dtype=f)
                e[ax] = 1
                vh, Fh = _sample(dtype, volume, qs + e, min_weight)
                vl, Fl = _sample(dtype, volume, qs - e, min_weight)
                nok &= vh & vl
                g[..., ax] = Fh - Fl
            len2 = (g * g).sum(-1)
            nok &= (len2 > 0) & np.isfinite(len2)
            nw = g / np.sqrt(np.where(nok, len2, 1))[..., None]
            nc = nw @ R.T                      # R n_w
            pc = dc * zs[..., None]
            nc = np.where(((nc * pc).sum(-1) > 0)[..., None], -nc, nc)
            fl = np.where(hit & ~nok, fl | NO_NORMAL, fl).astype(np.uint8)
            flags[v] = fl
            depth[v] = np.where(hit, zs, 0)
            vnmap[v] = np.where((hit & nok)[..., None], np.concatenate([nc, zs[..., None]], axis=-1), 0)
            if color is not None:
                color[v] = np.where(hit[None], np.moveaxis(_color(dtype, color_volume, qs), -1, 0), 0)
            if not with_ambiguous:
                continue
            # ---- next to a decision
            upto = np.where(found, ks, K - 1)                          # the samples that matter: k <= k*, or all of a miss
            kk = np.arange(K)[None, None, :]
            need = (kk <= upto[..., None]) & np.all((q > -1) & (q < n), axis=-1)   # (outside that box: invalid at all nine positions)
            qn = q[need].astype(np.float64)                            # [S, 3]
            lax = np.zeros(len(qn), dtype=bool)                        # could be decisive somewhere
            sure = np.ones(len(qn), dtype=bool)                        # decisive everywhere
            pos_sure = np.ones(len(qn), dtype=bool)                    # valid with F >= EPS_F everywhere
            pos_lax = np.zeros(len(qn), dtype=bool)                    # valid with F > -EPS_F somewhere
            for s in SHIFTS:
                va, Fa = _sample(np.float64, volume, qn + s, min_weight, EPS_W)
                vb = va if EPS_W == 0.0 else _sample(np.float64, volume, qn + s, min_weight, -EPS_W)[0]
                lax |= va & (Fa <= EPS_F)
                sure &= vb & (Fa <= -EPS_F)
                pos_sure &= vb & (Fa >= EPS_F)
                pos_lax |= va & (Fa > -EPS_F)

            def full(a):  # back to [H, W, K]; the samples left out are invalid at all nine positions
                out = np.zeros((H, W, K), dtype=bool)
                out[need] = a
                return out
            lax, sure, pos_sure, pos_lax = full(lax), full(sure), full(pos_sure), full(pos_lax)
            near_end = (np.abs(z.astype(np.float64) - float(dmax)) < EPS_Z)[None, None, :]
            lax_live = lax & (live | near_end)
            before = kk < np.where(found, ks, K)[..., None]
            amb = (lax_live & before).any(axis=-1)
            amb |= found & ~sure[yy, xx, ks]
            amb |= found & near_end[0, 0][ks]
            amb |= hit & ~pos_sure[yy, xx, kp]
            amb |= found & ~hit & (ks >= 1) & pos_lax[yy, xx, kp]
            # the normal's six evaluations
            for ax in range(3):
                for sgn in (-1.0, 1.0):
                    e = np.zeros(3)
                    e[ax] = sgn
                    states = []
                    for s in SHIFTS:
                        states.append(_sample(np.float64, volume, qs.astype(np.float64) + e + s, min_weight, EPS_W)[0])
                        if EPS_W != 0.0:
                            states.append(_sample(np.float64, volume, qs.astype(np.float64) + e + s, min_weight, -EPS_W)[0])
                    states = np.stack(states)
                    amb |= hit & (states.any(axis=0) != states.all(axis=0))
            amb |= hit & nok & (np.sqrt(np.where(nok, len2, 1)) < EPS_G)
            ambiguous[v] = amb
    return dict(depth=depth, vnmap=vnmap, color=color, flags=flags, ambiguous=ambiguous)


def raycast(volume, color_volume, origin, voxel, views, fx, fy, cx, cy, H, W, *, depth_range=(0.05, INF), step=None, min_weight=1.0):
    """-> dict(depth [V,H,W], vnmap [V,H,W,4], color [V,3,H,W] or None, flags uint8 [V,H,W], ambiguous bool [V,H,W]) in float64"""
    return _raycast(np.float64, volume, color_volume, origin, voxel, views, fx, fy, cx, cy, H, W, depth_range, step, min_weight, True)


def raycast32(volume, color_volume, origin, voxel, views, fx, fy, cx, cy, H, W, *, depth_range=(0.05, INF), step=None, min_weight=1.0):
    """the same arithmetic in float32 numpy: what float32 costs, to size the tolerance (its `ambiguous` is empty)"""
    return _raycast(np.float32, volume, color_volume, origin, voxel, views, fx, fy, cx, cy, H, W, depth_range, step, min_weight, False)


def bricks(volume, *, min_weight=1.0):
    """uint8 [ceil((nz-1)/8), ceil((ny-1)/8), ceil((nx-1)/8)]: 1 iff the brick holds a cell whose 8 weights are >= min_weight and
    that has a corner with tsdf <= 0"""
    nz, ny, nx = volume.shape[:3]
    shape = tuple(-(-(m - 1) // 8) for m in (nz, ny, nx))
    out = np.zeros(shape, dtype=np.uint8)
    if min(nx, ny, nz) < 2:
        return out
    with np.errstate(all="ignore"):
        ok, neg = volume[..., 1] >= np.float32(min_weight), volume[..., 0] <= 0
    valid = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    any_neg = np.zeros(valid.shape, dtype=bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                valid &= ok[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
                any_neg |= neg[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    for cz, cy, cx in zip(*np.nonzero(valid & any_neg)):
        out[cz // 8, cy // 8, cx // 8] = 1
    return out


# ---- the volumes and views the GPU tests ray-cast: name -> dict(volume, color, origin, voxel, views, fx, fy, cx, cy, H, W, opts)

def _colors(dims, seed=3):
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(0.05, 0.95, (nz, ny, nx, 3)), np.zeros((nz, ny, nx, 1))], axis=-1).astype(np.float32)


_FUSED = {}


def fused_main():
    """MAIN's 40 x 36 x 28 lattice fused from main_scene(3) by the float64 model, stored as float32 (volume, colour)"""
    if "main" not in _FUSED:
        vol, col, _, _ = T.run(T.main_scene(3))
        _FUSED["main"] = (np.ascontiguousarray(vol.astype(np.float32)), np.ascontiguousarray(col.astype(np.float32)))
    return _FUSED["main"]


def sphere_case(dims, origin, voxel, center, radius, **cam):
    vol = T.sdf_volume(dims, origin, voxel, 4.0 * voxel, T.sphere_sdf(center, radius))
    return dict(volume=vol, color=_colors(dims), origin=origin, voxel=voxel, **cam)


IMAGES = {
    "1x1": dict(H=1, W=1, fx=0.9, fy=0.9, cx=0.1, cy=-0.1),
    "17x15": dict(H=15, W=17, fx=16.0, fy=16.0, cx=8.2, cy=7.3),
    "37x29": dict(H=29, W=37, fx=33.0, fy=35.0, cx=20.7, cy=11.2),
    "64x48": dict(H=T.MAIN["H"], W=T.MAIN["W"], fx=T.MAIN["fx"], fy=T.MAIN["fy"], cx=T.MAIN["cx"], cy=T.MAIN["cy"]),
}
# poses around the MAIN scene (a sphere of radius 0.55 at about (0, 0, 2.05) in front of a wall at z = 3.2)
VIEWS3 = np.stack([T.pose(0.02, -0.11, 0.01, [0.21, 0.03, 0.02]), T.pose(-0.06, 0.13, -0.02, [-0.17, -0.05, 0.04]),
                   T.pose(0.1, 0.05, 0.2, [-0.03, 0.12, 0.01])])


def _small(dims, origin, voxel, center, radius, image, views):
    return dict(sphere_case(dims, origin, voxel, center, radius, **IMAGES[image]), views=views)


def cases():
    """every volume and camera the GPU tests compare with the model (built on first use)"""
    main_vol, main_col = fused_main()
    main = dict(volume=main_vol, color=main_col, origin=T.MAIN["origin"], voxel=T.MAIN["voxel"])
    front = T.pose(0.0, 0.0, 0.0, [0.0, 0.0, 0.0])[None]
    c = {
        "main-64x48-v3": dict(main, views=VIEWS3, **IMAGES["64x48"]),
        "main-64x48-v1": dict(main, views=VIEWS3[1:2], **IMAGES["64x48"]),
        "main-37x29-v3": dict(main, views=VIEWS3, **IMAGES["37x29"]),
        "main-17x15-v1": dict(main, views=VIEWS3[:1], **IMAGES["17x15"]),
        "main-1x1-v3": dict(main, views=VIEWS3, **IMAGES["1x1"]),
        # a lattice without a cell: all misses
        "lattice-1x1x1": _small((1, 1, 1), (0.011, -0.017, 1.47), 0.05, (0.0, 0.0, 1.5), 0.3, "17x15", front),
        # one cell, the sphere's surface running through it
        "lattice-2x2x2": _small((2, 2, 2), (-0.023, -0.027, 1.031), 0.05, (0.0, 0.0, 1.35), 0.3, "17x15", front),
        # exactly one brick
        "lattice-9x9x9": _small((9, 9, 9), (-0.21, -0.19, 0.9), 0.05, (0.013, -0.007, 1.31), 0.2, "37x29", VIEWS3[:1] * 1),
        # two bricks and a partial one along x, a brick and one cell along y, one brick along z
        "lattice-17x10x9": _small((17, 10, 9), (-0.42, -0.23, 0.9), 0.05, (0.017, 0.011, 1.33), 0.21, "37x29", VIEWS3),
    }
    return c


def look_from(center, rx, ry, rz):
    """W2C^T [4, 4] float32 of a camera at `center` with the rotation Rz Ry Rx"""
    m = T.pose(rx, ry, rz, [0.0, 0.0, 0.0]).astype(np.float64).T
    m[:3, 3] = -m[:3, :3] @ np.asarray(center, dtype=np.float64)
    return m.T.astype(np.float32)


def extra_cases():
    """the cases of the GPU tests' invariants and options, all compared with the model as well"""
    main_vol, main_col = fused_main()
    main = dict(volume=main_vol, color=main_col, origin=T.MAIN["origin"], voxel=T.MAIN["voxel"], **IMAGES["64x48"])
    one = VIEWS3[:1]
    # 25^3 samples = 3^3 bricks, lattice line x = y = 8 (an edge shared by four bricks) on the optical axis of pixel (8, 7): that
    # ray runs along the edge, its neighbours leave it at grazing angles through the bricks' corners and faces
    h = 0.05
    graze = sphere_case((25, 25, 25), (-8 * h, -8 * h, 1.0), h, (4 * h, 4 * h, 1.0 + 16 * h), 4.3 * h,
                        H=15, W=17, fx=40.0, fy=40.0, cx=8.0, cy=7.0)
    return {
        "graze": dict(graze, views=np.stack([T.pose(0.0, 0.0, 0.0, [0.0, 0.0, 0.0]), T.pose(0.0, 0.0, 0.0, [0.0, 0.0, 0.25]),
                                             look_from((8 * h, 8 * h, 0.6), 0.0, -0.2, 0.0)])),
        # a camera inside the lattice: inside the sphere (every ray starts below the surface) and in free space beside it
        "inside": dict(main, views=np.stack([look_from((0.03, -0.02, 1.8), 0.0, 0.0, 0.0), look_from((-0.8, -0.6, 1.45), 0.2, -0.55, 0.0)])),
        "away": dict(main, views=np.stack([look_from((0.0, 0.0, 0.0), 0.0, np.pi, 0.0), look_from((1.5, 0.2, 1.9), 0.1, -1.3, 0.0)])),
        "step-voxel": dict(main, views=one, opts=dict(step=0.05)),
        "step-fine": dict(main, views=one, opts=dict(step=0.0171)),
        "range": dict(main, views=one, opts=dict(depth_range=(1.37, 1.93))),
        "min-beyond": dict(main, views=one, opts=dict(depth_range=(1.6, INF))),
        "max-in-front": dict(main, views=one, opts=dict(depth_range=(0.05, 1.4))),
        "weight-2": dict(main, views=one, opts=dict(min_weight=2.0)),
        "weight-10": dict(main, views=one, opts=dict(min_weight=10.0)),
    }


def run(case, fn=raycast, with_color=True, **opts):
    o = dict(case.get("opts", {}))
    o.update(opts)
    return fn(case["volume"], case["color"] if with_color else None, case["origin"], case["voxel"], case["views"], case["fx"], case["fy"],
              case["cx"], case["cy"], case["H"], case["W"], **o)


_REFERENCES = {}


def _reference(name, fn):
    if (name, fn) not in _REFERENCES:
        case = cases()[name] if name in cases() else extra_cases()[name]
        _REFERENCES[name, fn] = run(case, fn)
    return _REFERENCES[name, fn]


def reference(name):
    """the float64 model's result of a named case (computed once; do not change it)"""
    return _reference(name, raycast)


def reference32(name):
    return _reference(name, raycast32)
