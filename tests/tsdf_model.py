"""A numpy model of the TSDF steps (include/dgr_hip.h: dgr_tsdf_integrate, dgr_mesh_plan, dgr_mesh_emit) that shares no code with
the kernels: `integrate` is the fusion rule in float64 from the same float32 inputs, with the mask of the samples that sit next
to a decision; `integrate32` the same arithmetic in float32 (it only sizes the tolerance); `triangles` marching tetrahedra
without a case table: per tetrahedron the sign-changing edges are intersected, the polygon is ordered geometrically around the
gradient of the four values, started at the edge with the smallest corner pair and fanned from there.  Also the scenes the
tests fuse and the analytic distance fields they extract from."""
import functools
import itertools

import numpy as np

PIXEL_EPS, NEAR_EPS, TRUNC_EPS = 1e-3, 1e-5, 1e-5   # what `ambiguous` means (the issue's three margins)
INF = float("inf")


def lattice(origin, voxel, dims, dtype=np.float64):
    """sample positions [Nz, Ny, Nx] per axis, from the float32 origin and voxel size"""
    o, h = [dtype(np.float32(v)) for v in origin], dtype(np.float32(voxel))
    nx, ny, nz = dims
    x = o[0] + h * np.arange(nx, dtype=dtype)
    y = o[1] + h * np.arange(ny, dtype=dtype)
    z = o[2] + h * np.arange(nz, dtype=dtype)
    return np.broadcast_arrays(x[None, None, :], y[None, :, None], z[:, None, None])


def _integrate(dtype, volume, color_volume, origin, voxel, truncation, depth, views, fx, fy, cx, cy, color, mask, mask_threshold,
               weight, depth_range, near, max_weight):
    f = dtype
    dims = volume.shape[2], volume.shape[1], volume.shape[0]
    X, Y, Z = lattice(origin, voxel, dims, dtype)
    tsdf, w = volume[..., 0].astype(f), volume[..., 1].astype(f)
    col = None if color_volume is None else color_volume.astype(f)
    fx, fy, cx, cy, trunc, weight, near = (f(np.float32(v)) for v in (fx, fy, cx, cy, truncation, weight, near))
    lo, hi, max_weight, thr = (f(np.float32(v)) for v in (depth_range[0], depth_range[1], max_weight, mask_threshold))
    V, H, W = depth.shape
    ambiguous = np.zeros(tsdf.shape, dtype=bool)
    touched = np.zeros(tsdf.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for v in range(V):
            m = views[v].astype(f)  # W2C^T: R[j][i] at [i, j], t[j] at [3, j]
            pc = [m[0, j] * X + m[1, j] * Y + m[2, j] * Z + m[3, j] for j in range(3)]
            z = pc[2]
            ok = z > near
            u, vv = fx * pc[0] / z + cx, fy * pc[1] / z + cy
            fu, fv = np.floor(u + f(0.5)), np.floor(vv + f(0.5))
            ok &= (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            qx, qy = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
            d = depth[v][qy, qx].astype(f)
            ok &= (d > lo) & (d < hi)
            if mask is not None:
                ok &= ~(mask[v][qy, qx].astype(f) <= thr)
            sdf = d - z
            ok &= ~(sdf < -trunc)
            t = np.minimum(f(1.0), sdf / trunc)
            wn = w + weight
            tsdf = np.where(ok, (tsdf * w + t * weight) / wn, tsdf)
            if color is not None:
                for c in range(3):
                    col[..., c] = np.where(ok, (col[..., c] * w + color[v, c][qy, qx].astype(f) * weight) / wn, col[..., c])
            w = np.where(ok, np.minimum(wn, max_weight), w)
            touched |= ok
            # next to a decision: the near plane; a pixel boundary (where the choice of pixel can matter: in front of the near
            # plane, the pixel or its neighbour inside the image); the truncation (of the pixel this model chose)
            front = z > near - NEAR_EPS
            edge = (np.abs(u + 0.5 - np.round(u + 0.5)) < PIXEL_EPS) | (np.abs(vv + 0.5 - np.round(vv + 0.5)) < PIXEL_EPS)
            around = (fu >= -1) & (fu <= W) & (fv >= -1) & (fv <= H)
            ambiguous |= np.abs(z - near) < NEAR_EPS
            ambiguous |= front & edge & around
            ambiguous |= front & np.isfinite(sdf) & (np.abs(sdf + trunc) < TRUNC_EPS)
    out = np.stack([tsdf, w], axis=-1)
    return out, col, ambiguous, touched


def integrate(volume, color_volume, origin, voxel, truncation, depth, views, fx, fy, cx, cy, *, color=None, mask=None,
              mask_threshold=0.99, weight=1.0, depth_range=(0.0, INF), near=0.05, max_weight=INF):
    """-> (volume [Nz, Ny, Nx, 2], color volume or None, ambiguous [Nz, Ny, Nx], touched [Nz, Ny, Nx]) in float64"""
    return _integrate(np.float64, volume, color_volume, origin, voxel, truncation, depth, views, fx, fy, cx, cy, color, mask,
                      mask_threshold, weight, depth_range, near, max_weight)


def integrate32(volume, color_volume, origin, voxel, truncation, depth, views, fx, fy, cx, cy, *, color=None, mask=None,
                mask_threshold=0.99, weight=1.0, depth_range=(0.0, INF), near=0.05, max_weight=INF):
    """the same arithmetic in float32 numpy: what float32 costs, to size the tolerance"""
    return _integrate(np.float32, volume, color_volume, origin, voxel, truncation, depth, views, fx, fy, cx, cy, color, mask,
                      mask_threshold, weight, depth_range, near, max_weight)


# ---- marching tetrahedra

AXIS_ORDERS = [(a, b) for a in (1, 2, 4) for b in (1, 2, 4) if a != b]  # (1,2) (1,4) (2,1) (2,4) (4,1) (4,2): the documented order


def _corner(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def _polygon(vals, corners):
    """the crossing polygon of one tetrahedron: [(edge key, A, B, t)] in cyclic order with the normal along the gradient, started
    at the smallest edge key; [] without a sign change.  vals: the four float32 values as float64; corners: their corner numbers"""
    inside = [v < 0 for v in vals]
    if all(inside) or not any(inside):
        return []
    pts = []
    for i, j in itertools.combinations(range(4), 2):
        if inside[i] != inside[j]:
            A, B, va, vb = (corners[i], corners[j], vals[i], vals[j]) if corners[i] < corners[j] else (corners[j], corners[i], vals[j], vals[i])
            t = va / (va - vb)
            pts.append((A * 8 + B, A, B, t, _corner(A) + t * (_corner(B) - _corner(A))))
    # the gradient of the linear interpolant: (p_i - p_0) . g = v_i - v_0
    M = np.array([_corner(corners[i]) - _corner(corners[0]) for i in (1, 2, 3)])
    g = np.linalg.solve(M, np.array([vals[i] - vals[0] for i in (1, 2, 3)]))
    g /= np.linalg.norm(g)
    e1 = np.cross(g, [1.0, 0.0, 0.0] if abs(g[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(g, e1)
    c = np.mean([p[4] for p in pts], axis=0)
    pts.sort(key=lambda p: np.arctan2((p[4] - c) @ e2, (p[4] - c) @ e1))  # counter-clockwise seen from +g: normal along +g
    first = min(range(len(pts)), key=lambda i: pts[i][0])
    return pts[first:] + pts[:first]


def triangles(volume, origin, voxel, *, color=None, min_weight=1.0):
    """-> (count per cell [cells] int, vertices [T, 3, 3] float64, colours [T, 3, 3] float64 or None), triangles ordered by cell
    (x fastest), tetrahedron, triangle"""
    nz, ny, nx = volume.shape[:3]
    if min(nx, ny, nz) < 2:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 3, 3)), None if color is None else np.zeros((0, 3, 3))
    val, w = volume[..., 0].astype(np.float64), volume[..., 1]
    o, h = np.array([np.float32(v) for v in origin], dtype=np.float64), np.float64(np.float32(voxel))

    def corner_view(a, c):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    valid = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    n_in = np.zeros(valid.shape, dtype=np.int64)
    for c in range(8):
        valid &= corner_view(w, c) >= np.float32(min_weight)
        n_in += corner_view(val, c) < 0
    crossing = valid & (n_in > 0) & (n_in < 8)
    counts = np.zeros(valid.shape, dtype=np.int64)
    verts, cols = [], []
    for cz, cy, cx in zip(*np.nonzero(crossing)):  # (row-major over [z, y, x]: ascending linear cell index)
        base = np.array([cx, cy, cz], dtype=np.float64)
        cell_val = [val[cz + ((c >> 2) & 1), cy + ((c >> 1) & 1), cx + (c & 1)] for c in range(8)]
        for a, b in AXIS_ORDERS:
            corners = [0, a, a | b, 7]
            poly = _polygon([cell_val[c] for c in corners], corners)
            for k in range(1, len(poly) - 1):
                tri, tcol = [], []
                for _, A, B, t, _p in (poly[0], poly[k], poly[k + 1]):
                    pa, pb = o + h * (base + _corner(A)), o + h * (base + _corner(B))
                    tri.append(pa + t * (pb - pa))
                    if color is not None:
                        ia, ib = (base + _corner(A)).astype(int), (base + _corner(B)).astype(int)
                        ca = color[ia[2], ia[1], ia[0], :3].astype(np.float64)
                        cb = color[ib[2], ib[1], ib[0], :3].astype(np.float64)
                        tcol.append(ca + t * (cb - ca))
                verts.append(tri)
                cols.append(tcol)
                counts[cz, cy, cx] += 1
    V = np.array(verts, dtype=np.float64).reshape(-1, 3, 3)
    return counts.reshape(-1), V, (np.array(cols, dtype=np.float64).reshape(-1, 3, 3) if color is not None else None)


# ---- scenes

def pose(rx, ry, rz, t):
    """W2C^T [4, 4] float32 of the rotation Rz Ry Rx and the translation t"""
    cx_, sx, cy_, sy, cz_, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz_, -sz, 0], [sz, cz_, 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = Rz @ Ry @ Rx
    m[:3, 3] = t
    return m.T.astype(np.float32)


SPHERE_C, SPHERE_R, WALL_Z = np.array([0.03, -0.02, 2.05]), 0.55, 3.2


def render_scene(view, H, W, fx, fy, cx, cy, holes=True):
    """depth [H, W] float32 and colour [3, H, W] float32 of the sphere in front of the wall z = WALL_Z, seen by the W2C^T `view`
    (z-depth along the camera axis, by ray casting in float64); `holes`: a regular pattern of zero-depth pixels"""
    m = view.astype(np.float64).T
    R, t = m[:3, :3], m[:3, 3]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    dirs_c = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], axis=-1)  # z = 1: the ray parameter IS the depth
    o_w = -R.T @ t
    d_w = dirs_c @ R  # R^T d per pixel
    depth = np.where(d_w[..., 2] > 1e-9, (WALL_Z - o_w[2]) / np.where(d_w[..., 2] > 1e-9, d_w[..., 2], 1.0), 0.0)
    oc = o_w - SPHERE_C
    A, B, C = (d_w * d_w).sum(-1), 2.0 * (d_w @ oc), oc @ oc - SPHERE_R ** 2
    disc = B * B - 4 * A * C
    s = (-B - np.sqrt(np.maximum(disc, 0.0))) / (2 * A)
    hit = (disc > 0) & (s > 0)
    depth = np.where(hit, s, depth)
    pw = o_w + depth[..., None] * d_w
    color = np.stack([0.5 + 0.4 * np.sin(3.0 * pw[..., 0]), 0.5 + 0.4 * np.cos(2.0 * pw[..., 1]), np.where(hit, 0.9, 0.2)], axis=0)
    if holes:
        depth = np.where((xs % 7 == 3) & (ys % 5 == 1), 0.0, depth)
    return depth.astype(np.float32), color.astype(np.float32)


MAIN = dict(dims=(40, 36, 28), voxel=0.05, origin=(-1.0, -0.9, 1.3), H=48, W=64, fx=60.0, fy=60.0, cx=31.3, cy=23.6)
MAIN_POSES = [pose(0.0, 0.0, 0.0, [0.0, 0.0, 0.0]), pose(0.05, -0.21, 0.03, [0.38, 0.02, 0.05]),
              pose(-0.12, 0.26, -0.04, [-0.33, -0.1, 0.1]), pose(0.2, 0.1, 0.1, [-0.1, 0.3, 0.02]),
              pose(-0.08, -0.12, 0.29, [0.15, -0.2, -0.05])]


def main_scene(V):
    """the issue's scene with the first V of the five poses: dict(depth [V,H,W], color [V,3,H,W], views [V,4,4], **MAIN)"""
    s = dict(MAIN)
    frames = [render_scene(p, s["H"], s["W"], s["fx"], s["fy"], s["cx"], s["cy"]) for p in MAIN_POSES[:V]]
    s.update(depth=np.stack([f[0] for f in frames]), color=np.stack([f[1] for f in frames]), views=np.stack(MAIN_POSES[:V]))
    return s


def sdf_volume(dims, origin, voxel, truncation, fn, weight=1.0):
    """[Nz, Ny, Nx, 2] float32: the analytic distance fn(x, y, z) / truncation clipped to [-1, 1], and a constant weight"""
    X, Y, Z = lattice(origin, voxel, dims)
    v = np.clip(fn(X, Y, Z) / truncation, -1.0, 1.0).astype(np.float32)
    return np.ascontiguousarray(np.stack([v, np.full(v.shape, weight, dtype=np.float32)], axis=-1))


def sphere_sdf(c, r):
    return lambda X, Y, Z: np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r


def torus_sdf(c, R, r):
    return lambda X, Y, Z: np.sqrt((np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2) - R) ** 2 + (Z - c[2]) ** 2) - r


def scene(V=3, **over):
    """main_scene with some of MAIN's entries replaced (dims, origin, voxel, H, W, fx, fy, cx, cy)"""
    s = dict(MAIN)
    s.update(over)
    frames = [render_scene(p, s["H"], s["W"], s["fx"], s["fy"], s["cx"], s["cy"]) for p in MAIN_POSES[:V]]
    s.update(depth=np.stack([f[0] for f in frames]), color=np.stack([f[1] for f in frames]), views=np.stack(MAIN_POSES[:V]))
    return s


# every scene the GPU tests fuse and compare with the model: name -> scene() arguments
CASES = {
    "main-1": dict(V=1), "main-3": dict(V=3), "main-5": dict(V=5),
    "lattice-1x1x1": dict(V=2, dims=(1, 1, 1), origin=(0.011, -0.017, 1.47)),
    "lattice-65x3x2": dict(V=3, dims=(65, 3, 2), origin=(-1.6, -0.07, 1.62)),
    "lattice-7x5x3": dict(V=3, dims=(7, 5, 3), origin=(-0.2, -0.1, 1.45), voxel=0.04),
    "image-1x1": dict(V=2, H=1, W=1, fx=0.9, fy=0.9, cx=0.1, cy=-0.1),
    "image-37x29": dict(V=3, H=29, W=37, fx=33.0, fy=35.0, cx=17.7, cy=14.2),
}


def run(s, fn=integrate, volume=None, color_volume=None, with_color=True, **opts):
    """`fn` (integrate or integrate32) on a scene() dict, from an empty volume unless one is given; truncation = 4 voxels"""
    nx, ny, nz = s["dims"]
    volume = np.zeros((nz, ny, nx, 2), dtype=np.float32) if volume is None else volume
    if with_color and color_volume is None:
        color_volume = np.zeros((nz, ny, nx, 4), dtype=np.float32)
    return fn(volume, color_volume if with_color else None, s["origin"], s["voxel"], np.float32(4.0 * s["voxel"]), s["depth"], s["views"],
              s["fx"], s["fy"], s["cx"], s["cy"], color=s["color"] if with_color else None, **opts)


def pattern(s, seed=5):
    """a volume that is recognisably not empty: tsdf in (-1, 1) without zeros, weights in [0.5, 3] (quarters: their sums with a
    view's weight are exact in float32 as in float64, so the weights can be compared for equality), colours in (0, 1)"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = s["dims"]
    tsdf = rng.uniform(0.05, 0.95, (nz, ny, nx)) * rng.choice([-1.0, 1.0], (nz, ny, nx))
    vol = np.stack([tsdf, rng.integers(2, 13, (nz, ny, nx)) / 4.0], axis=-1).astype(np.float32)
    col = np.concatenate([rng.uniform(0.01, 0.99, (nz, ny, nx, 3)), np.zeros((nz, ny, nx, 1))], axis=-1).astype(np.float32)
    return vol, col


# ---- scenes for the view loop and the brick culling of the integrate kernel: a workgroup owns a brick of 64 x 4 x 1 samples, tests
# the views in chunks of 256 (four ballots of 64) and walks the views its brick can see

BRICK_X, BRICK_Y = 64, 4


def pose_at(c, rx, ry, rz):
    """`pose` given by the camera centre c: t = -R c"""
    R = pose(rx, ry, rz, [0.0, 0.0, 0.0]).astype(np.float64).T[:3, :3]
    return pose(rx, ry, rz, -R @ np.asarray(c, dtype=np.float64))


def with_frames(s, poses, holes=True):
    """the scene dict `s` with `poses` and what they see of the sphere and the wall"""
    frames = [render_scene(p, s["H"], s["W"], s["fx"], s["fy"], s["cx"], s["cy"], holes) for p in poses]
    s.update(depth=np.stack([f[0] for f in frames]), color=np.stack([f[1] for f in frames]), views=np.stack(poses))
    return s


def sub_scene(s, index):
    """the scene with the views `index` (a list or a slice) only, in that order"""
    return dict(s, depth=s["depth"][index], color=s["color"][index], views=s["views"][index])


def live_pose(rng):
    """a pose that sees the lattices in front of the identity: up to +-0.25 rad and +-0.3 m around it"""
    return pose(*rng.uniform(-0.25, 0.25, 3), rng.uniform(-0.3, 0.3, 3))


# poses that see nothing of a lattice in front of the identity, one kind per test of the culling (rx, ry, t): facing away and far
# behind the camera (`behind`), and the lattice past each of the image's four sides
BLIND_KINDS = [(0.0, np.pi, (0.0, 0.0, 0.0)), (0.0, 1.4, (0.0, 0.0, 0.0)), (-1.3, 0.0, (0.0, 0.0, 0.0)), (0.0, 0.0, (0.0, 0.0, -10.0)),
               (0.0, -1.4, (0.0, 0.0, 0.0)), (1.3, 0.0, (0.0, 0.0, 0.0))]
BLIND_DEPTH, BLIND_COLOR = 2.0, 0.5


def blind_pose(k, rng):
    """the k-th kind (in rotation), jittered so that no two blind poses are equal"""
    rx, ry, t = BLIND_KINDS[k % len(BLIND_KINDS)]
    j = rng.uniform(-1.0, 1.0, 5)
    return pose(rx + 0.03 * j[0], ry + 0.03 * j[1], 0.0, np.array(t) + 0.05 * j[2:])


def many_view_scene(V, live, dims, origin, voxel, seed):
    """V views of which only the indices `live` see the lattice: distinct seeded poses with their rendered depth and colour; the
    others are blind poses with a constant valid depth and a constant colour, so that a blind image under a live pose, or a live
    image under a blind pose, would change the result.  `live` is kept in the dict (sorted)."""
    rng = np.random.default_rng(seed)
    s = dict(MAIN, dims=tuple(dims), origin=tuple(origin), voxel=voxel, live=sorted(int(v) for v in live))
    assert len(set(s["live"])) == len(s["live"]) and all(0 <= v < V for v in s["live"])
    H, W = s["H"], s["W"]
    depth = np.full((V, H, W), BLIND_DEPTH, dtype=np.float32)
    color = np.full((V, 3, H, W), BLIND_COLOR, dtype=np.float32)
    views = np.stack([blind_pose(k, rng) for k in range(V)])
    for v in s["live"]:
        views[v] = live_pose(rng)
        depth[v], color[v] = render_scene(views[v], H, W, s["fx"], s["fy"], s["cx"], s["cy"])
    s.update(depth=depth, color=color, views=views)
    return s


def blind_views(s):
    return [v for v in range(len(s["views"])) if v not in s["live"]]


# the lattice of the many-view cases: two bricks along x and two along y, both hanging over the lattice's edge
MANY = dict(dims=(70, 6, 3), origin=(-1.7, -0.13, 1.6), voxel=0.05)
MANY_OPTS = dict(max_weight=3.0)
# name -> (V, live): a case per line of the view loop
MANY_CASES = {
    "64-high-half": (64, (31, 32, 63)),
    "65-wave-1": (65, (0, 63, 64)),
    "256-waves-1-3": (256, (64, 127, 128, 191, 192, 255)),
    "257-second-chunk": (257, (0, 63, 64, 255, 256)),
    "257-first-chunk-blind": (257, (256,)),
    "513-three-chunks": (513, (5, 64, 255, 256, 300, 511, 512)),
    "257-moved": (257, (1, 65, 256)),  # (the scene a captured 257-view call is replayed on)
}
# seeds at which no sample of a blind view sits within NEAR_EPS of the near plane (a pose that looks past the lattice has samples on
# both sides of it) and the ambiguous share stays well under the cap (tests/test_tsdf_model.py holds them to both)
MANY_SEEDS = {"64-high-half": 101, "65-wave-1": 101, "256-waves-1-3": 102, "257-second-chunk": 102, "257-first-chunk-blind": 102,
              "513-three-chunks": 102, "257-moved": 102}
ALL_LIVE = dict(V=300, dims=(7, 5, 3), origin=(-0.2, -0.1, 1.45), voxel=0.04, seed=7)  # every view live: no model, bits only


@functools.lru_cache(maxsize=None)
def many_case(name):
    """the scene of MANY_CASES[name] on the MANY lattice (shared: leave it unchanged)"""
    V, live = MANY_CASES[name]
    s = many_view_scene(V, live, seed=MANY_SEEDS[name], **MANY)
    for k in ("depth", "color", "views"):
        s[k].setflags(write=False)
    return s


# the lattice of the culling scenes: 3 x 3 x 12 bricks, the last along x two samples wide, the last along y two rows high
CULLING_LATTICE = dict(dims=(130, 10, 12), origin=(-1.6, -0.12, 1.4), voxel=0.025)
# name -> (scene entries replaced, [(camera centre, rx, ry, rz)] of its two views, options of the call)
CULLING = {
    "inside": ({}, [((-0.6, 0.0, 1.5), 0.0, 1.0, 0.0), ((0.7, -0.03, 1.6), 0.05, -1.0, 0.0)], {}),
    "roll": ({}, [((0.1, 0.0, 0.2), 0.0, 0.1, 0.785), ((-0.2, 0.05, 0.3), 0.05, -0.15, -2.2)], {}),
    "near-oblique": ({}, [((0.3, 0.0, 0.2), 0.0, 0.6, 0.0), ((1.2, 0.02, 0.25), 0.03, -0.6, 0.0)], dict(near=1.3)),
    "pp-outside": (dict(cx=-20.0, cy=60.0), [((-0.8, 0.5, 0.3), 0.0, 0.0, 0.0), ((-1.5, 0.4, 0.5), 0.05, 0.1, -0.05)], {}),
    "aniso": (dict(fx=25.0, fy=140.0), [((0.0, 0.25, 0.0), 0.0, 0.0, 0.0), ((0.4, 0.3, 0.1), -0.05, 0.3, 0.1)], {}),
    "minus-x": ({}, [((0.9, 0.0, 1.5), 0.0, np.pi / 2 - 0.1, 0.0), ((-0.8, -0.02, 1.6), 0.0, -np.pi / 2 + 0.1, 0.0)], {}),
    # The side planes' margins where they are widest in pixels: the culling keeps one pixel more than the image, which at depth Z is
    # a margin of Z in the units of its comparisons (fx X + c Z against 0), so a margin wrong by some delta costs delta / Z pixels,
    # and shows only on a brick that lies whole within that many pixels of an image border.  The last brick along x (two samples)
    # seen end-on from 0.25 m, along -x, by a principal point near the image's corner: the layer 8.3 mm beside the camera's axis
    # lands in pixel column W - 2 of the first view and, rolled a quarter turn, in pixel row H - 2 of the second.
    "edge-pixels": (dict(cx=60.0, cy=44.0), [((1.85, 0.0, 1.55 - 0.25 / 30.0), 0.0, np.pi / 2, 0.0),
                                              ((1.85, 0.0, 1.55 - 0.25 / 30.0), 0.0, np.pi / 2, np.pi / 2)], {}),
    "sideways": ({}, [((-2.2, 0.0, 1.5), 0.0, -np.pi / 2 + 0.15, 0.0), ((2.3, 0.02, 1.45), 0.0, np.pi / 2 - 0.2, 0.0)], {}),
}


@functools.lru_cache(maxsize=None)
def culling_case(name):
    """-> (scene, options) of CULLING[name] (shared: leave them unchanged)"""
    over, poses, opts = CULLING[name]
    s = with_frames(dict(MAIN, **CULLING_LATTICE, **over), [pose_at(*p) for p in poses])
    for k in ("depth", "color", "views"):
        s[k].setflags(write=False)
    return s, dict(opts)


def brick_shares(touched):
    """the share of touched samples of every brick, [Nz, ceil(Ny / 4), ceil(Nx / 64)]"""
    nz, ny, nx = touched.shape
    by, bx = -(-ny // BRICK_Y), -(-nx // BRICK_X)
    out = np.zeros((nz, by, bx))
    for j in range(by):
        for i in range(bx):
            out[:, j, i] = touched[:, j * BRICK_Y:(j + 1) * BRICK_Y, i * BRICK_X:(i + 1) * BRICK_X].mean(axis=(1, 2))
    return out


def brick_corner_depths(s, view):
    """the camera depth of every brick's four corners (those of the lattice where the brick hangs over), [Nz, by, bx, 4]"""
    nx, ny, nz = s["dims"]
    m = view.astype(np.float64)
    o, h = [np.float64(np.float32(v)) for v in s["origin"]], np.float64(np.float32(s["voxel"]))
    x0 = np.arange(0, nx, BRICK_X)
    y0 = np.arange(0, ny, BRICK_Y)
    xs = np.stack([x0, np.minimum(x0 + BRICK_X - 1, nx - 1)])  # [2, bx]
    ys = np.stack([y0, np.minimum(y0 + BRICK_Y - 1, ny - 1)])
    z = o[2] + h * np.arange(nz)
    out = [m[0, 2] * (o[0] + h * xs[a])[None, None, :] + m[1, 2] * (o[1] + h * ys[b])[None, :, None] + m[2, 2] * z[:, None, None] + m[3, 2]
           for a in (0, 1) for b in (0, 1)]
    return np.stack(out, axis=-1)
