"""A numpy model of the TSDF steps (include/dgr_hip.h: dgr_tsdf_integrate, dgr_mesh_plan, dgr_mesh_emit) that shares no code with
the kernels: `integrate` is the fusion rule in float64 from the same float32 inputs, with the mask of the samples that sit next
to a decision; `integrate32` the same arithmetic in float32 (it only sizes the tolerance); `triangles` marching tetrahedra
without a case table: per tetrahedron the sign-changing edges are intersected, the polygon is ordered geometrically around the
gradient of the four values, started at the edge with the smallest corner pair and fanned from there.  Also the scenes the
tests fuse and the analytic distance fields they extract from."""
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
