"""Frame-to-model ICP as include/dgr_hip.h defines it (dgr_depth_normals, dgr_icp_step) and slam.icp_align, restated in float64
numpy on the CPU.  Written from that text.  Beside each result it returns what a comparison with an fp32 kernel needs:

Ambiguity marks.  A normal-map pixel or a candidate is *ambiguous* when one of its threshold tests is decided by less than the
fp32 rounding of the quantities compared, so that the kernel may decide either way.  The margins are computed per pixel from the
magnitudes that enter the test (below), not tuned.  Raw fp32 comparisons of inputs (the depth range, the mask, d > 0) are decided
exactly and never marked.

Error bounds for the sums.  For each of the 28 sums S = sum term_i the model returns B = sum bound_i, bound_i the first-order
fp32 evaluation error of term_i with u = 2^-24 per rounding.  The roundings are counted on csrc/icp.hip's step kernel as if no
multiply-add were fused (fusing removes roundings):
  p      = ((x - cx) * inv_f) * d            2 roundings + inv_f's own + 1 spare = 4 u |p|; p_z = d is exact
  q_j    = r_j0 p_0 + r_j1 p_1 + r_j2 d + t_j   3 products (1 each), 3 additions (1 each, on the partial sums), the error of p:
                                             8 u (|r_j0 p_0| + |r_j1 p_1| + |r_j2 d| + |t_j|).  rel itself is formed in double and
                                             rounded once by kernel and model alike: no error
  v_m    = ((px - cx) * inv_f) * d_m         4 u |v_m| in x and y, exact in z
  e      = q - v_m                           1 rounding: dq + dv_m + u |e|
  r      = n . e                             3 products, 2 additions: sum |n_j| de_j + 3 u sum |n_j e_j| -- the cancellation in
                                             n . (q - v_m) is therefore bounded on |q| + |v_m|, not on |r|
  J_rot  = q x n                             per entry 2 products, 1 subtraction: |n_b| dq_a + |n_a| dq_b + 2 u (|q_a n_b| + |q_b n_a|);
                                             J_trans = n is exact
  w      = delta / |r| where |r| > delta     1 division: w (dr / |r| + u); also charged within dr of the switch; 0 where w = 1
  terms  (w J_i) J_j, (w J_i) r, (w r) r     2 roundings each on top of the propagated errors
The double accumulation is not in B: the tests add 2^-50 sum |term_i| for it.
A candidate whose landing position is within its error of a pixel's edge may read the neighbouring model pixel: its bound also
covers the largest change of the term among the neighbours in question.

The normal map's per-pixel bound follows the same way: the differences a, b of unprojected neighbours carry 5 u (|V+| + |V-|)
per entry, the cross product 2 more roundings on its products, the normalisation 4.
"""
import numpy as np

U = 2.0 ** -24
VALID, INSIDE, ASSOCIATED = 1, 2, 4
BLOCK = 2048
INF = float("inf")
DAMPING_FLOOR = 1e-3  # include/dgr_hip.h: M = A + damping diag(max(A_ii, 1e-3 max A_ii))
TWIST = np.array([0.012, -0.015, 0.008, 0.02, -0.015, 0.018])  # (omega | v) of the test scene's current frame


def f32(x):
    """a parameter: formed in float64, rounded once to fp32 (what the C ABI receives), carried on as float64"""
    return float(np.float32(x))


def candidates(W, H, stride):
    xs, ys = np.arange(0, W, stride), np.arange(0, H, stride)
    return np.tile(xs, len(ys)), np.repeat(ys, len(xs))


# ------------------------------------------------------------------------------------------------------------ rigid motions
def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi, mutate=None):
    """(R, t) of the twist (omega | v): Rodrigues, the series below theta^2 = 1e-6.  `mutate`: "series_only" (the series at
    every theta: a deliberately wrong model)"""
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th2 = float(w @ w)
    if th2 < 1e-6 or mutate == "series_only":
        A = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0)
        B = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0)
        C = 1.0 / 6.0 - th2 / 120.0 * (1.0 - th2 / 42.0)
    else:
        th = np.sqrt(th2)
        A, B, C = np.sin(th) / th, 2.0 * np.sin(0.5 * th) ** 2 / th2, (th - np.sin(th)) / (th2 * th)
    K = skew(w)
    K2 = K @ K
    return np.eye(3) + A * K + B * K2, (np.eye(3) + B * K + C * K2) @ v


def pose_of(view):
    """(R, t) of 16 floats holding W2C^T, float64"""
    m = np.asarray(view, np.float64).reshape(4, 4).T
    return m[:3, :3].copy(), m[:3, 3].copy()


def w2ct(R, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return np.ascontiguousarray(m.T.astype(np.float32))


QUAT_BRANCHES = ("trace", "x", "y", "z")
POSE_MUTANTS = ("quat_branch_x", "quat_branch_y", "quat_branch_z", "no_sign_fix", "series_only")


def quat_branch(R):
    """which of Shepperd's branches rotation_to_quat takes on R: one of QUAT_BRANCHES"""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0.0:
        return "trace"
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        return "x"
    return "y" if R[1, 1] > R[2, 2] else "z"


def rotation_to_quat(R, mutate=None):
    """(r, x, y, z), unit, r >= 0: Shepperd's branches.  `mutate`: "quat_branch_x", "quat_branch_y", "quat_branch_z" (one
    off-diagonal sum of that branch with a wrong sign), "no_sign_fix" (r < 0 is kept) -- deliberately wrong models"""
    branch = quat_branch(R)
    wrong = -1.0 if mutate == "quat_branch_" + branch else 1.0
    if branch == "trace":
        s = 2.0 * np.sqrt(R[0, 0] + R[1, 1] + R[2, 2] + 1.0)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif branch == "x":
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + wrong * R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif branch == "y":
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + wrong * R[2, 1]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + wrong * R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q) / np.linalg.norm(q)
    return -q if q[0] < 0.0 and mutate != "no_sign_fix" else q


def quat_to_rotation(q):
    r, x, y, z = q
    d = r * r - (x * x + y * y + z * z)
    return np.array([[d + 2 * x * x, 2 * x * y - 2 * r * z, 2 * x * z + 2 * r * y],
                     [2 * x * y + 2 * r * z, d + 2 * y * y, 2 * y * z - 2 * r * x],
                     [2 * x * z - 2 * r * y, 2 * y * z + 2 * r * x, d + 2 * z * z]])


def pose_error(view, true_view):
    """(rotation angle between the two poses in rad, distance between the two camera centres).  The angle from the antisymmetric
    part of R R_true^T (its sine) against the trace (its cosine): fp32 poses are orthonormal to 1e-7 only, which the trace alone
    would turn into an angle of 3e-4"""
    R, t = pose_of(view)
    Rt, tt = pose_of(true_view)
    D = R @ Rt.T
    sine = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(sine, 0.5 * (np.trace(D) - 1.0))), float(np.linalg.norm(R.T @ t - Rt.T @ tt))


# ------------------------------------------------------------------------------------------------------------------- scene
def intrinsics(W, H):
    return 0.8 * W, 0.75 * W, (W - 1) / 2 + 0.07 * W, (H - 1) / 2 - 0.05 * H


def plane_depth(W, H, fx, fy, cx, cy, view, planes=((0, 1.6), (1, 1.1), (2, 3.0))):
    """Depth of the room corner (planes axis = value) seen from the pose `view` (W2C^T, fp32): ray-plane intersection in float64,
    rounded to fp32; 0 where a ray meets no plane"""
    R, t = pose_of(view)
    centre = -R.T @ t
    fx, fy, cx, cy = (f32(v) for v in (fx, fy, cx, cy))
    y, x = np.mgrid[0:H, 0:W]
    rays = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones((H, W))], -1) @ R  # the camera rays in the world (R^T ray)
    depth = np.full((H, W), np.inf)
    for axis, value in planes:
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (value - centre[axis]) / rays[..., axis]
        depth = np.where((s > 0) & (s < depth), s, depth)
    return np.where(np.isfinite(depth), depth, 0.0).astype(np.float32)


def corner_scene(W, H, twist=TWIST):
    """The room corner x = 1.6, y = 1.1, z = 3.0 from a camera at (0.2, -0.1, 0.3) that looks into it, rolled 0.1 rad (the model
    pose), and from that pose moved by `twist` (the current frame, whose pose ICP is to find)."""
    fx, fy, cx, cy = intrinsics(W, H)
    centre = np.array([0.2, -0.1, 0.3])
    z = np.array([1.6, 1.1, 3.0]) - centre
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    roll = np.array([[np.cos(0.1), -np.sin(0.1), 0.0], [np.sin(0.1), np.cos(0.1), 0.0], [0.0, 0.0, 1.0]])
    Rm = roll @ np.stack([x, y, z])
    tm = -Rm @ centre
    Re, te = se3_exp(twist)
    model_view, true_view = w2ct(Rm, tm), w2ct(Re @ Rm, Re @ tm + te)
    return dict(W=W, H=H, fx=fx, fy=fy, cx=cx, cy=cy, model_view=model_view, true_view=true_view,
                model_depth=plane_depth(W, H, fx, fy, cx, cy, model_view), depth_obs=plane_depth(W, H, fx, fy, cx, cy, true_view))


# ------------------------------------------------------------------------------------------------------------ world frames
def move_world(view, Rt, c, model_view=None):
    """The same camera seen from another world frame, X' = G X + c with G^T = Rm^T Rt, Rm the rotation of the scene's
    `model_view` (None: `view` is the model's): the pose (R, t) becomes (R G^T, t - R G^T c), rounded once to fp32.  The model's
    own rotation becomes Rt (to the orthonormality of an fp32 pose).  Applied to every pose of a scene alike; what lives in the
    camera frame -- depth images, normal maps, intensity maps -- does not change."""
    R, t = pose_of(view)
    Rm, _ = pose_of(view if model_view is None else model_view)
    RG = R @ (Rm.T @ np.asarray(Rt, np.float64))
    return w2ct(RG, t - RG @ np.asarray(c, np.float64))


def move_scene(s, name):
    """a copy of the scene (or frame) `s` with model_view, view_in (where it has one) and true_view moved to WORLD_FRAMES[name]"""
    Rt, c = WORLD_FRAMES[name]
    out = dict(s)
    for k in ("model_view", "view_in", "true_view"):
        if k in s:
            out[k] = move_world(s[k], Rt, c, s["model_view"])
    return out


def _axis_rotation(axis, angle):
    i, j = (axis + 1) % 3, (axis + 2) % 3
    R = np.eye(3)
    R[i, i] = R[j, j] = np.cos(angle)
    R[i, j], R[j, i] = -np.sin(angle), np.sin(angle)
    return R


def _world_frames():
    """name -> (Rt, c): the model camera's rotation in the moved world and the moved world's origin shift.
    identity: the control.  half_x, half_y, half_z: the half turns, where the model's, the input's and the output's rotations all
    take Shepperd's diagonal branch x, y, z at a trace of -1 + O(twist^2).  near_x, near_y, near_z: rot_a(2.9) rot_b(0.2), a generic
    rotation inside each diagonal branch.  perm120: the cyclic permutation, trace 0.  far: near_y at |c| = 100 m, where the
    translations are large and cancel in rel.  random0 .. random31: seeded random rotations.  |c| <= 5 m but for far."""
    rng = np.random.default_rng(2024)

    def shift(length):
        d = rng.standard_normal(3)
        return d / np.linalg.norm(d) * length

    near = [_axis_rotation(a, 2.9) @ _axis_rotation((a + 1) % 3, 0.2) for a in range(3)]
    frames = {"identity": (np.eye(3), np.zeros(3))}
    for a, n in enumerate("xyz"):
        frames["half_" + n] = (np.diag([1.0 if k == a else -1.0 for k in range(3)]), shift(rng.uniform(1.0, 5.0)))
    for a, n in enumerate("xyz"):
        frames["near_" + n] = (near[a], shift(rng.uniform(1.0, 5.0)))
    frames["perm120"] = (np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), shift(rng.uniform(1.0, 5.0)))
    frames["far"] = (near[1], shift(100.0))
    for k in range(32):
        q = rng.standard_normal(4)
        frames[f"random{k}"] = (quat_to_rotation(q / np.linalg.norm(q)), shift(rng.uniform(0.0, 5.0)))
    return frames


WORLD_FRAMES = _world_frames()
NAMED_FRAMES = tuple(n for n in WORLD_FRAMES if not n.startswith("random"))
RANDOM_FRAMES = tuple(n for n in WORLD_FRAMES if n.startswith("random"))


def fronto_parallel_scene(W, H, depth=2.0):
    """A plane at constant depth seen head-on by both poses: A has exactly zero rows for omega_z, v_x, v_y"""
    fx, fy, cx, cy = intrinsics(W, H)
    eye = np.eye(4, dtype=np.float32)
    img = np.full((H, W), depth, np.float32)
    return dict(W=W, H=H, fx=fx, fy=fy, cx=cx, cy=cy, model_view=eye, true_view=eye, model_depth=img, depth_obs=img.copy())


# ----------------------------------------------------------------------------------------------------------------- normals
def depth_normals_model(depth, fx, fy, cx, cy, *, depth_range=(0.0, INF), max_jump=0.1, mask_image=None, mask_threshold=0.99):
    """depth [H,W] float32.  Returns a dict: vnmap float64 [H,W,4] (n, d; zeros where unusable), usable bool [H,W], ambiguous bool
    [H,W], bound float64 [H,W] (on every component of n at a usable pixel).
    Handed float64 depths the model evaluates the definition itself: the depths are not rounded to fp32 and 1 / fx, 1 / fy are the
    float64 quotients, not the fp32 values the kernel is given (the closed-form checks; marks and bounds then mean nothing)."""
    exact = np.asarray(depth).dtype == np.float64
    depth = np.asarray(depth, np.float64 if exact else np.float32)
    H, W = depth.shape
    fx, fy, cx, cy, mj = (f32(v) for v in (fx, fy, cx, cy, max_jump))
    ifx, ify = (1.0 / fx, 1.0 / fy) if exact else (f32(1.0 / fx), f32(1.0 / fy))
    lo, hi = np.float32(depth_range[0]), np.float32(depth_range[1])
    with np.errstate(invalid="ignore"):
        good = (depth > lo) & (depth < hi)
    usable = np.zeros((H, W), bool)
    ambiguous = np.zeros((H, W), bool)
    vn = np.zeros((H, W, 4))
    bound = np.zeros((H, W))
    if H < 3 or W < 3:
        return dict(vnmap=vn, usable=usable, ambiguous=ambiguous, bound=bound)
    c = (slice(1, -1), slice(1, -1))
    nb = {"l": (slice(1, -1), slice(0, -2)), "r": (slice(1, -1), slice(2, None)), "u": (slice(0, -2), slice(1, -1)),
          "d": (slice(2, None), slice(1, -1))}
    ok = good[c].copy()
    for s in nb.values():
        ok &= good[s]
    if mask_image is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(mask_image, np.float32)[c] > np.float32(mask_threshold)
    D = np.where(good, depth, 1.0).astype(np.float64)
    dc = D[c]
    amb = np.zeros_like(ok)
    for s in nb.values():
        diff, lim = np.abs(D[s] - dc), mj * dc
        ok &= diff <= lim
        amb |= np.abs(diff - lim) <= 2 * U * (diff + lim)
    y, x = np.mgrid[1:H - 1, 1:W - 1]
    X, Y = (x - cx) * ifx, (y - cy) * ify
    Xl, Xr, Yu, Yd = (x - 1 - cx) * ifx, (x + 1 - cx) * ifx, (y - 1 - cy) * ify, (y + 1 - cy) * ify
    dl, dr, du, dd = (D[nb[k]] for k in "lrud")
    a = np.stack([Xr * dr - Xl * dl, Y * dr - Y * dl, dr - dl], -1)
    b = np.stack([X * dd - X * du, Yd * dd - Yu * du, dd - du], -1)
    da = 5 * U * np.stack([np.abs(Xr * dr) + np.abs(Xl * dl), np.abs(Y) * (dr + dl), dr + dl], -1)
    db = 5 * U * np.stack([np.abs(X) * (dd + du), np.abs(Yd * dd) + np.abs(Yu * du), dd + du], -1)
    cr = np.cross(a, b)
    aa, ab = np.abs(a), np.abs(b)
    rot = lambda v: np.stack([v[..., 1], v[..., 2], v[..., 0]], -1), lambda v: np.stack([v[..., 2], v[..., 0], v[..., 1]], -1)  # noqa: E731
    r1, r2 = rot
    # |d(a x b)|_k <= da_i |b_j| + |a_i| db_j + (the same with i, j swapped) + 2 u (|a_i b_j| + |a_j b_i|)
    dcr = (r1(da) * r2(ab) + r1(aa) * r2(db) + r2(da) * r1(ab) + r2(aa) * r1(db) + 2 * U * (r1(aa) * r2(ab) + r2(aa) * r1(ab)))
    length = np.linalg.norm(cr, axis=-1)
    dlen = np.linalg.norm(dcr, axis=-1)
    nonzero = length > 0.0
    ok_before = ok.copy()
    ok &= nonzero
    amb |= ok_before & (length <= dlen)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where(ok[..., None], cr / length[..., None], 0.0)
        err = np.where(ok, (np.linalg.norm(dcr, axis=-1) + dlen) / length + 4 * U, 0.0)
    V = np.stack([X * dc, Y * dc, dc], -1)
    facing = np.sum(n * V, -1)
    dfacing = err * np.sum(np.abs(V), -1) + 4 * U * np.sum(np.abs(n * V), -1)
    amb |= ok & (np.abs(facing) <= dfacing)
    n = np.where((facing > 0.0)[..., None], -n, n)
    usable[c], ambiguous[c], bound[c] = ok, amb & ok_before, err
    vn[c] = np.where(ok[..., None], np.concatenate([n, dc[..., None]], -1), 0.0)
    return dict(vnmap=vn, usable=usable, ambiguous=ambiguous, bound=bound)


# -------------------------------------------------------------------------------------------------------------------- step
def relative_transform(model_view, view_in):
    """rel = T_model T_in^-1 formed in float64 from the two fp32 matrices and rounded once to fp32 (R [3,3], t [3] as float64)"""
    Rm, tm = pose_of(model_view)
    Ri, ti = pose_of(view_in)
    R = Rm @ Ri.T
    return R.astype(np.float32).astype(np.float64), (tm - R @ ti).astype(np.float32).astype(np.float64)


def _terms(J, dJ, r, dr, w, dw):
    """[S,28] terms and bounds: A's upper triangle row-major, b, w r^2"""
    terms, bounds = [], []
    for i in range(6):
        for j in range(i, 6):
            terms.append(w * J[:, i] * J[:, j])
            bounds.append(np.abs(J[:, i] * J[:, j]) * dw + w * (np.abs(J[:, j]) * dJ[:, i] + np.abs(J[:, i]) * dJ[:, j]) +
                          2 * U * np.abs(terms[-1]))
    for i in range(6):
        terms.append(w * J[:, i] * r)
        bounds.append(np.abs(J[:, i] * r) * dw + w * (np.abs(r) * dJ[:, i] + np.abs(J[:, i]) * dr) + 2 * U * np.abs(terms[-1]))
    terms.append(w * r * r)
    bounds.append(r * r * dw + 2 * w * np.abs(r) * dr + 2 * U * terms[-1])
    return np.stack(terms, 1), np.stack(bounds, 1)


def icp_step_model(depth_obs, vn_obs, vn_model, model_view, view_in, fx, fy, cx, cy, *, stride=1, depth_range=(0.0, INF),
                   dist_max=0.1, normal_cos_min=0.8, huber_delta=INF, mutate=None):
    """depth_obs [H,W] float32, vn_obs [H,W,4] float32 or None, vn_model [H,W,4] float32 (the maps the kernel is given), the two
    poses [4,4] float32.  Returns a dict: flags uint8 [S], ambiguous bool [S], terms and bounds float64 [S,28] (rows of candidates
    that are nowhere inside are zero), S; `sums(selection)` evaluates the 28 sums, their bounds B and sum |term| over any set.
    `mutate`: one of the deliberately wrong models ("cross_sign", "transpose_rotation", "ignore_w", "drop_block")."""
    depth_obs = np.asarray(depth_obs, np.float32)
    vn_model = np.asarray(vn_model, np.float32)
    H, W = depth_obs.shape
    fx, fy, cx, cy, dmax, cmin, delta = (f32(v) for v in (fx, fy, cx, cy, dist_max, normal_cos_min, huber_delta))
    ifx, ify = f32(1.0 / fx), f32(1.0 / fy)
    lo, hi = np.float32(depth_range[0]), np.float32(depth_range[1])
    x, y = candidates(W, H, stride)
    S = len(x)
    d32 = depth_obs[y, x]
    with np.errstate(invalid="ignore"):
        valid = (d32 > lo) & (d32 < hi)
    no = None
    if vn_obs is not None:
        vo = np.asarray(vn_obs, np.float32)[y, x]
        with np.errstate(invalid="ignore"):
            valid &= vo[:, 3] > 0
        no = np.where(valid[:, None], vo[:, :3], 0.0).astype(np.float64)
    d = np.where(valid, d32, 1.0).astype(np.float64)
    R, t = relative_transform(model_view, view_in)
    if mutate == "transpose_rotation":
        R = R.T
    p = np.stack([(x - cx) * ifx * d, (y - cy) * ify * d, d], 1)
    q = p @ R.T + t
    dq = 8 * U * (np.abs(p) @ np.abs(R).T + np.abs(t))
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = fx * q[:, 0] / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy
        du = fx / np.abs(q[:, 2]) * (dq[:, 0] + np.abs(q[:, 0] / q[:, 2]) * dq[:, 2]) + 4 * U * (np.abs(u - cx) + abs(cx) + 0.5)
        dv = fy / np.abs(q[:, 2]) * (dq[:, 1] + np.abs(q[:, 1] / q[:, 2]) * dq[:, 2]) + 4 * U * (np.abs(v - cy) + abs(cy) + 0.5)
    front = q[:, 2] > 0.0
    amb_front = np.abs(q[:, 2]) <= dq[:, 2]
    ok_uv = valid & front & np.isfinite(u) & np.isfinite(v)
    uh, vh = np.where(ok_uv, u + 0.5, 0.5), np.where(ok_uv, v + 0.5, 0.5)
    px, py = np.floor(uh), np.floor(vh)
    near_x, near_y = ok_uv & (np.abs(uh - np.rint(uh)) <= du), ok_uv & (np.abs(vh - np.rint(vh)) <= dv)
    px_alt, py_alt = np.where(uh - px < 0.5, px - 1, px + 1), np.where(vh - py < 0.5, py - 1, py + 1)

    def pair(px, py):
        in_image = ok_uv & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        m32 = vn_model[np.clip(py, 0, H - 1).astype(np.int64), np.clip(px, 0, W - 1).astype(np.int64)]
        with np.errstate(invalid="ignore"):
            inside = in_image & (m32[:, 3] > 0)
        m = np.where(inside[:, None], m32, 0.0).astype(np.float64)
        n, dm = m[:, :3], m[:, 3]
        vm = np.stack([(px - cx) * ifx * dm, (py - cy) * ify * dm, dm], 1)
        dvm = 4 * U * np.abs(vm) * np.array([1.0, 1.0, 0.0])
        e = q - vm
        de = dq + dvm + U * np.abs(e)
        dist = np.linalg.norm(e, axis=1)
        ddist = np.linalg.norm(de, axis=1) + 3 * U * dist
        associated = inside & (dist <= dmax)
        amb = inside & (np.abs(dist - dmax) <= ddist)
        if no is not None:
            rn = no @ R.T
            cosine = np.sum(rn * n, 1)
            dcos = np.sum(np.abs(n) * (3 * U * (np.abs(no) @ np.abs(R).T)), 1) + 3 * U * np.sum(np.abs(rn * n), 1)
            associated &= cosine >= cmin
            amb |= inside & (np.abs(cosine - cmin) <= dcos)
        r = np.sum(n * e, 1)
        dr = np.sum(np.abs(n) * de, 1) + 3 * U * np.sum(np.abs(n * e), 1)
        Jr = np.cross(q, n)
        if mutate == "cross_sign":
            Jr = -Jr
        aq, an = np.abs(q), np.abs(n)
        dJr = np.stack([an[:, 2] * dq[:, 1] + an[:, 1] * dq[:, 2] + 2 * U * (aq[:, 1] * an[:, 2] + aq[:, 2] * an[:, 1]),
                        an[:, 0] * dq[:, 2] + an[:, 2] * dq[:, 0] + 2 * U * (aq[:, 2] * an[:, 0] + aq[:, 0] * an[:, 2]),
                        an[:, 1] * dq[:, 0] + an[:, 0] * dq[:, 1] + 2 * U * (aq[:, 0] * an[:, 1] + aq[:, 1] * an[:, 0])], 1)
        J, dJ = np.concatenate([Jr, n], 1), np.concatenate([dJr, np.zeros_like(n)], 1)
        ar = np.abs(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(ar <= delta, 1.0, delta / ar)
            dw = np.where((ar >= delta - dr) & (ar > 0), np.minimum(w, 1.0) * (dr / ar + U), 0.0)
        if mutate == "ignore_w":
            w, dw = np.ones_like(w), np.zeros_like(w)
        terms, bounds = _terms(J, dJ, r, dr, w, dw)
        keep = inside[:, None]
        return inside, associated, amb, np.where(keep, terms, 0.0), np.where(keep, bounds, 0.0)

    inside, associated, amb, terms, bounds = pair(px, py)
    # a landing position within its error of a pixel's edge: the neighbouring pixel may be the one read
    for near, ax, ay in ((near_x, px_alt, py), (near_y, px, py_alt), (near_x & near_y, px_alt, py_alt)):
        if near.any():
            in2, _, _, t2, b2 = pair(np.where(near, ax, px), np.where(near, ay, py))
            use = near & in2
            swap = use & ~inside  # (the model's own pixel is outside or empty: the neighbour's term stands in)
            change = np.where((use & inside)[:, None], np.abs(t2 - terms) + b2, 0.0)
            terms = np.where(swap[:, None], t2, terms)
            bounds = np.where(swap[:, None], b2, np.maximum(bounds, change + np.where(use[:, None], bounds, 0.0)))
    ambiguous = valid & (amb_front | near_x | near_y | amb)
    flags = (valid * VALID + inside * INSIDE + associated * ASSOCIATED).astype(np.uint8)
    block_kept = np.arange(S) >= BLOCK if mutate == "drop_block" else np.ones(S, bool)

    def sums(selection=None):
        """(the 29 sums, B [28], sum |term| [28]) over `selection` (bool [S]; None: the model's own associated set)"""
        sel = (associated if selection is None else np.asarray(selection, bool)) & block_kept
        return (np.concatenate([terms[sel].sum(0), [float(sel.sum())]]), bounds[sel].sum(0), np.abs(terms[sel]).sum(0))

    return dict(flags=flags, ambiguous=ambiguous, terms=terms, bounds=bounds, S=S, sums=sums, valid=int(valid.sum()),
                associated=associated)


def unpack(sums29):
    """(A [6,6], b [6], sum w r^2, count) of the 29 sums"""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums29[:21]
    A = A + np.triu(A, 1).T
    return A, np.asarray(sums29[21:27], np.float64), float(sums29[27]), float(sums29[28])


def solve(sums29, *, damping=0.0, rcond=1e-8, min_points=6):
    """The finisher's solve in float64, the one every pose step's model uses: M xi = -b by LDL^T, M = A damped, and the refusals.
    Returns ok, xi [6] (zeros when refused), cond (of A; inf when singular), cond_solved (of the damped matrix the solve
    factorises)."""
    sums29 = np.asarray(sums29, np.float64)
    A, b, _, count = unpack(sums29)
    damping, rcond = f32(damping), f32(rcond)
    ok = count >= min_points and bool(np.all(np.isfinite(sums29[:28])))
    diag = np.diag(A).copy()
    max_diag = max(0.0, float(diag.max())) if ok else 0.0
    M = A + damping * np.diag(np.maximum(diag, DAMPING_FLOOR * max_diag))
    L, D = np.eye(6), np.zeros(6)
    xi = np.zeros(6)
    with np.errstate(all="ignore"):
        for j in range(6):
            D[j] = M[j, j] - np.sum(L[j, :j] ** 2 * D[:j])
            ok = ok and bool(D[j] > rcond * max_diag and D[j] > 0.0)
            for i in range(j + 1, 6):
                L[i, j] = (M[i, j] - np.sum(L[i, :j] * L[j, :j] * D[:j])) / D[j]
        if ok:
            z = np.linalg.solve(L, -b)
            xi = np.linalg.solve(L.T, z / D)
            ok = bool(np.all(np.isfinite(xi)))
        eig = np.linalg.eigvalsh(A) if np.all(np.isfinite(A)) else np.array([0.0, 1.0])
        cond = float(eig[-1] / eig[0]) if eig[0] > 0 else INF
        eig = np.linalg.eigvalsh(M) if np.all(np.isfinite(M)) else np.array([0.0, 1.0])
        cond_solved = float(eig[-1] / eig[0]) if eig[0] > 0 else INF
    return ok, xi if ok else np.zeros(6), cond, cond_solved


def solve_update(sums29, model_view, view_in, *, mutate=None, **kw):
    """The finisher in float64: `solve` (its keywords), the update.  Returns a dict: ok, xi [6], cond, cond_solved (solve's),
    viewmatrix float32 [4,4], quat float32 [4], trans float32 [3], omega, v (the norms; 0 when refused),
    branch (Shepperd's, of the rotation whose quaternion is returned).  `mutate`: one of POSE_MUTANTS, the deliberately wrong
    finishers (rotation_to_quat's and se3_exp's)."""
    ok, xi, cond, cond_solved = solve(sums29, **kw)
    Ri, ti = pose_of(view_in)
    view_in = np.asarray(view_in, np.float32).reshape(4, 4)
    if ok:
        Rm, tm = pose_of(model_view)
        Re, te = se3_exp(-xi, mutate)
        R1, t1 = Re @ Rm, Re @ tm + te
        R2, t2 = Rm.T @ R1, Rm.T @ (t1 - tm)
        Ro, to = Ri @ R2, Ri @ t2 + ti
        quat, branch = rotation_to_quat(Ro, mutate), quat_branch(Ro)
        view, trans = w2ct(quat_to_rotation(quat), to), to.astype(np.float32)
    else:
        quat, branch, view, trans = rotation_to_quat(Ri, mutate), quat_branch(Ri), view_in.copy(), view_in[3, :3].copy()
    return dict(ok=ok, xi=xi, cond=cond, cond_solved=cond_solved, viewmatrix=view, quat=quat.astype(np.float32), trans=trans,
                omega=float(np.linalg.norm(xi[:3])), v=float(np.linalg.norm(xi[3:])), branch=branch)


ULP = 2.0 ** -23  # of 1.0


def pose_figures(view, quat, trans, want):
    """A finisher's pose (float32 viewmatrix [4,4], quat [4], trans [3]) against solve_update's `want` of the same sums, as
    figures: ulps [4,4] of the viewmatrix in the ulp of want's entries and the `allowed` number of them, rot (the largest
    |R(quat) - R| against the viewmatrix's own rotation), norm (|quat|), r (quat[0]), trans_bits (trans carries the viewmatrix's
    translation row bit for bit), last_column (0, 0, 0, 1 where the step was accepted).
    Both sides are float64: they differ by the solve's rounding, the factorised matrix's condition number (A's without damping)
    times 2^-53 times a small constant (16 here) relative to xi, which is at most of order 1 against matrix entries of order 1 --
    in fp32 ulps of an entry 16 cond(A) 2^-29, nothing at cond(A) <= 1e3 and 0.03 ulp at 1e6 -- on top of the 2 ulp that the two
    roundings to fp32 may differ by.  A refused step carries the input's bits: no tolerance."""
    view, quat, trans = (np.asarray(a, np.float32) for a in (view, quat, trans))
    ulps = np.abs(view.astype(np.float64) - want["viewmatrix"]) / np.spacing(np.abs(want["viewmatrix"]) + np.float32(1e-30))
    allowed = 2.0 + 16.0 * want["cond_solved"] * 2.0 ** -29 if want["ok"] else 0.0
    R = quat_to_rotation(quat.astype(np.float64))
    return dict(ulps=ulps, allowed=allowed, rot=float(np.abs(R - view.astype(np.float64)[:3, :3].T).max()),
                norm=float(np.linalg.norm(quat.astype(np.float64))), r=float(quat[0]),
                trans_bits=bool(np.array_equal(trans.view(np.uint32), view[3, :3].view(np.uint32))),
                last_column=view[:, 3].tolist() == [0.0, 0.0, 0.0, 1.0] or not want["ok"])


def pose_holds(fig):
    """the standard the figures are held to: check_pose's (tests/test_hip_icp.py)"""
    return bool((fig["ulps"] <= fig["allowed"]).all() and fig["last_column"] and fig["rot"] <= 4 * ULP and
                abs(fig["norm"] - 1.0) <= 2 * ULP and fig["r"] >= 0 and fig["trans_bits"])


def icp_align_model(depth_obs, model_depth, viewmatrix, model_viewmatrix, fx, fy, cx, cy, *, iterations=10, strides=None,
                    opacity_map=None, silhouette_threshold=0.99, depth_range=(0.0, INF), max_jump=0.1, dist_max=0.1,
                    normal_cos_min=0.8, use_obs_normals=True, huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6):
    """slam.icp_align in float64 (the maps rounded to fp32, as the kernel's are).  Returns a dict: viewmatrix, quat, trans, and per
    iteration: ok, count, marked (the number of ambiguous candidates)."""
    strides = (1,) * iterations if strides is None else tuple(strides)
    kw = dict(depth_range=depth_range, max_jump=max_jump)
    vn_model = depth_normals_model(model_depth, fx, fy, cx, cy, mask_image=opacity_map, mask_threshold=silhouette_threshold,
                                   **kw)["vnmap"].astype(np.float32)
    vn_obs = depth_normals_model(depth_obs, fx, fy, cx, cy, **kw)["vnmap"].astype(np.float32) if use_obs_normals else None
    view = np.asarray(model_viewmatrix if viewmatrix is None else viewmatrix, np.float32).reshape(4, 4)
    oks, counts, marked = [], [], []
    out = None
    for stride in strides:
        m = icp_step_model(depth_obs, vn_obs, vn_model, model_viewmatrix, view, fx, fy, cx, cy, stride=stride,
                           depth_range=depth_range, dist_max=dist_max, normal_cos_min=normal_cos_min, huber_delta=huber_delta)
        s29, _, _ = m["sums"]()
        out = solve_update(s29, model_viewmatrix, view, damping=damping, rcond=rcond, min_points=min_points)
        view = out["viewmatrix"]
        oks.append(out["ok"]), counts.append(int(s29[28])), marked.append(int(m["ambiguous"].sum()))
    return dict(viewmatrix=view, quat=out["quat"], trans=out["trans"], ok=oks, count=counts, marked=marked)
