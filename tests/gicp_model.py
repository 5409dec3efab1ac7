"""Generalized ICP as include/dgr_hip.h defines it (dgr_point_covariances, dgr_gicp_step) and slam.gicp_align, restated in
float64 numpy on the CPU.  Written from that text.  Beside each result it returns what a comparison with the kernels needs.

Covariances.  Kernel and model run the same rule in double, so they differ by the roundings of double arithmetic alone and by
the one rounding to fp32 of each output.  With n neighbours and m = max |p| over the neighbourhood, u = 2^-53:
  mu      n additions and a division                               (n + 1) u m per component
  d       = p - mu, |d| <= 2 m                                     (n + 2) u m
  d_a d_b two factors' errors and the product's rounding           4 (n + 2) u m^2 + 4 u m^2
  C_ab    n such terms added and divided by n                      + 4 (n + 1) u m^2           => (8 n + 16) u m^2
and as much again for the model's own double arithmetic.  A RAW entry's bound is therefore U32 |C_ab| + 2 (8 n + 16) u m^2.
What depends on the normal v_0 (PLANE rows, normals, the frame) is determined by C only as well as the gap lambda_1 - lambda_0
allows: dv_0 <= 2 dC / (lambda_1 - lambda_0) (first-order perturbation of a simple eigenvector, dC the Frobenius size of the
bound above, doubled for the Jacobi rotations' own roundings).  A row is MARKED (`ambiguous`) when that exceeds a quarter of an
fp32 ulp of 1, i.e. when v_0 is not determined at fp32 resolution, or when the orientation test's dot product is within its
error of zero; tests may leave out marked rows (at most 1 %).  A PLANE entry's bound is U32 |entry| + 2 dv_0, a normal's
U32 |v| + dv_0.

Step.  The association is the kNN twin's (tests/knn_model.py) on the float32 twin of the transform: no tolerance.  Per pair the
terms are polynomials of degree <= 2 in q, linear in M = C^-1 and in e, about 20 operations each, on top of M's own error,
which the adjugate's cancellations put at 16 cond(C) u relative to |M|.  With mag the size of a term's products before any
cancellation -- w |M| (|q| + 1)^2 for A, w |M| (|q| + 1) |e| for b, w s^2 -- and N pairs added in another order than the
model's (N u sum |term| each way), the bound of a sum is (2 N + 32 + 16 max cond(C)) u sum mag.  Huber's weight is continuous
at s = huber_delta, so a pair within rounding of the switch changes a term by less than that and needs no mark.
Solve and update: icp_model's figures (pose_figures, pose_holds) on the model fed the kernel's own sums.
"""
import numpy as np

import icp_model as im
import knn_model as km

U32 = 2.0 ** -24
U64 = 2.0 ** -53
VALID, ASSOCIATED, SINGULAR = 1, 2, 4
RAW, PLANE = 0, 1
SWEEPS = 16
BLOCK = 2048
INF = float("inf")
COV_MUTANTS = ("n_minus_1",)
STEP_MUTANTS = ("transpose_rotation", "drop_source_cov", "skew_sign")
UPDATE_MUTANTS = ("right_update",)


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------- covariances
def neighbourhood_sizes(idx, P):
    """n per row: the leading entries in [0, P)"""
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < P)
    return np.where(ok.all(1), idx.shape[1], np.argmin(ok, axis=1)).astype(np.int64)


def jacobi_eigen(C):
    """[P,3,3] symmetric -> (diag [P,3], V [P,3,3]) by the header's cyclic Jacobi: pairs (0,1), (0,2), (1,2), 16 sweeps at most"""
    A, P = np.array(C, np.float64), len(C)
    V = np.tile(np.eye(3), (P, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            off = (A[:, 0, 1] != 0) | (A[:, 0, 2] != 0) | (A[:, 1, 2] != 0)
            if not off.any():
                break
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = A[:, p, q].copy()
                act = off & (apq != 0)
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * np.where(act, apq, 1.0))
                t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                t, c, s = np.where(act, t, 0.0), np.where(act, c, 1.0), np.where(act, s, 0.0)
                A[:, p, p] = A[:, p, p] - t * apq
                A[:, q, q] = A[:, q, q] + t * apq
                A[:, p, q] = A[:, q, p] = np.where(act, 0.0, apq)
                arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                A[:, r, p] = A[:, p, r] = c * arp - s * arq
                A[:, r, q] = A[:, q, r] = s * arp + c * arq
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = c[:, None] * vp - s[:, None] * vq
                V[:, :, q] = s[:, None] * vp + c[:, None] * vq
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1), V


def _sorted_pairs(lam, V):
    """ascending, ties keeping column order: the kernel's three compare-and-swaps (0,1), (1,2), (0,1)"""
    lam, V = lam.copy(), V.copy()
    for a, b in ((0, 1), (1, 2), (0, 1)):
        sw = lam[:, a] > lam[:, b]
        la, lb = lam[:, a].copy(), lam[:, b].copy()
        lam[:, a], lam[:, b] = np.where(sw, lb, la), np.where(sw, la, lb)
        va, vb = V[:, :, a].copy(), V[:, :, b].copy()
        V[:, :, a], V[:, :, b] = np.where(sw[:, None], vb, va), np.where(sw[:, None], va, vb)
    return lam, V


def covariances_model(points, idx, *, mode=PLANE, epsilon=1e-3, min_neighbours=4, scale_floor=1e-4, viewpoint=None, mutate=None):
    """points [P,3] float32, idx [P,k] int.  Returns a dict of float64 arrays: valid bool [P], n [P], C [P,3,3] (the covariance),
    lam [P,3] ascending, V [P,3,3] their columns, cov [P,8] (the packed row before its rounding), cov_bound [P,6], sigma_bound [P],
    normals [P,4],
    normal_bound [P], log_scales [P,3], frame [P,3,3] (columns v_2, +-v_1, oriented v_0; det +1), quats [P,4], ambiguous bool [P]
    (v_0 or its orientation not determined at fp32 resolution), gap [P] = (lambda_1 - lambda_0) / lambda_2.
    `mutate`: "n_minus_1" (the sample covariance: a deliberately wrong model)."""
    pts32 = np.ascontiguousarray(points, np.float32)
    P, idx = len(pts32), np.asarray(idx, np.int64)
    k = idx.shape[1]
    n = neighbourhood_sizes(idx, P)
    slot = np.arange(k)[None, :] < n[:, None]
    safe = np.where(slot, idx, 0)
    finite = np.isfinite(pts32).all(1)
    valid = finite & np.where(slot, finite[safe], True).all(1) & (n >= min_neighbours)
    pts = np.where(finite[:, None], pts32, 0.0).astype(np.float64)
    nb = np.where(slot[:, :, None], pts[safe], 0.0)  # [P,k,3]
    dn = np.maximum(n, 1).astype(np.float64)
    mu = np.zeros((P, 3))
    for s in range(k):  # in the row's order
        mu = mu + nb[:, s]
    mu = mu / dn[:, None]
    C = np.zeros((P, 3, 3))
    for s in range(k):
        d = np.where(slot[:, s, None], nb[:, s] - mu, 0.0)
        C = C + d[:, :, None] * d[:, None, :]
    C = C / (np.maximum(dn - 1.0, 1.0) if mutate == "n_minus_1" else dn)[:, None, None]
    C = np.where(valid[:, None, None], C, 0.0)
    lam, V = jacobi_eigen(C)
    lam, V = _sorted_pairs(np.maximum(lam, 0.0), V)
    valid = valid & (lam[:, 2] > 0) & np.isfinite(lam[:, 2])
    z = lambda a: np.where(valid.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0.0)  # noqa: E731
    with np.errstate(all="ignore"):
        sigma = z(lam[:, 0] / ((lam[:, 0] + lam[:, 1]) + lam[:, 2]))
        gap = z((lam[:, 1] - lam[:, 0]) / lam[:, 2])
        m = np.where(slot, np.abs(nb).max(2), 0.0).max(1)
        dC = 2.0 * (8.0 * n + 16.0) * U64 * m * m
        dv0 = np.where(valid, 2.0 * 3.0 * dC / np.maximum(lam[:, 1] - lam[:, 0], 1e-300) + 8 * U64, 0.0)
    v0 = V[:, :, 0].copy()
    if viewpoint is not None:
        vp = np.array([f32(v) for v in viewpoint])
        dot = np.sum(v0 * (vp[None, :] - pts), 1)
        ddot = dv0 * np.abs(vp[None, :] - pts).sum(1) + 8 * U64 * np.abs(v0 * (vp[None, :] - pts)).sum(1)
        flip, amb_o = dot < 0.0, np.abs(dot) <= ddot
    else:
        av = np.abs(v0)
        first = np.where((av[:, 0] >= av[:, 1]) & (av[:, 0] >= av[:, 2]), 0, np.where(av[:, 1] >= av[:, 2], 1, 2))
        lead = np.take_along_axis(v0, first[:, None], 1)[:, 0]
        flip = lead < 0.0
        srt = np.sort(av, 1)
        amb_o = (srt[:, 2] - srt[:, 1] <= 2 * dv0) | (np.abs(lead) <= dv0)
    v0 = np.where(flip[:, None], -v0, v0)
    ambiguous = valid & ((dv0 > 0.25 * 2.0 ** -23) | amb_o)
    if mode == PLANE:
        g = 1.0 - f32(epsilon)
        six = np.stack([1.0 - g * v0[:, 0] * v0[:, 0], -(g * v0[:, 0] * v0[:, 1]), -(g * v0[:, 0] * v0[:, 2]),
                        1.0 - g * v0[:, 1] * v0[:, 1], -(g * v0[:, 1] * v0[:, 2]), 1.0 - g * v0[:, 2] * v0[:, 2]], 1)
        cov_bound = U32 * np.abs(six) + 2.0 * dv0[:, None]
    else:
        six = np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1)
        cov_bound = U32 * np.abs(six) + dC[:, None]
    cov = z(np.concatenate([six, sigma[:, None], n[:, None].astype(np.float64)], 1))
    normals = z(np.concatenate([v0, sigma[:, None]], 1))
    floor2 = f32(scale_floor) ** 2
    with np.errstate(all="ignore"):
        log_scales = z(0.5 * np.log(np.maximum(lam[:, ::-1], floor2)))
    frame = np.stack([V[:, :, 2], V[:, :, 1], v0], 2)
    neg = np.linalg.det(frame) < 0
    frame[:, :, 1] = np.where(neg[:, None], -frame[:, :, 1], frame[:, :, 1])
    quats = np.zeros((P, 4))
    for i in np.flatnonzero(valid):
        quats[i] = im.rotation_to_quat(frame[i])
    with np.errstate(all="ignore"):  # sigma = lambda_0 / trace: lambda_0 carries C's error (Frobenius 3 dC), the quotient one rounding
        sigma_bound = z(U32 * sigma + 8.0 * 3.0 * dC / np.where(valid, lam.sum(1), 1.0))
    return dict(valid=valid, n=n, C=C, lam=z(lam), V=V, cov=cov, cov_bound=z(cov_bound), sigma_bound=sigma_bound, normals=normals,
                normal_bound=z(U32 + dv0), log_scales=log_scales, frame=z(frame), quats=quats, ambiguous=ambiguous, gap=gap,
                sigma=sigma)


def pack_cov(C, n=1.0, sigma=0.0):
    """[P,3,3] -> the packed float32 rows [P,8]"""
    C = np.asarray(C, np.float64)
    P = len(C)
    rows = np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2], np.broadcast_to(sigma, (P,)),
                     np.broadcast_to(n, (P,))], 1)
    return np.ascontiguousarray(rows, np.float32)


def unpack_cov(rows):
    """packed rows [P,8] (float32) -> (C [P,3,3] float64, valid bool [P])"""
    r = np.asarray(rows, np.float32).astype(np.float64)
    C = np.stack([r[:, [0, 1, 2]], r[:, [1, 3, 4]], r[:, [2, 4, 5]]], 1)
    with np.errstate(invalid="ignore"):
        return C, r[:, 7] > 0


# -------------------------------------------------------------------------------------------------------------------- step
def motion_of(T):
    """(R, t) float64 of 16 floats holding the motion transposed, the translation at [12..14]"""
    return im.pose_of(T)


def as_transform(R, t):
    return im.w2ct(R, t)


def transform32(T, source):
    """the float32 twin of gicp_transform_kernel: q_j = ((R_j0 a_0 + R_j1 a_1) + R_j2 a_2) + t_j, every operation rounded once"""
    T = np.asarray(T, np.float32).reshape(16)
    a = np.ascontiguousarray(source, np.float32)
    q = np.empty_like(a)
    with np.errstate(all="ignore"):
        for j in range(3):
            x = T[j] * a[:, 0]
            y = T[4 + j] * a[:, 1]
            z = T[8 + j] * a[:, 2]
            q[:, j] = ((x + y) + z) + T[12 + j]
    assert q.dtype == np.float32
    return q


def max_dist2(dist_max):
    """the fp32 product dist_max * dist_max"""
    with np.errstate(over="ignore"):
        return np.float32(dist_max) * np.float32(dist_max)


def associate(target, q, dist_max):
    """idx int32 [S]: the kNN twin's answer for k = 1 in cross mode"""
    return km.knn32(target, q, k=1, max_dist2=max_dist2(dist_max))[1][:, 0]


def skew(q):
    o = np.zeros(len(q))
    return np.stack([np.stack([o, -q[:, 2], q[:, 1]], 1), np.stack([q[:, 2], o, -q[:, 0]], 1), np.stack([-q[:, 1], q[:, 0], o], 1)], 1)


def gicp_step_model(target, target_cov, source, source_cov, T, *, dist_max=INF, huber_delta=INF, idx=None, mutate=None):
    """target [N,3], source [S,3] float32; target_cov [N,8], source_cov [S,8] float32 or None; T the motion (16 floats).
    Returns a dict: q float32 [S,3] (the twin's), idx int32 [S], flags uint8 [S], terms and mags float64 [S,28] (zero rows for
    pairs that take no part), cond_max, and `sums(selection=None)` -> (the 29 sums, the bound [28]).  `idx`: an association to use
    in place of the twin's.  `mutate`: one of STEP_MUTANTS, the deliberately wrong models."""
    target, source = np.ascontiguousarray(target, np.float32), np.ascontiguousarray(source, np.float32)
    S, N = len(source), len(target)
    q32 = transform32(T, source)
    idx = associate(target, q32, dist_max) if idx is None else np.asarray(idx, np.int32)
    R, _ = motion_of(T)
    valid = np.isfinite(q32).all(1)
    CA = np.zeros((S, 3, 3))
    if source_cov is not None:
        CA, ok = unpack_cov(source_cov)
        valid &= ok
    j = np.where((idx >= 0) & (idx < N), idx, 0)
    associated = valid & (idx >= 0) & (idx < N)
    CB = np.zeros((S, 3, 3))
    if target_cov is not None:
        CBt, ok = unpack_cov(target_cov)
        CB = CBt[j]
        associated &= ok[j]
    q = np.where(associated[:, None], q32, 0.0).astype(np.float64)
    b = np.where(associated[:, None], target[j], 0.0).astype(np.float64)
    e = q - b
    Rc = R.T if mutate == "transpose_rotation" else R
    if source_cov is not None and mutate != "drop_source_cov":
        C = CB + Rc[None] @ CA @ Rc.T[None]
    elif target_cov is not None or source_cov is not None:
        C = CB.copy()
    else:
        C = np.tile(np.eye(3), (S, 1, 1))
    C = np.where(associated[:, None, None], C, np.eye(3)[None])
    c00, c01, c02, c11, c12, c22 = C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]
    a00, a01, a02 = c11 * c22 - c12 * c12, c02 * c12 - c01 * c22, c01 * c12 - c02 * c11
    a11, a12, a22 = c00 * c22 - c02 * c02, c01 * c02 - c00 * c12, c00 * c11 - c01 * c01
    det = (c00 * a00 + c01 * a01) + c02 * a02
    with np.errstate(all="ignore"):
        singular = associated & ~((det > 0) & np.isfinite(det))
        used = associated & ~singular
        sd = np.where(used, det, 1.0)
        M = np.stack([np.stack([a00, a01, a02], 1), np.stack([a01, a11, a12], 1), np.stack([a02, a12, a22], 1)], 1) / sd[:, None, None]
        M = np.where(used[:, None, None], M, 0.0)
        g = np.einsum("sab,sb->sa", M, e)
        s2 = np.maximum(np.einsum("sa,sa->s", e, g), 0.0)
        s = np.sqrt(s2)
        delta = f32(huber_delta)
        w = np.where(s <= delta, 1.0, delta / np.where(s > 0, s, 1.0))
        eig = np.linalg.eigvalsh(np.where(used[:, None, None], C, np.eye(3)[None]))
        cond_max = float(np.max(np.where(used, eig[:, 2] / np.maximum(eig[:, 0], 1e-300), 1.0))) if S else 1.0
    J = np.concatenate([(1.0 if mutate == "skew_sign" else -1.0) * skew(q), np.tile(np.eye(3), (S, 1, 1))], 2)  # [S,3,6]
    A = np.einsum("sai,sab,sbj->sij", J, M, J) * w[:, None, None]
    bb = np.einsum("sai,sa->si", J, g) * w[:, None]
    iu = np.triu_indices(6)
    terms = np.concatenate([A[:, iu[0], iu[1]], bb, (w * s2)[:, None]], 1)
    Mn = np.abs(M).sum((1, 2))
    ql, el = np.abs(q).sum(1) + 1.0, np.abs(e).sum(1)
    mags = np.concatenate([np.repeat((w * Mn * ql * ql)[:, None], 21, 1), np.repeat((w * Mn * ql * el)[:, None], 6, 1),
                           (w * s2)[:, None]], 1)
    terms, mags = np.where(used[:, None], terms, 0.0), np.where(used[:, None], mags, 0.0)
    flags = (valid * VALID + associated * ASSOCIATED + singular * SINGULAR).astype(np.uint8)

    def sums(selection=None):
        sel = used if selection is None else (np.asarray(selection, bool) & used)
        count = float(sel.sum())
        bound = (2.0 * count + 32.0 + 16.0 * cond_max) * U64 * mags[sel].sum(0)
        return np.concatenate([terms[sel].sum(0), [count]]), bound

    return dict(q=q32, idx=idx.astype(np.int32), flags=flags, terms=terms, mags=mags, used=used, cond_max=cond_max, sums=sums, S=S)


def solve_update(sums29, T_in, *, mutate=None, **kw):
    """The finisher in float64: icp_model.solve (its keywords), the update T_out = exp(xi) T_in.  Returns icp_model.solve_update's
    dict (`viewmatrix` is the motion, float32 [4,4]), so that icp_model.pose_figures and pose_holds apply.
    `mutate`: "right_update" (T_in exp(xi): a deliberately wrong model)."""
    ok, xi, cond, cond_solved = im.solve(sums29, **kw)
    Ri, ti = motion_of(T_in)
    T_in = np.asarray(T_in, np.float32).reshape(4, 4)
    if ok:
        Re, te = im.se3_exp(xi)
        Ro, to = (Ri @ Re, Ri @ te + ti) if mutate == "right_update" else (Re @ Ri, Re @ ti + te)
        quat, branch = im.rotation_to_quat(Ro), im.quat_branch(Ro)
        out, trans = as_transform(im.quat_to_rotation(quat), to), to.astype(np.float32)
    else:
        quat, branch, out, trans = im.rotation_to_quat(Ri), im.quat_branch(Ri), T_in.copy(), T_in[3, :3].copy()
    return dict(ok=ok, xi=xi, cond=cond, cond_solved=cond_solved, viewmatrix=out, quat=quat.astype(np.float32), trans=trans,
                omega=float(np.linalg.norm(xi[:3])), v=float(np.linalg.norm(xi[3:])), branch=branch)


def gicp_align_model(source, target, *, transform=None, source_cov=None, target_cov=None, iterations=15, dist_max=INF,
                     huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6, mutate=None):
    """slam.gicp_align in float64.  Returns a dict: transform float32 [4,4], quat, trans, and per iteration ok, count, cond."""
    T = np.eye(4, dtype=np.float32) if transform is None else np.asarray(transform, np.float32).reshape(4, 4).copy()
    oks, counts, conds, out = [], [], [], None
    for _ in range(iterations):
        m = gicp_step_model(target, target_cov, source, source_cov, T, dist_max=dist_max, huber_delta=huber_delta,
                            mutate=mutate if mutate in STEP_MUTANTS else None)
        s29, _ = m["sums"]()
        out = solve_update(s29, T, damping=damping, rcond=rcond, min_points=min_points,
                           mutate=mutate if mutate in UPDATE_MUTANTS else None)
        T = out["viewmatrix"]
        oks.append(out["ok"]), counts.append(int(s29[28])), conds.append(out["cond"])
    return dict(transform=T, quat=out["quat"], trans=out["trans"], ok=oks, count=counts, cond=conds)


def transform_error(T, T_true):
    """(rotation angle between the two motions in rad, distance between their translations)"""
    R, t = motion_of(T)
    Rt, tt = motion_of(T_true)
    D = R @ Rt.T
    sine = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(sine, 0.5 * (np.trace(D) - 1.0))), float(np.linalg.norm(t - tt))


# ------------------------------------------------------------------------------------------------------------------ scenes
def unproject32(depth, fx, fy, cx, cy, stride=1, depth_range=(0.0, INF)):
    """the float32 twin of slam.unproject_depth: ((x - cx) / fx * d, (y - cy) / fy * d, d), NaN rows for unusable pixels"""
    d = np.asarray(depth, np.float32)[::stride, ::stride]
    H, W = d.shape
    x = (np.arange(W, dtype=np.float32) * np.float32(stride))[None, :]
    y = (np.arange(H, dtype=np.float32) * np.float32(stride))[:, None]
    with np.errstate(invalid="ignore"):
        ok = (d > np.float32(depth_range[0])) & (d < np.float32(depth_range[1]))
        d = np.where(ok, d, np.float32(np.nan))
        X = (x - np.float32(cx)) / np.float32(fx) * d
        Y = (y - np.float32(cy)) / np.float32(fy) * d
    return np.ascontiguousarray(np.stack([np.broadcast_to(X, d.shape), np.broadcast_to(Y, d.shape), d], -1).reshape(-1, 3), np.float32)


def corner_clouds(W, H, stride=1, twist=im.TWIST):
    """icp_model.corner_scene as two clouds: `target` the model frame's depth unprojected (its camera's coordinates), `source` the
    current frame's; `truth`, the motion that takes source to target coordinates (T_model T_true^-1, float32, transposed)."""
    s = im.corner_scene(W, H, twist)
    kw = dict(fx=s["fx"], fy=s["fy"], cx=s["cx"], cy=s["cy"], stride=stride)
    Rm, tm = im.pose_of(s["model_view"])
    Rt, tt = im.pose_of(s["true_view"])
    R = Rm @ Rt.T
    return dict(target=unproject32(s["model_depth"], **kw), source=unproject32(s["depth_obs"], **kw), truth=as_transform(R, tm - R @ tt),
                scene=s)


def self_neighbours(points, k, include_self=True):
    """idx [P,k] of the kNN twin in self mode"""
    return km.knn32(points, None, k=k, exclude_self=not include_self)[1]
