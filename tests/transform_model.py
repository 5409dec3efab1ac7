"""A numpy restatement of the map correction (include/dgr_hip.h: dgr_transform_*), written from the stated semantics and not from
the kernels.  `plan_model` and `transform_model` work in float64; `replica` repeats the kernels' fp32 operation order; `bars` gives,
per value, the distance the two may differ by.  The SH band matrices are NOT formed the kernels' way (a constant inverse over
2 l + 1 directions) but by least squares over 64 seeded directions.

Bars.  u = 2^-24 is the relative error of one fp32 rounding.  A result that is a sum of terms, each of which passed through at most N
roundings (a record value rounded once, a product, the additions after it), is off by at most about N u times the sum of the terms'
magnitudes; one more u stands for the second-order terms and the float64 side.  The counts, per kind (fused multiply-adds round once):
    XYZ value        3   (A and t are the caller's fp32 values, exact in the record; three fma)        x (|A||x| + |t|)
    XYZ moment 1     6   (R rounded, product, two fma; 1 / s rounded, the product with it)            x |R||m| / s
    XYZ moment 2     8   (R rounded twice over in R^2, the square, product, two fma; 1 / s^2, product) x R^2 v / s^2
    QUAT value, m 1  5   (q_R rounded, product, three fma)                                            x |L||q|
    QUAT moment 2    7   (two for q_R in the square, the square, product, three fma)                  x L^2 v
    LOG_SCALE        2   (log s rounded, the addition)                                                x (|x| + |log s|)
    SH band l        2 l + 2 (M_l rounded, product, 2 l fma); moment 2: 2 l + 4                        x |M_l||c|
None of them was tuned on what the kernels give."""
import numpy as np

U = 2.0 ** -24
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
C64 = (C1, C2, C3)
# the constants as the kernels hold them (csrc/gaussian_math.h: float literals)
C32 = (float(np.float32(C1)), tuple(float(np.float32(c)) for c in C2), tuple(float(np.float32(c)) for c in C3))
ROUNDINGS = {"xyz": (3, 6, 8), "quat": (5, 5, 7), "log_scale": (2,), "sh": lambda l: (2 * l + 2, 2 * l + 2, 2 * l + 4)}
WORST_ROUNDINGS = 2 * 3 + 4 + 1  # the largest count above (band 3, second moment), with the one for the second order
VALUE, MOMENT1, MOMENT2 = range(3)
MUTANTS = ("sh_unrotated", "sh_transposed", "quat_right", "moment1_times_s", "no_log_s", "anchor_off_by_one", "dc_rotated")


def band(l, D, C=C32):
    """B_l at the unit directions D [n, 3] -> [2 l + 1, n]: computeColorFromSH's basis functions, its signs, its order"""
    x, y, z = np.asarray(D, np.float64).T
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    c1, c2, c3 = C
    if l == 1:
        return np.stack([-c1 * y, c1 * z, -c1 * x])
    if l == 2:
        return np.stack([c2[0] * xy, c2[1] * yz, c2[2] * (2 * zz - xx - yy), c2[3] * xz, c2[4] * (xx - yy)])
    return np.stack([c3[0] * y * (3 * xx - yy), c3[1] * xy * z, c3[2] * y * (4 * zz - xx - yy), c3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                     c3[4] * x * (4 * zz - xx - yy), c3[5] * z * (xx - yy), c3[6] * x * (xx - 3 * yy)])


_DIRS = np.random.RandomState(5).standard_normal((64, 3))
_DIRS /= np.linalg.norm(_DIRS, axis=1, keepdims=True)


def band_matrix(l, R, C=C32):
    """M_l with B_l(R d) = M_l B_l(d): the least-squares solution over 64 directions (exact: the band is invariant)"""
    Y, Yr = band(l, _DIRS, C), band(l, _DIRS @ np.asarray(R, np.float64).T, C)
    return np.linalg.lstsq(Y.T, Yr.T, rcond=None)[0].T


def rotation_of(q):
    r, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def shepperd(N):
    """the unit quaternion (r, x, y, z) of the rotation N: the largest of the trace and the diagonal picks the branch"""
    tr = N[0, 0] + N[1, 1] + N[2, 2]
    if tr >= N[0, 0] and tr >= N[1, 1] and tr >= N[2, 2]:
        q = [1 + tr, N[2, 1] - N[1, 2], N[0, 2] - N[2, 0], N[1, 0] - N[0, 1]]
    elif N[0, 0] >= N[1, 1] and N[0, 0] >= N[2, 2]:
        q = [N[2, 1] - N[1, 2], 1 + 2 * N[0, 0] - tr, N[0, 1] + N[1, 0], N[0, 2] + N[2, 0]]
    elif N[1, 1] >= N[2, 2]:
        q = [N[0, 2] - N[2, 0], N[0, 1] + N[1, 0], 1 + 2 * N[1, 1] - tr, N[1, 2] + N[2, 1]]
    else:
        q = [N[1, 0] - N[0, 1], N[0, 2] + N[2, 0], N[1, 2] + N[2, 1], 1 + 2 * N[2, 2] - tr]
    q = np.array(q, np.float64)
    return q / np.sqrt((q * q).sum())


def quat_left(q):
    """L(q): q (x) p = L(q) p for quaternions (r, x, y, z)"""
    a, b, c, d = q
    return np.array([[a, -b, -c, -d], [b, a, -d, c], [c, d, a, -b], [d, -c, b, a]])


def quat_right(q):
    """p (x) q = Rt(q) p"""
    a, b, c, d = q
    return np.array([[a, -b, -c, -d], [b, a, d, -c], [c, -d, a, b], [d, c, -b, a]])


def plan_model(T, C=C32):
    """One transform (fp32 [4, 4]) -> None when it is invalid, else the float64 record: A, t, s, q, R, log_s, M (a dict l -> M_l)"""
    T = np.asarray(T, np.float32).astype(np.float64)
    if not np.isfinite(T).all():
        return None
    A, t = T[:3, :3], T[:3, 3]
    det = np.linalg.det(A)
    if not det > 0:
        return None
    s = np.cbrt(det)
    if not np.abs(A.T @ A / (s * s) - np.eye(3)).max() <= 1e-3:
        return None
    q = shepperd(A / s)
    R = rotation_of(q)
    return dict(A=A, t=t, s=s, q=q, R=R, log_s=np.log(s), M={l: band_matrix(l, R, C) for l in (1, 2, 3)})


def classify(anchor, plans, P):
    """(index of each row's transform or -1, counts4): which rows move"""
    K = len(plans)
    a = np.zeros(P, np.float32) if anchor is None else np.asarray(anchor, np.float32).reshape(P)
    with np.errstate(invalid="ignore"):
        named = (a >= 0) & (a < K) & (a == np.trunc(a))
    idx = np.where(named, np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)
    valid = np.array([p is not None for p in plans])
    moved = named & valid[np.clip(idx, 0, K - 1)]
    counts = (int(moved.sum()), int((~named).sum()), int((~valid).sum()), int((named & ~moved).sum()))
    return np.where(moved, idx, -1), counts


def sh_bands(width):
    """[(l, first float, floats)] of the complete bands in `width` floats above the DC row"""
    return [(l, 3 * (l * l - 1), 3 * (2 * l + 1)) for l in (1, 2, 3) if 3 * ((l + 1) ** 2 - 1) <= width]


def linear_parts(kind, order, plan, skip=0, k=None):
    """What a tensor of `kind` / `order` does to a row under `plan`, as a list of (slice of the row, W, offset, scale, N): the slice
    becomes scale * (W @ slice) + offset per channel layout, N the count of roundings of its bar.  SH slices are [n, 3] blocks."""
    if kind == "xyz":
        if order == VALUE:
            return [(slice(0, 3), plan["A"], plan["t"], 1.0, 3)]
        if order == MOMENT1:
            return [(slice(0, 3), plan["R"], 0.0, 1.0 / plan["s"], 6)]
        return [(slice(0, 3), plan["R"] ** 2, 0.0, 1.0 / plan["s"] ** 2, 8)]
    if kind == "quat":
        L = quat_left(plan["q"])
        return [(slice(0, 4), L ** 2 if order == MOMENT2 else L, 0.0, 1.0, 7 if order == MOMENT2 else 5)]
    if kind == "sh":
        out = []
        for l, first, n in sh_bands(k - skip):
            M = plan["M"][l]
            out.append((slice(skip + first, skip + first + n), M ** 2 if order == MOMENT2 else M, 0.0, 1.0,
                        2 * l + (4 if order == MOMENT2 else 2)))
        return out
    raise ValueError(kind)


def transform_model(t, kind, order, idx, plans, skip=0):
    """The float64 result and the per-value bar of one tensor [P, k] (fp32 in); rows with idx < 0 are returned as they are with a
    bar of 0 (they must keep their bits)."""
    x = np.asarray(t, np.float32)
    P = x.shape[0]
    x = x.reshape(P, -1)
    out, bar = x.astype(np.float64), np.zeros(x.shape, np.float64)
    for kk in np.unique(idx[idx >= 0]):
        rows, plan = np.flatnonzero(idx == kk), plans[kk]
        v = x[rows].astype(np.float64)
        if kind == "log_scale":
            out[rows] = v + plan["log_s"]
            bar[rows] = (2 + 1) * U * (np.abs(v) + abs(plan["log_s"]))
            continue
        for sl, W, offset, scale, N in linear_parts(kind, order, plan, skip, x.shape[1]):
            block = v[:, sl]
            if kind == "sh":  # [rows, n, 3]: W acts on the coefficient axis
                block = block.reshape(len(rows), -1, 3)
                res = np.einsum("ij,rjc->ric", W, block)
                mag = np.einsum("ij,rjc->ric", np.abs(W), np.abs(block))
                out[rows, sl], bar[rows, sl] = res.reshape(len(rows), -1), ((N + 1) * U * mag).reshape(len(rows), -1)
            else:
                out[rows, sl] = scale * (block @ W.T) + offset
                bar[rows, sl] = (N + 1) * U * (scale * (np.abs(block) @ np.abs(W).T) + np.abs(offset))
    return out.reshape(np.shape(t)), bar.reshape(np.shape(t))


def path_bar(t, kind, order, idx, plans_first, plans_second, skip=0):
    """The per-value bar of `transform_model` for two calls in a row, transform k of `plans_first` and then transform k of
    `plans_second`: the same counts of roundings on the magnitudes of the terms those two calls sum, |W_2| (|W_1| |x| + |t_1|) + |t_2|
    (never less than the |W_2 W_1| |x| + |t| of the one call with the product)."""
    x = np.asarray(t, np.float32)
    P = x.shape[0]
    x = x.reshape(P, -1)
    bar = np.zeros(x.shape, np.float64)
    for kk in np.unique(idx[idx >= 0]):
        rows, first, second = np.flatnonzero(idx == kk), plans_first[kk], plans_second[kk]
        v = np.abs(x[rows].astype(np.float64))
        if kind == "log_scale":
            bar[rows] = (2 + 1) * U * (v + abs(first["log_s"]) + abs(second["log_s"]))
            continue
        parts = zip(linear_parts(kind, order, first, skip, x.shape[1]), linear_parts(kind, order, second, skip, x.shape[1]))
        for (sl, W1, off1, scale1, N), (_, W2, off2, scale2, _) in parts:
            block = v[:, sl]
            if kind == "sh":
                block = block.reshape(len(rows), -1, 3)
                mag = np.einsum("ij,jk,rkc->ric", np.abs(W2), np.abs(W1), block).reshape(len(rows), -1)
            else:
                mag = scale2 * ((scale1 * (block @ np.abs(W1).T) + np.abs(off1)) @ np.abs(W2).T) + np.abs(off2)
            bar[rows, sl] = (N + 1) * U * mag
    return bar.reshape(np.shape(t))


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64; the sum is rounded to float64 and then to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _chain(W, cols, start=None):
    """row i: ((W_i0 c_0 [+ start_i]) then fma over j = 1 ..), all fp32; W [n, n] fp32, cols a list of n fp32 arrays"""
    out = []
    for i in range(W.shape[0]):
        acc = W[i, 0] * cols[0] if start is None else _fma(np.broadcast_to(W[i, 0], cols[0].shape), cols[0], start[i])
        for j in range(1, W.shape[1]):
            acc = _fma(np.broadcast_to(W[i, j], cols[j].shape), cols[j], acc)
        out.append(acc.astype(np.float32))
    return out


def replica(t, kind, order, idx, plans, skip=0, mutant=None):
    """The kernels' fp32 operation order on one tensor (records rounded once to fp32, products and fma in fp32), with an optional
    MUTANT of the semantics.  Returns a float32 array; untouched rows are the input's bits."""
    x = np.array(t, np.float32, copy=True)
    shape = x.shape
    P = shape[0]
    x = x.reshape(P, -1)
    src = x.copy()
    if mutant == "anchor_off_by_one":
        idx = np.where(idx >= 0, (idx + 1) % len(plans), -1)
        idx = np.where((idx >= 0) & np.array([plans[i] is not None for i in np.clip(idx, 0, None)]), idx, -1)
    sq = (lambda m: m * m) if order == MOMENT2 else (lambda m: m)
    for kk in np.unique(idx[idx >= 0]):
        rows, plan = np.flatnonzero(idx == kk), plans[kk]
        v = src[rows]
        if kind == "log_scale":
            if mutant != "no_log_s":
                x[rows] = v + np.float32(plan["log_s"])
        elif kind == "xyz":
            cols = [v[:, j] for j in range(3)]
            if order == VALUE:
                res = _chain(_f32(plan["A"]), cols, start=_f32(plan["t"]))
            else:
                s = plan["s"]
                scale = np.float32(1.0 / (s * s) if order == MOMENT2 else (s if mutant == "moment1_times_s" else 1.0 / s))
                res = [r * scale for r in _chain(sq(_f32(plan["R"])), cols)]
            x[rows] = np.stack(res, axis=1)
        elif kind == "quat":
            L = (quat_right if mutant == "quat_right" else quat_left)(_f32(plan["q"]))
            x[rows] = np.stack(_chain(sq(L.astype(np.float32)), [v[:, j] for j in range(4)]), axis=1)
        elif kind == "sh":
            lead = 0 if mutant == "dc_rotated" and skip else skip
            for l, first, n in sh_bands(x.shape[1] - skip):
                if mutant == "sh_unrotated":
                    continue
                M = _f32(plan["M"][l].T if mutant == "sh_transposed" else plan["M"][l])
                block = v[:, lead + first:lead + first + n].reshape(len(rows), -1, 3)
                for ch in range(3):
                    res = _chain(sq(M), [block[:, j, ch] for j in range(2 * l + 1)])
                    x[rows, lead + first + ch:lead + first + n:3] = np.stack(res, axis=1)
    return x.reshape(shape)


def within(got, want, bar):
    """got (fp32) against the float64 model: every value within its bar, and bit-equal where the bar is 0"""
    return bool((np.abs(np.asarray(got, np.float64) - want) <= bar).all())


def random_rotation(rng):
    q = rng.standard_normal(4)
    return rotation_of(q / np.linalg.norm(q))


def random_sim3(rng, s=1.0, spread=2.0):
    """a fp32 [4, 4] Sim(3) matrix with scale s"""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = s * random_rotation(rng), spread * rng.standard_normal(3)
    return T.astype(np.float32)
