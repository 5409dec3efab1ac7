"""Brute-force models of the k-nearest-neighbour rule of include/dgr_hip.h (dgr_knn_search), in numpy.

`knn32` is the float32 twin: the distance in the rule's operation order with every step an explicit np.float32 operation (no
einsum, no dot: numpy rounds each elementwise float32 operation once and fuses nothing), the candidates ordered by
np.lexsort over (d2, index), the mean added left to right and divided once.  The kernels must reproduce it bit for bit.
`knn64` is the same rule with the distance in float64, the yardstick of the twin itself."""
import numpy as np

INF32 = np.float32(np.inf)


def valid_rows(a):
    return np.isfinite(np.asarray(a, np.float32)).all(axis=1)


def dist2_32(q, p):
    """[Q,3] x [P,3] -> [Q,P] float32: ((dx dx) + (dy dy)) + (dz dz), d = p - q, each operation rounded once"""
    q, p = np.asarray(q, np.float32), np.asarray(p, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = p[None, :, 0] - q[:, None, 0]
        dy = p[None, :, 1] - q[:, None, 1]
        dz = p[None, :, 2] - q[:, None, 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        s = xx + yy
        d2 = s + zz
    assert d2.dtype == np.float32
    return d2


def dist2_64(q, p):
    q, p = np.asarray(q, np.float32).astype(np.float64), np.asarray(p, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        d = p[None, :, :] - q[:, None, :]
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def _knn(dist_fn, out_dtype, points, queries, k, exclude_self, max_dist2, chunk):
    points = np.ascontiguousarray(points, np.float32)
    self_mode = queries is None
    if exclude_self is None:
        exclude_self = self_mode
    assert self_mode or not exclude_self
    q_all = points if self_mode else np.ascontiguousarray(queries, np.float32)
    P, Q = len(points), len(q_all)
    pv, qv = valid_rows(points), valid_rows(q_all)
    cand = np.flatnonzero(pv)  # ascending indices: lexsort's last tie-break then equals the index order
    dist2 = np.full((Q, k), np.inf, out_dtype)
    idx = np.full((Q, k), -1, np.int32)
    count = np.zeros(Q, np.int32)
    for a in range(0, Q, chunk):
        rows = np.arange(a, min(a + chunk, Q))
        rows = rows[qv[rows]]
        if not len(rows) or not len(cand):
            continue
        d2 = dist_fn(q_all[rows], points[cand])
        admitted = d2 <= max_dist2
        if exclude_self:
            admitted &= cand[None, :] != rows[:, None]
        # only to save time: a row's k-th smallest admitted distance (NaN sorts last: with fewer than k it is NaN and nothing
        # is dropped); what is above it cannot be among the first k.  The order itself is lexsort's, below.
        kth = np.partition(np.where(admitted, d2, np.nan), min(k, len(cand)) - 1, axis=1)[:, min(k, len(cand)) - 1]
        with np.errstate(invalid="ignore"):
            admitted &= ~(d2 > kth[:, None])
        for r, row in enumerate(rows):
            ok = admitted[r]
            c, d = cand[ok], d2[r][ok]
            order = np.lexsort((c, d))[:k]
            n = len(order)
            dist2[row, :n], idx[row, :n], count[row] = d[order], c[order], n
    return dist2, idx, count


def knn32(points, queries=None, k=3, exclude_self=None, max_dist2=np.inf, chunk=256):
    """(dist2 [Q,k] float32, idx [Q,k] int32, count [Q] int32, mean_dist2 [Q] float32) of the rule, the bits the kernels give"""
    dist2, idx, count = _knn(dist2_32, np.float32, points, queries, k, exclude_self, np.float32(max_dist2), chunk)
    return dist2, idx, count, mean32(dist2)


def mean32(dist2):
    """mean_dist2 of [Q,k] ascending float32 distances: added left to right, then one division by float32(k)"""
    dist2 = np.asarray(dist2, np.float32)
    with np.errstate(over="ignore"):
        s = dist2[:, 0].copy()
        for j in range(1, dist2.shape[1]):
            s = s + dist2[:, j]
        mean = s / np.float32(dist2.shape[1])
    assert mean.dtype == np.float32
    return mean


def first_k(ref, k):
    """the rule's answer for k from its answer for a larger k (the first k of the same order): (dist2, idx, count, mean_dist2)"""
    dist2, idx, count, _ = ref
    d = np.ascontiguousarray(dist2[:, :k])
    return d, np.ascontiguousarray(idx[:, :k]), np.minimum(count, k).astype(np.int32), mean32(d)


def knn64(points, queries=None, k=3, exclude_self=None, max_dist2=np.inf, chunk=256):
    """the same selection with the distance in float64: (dist2 float64, idx, count)"""
    return _knn(dist2_64, np.float64, points, queries, k, exclude_self, float(max_dist2), chunk)


def max_distance_squared(d):
    """what dgr_amd.knn makes of max_distance: squared in float64, rounded once"""
    with np.errstate(over="ignore"):
        return np.float32(np.float64(d) * np.float64(d))


def lattice(n):
    """the n x n x n integer lattice, x fastest: point i = (i % n, i // n % n, i // n^2)"""
    g = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
