"""Brute-force models of the k-nearest-neighbour rule of include/dgr_hip.h (dgr_knn_search), in numpy.

`knn32` is the float32 twin: the distance in the rule's operation order with every step an explicit np.float32 operation (no
einsum, no dot: numpy rounds each elementwise float32 operation once and fuses nothing), the candidates ordered by
np.lexsort over (d2, index), the mean added left to right and divided once.  The kernels must reproduce it bit for bit.
`knn64` is the same rule with the distance in float64, the yardstick of the twin itself.

`morton_keys32` / `morton_order32` are the twin of the BUILD as knn.hip states it (the box of the valid points, a 30-bit Morton key
on it, a stable sort of (key, index)), and `index_view` reads what dgr_knn_build wrote, so that a test can hold the index itself to
that statement: the search's answers do not depend on it, only its speed does.  Below them the data sets and the cached references
that the CPU tests (tests/test_knn_model.py) and the GPU tests (tests/test_hip_knn.py) share."""
import functools
import types

import numpy as np

INF32 = np.float32(np.inf)


def valid_rows(a):
    return np.isfinite(np.asarray(a, np.float32)).all(axis=1)


def _dist2_32(q, p):
    """q and p [..., 3] float32 that broadcast against each other: ((dx dx) + (dy dy)) + (dz dz), d = p - q"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = p[..., 0] - q[..., 0]
        dy = p[..., 1] - q[..., 1]
        dz = p[..., 2] - q[..., 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        s = xx + yy
        d2 = s + zz
    assert d2.dtype == np.float32
    return d2


def dist2_32(q, p):
    """[Q,3] x [P,3] -> [Q,P] float32: ((dx dx) + (dy dy)) + (dz dz), d = p - q, each operation rounded once"""
    q, p = np.asarray(q, np.float32), np.asarray(p, np.float32)
    return _dist2_32(q[:, None, :], p[None, :, :])


def dist2_of_pairs32(queries, points, idx):
    """[Q,k] float32: the same distance from query r to points[idx[r, j]] alone; +inf where idx is -1"""
    q, p, idx = np.asarray(queries, np.float32), np.asarray(points, np.float32), np.asarray(idx)
    d2 = _dist2_32(q[:, None, :], p[np.maximum(idx, 0)])
    return np.where(idx >= 0, d2, INF32)


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


def within(ref, k, max_dist2):
    """the rule's answer for k within max_dist2 from its unlimited answer for a larger k: admission is monotone in d2, so it is
    the first k of the same order cut where d2 > max_dist2"""
    d, i, _, _ = first_k(ref, k)
    out = ~(d <= np.float32(max_dist2))  # (an empty slot holds +inf and -1 already)
    d, i = np.where(out, INF32, d), np.where(out | (i < 0), -1, i).astype(np.int32)
    return d, i, (i >= 0).sum(axis=1).astype(np.int32), mean32(d)


# ---- the build (csrc/knn.hip: "build")
KEY_INVALID = np.uint32(0xFFFFFFFF)
LEAF = 256          # records per leaf
BLOCK = 64 * LEAF   # records per block of 64 leaves, the unit of the search's sweep


def order_bits(f):
    """float32 -> uint32 of the same order (-0.0 below +0.0): the form the index header keeps its box in"""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def order_float(u):
    u = np.ascontiguousarray(u, np.uint32)
    return (u ^ np.where(u >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def box_bits(points):
    """(lo [3], hi [3]) uint32: the box of the valid rows as order-mapped bits; without a valid row (+inf, -inf)"""
    b = order_bits(np.asarray(points, np.float32)[valid_rows(points)])
    if not len(b):
        return order_bits(np.full(3, np.inf, np.float32)), order_bits(np.full(3, -np.inf, np.float32))
    return b.min(axis=0), b.max(axis=0)


def quanta32(points, box_points=None):
    """[P,3] uint32: each coordinate of the valid rows on the 1024 steps of the box's axis (invalid rows: 0).  e = hi - lo; 0
    unless e > 0 and finite; else t = ((p - lo) / e) * 1024, each operation one float32 rounding; 1023 if t >= 1023, trunc(t) if
    t > 0, else 0."""
    p = np.ascontiguousarray(points, np.float32)
    lo, hi = (order_float(b) for b in box_bits(p if box_points is None else box_points))
    ok = valid_rows(p)
    q = np.zeros(p.shape, np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        e = hi - lo
        for a in range(3):
            if not (e[a] > 0 and np.isfinite(e[a])):
                continue
            d = p[ok, a] - lo[a]
            r = d / e[a]
            t = r * np.float32(1024.0)
            assert t.dtype == np.float32
            q[ok, a] = np.where(t >= 1023, 1023, np.where(t > 0, np.minimum(t, 1023), 0)).astype(np.uint32)
    return q


def spread3(x):
    """the 10 low bits of x, two zero bits after each (the magic-mask form knn.hip uses)"""
    x = np.asarray(x, np.uint32) & np.uint32(0x3FF)
    x = (x | (x << np.uint32(16))) & np.uint32(0x30000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x30C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x9249249)
    return x


def interleave3(q):
    """[N,3] 10-bit quanta -> the 30-bit key: x in bit 0, y in bit 1, z in bit 2 of every triple"""
    q = np.asarray(q, np.uint32)
    return spread3(q[:, 0]) | (spread3(q[:, 1]) << np.uint32(1)) | (spread3(q[:, 2]) << np.uint32(2))


def morton_keys32(points, box_points=None):
    """[P] uint32: the key of every row on the box of the valid rows of box_points (default: points); invalid rows 0xFFFFFFFF"""
    return np.where(valid_rows(points), interleave3(quanta32(points, box_points)), KEY_INVALID)


def morton_order32(points, box_points=None):
    """[P]: the rows in the index's order: by key, equal keys by ascending index (a stable sort); the invalid rows come last"""
    key = morton_keys32(points, box_points)
    return np.lexsort((np.arange(len(key)), key))


def index_view(index_bytes, P):
    """What dgr_knn_build wrote, parsed.  THE ONE PLACE IN THE TESTS THAT KNOWS THE LAYOUT (KnnHeader / KnnIndexView in
    csrc/knn.hip): 64 bytes of header (lo[3], hi[3] as order-mapped uint32, n_valid int32), P records of float4 (x, y, z, the bits
    of the row), ceil(P / 256) float4 leaf_lo (the minimum, the bits of the leaf's first key), as many leaf_hi (the maximum, the
    bits of the count)."""
    raw = np.ascontiguousarray(index_bytes, np.uint8)
    B = (P + LEAF - 1) // LEAF
    assert raw.size == 64 + 16 * P + 32 * B, (raw.size, P)
    head = raw[:64].view(np.uint32)
    recs = raw[64:64 + 16 * P].view(np.uint32).reshape(P, 4)
    leaves = raw[64 + 16 * P:].view(np.uint32).reshape(2, B, 4)
    return types.SimpleNamespace(
        lo=head[0:3].copy(), hi=head[3:6].copy(), n_valid=int(head[6:7].view(np.int32)[0]),
        xyz=recs[:, :3].copy().view(np.float32), row=recs[:, 3].copy().view(np.int32),
        leaf_lo=leaves[0, :, :3].copy().view(np.float32), leaf_key=leaves[0, :, 3].copy(),
        leaf_hi=leaves[1, :, :3].copy().view(np.float32), leaf_count=leaves[1, :, 3].copy().view(np.int32))


# ---- data sets and references that the CPU and the GPU tests share
def uniform_cloud(n, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3), dtype=np.float32) * np.float32(hi - lo) + np.float32(lo)).astype(np.float32)


def spoil(p, rows):
    """a NaN, a +inf or a -inf in varying columns of the given rows, in place"""
    for j, r in enumerate(rows):
        p[r, j % 3] = (np.nan, np.inf, -np.inf)[j % 3 if j % 2 else (j // 2) % 3]
    return p


SMALL = ("none_valid", "one_valid", "leaf_edge_valid", "overflow_extent", "subnormal")


@functools.lru_cache(maxsize=None)
def small_dataset(name):
    if name == "none_valid":
        return spoil(uniform_cloud(70, 51), range(70))
    if name == "one_valid":
        return spoil(uniform_cloud(70, 51), [r for r in range(70) if r != 37])
    if name == "leaf_edge_valid":  # 600 rows, 256 of them valid: one full leaf and two empty ones
        return spoil(uniform_cloud(600, 52), np.sort(np.random.default_rng(53).permutation(600)[:344]))
    if name == "overflow_extent":  # hi - lo = +inf on x
        p = uniform_cloud(304, 54)
        p[[11, 150, 207, 303], 0] = (3e38, -3e38, -3e38, 3e38)
        return p
    if name == "subnormal":  # every squared distance is a subnormal number or zero
        return uniform_cloud(500, 55) * np.float32(2.0 ** -66)
    raise KeyError(name)


def _sampled_case(p, rows, **more):
    """p, its Morton order, the block of 64 leaves of every row, `rows` (ascending) and the twin's k = 16 answers for them with
    and without the own point, from ONE brute-force pass at k = 17"""
    P = len(p)
    assert len(np.unique(p, axis=0)) == P
    order = morton_order32(p)
    block = np.empty(P, np.int64)
    block[order] = np.arange(P) // BLOCK
    rows = np.unique(rows(order, block) if callable(rows) else rows)
    d, i, c, _ = knn32(p, p[rows], 17)
    # the points are distinct: a row's own point is its one candidate at d2 = 0, and without it the others follow as they do with it
    assert (c == 17).all() and np.array_equal(i[:, 0], rows) and (d[:, 0] == 0).all()
    d_in, i_in = np.ascontiguousarray(d[:, :16]), np.ascontiguousarray(i[:, :16])
    d_ex, i_ex = np.ascontiguousarray(d[:, 1:]), np.ascontiguousarray(i[:, 1:])
    full = np.full(len(rows), 16, np.int32)
    return types.SimpleNamespace(p=p, order=order, block=block, rows=rows, with_self=(d_in, i_in, full, mean32(d_in)),
                                 exclude_self=(d_ex, i_ex, full, mean32(d_ex)), **more)


@functools.lru_cache(maxsize=None)
def cloud50000_case():
    """50 000 uniform points: 196 leaves, that is three full blocks of 64 leaves and a fourth of four leaves (848 records).  The
    rows that are compared with brute force: of each full block the 1000 nearest the plane z = 0.5 (where Morton order separates
    neighbours by two blocks), and the first and the last 64 of the order (the last 64 lie in the fourth block).  `plane[b]`:
    the 1000 rows of block b."""
    p = uniform_cloud(50000, 50000)
    off_plane = np.abs(p[:, 2].astype(np.float64) - 0.5)
    plane = []

    def rows(order, block):
        for b in range(3):
            mine = np.flatnonzero(block == b)
            plane.append(mine[np.argsort(off_plane[mine], kind="stable")[:1000]])
        return np.concatenate(plane + [order[:64], order[-64:]])
    return _sampled_case(p, rows, plane=plane)


@functools.lru_cache(maxsize=None)
def collapsed_case():
    """65 000 uniform points and one 1e6 extents away: every key but the outlier's is 0, the index's order is the rows' own, the
    four blocks of 64 leaves are quarters of the rows and every point's neighbours lie anywhere in them, so the sweep has to reach
    own_block - 3 and own_block + 3.  The rows that are compared: the first and the last 64 of every block."""
    p = np.concatenate([uniform_cloud(65000, 65000), np.full((1, 3), 1e6, np.float32)])
    ends = np.concatenate([np.arange(b * BLOCK, b * BLOCK + 64) for b in range(4)] + [np.arange(min((b + 1) * BLOCK, len(p)) - 64,
                                                                                              min((b + 1) * BLOCK, len(p))) for b in range(4)])
    return _sampled_case(p, lambda order, block: order[ends])


@functools.lru_cache(maxsize=None)
def two_sort_block_queries():
    """4200 queries for cross mode (more than one sort block of 4096 keys): 4000 uniform in [-0.25, 1.25]^3, 100 copies of points
    of cloud50000_case(), 100 invalid rows, shuffled"""
    p = cloud50000_case().p
    q = np.concatenate([uniform_cloud(4000, 61, -0.25, 1.25), p[np.random.default_rng(62).choice(len(p), 100, replace=False)],
                        spoil(uniform_cloud(100, 63), range(100))])
    return q[np.random.default_rng(64).permutation(len(q))]


@functools.lru_cache(maxsize=None)
def two_sort_block_reference():
    """the twin's k = 16 answer for two_sort_block_queries() against the 50 000 points"""
    return knn32(cloud50000_case().p, two_sort_block_queries(), 16)
