"""The brute-force models of the kNN rule (tests/knn_model.py) without a GPU: the float32 twin against float64, closed forms on
the integer lattice, and the conventions of include/dgr_hip.h (fewer than k neighbours, invalid rows, exclude_self, a neighbour
exactly on the radius)."""
import numpy as np
import pytest

import knn_model as M

# five roundings along the longest path of d2: the difference (its error enters the square twice), the product and the two
# sums, all terms positive: a relative error of at most (1 + 2^-24)^5 - 1
REL = (1.0 + 2.0 ** -24) ** 5 - 1.0


def cloud(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3), dtype=np.float32) * np.float32(scale)).astype(np.float32)


def test_the_twin_uses_float32_steps_only():
    p = cloud(50, 1)
    assert M.dist2_32(p[:7], p).dtype == np.float32
    d2, idx, count, mean = M.knn32(p, k=4)
    assert d2.dtype == np.float32 and idx.dtype == np.int32 and count.dtype == np.int32 and mean.dtype == np.float32


@pytest.mark.parametrize("seed, scale", [(2, 1.0), (3, 1000.0), (4, 1e-3)])
def test_every_distance_is_within_five_roundings_of_float64(seed, scale):
    p, q = cloud(400, seed, scale), cloud(90, seed + 10, scale)
    d32, d64 = M.dist2_32(q, p).astype(np.float64), M.dist2_64(q, p)
    assert (np.abs(d32 - d64) <= REL * d64).all()
    assert REL < 3.0e-7


@pytest.mark.parametrize("k", [1, 3, 8])
def test_the_selections_agree_with_float64_wherever_the_gaps_exceed_the_bound(k):
    p, q = cloud(700, 5), cloud(120, 6)
    for queries in (None, q):
        d32, i32, c32, _ = M.knn32(p, queries, k)
        d64, i64, c64 = M.knn64(p, queries, k + 1)
        assert np.array_equal(c32, np.minimum(c64, k))
        # a rank is decided when the float64 gaps to both neighbours in the order exceed the two distances' error bounds
        gap_ok = np.diff(d64, axis=1) > 2.0 * REL * d64[:, 1:]
        decided = gap_ok[:, :k].copy()
        decided[:, 1:] &= gap_ok[:, :k - 1]
        assert decided.mean() > 0.99
        assert np.array_equal(i32[decided], i64[:, :k][decided])
        assert (np.abs(d32.astype(np.float64) - d64[:, :k]) <= REL * d64[:, :k]).all()


def test_lattice_interior_points_have_their_six_face_neighbours_at_one_and_the_lowest_indices_win():
    n = 6
    p = M.lattice(n)
    d2, idx, count, mean = M.knn32(p, k=6)
    i = np.arange(n ** 3)
    x, y, z = i % n, i // n % n, i // n ** 2
    interior = (x > 0) & (x < n - 1) & (y > 0) & (y < n - 1) & (z > 0) & (z < n - 1)
    assert interior.sum() == (n - 2) ** 3
    want = np.stack([i - n * n, i - n, i - 1, i + 1, i + n, i + n * n], axis=1)  # ascending indices
    assert (d2[interior] == 1.0).all() and np.array_equal(idx[interior], want[interior]) and (mean[interior] == 1.0).all()
    # k = 3 of six equidistant candidates: the three lowest indices
    d3, i3, _, _ = M.knn32(p, k=3)
    assert np.array_equal(i3[interior], want[interior][:, :3])
    # a corner has three neighbours at 1, then three at 2
    assert d2[0].tolist() == [1, 1, 1, 2, 2, 2] and idx[0].tolist() == [1, n, n * n, n + 1, n * n + 1, n * n + n]


def test_fewer_than_k_neighbours():
    p = cloud(3, 7)
    d2, idx, count, mean = M.knn32(p, k=3)
    assert count.tolist() == [2, 2, 2] and (idx[:, 2] == -1).all() and np.isposinf(d2[:, 2]).all() and np.isposinf(mean).all()
    assert (idx[:, :2] >= 0).all() and np.isfinite(d2[:, :2]).all()
    d2, idx, count, mean = M.knn32(p[:1], k=1)
    assert count.tolist() == [0] and idx.tolist() == [[-1]] and np.isposinf(d2).all() and np.isposinf(mean).all()
    d2, idx, count, mean = M.knn32(p[:1], k=2, exclude_self=False)
    assert count.tolist() == [1] and idx.tolist() == [[0, -1]] and d2[0, 0] == 0.0 and np.isposinf(mean).all()


def test_invalid_rows_are_never_returned_and_find_nothing():
    p = cloud(40, 8)
    p[3, 1] = np.nan
    p[17, 0] = np.inf
    p[29, 2] = -np.inf
    bad = [3, 17, 29]
    d2, idx, count, mean = M.knn32(p, k=5)
    assert not np.isin(idx, bad).any()
    assert (count[bad] == 0).all() and (idx[bad] == -1).all() and np.isposinf(d2[bad]).all() and np.isposinf(mean[bad]).all()
    ok = np.setdiff1d(np.arange(40), bad)
    assert (count[ok] == 5).all()
    q = cloud(4, 9)
    q[2, 0] = np.nan
    d2, idx, count, _ = M.knn32(p, q, k=2)
    assert count.tolist() == [2, 2, 0, 2] and not np.isin(idx, bad).any()


def test_exclude_self_rejects_the_own_index_only():
    p = cloud(20, 10)
    p[5] = p[4]
    p[6] = p[4]
    d_in, i_in, _, _ = M.knn32(p, k=3, exclude_self=False)
    assert i_in[4].tolist() == [4, 5, 6] and i_in[5].tolist() == [4, 5, 6] and (d_in[4] == 0).all()
    d_ex, i_ex, _, _ = M.knn32(p, k=2)  # the default of self mode
    assert i_ex[4].tolist() == [5, 6] and i_ex[5].tolist() == [4, 6] and i_ex[6].tolist() == [4, 5] and (d_ex[4:7] == 0).all()
    assert (i_ex != np.arange(20)[:, None]).all()
    with pytest.raises(AssertionError):
        M.knn32(p, p[:3], k=2, exclude_self=True)


def test_a_neighbour_exactly_on_the_radius_is_admitted():
    p = M.lattice(4)
    r2 = M.max_distance_squared(1.0)
    assert r2 == np.float32(1.0)
    d2, idx, count, mean = M.knn32(p, k=8, max_dist2=r2)
    x, y, z = (p[:, a].astype(int) for a in range(3))
    faces = sum(((c > 0).astype(int) + (c < 3).astype(int)) for c in (x, y, z))
    assert np.array_equal(count, faces) and count.min() == 3 and count.max() == 6
    assert ((d2 == 1.0) == (idx >= 0)).all() and np.isposinf(mean).all()
    just_below = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert M.knn32(p, k=8, max_dist2=just_below)[2].max() == 0
    # sqrt(2) squared in float64 rounds to the float32 above 2: the edge neighbours at d2 = 2 are inside
    assert M.max_distance_squared(np.sqrt(2.0)) >= np.float32(2.0)


def test_huge_coordinates_give_infinite_distances_that_are_admitted():
    p = np.array([[1e30, 0, 0], [-1e30, 0, 0], [1e30, 1, 0], [0, 0, 0]], np.float32)
    d2, idx, count, mean = M.knn32(p, k=3)
    assert count.tolist() == [3, 3, 3, 3] and not np.isnan(d2).any()
    assert idx[0].tolist() == [2, 1, 3] and d2[0, 0] == 1.0 and np.isposinf(d2[0, 1:]).all()
    assert idx[3].tolist() == [0, 1, 2] and np.isposinf(d2[3]).all()
