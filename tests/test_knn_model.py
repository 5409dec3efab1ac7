"""The brute-force models of the kNN rule (tests/knn_model.py) without a GPU: the float32 twin against float64, closed forms on
the integer lattice, and the conventions of include/dgr_hip.h (fewer than k neighbours, invalid rows, exclude_self, a neighbour
exactly on the radius).  Then the twin of the build (the box, the Morton key, the stable order, the parser of the index) and the
conditions under which the GPU tests of tests/test_hip_knn.py on the shared data sets mean something."""
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


def test_within_is_the_limited_answer():
    p, q = cloud(900, 11), cloud(200, 12)
    r2 = M.max_distance_squared(0.09)
    want, got = M.knn32(p, q, 5, max_dist2=r2), M.within(M.knn32(p, q, 9), 5, r2)
    assert 0 < (want[2] < 5).sum() < 200
    for w, g in zip(want, got):
        assert w.dtype == g.dtype and np.array_equal(w.view(np.uint32) if w.dtype == np.float32 else w,
                                                     g.view(np.uint32) if g.dtype == np.float32 else g)


# ---- the twin of the build
def test_the_magic_mask_interleave_is_the_bit_by_bit_interleave():
    q = np.random.default_rng(13).integers(0, 1024, (5000, 3)).astype(np.uint32)
    q[:4] = [[1023, 0, 0], [0, 1023, 0], [0, 0, 1023], [1023, 1023, 1023]]
    plain = np.zeros(len(q), np.uint64)
    for bit in range(10):
        for a in range(3):
            plain |= ((q[:, a].astype(np.uint64) >> bit) & 1) << (3 * bit + a)
    key = M.interleave3(q)
    assert key.dtype == np.uint32 and np.array_equal(key.astype(np.uint64), plain)
    assert key[:4].tolist() == [0x09249249, 0x12492492, 0x24924924, 0x3FFFFFFF]


def test_the_order_mapping_keeps_the_order_of_the_floats():
    f = np.array([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, np.inf], np.float32)
    u = M.order_bits(f)
    assert u.dtype == np.uint32 and (np.diff(u.astype(np.int64)) > 0).all()
    assert np.array_equal(M.order_float(u).view(np.uint32), f.view(np.uint32))
    assert u[0] == 0x007FFFFF and u[-1] == 0xFF800000  # what the build starts its maximum and its minimum from


def test_keys_of_valid_rows_are_below_2_to_the_30_and_invalid_rows_get_all_ones():
    p = cloud(3000, 14)
    bad = np.random.default_rng(15).choice(3000, 200, replace=False)
    M.spoil(p, bad)
    key = M.morton_keys32(p)
    ok = M.valid_rows(p)
    assert key.dtype == np.uint32 and ok.sum() == 2800
    assert (key[ok] < 2 ** 30).all() and (key[~ok] == 0xFFFFFFFF).all()
    # every axis reaches the key, in its own bits: x in bit 0, y in bit 1, z in bit 2 of every triple
    q = M.quanta32(p)
    for a in range(3):
        assert q[ok, a].min() == 0 and q[ok, a].max() == 1023
        assert np.array_equal((key[ok] >> a) & 0x09249249, M.spread3(q[ok, a]))
    # the order is a permutation, the invalid rows last and in index order, equal keys in index order
    order = M.morton_order32(p)
    assert np.array_equal(np.sort(order), np.arange(3000))
    assert np.array_equal(order[2800:], np.sort(bad))
    k_sorted = key[order].astype(np.int64)
    assert (np.diff(k_sorted) >= 0).all() and (np.diff(order)[np.diff(k_sorted) == 0] > 0).all()


def test_equal_keys_keep_their_index_order():
    p = np.repeat(cloud(40, 16), 5, axis=0)[np.random.default_rng(17).permutation(200)]
    key, order = M.morton_keys32(p), M.morton_order32(p)
    same = np.diff(key[order].astype(np.int64)) == 0
    assert same.sum() >= 160 and (np.diff(order)[same] > 0).all()


def test_zero_and_infinite_extents_quantise_to_zero_and_the_upper_face_to_1023():
    p = cloud(300, 18)
    p[:, 1] = 0.25                  # zero extent
    p[7, 0], p[8, 0] = 3e38, -3e38  # hi - lo = +inf
    q = M.quanta32(p)
    assert (q[:, 0] == 0).all() and (q[:, 1] == 0).all() and q[:, 2].max() == 1023 and q[:, 2].min() == 0
    assert q[np.argmax(p[:, 2]), 2] == 1023 and q[np.argmin(p[:, 2]), 2] == 0
    # queries on another set's box: outside it they clamp to the faces, NaN rows get the invalid key
    box = cloud(100, 19)
    lo, hi = box.min(axis=0), box.max(axis=0)
    qs = np.array([lo - 1, hi + 1, hi, lo, [np.nan, 0, 0]], np.float32)
    assert M.quanta32(qs, box).tolist() == [[0] * 3, [1023] * 3, [1023] * 3, [0] * 3, [0] * 3]
    assert M.morton_keys32(qs, box).tolist() == [0, 0x3FFFFFFF, 0x3FFFFFFF, 0, 0xFFFFFFFF]
    # no valid row in the box: every extent is -inf, every key 0
    assert (M.morton_keys32(cloud(5, 20), np.full((3, 3), np.nan, np.float32)) == 0).all()


def test_index_view_reads_the_stated_layout():
    P = 300
    raw = np.zeros(64 + 16 * P + 32 * 2, np.uint8)
    head, body = raw[:64].view(np.uint32), raw[64:].view(np.uint32)
    head[:7] = [1, 2, 3, 4, 5, 6, 299]
    body[:] = np.arange(len(body))
    v = M.index_view(raw, P)
    assert v.lo.tolist() == [1, 2, 3] and v.hi.tolist() == [4, 5, 6] and v.n_valid == 299
    assert v.xyz.shape == (P, 3) and v.xyz.dtype == np.float32 and v.row.dtype == np.int32
    assert v.xyz.view(np.uint32)[1].tolist() == [4, 5, 6] and v.row[1] == 7 and v.row[P - 1] == 4 * P - 1
    assert v.leaf_lo.view(np.uint32).tolist() == [[4 * P, 4 * P + 1, 4 * P + 2], [4 * P + 4, 4 * P + 5, 4 * P + 6]]
    assert v.leaf_key.tolist() == [4 * P + 3, 4 * P + 7]
    assert v.leaf_hi.view(np.uint32)[0].tolist() == [4 * P + 8, 4 * P + 9, 4 * P + 10] and v.leaf_count.tolist() == [4 * P + 11, 4 * P + 15]
    with pytest.raises(AssertionError):
        M.index_view(raw, P + 1)


# ---- the shared data sets are what the GPU tests need them to be
def test_the_small_data_sets_are_what_they_claim():
    p = M.small_dataset("none_valid")
    assert p.shape == (70, 3) and not M.valid_rows(p).any() and np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any()
    for ref in (M.knn32(p, None, 16), M.knn32(p, None, 16, exclude_self=False), M.knn32(p, cloud(90, 21), 16)):
        d, i, c, m = ref
        assert (i == -1).all() and np.isposinf(d).all() and (c == 0).all() and np.isposinf(m).all()
    p = M.small_dataset("one_valid")
    assert p.shape == (70, 3) and np.flatnonzero(M.valid_rows(p)).tolist() == [37]
    assert M.knn32(p, None, 16, exclude_self=False)[2].tolist() == [0] * 37 + [1] + [0] * 32
    assert (M.knn32(p, None, 16)[2] == 0).all()
    p = M.small_dataset("leaf_edge_valid")
    ok = M.valid_rows(p)
    assert p.shape == (600, 3) and ok.sum() == M.LEAF and not ok[:300].all() and not ok[300:].all()
    p = M.small_dataset("overflow_extent")
    lo, hi = (M.order_float(b) for b in M.box_bits(p))
    with np.errstate(over="ignore"):
        assert M.valid_rows(p).all() and np.isposinf(hi[0] - lo[0]) and np.isfinite(hi[1:] - lo[1:]).all()
    assert ((M.morton_keys32(p) & 0x09249249) == 0).all() and (M.quanta32(p)[:, 1:].max(axis=0) == 1023).all()
    d = M.knn32(p, None, 16)[0]
    assert np.isposinf(d).any() and not np.isnan(d).any()


def test_the_subnormal_data_set_has_subnormal_distances_and_ties():
    p = M.small_dataset("subnormal")
    assert len(np.unique(p, axis=0)) == 500 and (np.abs(p) >= np.finfo(np.float32).tiny).all()  # the coordinates are normal
    for exclude_self in (True, False):
        d, i, c, _ = M.knn32(p, None, 16, exclude_self=exclude_self)
        assert (c == 16).all() and (d < np.finfo(np.float32).tiny).all()
        assert ((d > 0) & (d < np.finfo(np.float32).tiny)).mean() >= 0.9
        assert (np.diff(d, axis=1) == 0).any()  # equal distances: the index decides
    # flushed to zero, the answers would differ: every other point at d2 = 0, the 16 lowest indices
    assert not np.array_equal(M.knn32(p, None, 16)[1], M.knn32(np.zeros_like(p), None, 16)[1])


def reaching(case, mine, dst, k):
    """how many of the compared rows `mine` (a mask over case.rows) have one of their k true neighbours in block dst"""
    return int(((case.block[case.exclude_self[1][:, :k]] == dst).any(axis=1) & mine).sum())


def check_sampled_case(c):
    P = len(c.p)
    assert np.array_equal(np.sort(c.order), np.arange(P)) and (np.diff(c.rows) > 0).all()
    assert np.isin(c.order[:64], c.rows).all() and np.isin(c.order[-64:], c.rows).all()
    d, i, cnt, _ = c.exclude_self
    assert (i != c.rows[:, None]).all() and (cnt == 16).all() and (np.diff(d, axis=1) >= 0).all() and (d[:, 0] > 0).all()
    assert np.array_equal(c.with_self[1][:, 0], c.rows) and np.array_equal(c.with_self[1][:, 1:], i[:, :15])
    assert (c.with_self[0][:, 0] == 0).all() and np.array_equal(c.with_self[0][:, 1:], d[:, :15])


def test_cloud50000_has_neighbours_two_blocks_of_leaves_away():
    """what keeps the GPU test on 50 000 points from passing vacuously: compared rows of block 0 whose true neighbours lie in
    block 2 (the sweep has to reach own_block + 2) and the other way round.  Measured with this seed at k = 1, 4, 16: 34 / 109 /
    297 rows from block 0 to block 2 and 33 / 109 / 273 from block 2 to block 0 (uniformly random rows: 24 and 32 of 1500 at
    k = 16).  196 leaves are FOUR blocks, the fourth of four leaves in the far corner of the box: no compared row's neighbours are
    three blocks away here (that is collapsed_case's part)."""
    c = M.cloud50000_case()
    P = len(c.p)
    assert P == 50000 and (P + M.LEAF - 1) // M.LEAF == 196 and c.block.max() == 3 and (c.block == 3).sum() == P - 3 * M.BLOCK == 848
    check_sampled_case(c)
    assert all(len(rows) == 1000 and (c.block[rows] == b).all() and np.isin(rows, c.rows).all() for b, rows in enumerate(c.plane))
    assert (c.block[c.order[-64:]] == 3).all() and len(c.rows) == 3128
    for src, dst in ((0, 2), (2, 0)):
        mine = np.isin(c.rows, c.plane[src])
        for k, least in ((1, 25), (4, 80), (16, 200)):
            assert reaching(c, mine, dst, k) >= least, (src, dst, k, reaching(c, mine, dst, k))
    assert reaching(c, c.block[c.rows] == 0, 3, 16) == 0 and reaching(c, c.block[c.rows] == 3, 0, 16) == 0


def test_the_collapsed_case_has_neighbours_three_blocks_of_leaves_away():
    """every key but one is 0, the order is the rows' own, and of the 128 compared rows of a block a quarter find their nearest
    neighbour in any one other block.  Expected for uniform neighbours: 32 of 128 at k = 1, 87 at k = 4, 127 at k = 16 (a block
    holds a quarter of the points); required: 20, 70, 120.  Measured with this seed: 30 / 80 / 127 from block 0 to block 3 and
    36 / 91 / 128 from block 3 to block 0; the least of the twelve pairs of blocks 23 / 80 / 123."""
    c = M.collapsed_case()
    P = len(c.p)
    key = M.morton_keys32(c.p)
    assert P == 65001 and (key[:-1] == 0).all() and key[-1] == 0x3FFFFFFF and np.array_equal(c.order, np.arange(P))
    assert (P + M.LEAF - 1) // M.LEAF == 254 and c.block.max() == 3
    check_sampled_case(c)
    assert len(c.rows) == 512 and all((c.block[c.rows] == b).sum() == 128 for b in range(4))
    for src in range(4):
        for dst in range(4):
            if src != dst:
                got = [reaching(c, c.block[c.rows] == src, dst, k) for k in (1, 4, 16)]
                assert got[0] >= 20 and got[1] >= 70 and got[2] >= 120, (src, dst, got)


def test_the_cross_queries_fill_two_sort_blocks_and_end_in_an_invalid_wave():
    p, q = M.cloud50000_case().p, M.two_sort_block_queries()
    ok = M.valid_rows(q)
    assert len(q) == 4200 > 4096 and ok.sum() == 4100 and np.isnan(q).any() and np.isposinf(q).any() and np.isneginf(q).any()
    lo, hi = (M.order_float(b) for b in M.box_bits(p))
    for a in range(3):
        assert (q[ok, a] < lo[a]).sum() >= 50 and (q[ok, a] > hi[a]).sum() >= 50
    sorted_ok = ok[M.morton_order32(q, p)]
    assert sorted_ok[:4100].all() and not sorted_ok[4100:].any()
    waves = [sorted_ok[w:w + 64] for w in range(0, 4200, 64)]
    assert len(waves) == 66 and not waves[65].any() and waves[64].any() and not waves[64].all()
    d, i, c, _ = M.two_sort_block_reference()
    assert (c[ok] == 16).all() and (c[~ok] == 0).all() and (d[:, 0] == 0).sum() == 100
    # the queries' own leaves lie in every block of 64
    first_key = M.morton_keys32(p)[M.cloud50000_case().order][::M.LEAF]
    own = np.searchsorted(first_key, M.morton_keys32(q, p)[ok], side="right") - 1
    assert all(((np.maximum(own, 0) // 64) == b).sum() >= 500 for b in range(3))
    c4 = M.within(M.two_sort_block_reference(), 4, M.max_distance_squared(0.02))[2]
    assert ((c4 > 0) & (c4 < 4)).sum() >= 100 and (c4 == 4).sum() >= 50 and (c4 == 0).sum() >= 100


def test_huge_coordinates_give_infinite_distances_that_are_admitted():
    p = np.array([[1e30, 0, 0], [-1e30, 0, 0], [1e30, 1, 0], [0, 0, 0]], np.float32)
    d2, idx, count, mean = M.knn32(p, k=3)
    assert count.tolist() == [3, 3, 3, 3] and not np.isnan(d2).any()
    assert idx[0].tolist() == [2, 1, 3] and d2[0, 0] == 1.0 and np.isposinf(d2[0, 1:]).all()
    assert idx[3].tolist() == [0, 1, 2] and np.isposinf(d2[3]).all()
