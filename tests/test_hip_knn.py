"""dgr_knn_build / dgr_knn_search on the GPU against the float32 twin of the rule (tests/knn_model.py): idx, dist2, count and
mean_dist2 BIT FOR BIT, every element -- the arithmetic and the tie order are fully specified, so the twin alone decides.  The
shapes are the smallest at which the kernels can go wrong: fewer points than k, the 256-record leaf edge, 16 385 points (a second
block of 64 leaves, more than one sort block of 4096 keys, a partial last leaf), equal keys, zero extents, massive ties, an
outlier that puts everything else into one Morton cell, infinite distances, invalid rows.  Beyond those: every k from 1 to 16, four
blocks of 64 leaves (50 000 and 65 001 points, sampled rows against brute force, every row by what needs none), cross mode with
more than one sort block of queries, and the index itself against the twin of the build (knn_model.morton_order32, index_view)."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from dgr_amd import _capi, knn

import knn_model as M
from abi_checks import ROOT
from hip_helpers import T
from test_hip_guarded_buffers import GuardedTorch

pytestmark = pytest.mark.gpu
KS = (1, 3, 8, 16)
NAMES = ("dist2", "idx", "count", "mean_dist2")


def cloud(n, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3), dtype=np.float32) * np.float32(hi - lo) + np.float32(lo)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def dataset(name):
    if name.startswith("cloud"):
        n = int(name[5:])
        return cloud(n, n)
    if name == "coincident600":
        return np.tile(np.array([[0.3, -1.2, 5.0]], np.float32), (600, 1))
    if name == "line":  # along x: zero extent on y and z
        p = np.zeros((700, 3), np.float32)
        p[:, 0], p[:, 1], p[:, 2] = cloud(700, 21)[:, 0] * 4 - 2, 0.25, -3.0
        return p
    if name == "plane":  # z constant
        p = cloud(900, 22, -1.0, 1.0)
        p[:, 2] = 0.5
        return p
    if name == "lattice8":
        return M.lattice(8)
    if name == "duplicates":
        return np.repeat(cloud(300, 23), 2, axis=0)[np.random.default_rng(24).permutation(600)]
    if name == "outlier":  # 1e6 extents away: everything else falls into one Morton cell
        return np.concatenate([cloud(1000, 25), np.full((1, 3), 1e6, np.float32)])
    if name == "huge":  # d2 = +inf between them and to everything else
        far = np.array([[1e30, 0, 0], [-1e30, 0, 0], [1e30, 1, 0], [0, -1e30, 1e30]], np.float32)
        return np.concatenate([cloud(150, 26), far, cloud(150, 27)])
    if name == "invalid":  # 4 % NaN and +-inf rows scattered through the points
        p = cloud(3000, 28)
        rows = np.random.default_rng(29).choice(3000, 120, replace=False)
        for j, r in enumerate(rows):
            p[r, j % 3] = (np.nan, np.inf, -np.inf)[j % 3 if j % 2 else (j // 2) % 3]
        return p
    if name in M.SMALL:  # no valid row, one, exactly a leaf of them, an infinite extent, subnormal distances
        return M.small_dataset(name)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, exclude_self):
    """the twin's answer for k = 16; every smaller k is its first k (knn_model.first_k)"""
    p = dataset(name)
    if name == "cloud16385" and not exclude_self:
        # (to spare a second brute-force pass: the points are distinct, so a query's own point is its one candidate at d2 = 0 and
        #  the others follow as they do without it)
        assert len(np.unique(p, axis=0)) == len(p)
        d, i, c, _ = reference(name, True)
        assert (d[:, 0] > 0).all() and (c == 16).all()
        own = np.arange(len(p), dtype=np.int32)[:, None]
        d, i = np.concatenate([np.zeros_like(d[:, :1]), d[:, :15]], axis=1), np.concatenate([own, i[:, :15]], axis=1)
        return d, i, np.minimum(c + 1, 16).astype(np.int32), M.mean32(d)
    return M.knn32(p, None, 16, exclude_self=exclude_self, chunk=512)


def arrays(result):
    return tuple(None if t is None else t.cpu().numpy() for t in result)


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.flatnonzero((bits(g) != bits(w)).reshape(len(g), -1).any(axis=1))
        assert not len(bad), f"{what}: {name} differs in {len(bad)} rows, first {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}"


def search(index, queries=None, k=3, **kw):
    return arrays(knn.knn_search(index, queries, k, return_count=True, return_mean=True, **kw))


SELF = ("cloud1", "cloud2", "cloud3", "cloud4", "cloud255", "cloud256", "cloud257", "cloud16385", "coincident600", "line", "plane",
        "lattice8", "duplicates", "outlier", "huge", "invalid") + M.SMALL


@pytest.mark.parametrize("exclude_self", [True, False], ids=["exclude_self", "with_self"])
@pytest.mark.parametrize("name", SELF)
def test_self_mode_gives_the_twins_bits(name, exclude_self):
    ref = reference(name, exclude_self)
    index = knn.knn_build(T(dataset(name)))
    for k in KS:
        assert_same_bits(search(index, None, k, exclude_self=exclude_self), M.first_k(ref, k), f"{name} k={k}")


def test_the_data_sets_are_what_they_claim():
    """the properties the cases above are there for hold in the twin's answers"""
    d, i, c, m = reference("cloud3", True)
    assert c.tolist() == [2, 2, 2] and np.isposinf(m).all()
    d, i, c, m = reference("coincident600", True)
    assert (d == 0).all() and i[0].tolist() == list(range(1, 17)) and i[5].tolist() == [0, 1, 2, 3, 4] + list(range(6, 17))
    d, i, c, m = reference("huge", True)
    assert np.isposinf(d[150:154]).any() and not np.isnan(d).any() and (c == 16).all()
    p = dataset("invalid")
    bad = ~M.valid_rows(p)
    assert bad.sum() == 120 and np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any()
    d, i, c, m = reference("invalid", True)
    assert (c[bad] == 0).all() and (c[~bad] == 16).all() and not np.isin(i, np.flatnonzero(bad)).any()
    d, i, c, m = reference("lattice8", True)
    assert (d[:, :3] == 1).all()
    d, i, c, m = reference("duplicates", True)
    assert (d[:, 0] == 0).all() and (d[:, 1] > 0).all()
    # (tests/test_knn_model.py holds the generators of the next five to more)
    for exclude_self in (True, False):
        d, i, c, m = reference("none_valid", exclude_self)
        assert len(c) == 70 and (i == -1).all() and np.isposinf(d).all() and (c == 0).all() and np.isposinf(m).all()
        d, i, c, m = reference("one_valid", exclude_self)
        assert c.sum() == (0 if exclude_self else 1) and c[37] == (0 if exclude_self else 1) and np.isposinf(m).all()
        assert (i[37, 0] == 37 and d[37, 0] == 0) or exclude_self
    p = dataset("leaf_edge_valid")
    d, i, c, m = reference("leaf_edge_valid", True)
    assert len(p) == 600 and M.valid_rows(p).sum() == 256 and (c[M.valid_rows(p)] == 16).all() and (c[~M.valid_rows(p)] == 0).all()
    p = dataset("overflow_extent")
    d, i, c, m = reference("overflow_extent", True)
    with np.errstate(over="ignore"):
        assert M.valid_rows(p).all() and np.isposinf(p[:, 0].max() - p[:, 0].min()) and (M.quanta32(p)[:, 0] == 0).all()
    assert np.isposinf(d).any() and not np.isnan(d).any() and (c == 16).all()
    d, i, c, m = reference("subnormal", True)
    tiny = np.finfo(np.float32).tiny
    assert (c == 16).all() and ((d > 0) & (d < tiny)).mean() >= 0.9 and (d < tiny).all() and (np.diff(d, axis=1) == 0).any()


@functools.lru_cache(maxsize=None)
def cross_case():
    p = dataset("invalid")
    q = np.concatenate([cloud(500, 31, -0.5, 1.5), p[np.random.default_rng(32).choice(3000, 150, replace=False)], cloud(350, 33)])
    q = q[np.random.default_rng(34).permutation(1000)]
    q[0] = p[np.flatnonzero(M.valid_rows(p))[0]]  # (Q = 1: a query equal to a point)
    q[40] = (np.nan, 0.5, 0.5)        # a NaN query
    q[64] = (3.0, -2.0, 9.0)          # far outside the box
    q[900] = (np.inf, 0.0, 0.0)
    return p, q, M.knn32(p, q, 16, chunk=512)


@pytest.mark.parametrize("Q", [1, 65, 1000])
def test_cross_mode_gives_the_twins_bits(Q):
    p, q, ref = cross_case()
    index = knn.knn_build(T(p))
    want = tuple(a[:Q] for a in ref)
    assert Q < 65 or (want[2][40] == 0 and want[0][0, 0] == 0.0)
    for k in KS:
        assert_same_bits(search(index, T(q[:Q]), k), M.first_k(want, k), f"Q={Q} k={k}")
    if Q == 1000:
        assert want[2][900] == 0 and (want[2][np.isfinite(q).all(axis=1)] == 16).all()


def test_cross_mode_with_more_queries_than_points_and_one_indexed_point():
    p, q, _ = cross_case()
    for pts in (p[:1], p[:70]):
        index = knn.knn_build(T(pts))
        for k in (1, 8):
            assert_same_bits(search(index, T(q), k), M.knn32(pts, q, k), f"P={len(pts)} k={k}")


@pytest.mark.parametrize("radius, k, exclude_self", [(1.0, 8, True), (1.0, 3, True), (float(np.sqrt(2.0)), 16, True), (0.5, 3, True),
                                                     (0.5, 3, False), (0.0, 2, False), (1.0, 16, False)])
def test_max_distance_admits_a_neighbour_exactly_on_the_radius(radius, k, exclude_self):
    p = dataset("lattice8")
    r2 = M.max_distance_squared(radius)
    want = M.knn32(p, None, k, exclude_self=exclude_self, max_dist2=r2)
    if radius == 1.0 and exclude_self:
        assert want[2].min() == 3 and want[2].max() == min(6, k) and (want[0][want[1] >= 0] == 1.0).all()  # all ON the radius
    if radius == 0.5:
        assert (want[2] == (0 if exclude_self else 1)).all()
    got = search(knn.knn_build(T(p)), None, k, exclude_self=exclude_self, max_distance=radius)
    assert_same_bits(got, want, f"radius {radius} k={k}")


def test_max_distance_in_cross_mode():
    p, q, _ = cross_case()
    want = M.knn32(p, q, 8, max_dist2=M.max_distance_squared(0.12))
    assert 0 < (want[2] < 8).sum() < 1000 and (want[2] == 8).any()
    assert_same_bits(search(knn.knn_build(T(p)), T(q), 8, max_distance=0.12), want, "cross radius")


EVERY_K = [(name, flag) for name in ("lattice8", "duplicates", "cloud257", "invalid") for flag in (True, False)] + [("cross", False)]


@pytest.mark.parametrize("name, exclude_self", EVERY_K, ids=[f"{n}-{'exclude_self' if f else 'with_self'}" for n, f in EVERY_K[:-1]] + ["cross"])
def test_every_k_gives_the_twins_bits(name, exclude_self):
    """k = 1 .. 16: every k below the K of its kernel (slot k - 1 as what a candidate has to beat, the j < k output loops, the
    division by k) on data with ties, and K = 4, which KS does not reach"""
    if name == "cross":
        p, q, ref = cross_case()
        queries, kw = T(q), {}
    else:
        p, queries, ref, kw = dataset(name), None, reference(name, exclude_self), {"exclude_self": exclude_self}
    index = knn.knn_build(T(p))
    for k in range(1, 17):
        assert_same_bits(search(index, queries, k, **kw), M.first_k(ref, k), f"{name} k={k}")
    if name == "cross":
        r2 = M.max_distance_squared(0.12)
        for k in (4, 6):
            want = M.knn32(p, q, k, max_dist2=r2)
            assert ((want[2] > 0) & (want[2] < k)).any() and (want[2] == k).any()
            assert_same_bits(search(index, queries, k, max_distance=0.12), want, f"cross radius k={k}")


# ---- the index itself: the answers do not depend on it, so only reading it shows a build that is not the stated one
INDEXED = tuple(f"cloud{n}" for n in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16385)) + (
    "invalid", "coincident600", "line", "outlier", "huge") + M.SMALL


@pytest.mark.parametrize("name", INDEXED)
def test_the_index_is_the_stated_build(name):
    """the box of the valid points, the 30-bit Morton key on it, the stable sort of (key, index) and the leaves' exact boxes, first
    keys and counts, all bit for bit against the twin of the build (knn_model.morton_order32); P on the sort's edges (64 keys per
    round, 1024 per wave, 4096 per workgroup) and the leaf's (256)"""
    p = dataset(name)
    P, ok = len(p), M.valid_rows(p)
    n = int(ok.sum())
    v = M.index_view(knn.knn_build(T(p)).index.cpu().numpy(), P)
    assert v.n_valid == n
    lo, hi = M.box_bits(p)
    assert np.array_equal(v.lo, lo) and np.array_equal(v.hi, hi), (v.lo, lo, v.hi, hi)
    assert np.array_equal(np.sort(v.row), np.arange(P)), "the records' rows are no permutation"
    assert np.array_equal(bits(v.xyz), bits(p[v.row])), "a record does not hold its point's bits"
    order, key = M.morton_order32(p), M.morton_keys32(p)
    assert ok[order[:n]].all() and not ok[order[n:]].any()
    bad = np.flatnonzero(v.row[:n] != order[:n])
    assert not len(bad), f"{len(bad)} of {n} valid records out of the stated order, first at {bad[0]}: row {v.row[bad[0]]}, want {order[bad[0]]}"
    assert np.array_equal(v.row[n:], np.flatnonzero(~ok)), "the invalid rows do not follow in index order"
    for leaf in range(len(v.leaf_count)):
        first = leaf * M.LEAF
        count = min(M.LEAF, n - first)
        if count <= 0:
            assert v.leaf_count[leaf] == 0 and v.leaf_key[leaf] == 0xFFFFFFFF, leaf
            continue
        mine = v.xyz[first:first + count]
        assert v.leaf_count[leaf] == count and v.leaf_key[leaf] == key[v.row[first]], leaf
        assert np.array_equal(v.leaf_lo[leaf], mine.min(axis=0)) and np.array_equal(v.leaf_hi[leaf], mine.max(axis=0)), leaf


# ---- more than two blocks of 64 leaves, more than one sort block of queries
def check_every_row(p, got, k, exclude_self):
    """what holds for a right answer and needs no brute force"""
    d, i, c, m = got
    assert (c == k).all() and (i >= 0).all() and (i < len(p)).all()
    assert (d[:, 1:] >= d[:, :-1]).all()
    assert np.array_equal(bits(d), bits(M.dist2_of_pairs32(p, p, i))), "a dist2 is not the distance to its idx"
    assert (np.diff(np.sort(i, axis=1), axis=1) > 0).all(), "an index twice in a row"
    own = i == np.arange(len(p), dtype=np.int32)[:, None]
    assert not own.any() if exclude_self else own[:, 0].all()
    assert np.array_equal(bits(m), bits(M.mean32(d)))


@pytest.mark.parametrize("exclude_self", [True, False], ids=["exclude_self", "with_self"])
@pytest.mark.parametrize("k", [1, 4, 16])
@pytest.mark.parametrize("case", ["cloud50000", "collapsed"])
def test_self_mode_across_four_blocks_of_leaves(case, k, exclude_self):
    """the sweep own_block, -1, +1, -2, +2, -3, +3.  cloud50000: 196 leaves, the compared rows at the plane where the true
    neighbours are two blocks away; collapsed: 254 leaves in the rows' own order, the true neighbours in every block (the
    conditions: tests/test_knn_model.py).  The compared rows bit for bit, all rows by what needs no brute force."""
    c = M.cloud50000_case() if case == "cloud50000" else M.collapsed_case()
    got = search(knn.knn_build(T(c.p)), None, k, exclude_self=exclude_self)
    want = M.first_k(c.exclude_self if exclude_self else c.with_self, k)
    assert_same_bits(tuple(a[c.rows] for a in got), want, f"{case} k={k}")
    check_every_row(c.p, got, k, exclude_self)


def test_cross_mode_with_two_sort_blocks_of_queries():
    """4200 queries against the 196 leaves of cloud50000: a query sort of two sort blocks, the binary search for the own leaf over
    more than 64 leaves, own leaves in every block, queries outside the box on every side, a last wave of invalid queries alone
    and a mixed one before it (the conditions: tests/test_knn_model.py)"""
    p, q, ref = M.cloud50000_case().p, M.two_sort_block_queries(), M.two_sort_block_reference()
    index = knn.knn_build(T(p))
    for k in (1, 4, 16):
        assert_same_bits(search(index, T(q), k), M.first_k(ref, k), f"k={k}")
    want = M.within(ref, 4, M.max_distance_squared(0.02))
    assert ((want[2] > 0) & (want[2] < 4)).any() and (want[2] == 4).any()
    assert_same_bits(search(index, T(q), 4, max_distance=0.02), want, "radius 0.02")


def test_no_valid_point_in_cross_mode():
    q = cloud(90, 35)
    q[11] = np.nan
    for name in ("none_valid", "one_valid"):
        p = dataset(name)
        index = knn.knn_build(T(p))
        for k in (1, 5, 16):
            want = M.knn32(p, q, k)
            assert (want[2] == (name == "one_valid") * M.valid_rows(q)).all()
            assert_same_bits(search(index, T(q), k), want, f"{name} k={k}")


def test_distcuda2_through_the_drop_in_import(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "diff-gaussian-rasterization_amd", "simple_knn"))
    for name in ("simple_knn", "simple_knn._C"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    distCUDA2 = importlib.import_module("simple_knn._C").distCUDA2
    for name in ("invalid", "cloud16385", "cloud4", "cloud3", "cloud1"):
        got = distCUDA2(T(dataset(name))).cpu().numpy()
        want = M.first_k(reference(name, True), 3)[3]
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), name
    assert np.isposinf(distCUDA2(T(dataset("cloud3"))).cpu().numpy()).all()  # fewer than four valid points: +inf
    assert np.isfinite(distCUDA2(T(dataset("cloud4"))).cpu().numpy()).all()


def test_two_runs_give_equal_bits():
    pts = T(dataset("cloud16385"))
    runs = []
    for _ in range(2):
        index = knn.knn_build(pts)
        r = knn.knn_search(index, None, 8, return_count=True, return_mean=True)
        runs.append((index.index.clone(), *r))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_a_captured_build_and_search_reads_the_points_at_replay():
    first, second = dataset("cloud16385")[:5000], cloud(5000, 41, -2.0, 3.0)
    second[17] = np.nan
    pts, q = T(first.copy()), T(cloud(300, 42))
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        knn.knn_search(knn.knn_build(pts), q, 3)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            index = knn.knn_build(pts)
            own = knn.knn_search(index, None, 3, return_count=True, return_mean=True)
            cross = knn.knn_search(index, q, 3, return_count=True, return_mean=True)
    for now in (second, first):
        pts.copy_(T(now))
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(arrays(own), M.knn32(now, None, 3), "replayed self mode")
        assert_same_bits(arrays(cross), M.knn32(now, q.cpu().numpy(), 3), "replayed cross mode")


def test_nothing_is_written_outside_the_buffers(monkeypatch):
    guarded = GuardedTorch()
    monkeypatch.setattr(knn, "torch", guarded)
    p, q, ref = cross_case()
    for name in ("cloud1", "cloud257", "invalid"):
        index = knn.knn_build(T(dataset(name)))
        got = search(index, None, 16)
        assert guarded.check() >= 6  # index, scratch, four outputs
        assert_same_bits(got, reference(name, True), name)
    index = knn.knn_build(T(p[:300]))
    got = search(index, T(q), 3)  # more queries than points: a scratch of its own
    assert guarded.check() >= 7
    assert_same_bits(got, M.knn32(p[:300], q, 3), "cross")
    big = M.two_sort_block_queries()  # the scratch sized by 4200 queries: two sort blocks and the query records behind them
    assert _capi.load().dgr_knn_scratch_bytes(300, len(big)) > index.scratch.numel()  # (a scratch of its own again)
    got = search(index, T(big), 3)
    assert guarded.check() >= 5  # scratch, four outputs
    assert_same_bits(got, M.knn32(p[:300], big, 3), "cross, two sort blocks")
    assert knn.dist2(T(dataset("cloud257"))).shape == (257,) and guarded.check() >= 3


def test_each_output_alone_with_the_others_null():
    p = dataset("invalid")
    index = knn.knn_build(T(p))
    want = M.first_k(reference("invalid", True), 3)
    P, dev = len(p), index.points.device
    outs = {"dist2": torch.empty((P, 3), dtype=torch.float32, device=dev), "idx": torch.empty((P, 3), dtype=torch.int32, device=dev),
            "count": torch.empty((P,), dtype=torch.int32, device=dev), "mean_dist2": torch.empty((P,), dtype=torch.float32, device=dev)}
    for alone, w in zip(NAMES, want):
        args = [outs[n].data_ptr() if n == alone else None for n in NAMES]
        _capi.call("dgr_knn_search", dev, index.index.data_ptr(), P, index.points.data_ptr(), P, None, _capi.KnnParams(3, 1, float("inf")),
                   index.scratch.data_ptr(), *args)
        g = outs[alone].cpu().numpy()
        assert np.array_equal(bits(g), bits(w)), alone
