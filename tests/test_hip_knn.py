"""dgr_knn_build / dgr_knn_search on the GPU against the float32 twin of the rule (tests/knn_model.py): idx, dist2, count and
mean_dist2 BIT FOR BIT, every element -- the arithmetic and the tie order are fully specified, so the twin alone decides.  The
shapes are the smallest at which the kernels can go wrong: fewer points than k, the 256-record leaf edge, 16 385 points (a second
block of 64 leaves, more than one sort block of 4096 keys, a partial last leaf), equal keys, zero extents, massive ties, an
outlier that puts everything else into one Morton cell, infinite distances, invalid rows."""
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
        "lattice8", "duplicates", "outlier", "huge", "invalid")


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
