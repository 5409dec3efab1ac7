"""dgr_point_covariances and dgr_gicp_step on the GPU against the float64 model of their rules (tests/gicp_model.py): flags and
the association bit for bit, every float within the bound the model derives for it, the solve and update against the model fed the
kernel's own sums.  Shapes are the smallest at which the kernels can go wrong: fewer points than k, the 256-thread block edge,
the 2048-source block edge, 64 * 2048 + 1 sources (65 scratch rows: the finisher's second chunk)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dgr_amd import _capi, gicp, knn

import gicp_model as gm
import icp_model as im
from hip_helpers import T
from test_hip_guarded_buffers import GuardedTorch

pytestmark = pytest.mark.gpu
INF = float("inf")
ULP = 2.0 ** -23


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------------------------- covariances
@functools.lru_cache(maxsize=None)
def cloud(name):
    if name.startswith("random"):
        n = int(name[6:])  # (seeds at which the model marks no row at k = 3, 10, 16: seed 256 has three near-collinear triples)
        return np.random.default_rng(n + 1000).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    if name == "corner432":
        return gm.corner_clouds(24, 18)["source"]
    if name == "corner1920":
        return gm.corner_clouds(96, 80, 2)["target"]
    if name == "coincident600":
        return np.tile(np.array([[0.3, -1.2, 5.0]], np.float32), (600, 1))
    if name == "line":
        p = np.zeros((300, 3), np.float32)
        p[:, 0], p[:, 1], p[:, 2] = np.random.default_rng(3).uniform(-2, 2, 300), 0.25, -3.0
        return p
    if name == "lattice":  # the 3 x 3 patch of the plane z = 0, spacing 0.25
        g = np.array([-0.25, 0.0, 0.25], np.float32)
        y, x = np.meshgrid(g, g, indexing="ij")
        return np.stack([x.ravel(), y.ravel(), np.zeros(9, np.float32)], 1)
    if name == "invalid":  # NaN and +-inf rows scattered through a cloud
        p = cloud("random257").copy()
        for j, r in enumerate(np.random.default_rng(5).choice(257, 12, replace=False)):
            p[r, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
        return p
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def neighbours(name, k=16):
    """the kNN twin's rows for k = 16 with the point itself; a smaller k is their first k"""
    return gm.self_neighbours(cloud(name), k)


def run_cov(points, idx, *, mode=gm.PLANE, epsilon=1e-3, min_neighbours=4, scale_floor=1e-4, viewpoint=None,
            want=("cov", "normals", "log_scales", "quats", "flags")):
    """the C entry point on the given rows: a dict of numpy arrays (None for an output not asked for)"""
    P, k = idx.shape
    dev = torch.device("cuda")
    out = dict(cov=torch.empty((P, 8), device=dev), normals=torch.empty((P, 4), device=dev), log_scales=torch.empty((P, 3), device=dev),
               quats=torch.empty((P, 4), device=dev), flags=torch.empty((P,), dtype=torch.uint8, device=dev))
    for t in out.values():
        t.view(torch.uint8).fill_(0xAB)
    params = _capi.CovarianceParams(mode, epsilon, min_neighbours, scale_floor, (C.c_float * 3)(*(viewpoint or (0, 0, 0))),
                                    0 if viewpoint is None else 1)
    p, i = T(points), T(np.ascontiguousarray(idx, np.int32))
    _capi.call("dgr_point_covariances", dev, P, p.data_ptr(), k, i.data_ptr(), params,
               *(out[n].data_ptr() if n in want else None for n in ("cov", "normals", "log_scales", "quats", "flags")))
    return {n: (t.cpu().numpy() if n in want else None) for n, t in out.items()}


def check_cov(got, m, mode, what, v0_outputs=True):
    """every output against the model `m`; marked rows are left out of what depends on v_0: at most 1 % of the rows, unless the
    scene is one whose v_0 is undetermined by construction (`v0_outputs=False`: points on a line)"""
    valid, amb = m["valid"], m["ambiguous"]
    assert np.array_equal(got["flags"], valid.astype(np.uint8)), what
    for name in ("cov", "normals", "log_scales", "quats"):
        assert not bits(got[name])[~valid].any(), (what, name)  # all +0
    if v0_outputs:
        assert amb.sum() <= 0.01 * len(valid), (what, int(amb.sum()))
    if not valid.any():
        return
    cov = got["cov"].astype(np.float64)
    assert np.array_equal(cov[:, 7], m["cov"][:, 7]), what
    assert (np.abs(cov[:, 6] - m["cov"][:, 6]) <= m["sigma_bound"]).all(), what
    rows = valid & ~amb if mode == gm.PLANE else valid
    err = np.abs(cov[:, :6] - m["cov"][:, :6])
    assert (err[rows] <= m["cov_bound"][rows]).all(), (what, float((err - m["cov_bound"])[rows].max()))
    assert np.array_equal(bits(got["normals"][:, 3]), bits(got["cov"][:, 6])), what
    q = got["quats"].astype(np.float64)
    assert (np.abs(np.linalg.norm(q[valid], axis=1) - 1.0) <= 2 * ULP).all() and (q[valid, 0] >= 0).all(), what
    R = np.stack([im.quat_to_rotation(x) for x in q])
    assert (np.abs(np.linalg.det(R[valid]) - 1.0) <= 8 * ULP).all(), what
    # the Gaussian through R diag(exp(2 log s)) R^T against the model's sum max(lambda_i, floor^2) v_i v_i^T: unique whatever the
    # eigenvectors of a degenerate pair are.  fp32 roundings: 2 U |log s| relative on a variance, 4 U on a quaternion's components
    # (8 U on R's entries, twice in the product)
    ls = got["log_scales"].astype(np.float64)
    recon = (R * np.exp(2.0 * ls)[:, None, :]) @ R.transpose(0, 2, 1)
    lam = np.exp(2.0 * m["log_scales"])
    frame = np.stack([m["V"][:, :, 2], m["V"][:, :, 1], m["V"][:, :, 0]], 2)
    model = (frame * lam[:, None, :]) @ frame.transpose(0, 2, 1)
    tol = (32.0 + 4.0 * np.abs(m["log_scales"]).max(1)) * gm.U32 * lam.max(1)
    err = np.abs(recon - model).max((1, 2))
    assert (err[valid] <= tol[valid]).all(), (what, float((err / np.maximum(tol, 1e-300))[valid].max()))
    assert (np.abs(ls - m["log_scales"])[valid] <= 2 * gm.U32 * np.maximum(np.abs(m["log_scales"][valid]), 1.0)).all(), what
    # what depends on v_0, on the rows that determine it
    n = got["normals"].astype(np.float64)[:, :3]
    err = np.abs(n - m["normals"][:, :3]).max(1)
    keep = valid & ~amb
    assert (err[keep] <= m["normal_bound"][keep]).all(), (what, float(err[keep].max()))
    assert (np.abs(R[keep][:, :, 2] - m["normals"][keep, :3]).max(1) <= 16 * gm.U32 + m["normal_bound"][keep]).all(), what
    # ... and on EVERY valid row, marked or not: a unit normal in the span of the two flattest axes, n^T C n <= lambda_1 (a
    # component of 2^-24 along v_2 from the fp32 rounding adds 3 * 2^-48 lambda_2; 4 * 2^-24 lambda_2 is allowed), which a wrong
    # normal misses by its squared component along v_2 times lambda_2
    assert (np.abs(np.linalg.norm(n[valid], axis=1) - 1.0) <= 4 * gm.U32).all(), what
    rayleigh = np.einsum("pa,pab,pb->p", n, m["C"], n)
    lam = m["lam"]
    assert (rayleigh[valid] <= lam[valid, 1] + 4 * gm.U32 * lam[valid, 2]).all(), (what, float((rayleigh - lam[:, 1])[valid].max()))
    assert (np.abs(np.einsum("pa,pa->p", R[:, :, 2], n))[valid] >= 1.0 - 32 * gm.U32).all(), what  # the frame's third axis is the normal
    if not v0_outputs:  # the waiver is for thin triples only: coplanar (sigma at rounding level) and lambda_1 << lambda_2
        assert (m["sigma"][amb] <= 1e-12).all() and (lam[amb, 1] <= 1e-2 * lam[amb, 2]).all(), what


@pytest.mark.parametrize("k", [3, 10, 16])
@pytest.mark.parametrize("name", ["random1", "random4", "random5", "random255", "random256", "random257", "corner432", "corner1920"])
def test_covariances_match_the_model(name, k):
    p, idx = cloud(name), neighbours(name)[:, :k]
    mn = min(4, k)
    for mode, viewpoint in ((gm.PLANE, None), (gm.RAW, (0.0, 0.0, 0.0))):
        m = gm.covariances_model(p, idx, mode=mode, min_neighbours=mn, viewpoint=viewpoint)
        got = run_cov(p, idx, mode=mode, min_neighbours=mn, viewpoint=viewpoint)
        # (the corner clouds at k = 3: a pixel and its two nearest lie on or near a line of the grid, a triple so thin that the
        #  model's worst-case bound cannot promise v_0 at fp32 resolution: it marks nine rows in ten.  As for the line below,
        #  RAW, sigma, n, the flags and the Gaussian are held on every row, the normal to the model on the unmarked rows and to
        #  the neighbourhood itself -- n^T C n <= lambda_1 -- on all of them)
        check_cov(got, m, mode, f"{name} k={k} mode={mode}", v0_outputs=not (name.startswith("corner") and k == 3))
        if name == "random1":
            assert not m["valid"].any()
        if name.startswith("corner") and k == 10:
            assert m["valid"].all()


def test_lists_end_at_the_first_entry_out_of_range_and_nothing_is_read_out_of_bounds():
    p = cloud("random257")
    idx = neighbours("random257")[:, :10].copy()
    rng = np.random.default_rng(8)
    for r in range(257):
        kind = r % 6
        if kind == 1:
            idx[r, rng.integers(3, 10):] = -1
        elif kind == 2:
            idx[r, rng.integers(0, 10)] = 257  # the first index past the cloud
        elif kind == 3:
            idx[r, rng.integers(0, 10)] = rng.choice([2 ** 31 - 1, -2 ** 31, 1 << 24, -2])
        elif kind == 4:
            idx[r, 0] = -1  # an empty neighbourhood
    m = gm.covariances_model(p, idx, mode=gm.RAW)
    assert 0 < m["valid"].sum() < 257 and (m["n"] < 4).any() and (m["n"] == 0).any()
    check_cov(run_cov(p, idx, mode=gm.RAW), m, gm.RAW, "edited rows")


def test_non_finite_rows_coincident_points_and_a_line():
    p, idx = cloud("invalid"), neighbours("invalid")[:, :10]
    idx = idx.copy()
    bad = np.flatnonzero(~np.isfinite(p).all(1))
    idx[::7, 4] = bad[np.arange(len(idx[::7])) % len(bad)]  # invalid points inside otherwise good neighbourhoods
    for mode in (gm.RAW, gm.PLANE):
        m = gm.covariances_model(p, idx, mode=mode)
        assert not m["valid"][bad].any() and not m["valid"][::7].any() and m["valid"].any()
        check_cov(run_cov(p, idx, mode=mode), m, mode, "invalid rows")
    p, idx = cloud("coincident600"), neighbours("coincident600")[:, :10]
    got = run_cov(p, idx)
    assert not got["flags"].any() and not any(bits(got[n]).any() for n in ("cov", "normals", "log_scales", "quats"))
    # a line: lambda_0 = lambda_1 = 0, v_0 is any direction across it: RAW, sigma, n and the flags are determined
    p, idx = cloud("line"), neighbours("line")[:, :10]
    m = gm.covariances_model(p, idx, mode=gm.RAW)
    got = run_cov(p, idx, mode=gm.RAW)
    assert m["valid"].all() and np.array_equal(got["flags"], np.ones(300, np.uint8))
    cov = got["cov"].astype(np.float64)
    assert (np.abs(cov[:, :6] - m["cov"][:, :6]) <= m["cov_bound"]).all() and not cov[:, 6].any() and (cov[:, 7] == 10).all()


def test_the_plane_lattice_in_closed_form():
    p, idx = cloud("lattice"), np.tile(np.arange(9, dtype=np.int32), (9, 1))
    h2 = 0.0625
    raw = run_cov(p, idx, mode=gm.RAW, min_neighbours=3)
    want = np.float32([2 / 3 * h2, 0, 0, 2 / 3 * h2, 0, 0, 0, 9])
    assert (np.abs(raw["cov"].astype(np.float64) - want.astype(np.float64)) <= gm.U32 * want).all()
    assert np.array_equal(raw["normals"], np.tile(np.float32([0, 0, 1, 0]), (9, 1)))
    plane = run_cov(p, idx, mode=gm.PLANE, epsilon=1e-3, min_neighbours=3)
    assert np.array_equal(plane["cov"], np.tile(np.float32([1, 0, 0, 1, 0, np.float32(1.0 - (1.0 - gm.f32(1e-3))), 0, 9]), (9, 1)))
    # toward a viewpoint below the plane the normal turns over
    down = run_cov(p, idx, min_neighbours=3, viewpoint=(0.0, 0.0, -1.0))
    assert np.array_equal(down["normals"][:, :3], np.tile(np.float32([0, 0, -1]), (9, 1)))


def test_both_orientation_rules():
    p, idx = cloud("corner432"), neighbours("corner432")[:, :10]
    toward = run_cov(p, idx, viewpoint=(0.0, 0.0, 0.0))["normals"].astype(np.float64)
    assert (np.sum(toward[:, :3] * (0.0 - p.astype(np.float64)), 1) >= 0).all()  # depth_normals' facing convention
    m = gm.covariances_model(p, idx, viewpoint=(0.0, 0.0, 0.0))
    assert (np.abs(toward[:, :3] - m["normals"][:, :3]).max(1) <= m["normal_bound"]).all()
    plain = run_cov(p, idx)["normals"][:, :3]
    lead = np.take_along_axis(plain, np.abs(plain).argmax(1)[:, None], 1)
    assert (lead > 0).all()
    away = run_cov(p, idx, viewpoint=(0.0, 0.0, 100.0))["normals"][:, :3]
    assert np.array_equal(bits(away), bits(-toward[:, :3].astype(np.float32)))


def test_each_output_alone_carries_the_same_bits():
    p, idx = cloud("random257"), neighbours("random257")[:, :10]
    full = run_cov(p, idx, viewpoint=(0.1, 0.2, 0.3))
    for name in ("cov", "normals", "log_scales", "quats", "flags"):
        one = run_cov(p, idx, viewpoint=(0.1, 0.2, 0.3), want=(name,))
        assert np.array_equal(bits(one[name]), bits(full[name])), name


def test_the_wrapper_builds_its_own_neighbourhoods(monkeypatch):
    guarded = GuardedTorch()
    monkeypatch.setattr(gicp, "torch", guarded)
    monkeypatch.setattr(knn, "torch", guarded)
    for name, include_self in (("corner432", True), ("random257", False), ("random1", True)):
        p = cloud(name)
        out = gicp.point_covariances(T(p), k=10, include_self=include_self, viewpoint=(0, 0, 0), return_normals=True, return_gaussians=True)
        assert guarded.check() >= 8  # index, scratch, the search's two outputs, five outputs
        idx = gm.self_neighbours(p, 10, include_self)
        m = gm.covariances_model(p, idx, viewpoint=(0, 0, 0))
        got = dict(cov=out.cov.cpu().numpy(), normals=out.normals.cpu().numpy(), log_scales=out.log_scales.cpu().numpy(),
                   quats=out.quats.cpu().numpy(), flags=out.flags.cpu().numpy())
        check_cov(got, m, gm.PLANE, name)
    out = gicp.point_covariances(T(cloud("random5")), mode="raw")
    assert out.normals is None and out.log_scales is None and out.quats is None and isinstance(out.index, knn.KnnIndex)


# -------------------------------------------------------------------------------------------------------------------- step
BASE = 1920
SIZES = (1, 2047, 2048, 2049, 64 * 2048 + 1)


@functools.lru_cache(maxsize=None)
def pair_scene():
    """the room corner at 96 x 80, stride 2: 1920 target and 1920 source points, their model covariances rounded to fp32, an
    estimate halfway to the truth, and the twin's association of the base cloud at the radii the tests use"""
    c = gm.corner_clouds(96, 80, 2)
    R, t = im.se3_exp(-0.5 * im.TWIST)
    out = dict(target=c["target"], source=c["source"], truth=c["truth"], T=gm.as_transform(R, t))
    out["cs"] = gm.covariances_model(c["source"], neighbours_of(c["source"])).get("cov").astype(np.float32)
    out["ct"] = gm.covariances_model(c["target"], neighbours_of(c["target"])).get("cov").astype(np.float32)
    q = gm.transform32(out["T"], c["source"])
    out["idx"] = {d: gm.associate(c["target"], q, d) for d in (INF, 0.03)}
    return out


def neighbours_of(p):
    return gm.self_neighbours(p, 10)


def tiled(a, S):
    return None if a is None else np.ascontiguousarray(a[np.arange(S) % len(a)])


def run_step(sc, S, *, covs="both", T_in=None, dist_max=INF, alias=False, scratch=None, source=None, cs=None, ct=None, target=None,
             **kw):
    """gicp_step on the scene's clouds tiled to S sources: (GicpResult as numpy arrays, the device result)"""
    T_in = sc["T"] if T_in is None else T_in
    target = sc["target"] if target is None else target
    source = tiled(sc["source"], S) if source is None else source
    cs = (tiled(sc["cs"], S) if cs is None else cs) if covs in ("both", "source") else None
    ct = (sc["ct"] if ct is None else ct) if covs in ("both", "target") else None
    index = knn.knn_build(T(target))
    t_in = T(np.ascontiguousarray(T_in, np.float32).reshape(4, 4).copy())
    r = gicp.gicp_step(T(source), index, t_in, transform_out=t_in if alias else None, source_cov=None if cs is None else T(cs),
                       target_cov=None if ct is None else T(ct), max_distance=dist_max, return_idx=True, return_flags=True,
                       scratch=scratch, **kw)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in r), (source, cs, ct, target, T_in)


def check_step(got, inputs, *, dist_max=INF, idx=None, what="", entry_ulps=True, **kw):
    """idx and flags bit for bit, the sums within the model's bound, the solve and update against the model fed the kernel's sums.
    `entry_ulps=False`: the pose within 2 ulp OF ONE in place of 2 ulp of each entry -- for a scene whose exact answer has zero
    entries, where both sides hold rounding noise of 1e-19 that no ulp of its own measures"""
    transform, quat, trans, stats, gidx, flags = got
    source, cs, ct, target, T_in = inputs
    step_kw = {k: v for k, v in kw.items() if k == "huber_delta"}
    m = gm.gicp_step_model(target, ct, source, cs, T_in, dist_max=dist_max, idx=idx, **step_kw)
    assert np.array_equal(gidx, m["idx"]), what
    assert np.array_equal(flags, m["flags"]), what
    sums, bound = m["sums"]()
    stats = stats[0]
    assert stats[28] == sums[28], (what, stats[28], sums[28])
    err = np.abs(stats[:28] - sums[:28])
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
    want = gm.solve_update(stats[:29], T_in, **{k: v for k, v in kw.items() if k in ("damping", "rcond", "min_points")})
    assert stats[29] == (1.0 if want["ok"] else 0.0), what
    fig = im.pose_figures(transform, quat, trans, want)
    if entry_ulps:
        assert im.pose_holds(fig), (what, fig)
    else:
        assert np.abs(transform.astype(np.float64) - want["viewmatrix"]).max() <= 2 * ULP and fig["trans_bits"] and fig["last_column"], what
        assert np.abs(quat.astype(np.float64) - want["quat"]).max() <= 2 * ULP and abs(fig["norm"] - 1.0) <= 2 * ULP and fig["r"] >= 0, what
    if want["ok"]:
        assert abs(stats[30] - want["omega"]) <= 1e-9 * max(want["omega"], 1e-6) and abs(stats[31] - want["v"]) <= 1e-9 * max(want["v"], 1e-6)
    else:  # a refused step: the input's bits in every pose output
        assert np.array_equal(bits(transform), bits(np.asarray(T_in, np.float32).reshape(4, 4))) and stats[30] == 0 and stats[31] == 0
        assert np.array_equal(bits(trans), bits(np.asarray(T_in, np.float32).reshape(4, 4)[3, :3]))
    return m, want


@pytest.mark.parametrize("S", SIZES)
def test_step_matches_the_model_at_the_block_edges(S):
    sc = pair_scene()
    got, inputs = run_step(sc, S)
    m, want = check_step(got, inputs, idx=tiled(sc["idx"][INF], S), what=f"S={S}")
    assert want["ok"] == (S >= 6)  # one source: too few pairs, refused
    assert (m["flags"] == 3).all()


@pytest.mark.parametrize("covs", ["source", "target", "neither"])
def test_each_side_of_the_covariances(covs):
    sc = pair_scene()
    got, inputs = run_step(sc, 2049, covs=covs)
    _, want = check_step(got, inputs, idx=tiled(sc["idx"][INF], 2049), what=covs)
    assert want["ok"]


@pytest.mark.parametrize("delta", [0.2, 0.6])  # the median and the 99th percentile of s on this scene
def test_huber_weights(delta):
    sc = pair_scene()
    got, inputs = run_step(sc, 2049, huber_delta=delta)
    m, _ = check_step(got, inputs, idx=tiled(sc["idx"][INF], 2049), huber_delta=delta, what=f"huber {delta}")
    plain = gm.gicp_step_model(inputs[3], inputs[2], inputs[0], inputs[1], inputs[4], idx=m["idx"])
    changed = np.abs(plain["terms"][:, 27] - m["terms"][:, 27]) > 0
    assert 100 <= changed.sum() < 2049 if delta == 0.2 else 1 <= changed.sum() < 100  # weights on hundreds of pairs, and not on all


def test_the_radius_cuts_pairs_and_admits_one_exactly_on_it():
    sc = pair_scene()
    got, inputs = run_step(sc, 2049, dist_max=0.03)
    m, _ = check_step(got, inputs, dist_max=0.03, idx=tiled(sc["idx"][0.03], 2049), what="radius")
    cut = int((m["flags"] == 1).sum())
    assert 200 <= cut <= 1800, cut
    # d2 = 0.0625 = the fp32 square of 0.25: admitted; one ulp of 10.25 further: not
    target = np.float32([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10], [5, 5, 5], [-5, 5, 0], [0, -5, 5], [3, 3, -3]])
    source = target + np.float32([0.25, 0, 0])
    source[1, 0] = np.nextafter(np.float32(10.25), np.float32(11))
    got, inputs = run_step(sc, 8, covs="neither", target=target, source=source, T_in=np.eye(4, dtype=np.float32), dist_max=0.25)
    check_step(got, inputs, dist_max=0.25, what="on the radius", entry_ulps=False)  # (the answer is the pure shift (-0.25, 0, 0))
    assert got[4].tolist() == [0, -1, 2, 3, 4, 5, 6, 7] and got[5].tolist() == [3, 1, 3, 3, 3, 3, 3, 3] and got[3][0, 28] == 7


def test_invalid_rows_on_either_side_and_a_singular_pair():
    sc = pair_scene()
    S = 2049
    source, cs, ct = tiled(sc["source"], S).copy(), tiled(sc["cs"], S).copy(), sc["ct"].copy()
    source[5::97, 1] = np.nan
    source[11::131, 2] = np.inf
    cs[3::53] = 0.0  # invalid source rows
    ct[::9] = 0.0    # invalid target rows
    for covs in ("both", "target"):
        ctc = ct.copy()
        if covs == "target":
            ctc[1::9, :6], ctc[1::9, 7] = np.float32([1, 0, 0, 1, 0, 0]), 1.0  # diag(1, 1, 0): no inverse
        got, inputs = run_step(sc, S, covs=covs, source=source, cs=cs, ct=ctc)
        m, want = check_step(got, inputs, what=f"invalid rows, {covs}")
        kinds = set(m["flags"].tolist())
        assert {0, 1, 3} <= kinds and want["ok"] and ((7 in kinds) == (covs == "target")), kinds


def test_refusals_keep_the_inputs_bits():
    sc = pair_scene()
    # too few pairs
    got, inputs = run_step(sc, 2049, min_points=2050)
    _, want = check_step(got, inputs, idx=tiled(sc["idx"][INF], 2049), min_points=2050, what="min_points")
    assert not want["ok"]
    # a single plane in the point-to-plane limit (C = diag(big, big, 1)): rank 3, refused undamped, solved damped
    g = np.linspace(-1, 1, 12, dtype=np.float32)
    y, x = np.meshgrid(g, g, indexing="ij")
    target = np.stack([x.ravel(), y.ravel(), np.full(144, 2.0, np.float32)], 1)
    source = target + np.float32([0.0, 0.0, 0.05])
    ct = gm.pack_cov(np.diag([1e30, 1e30, 1.0])[None].repeat(144, 0))
    eye = np.eye(4, dtype=np.float32)
    for damping, ok in ((0.0, False), (1e-3, True)):
        got, inputs = run_step(sc, 144, covs="target", target=target, source=source, ct=ct, T_in=eye, damping=damping)
        _, want = check_step(got, inputs, damping=damping, what=f"plane, damping {damping}")
        assert want["ok"] == ok
    assert abs(want["xi"][5] + 0.05) <= 2e-4 and np.abs(want["xi"][[2, 3, 4]]).max() <= 1e-9


def test_aliasing_two_runs_and_one_scratch_for_calls_of_different_sizes():
    sc = pair_scene()
    big = SIZES[-1]
    scratch = torch.zeros((_capi.load().dgr_gicp_scratch_bytes(BASE, big),), dtype=torch.uint8, device="cuda")
    first, inputs = run_step(sc, big, scratch=scratch)
    one, inputs1 = run_step(sc, 1, scratch=scratch)
    again, _ = run_step(sc, big, scratch=scratch, alias=True)
    assert not scratch[:16].any()  # the ticket is left at zero
    for a, b in zip(first, again):
        assert np.array_equal(bits(a), bits(b))
    check_step(one, inputs1, idx=tiled(sc["idx"][INF], 1), what="S=1 on the big scratch")
    fresh, _ = run_step(sc, 1)
    for a, b in zip(one, fresh):
        assert np.array_equal(bits(a), bits(b))


def test_a_captured_align_reads_the_source_at_replay():
    sc = pair_scene()
    other = (sc["source"].astype(np.float64) @ im.se3_exp(0.3 * im.TWIST)[0].T + 0.004).astype(np.float32)
    src, tgt = T(sc["source"].copy()), T(sc["target"])
    cs, ct = T(sc["cs"]), T(sc["ct"])
    index = knn.knn_build(tgt)
    kw = dict(source_cov=cs, target_cov=ct, target_index=index, iterations=4, max_distance=0.5, return_idx=True, return_flags=True)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        gicp.gicp_align(src, tgt, **kw)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = gicp.gicp_align(src, tgt, **kw)
    for now in (other, sc["source"]):
        src.copy_(T(now))
        graph.replay()
        torch.cuda.synchronize()
        eager = gicp.gicp_align(T(now), tgt, **kw)
        for a, b in zip(out, eager):
            assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
        assert out.stats[:, 29].all()


def test_nothing_is_written_outside_the_buffers(monkeypatch):
    guarded = GuardedTorch()
    monkeypatch.setattr(gicp, "torch", guarded)
    monkeypatch.setattr(knn, "torch", guarded)
    sc = pair_scene()
    for S in (1, 2049):
        r = gicp.gicp_align(T(tiled(sc["source"], S)), T(sc["target"]), source_cov=T(tiled(sc["cs"], S)), target_cov=T(sc["ct"]),
                            iterations=2, return_idx=True, return_flags=True)
        assert guarded.check() >= 8  # index, its scratch, the pose, quat and trans, stats, idx, flags, the step's scratch
        assert bool(r.stats[-1, 29]) == (S > 1)


# -------------------------------------------------------------------------------------------------------------- end to end
def test_align_on_the_room_corner_from_the_test_twist():
    """24 x 18, k = 10, PLANE on both sides, from the identity (icp_model.TWIST away from the truth), 15 iterations.  Measured on an
    MI355X (profiles/gicp/measured.txt): the GPU's and the float64 model's errors to the truth agree to the digits printed."""
    c = gm.corner_clouds(24, 18)
    src, tgt = T(c["source"]), T(c["target"])
    cs = gicp.point_covariances(src, k=10)
    ct = gicp.point_covariances(tgt, k=10)
    out = gicp.gicp_align(src, tgt, source_cov=cs, target_cov=ct.cov, target_index=ct.index, iterations=15)
    torch.cuda.synchronize()
    model = gm.gicp_align_model(c["source"], c["target"], source_cov=cs.cov.cpu().numpy(), target_cov=ct.cov.cpu().numpy(), iterations=15)
    start = gm.transform_error(np.eye(4, dtype=np.float32), c["truth"])
    got, want = gm.transform_error(out.transform.cpu().numpy(), c["truth"]), gm.transform_error(model["transform"], c["truth"])
    print(f"gicp_align corner 24x18: start {start}, GPU {got}, float64 model {want}")
    assert out.stats[:, 29].cpu().numpy().all() and all(model["ok"])
    # the fp32 pose resolution pose_holds allows: 2 ulp of an entry (the factorised matrix's condition adds nothing at 10^2), on
    # three entries of a rotation's row and on a translation below 1 m
    slack = 2.0 * ULP * np.sqrt(3.0)
    assert got[0] <= want[0] + slack and got[1] <= want[1] + slack, (got, want)
    assert got[0] < 0.1 * start[0] and got[1] < 0.1 * start[1]
    stats = out.stats.cpu().numpy()
    want_last = gm.solve_update(stats[-1, :29], model["transform"])
    assert np.abs(np.linalg.norm(out.quat.cpu().numpy().astype(np.float64)) - 1) <= 2 * ULP and want_last["ok"]
