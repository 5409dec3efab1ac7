"""The generalized-ICP entry points (include/dgr_hip.h: dgr_point_covariances, dgr_gicp_scratch_bytes, dgr_gicp_step) and their
Python surface without a GPU: declared, exported and bound; the params structs against the header text; the size function; every
argument error refused with its message before any device call (FAKE pointers: nothing is dereferenced); the wrappers' refusals."""
import ctypes as C
import re

import pytest
import torch

from dgr_amd import _capi, gicp, knn, slam

from abi_checks import FAKE, OTHER, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_point_covariances", "dgr_gicp_scratch_bytes", "dgr_gicp_step")
NAN, INF = float("nan"), float("inf")


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_point_covariances": 11, "dgr_gicp_scratch_bytes": 2, "dgr_gicp_step": 17})
    assert _capi._SIGS["dgr_gicp_scratch_bytes"][0] is C.c_size_t


def _fields(struct):
    body = header_text().split("} %s;" % struct)[0].rsplit("typedef struct %s {" % struct, 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, names = decl.strip().split(None, 1)
            out += [(n.strip(), ctype) for n in names.split(",")]
    return out


def test_the_params_structs_match_the_header_text():
    names = {C.c_int: "int", C.c_float: "float"}
    cov = _fields("dgr_covariance_params")
    assert cov == [("mode", "int"), ("epsilon", "float"), ("min_neighbours", "int"), ("scale_floor", "float"),
                   ("viewpoint[3]", "float"), ("has_viewpoint", "int")]
    P = _capi.CovarianceParams
    assert [n for n, _ in P._fields_] == [n.split("[")[0] for n, _ in cov]
    assert P._fields_[4][1] is _capi._f * 3 and [names[t] for n, t in P._fields_ if n != "viewpoint"] == [t for n, t in cov if "[" not in n]
    assert C.sizeof(P) == 32 and [getattr(P, n).offset for n, _ in P._fields_] == [0, 4, 8, 12, 16, 28]
    step = _fields("dgr_gicp_params")
    assert step == [("dist_max", "float"), ("huber_delta", "float"), ("damping", "float"), ("rcond", "float"), ("min_points", "int")]
    G = _capi.GicpParams
    assert [(n, names[t]) for n, t in G._fields_] == step
    assert C.sizeof(G) == 20 and [getattr(G, n).offset for n, _ in step] == [0, 4, 8, 12, 16]
    text = header_text()
    assert "#define DGR_COV_RAW 0\n" in text and "#define DGR_COV_PLANE 1\n" in text and (_capi.COV_RAW, _capi.COV_PLANE) == (0, 1)


def test_the_header_states_the_rules():
    text = header_text()
    doc = text[text.index("generalized ICP over the kNN index"):text.index("typedef struct dgr_gicp_params")]
    for word in ("(0,1), (0,2), (1,2)", "16 sweeps", "ties keeping column order", "DGR_COV_PLANE", "I - (1 - epsilon) v_0 v_0^T",
                 "__fmul_rn", "__fadd_rn", "((R00 a0 + R01 a1) + R02 a2) + t0", "dist_max * dist_max", "adj(C) / det(C)",
                 "[-[q]x | I]", "exp(xi) T_in", "MUST BE ZERO", "bit 2 singular", "DGR_KNN_MAX_K"):
        assert word in doc, word


def test_the_size_function_refuses_bad_shapes_and_covers_its_parts():
    lib = _capi.load()
    for bad in (0, -1, (1 << 24) + 1, -(1 << 31)):
        assert lib.dgr_gicp_scratch_bytes(bad, 10) == 0 and lib.dgr_gicp_scratch_bytes(10, bad) == 0
    for n in (1, 1920, 100000, 1 << 24):
        last = 0
        for s in (1, 2047, 2048, 2049, 64 * 2048 + 1, 1 << 24):
            b = lib.dgr_gicp_scratch_bytes(n, s)
            # the ticket's header, a 256-byte row per block of 2048 sources, q and idx, the search's own scratch
            assert b % 256 == 0 and b >= 256 + 256 * -(-s // 2048) + 16 * s + lib.dgr_knn_scratch_bytes(n, s) and b >= last
            last = b


def _cov(P=100, points=FAKE, k=10, idx=FAKE, params=True, mode=1, epsilon=1e-3, min_neighbours=4, scale_floor=1e-4,
         viewpoint=(0.0, 0.0, 0.0), has_viewpoint=0, cov=FAKE, normals=FAKE, log_scales=FAKE, quats=FAKE, flags=FAKE):
    p = _capi.CovarianceParams(mode, epsilon, min_neighbours, scale_floor, (C.c_float * 3)(*viewpoint), has_viewpoint) if params else None
    return _capi.load().dgr_point_covariances(None, P, points, k, idx, p, cov, normals, log_scales, quats, flags)


@pytest.mark.parametrize("case, text", [
    (dict(P=0), "n_points must be 1 .. 2^24"), (dict(P=-3), "n_points must be 1 .. 2^24"), (dict(P=(1 << 24) + 1), "n_points must be 1 .. 2^24"),
    (dict(k=0, min_neighbours=3), "k must be 1 .. 16"), (dict(k=17), "k must be 1 .. 16"), (dict(k=-1), "k must be 1 .. 16"),
    (dict(points=None), "points is NULL"), (dict(idx=None), "idx is NULL"), (dict(params=False), "params is NULL"),
    (dict(cov=None, normals=None, log_scales=None, quats=None, flags=None), "no output given"),
    (dict(cov=FAKE + 8), "cov is not 16-byte aligned"), (dict(cov=FAKE + 4), "cov is not 16-byte aligned"),
    (dict(normals=FAKE + 2), "not 4-byte aligned"), (dict(idx=FAKE + 1), "not 4-byte aligned"),
    (dict(mode=2), "unknown mode"), (dict(mode=-1), "unknown mode"),
    (dict(epsilon=0.0), "epsilon must lie in (0, 1]"), (dict(epsilon=1.5), "epsilon must lie in (0, 1]"),
    (dict(epsilon=-1e-3), "epsilon must lie in (0, 1]"), (dict(epsilon=NAN), "epsilon must lie in (0, 1]"),
    (dict(min_neighbours=2), "min_neighbours must be 3 .. k"), (dict(min_neighbours=11), "min_neighbours must be 3 .. k"),
    (dict(k=2, min_neighbours=3), "min_neighbours must be 3 .. k"),
    (dict(scale_floor=NAN), "scale_floor is NaN"),
    (dict(has_viewpoint=1, viewpoint=(0.0, NAN, 0.0)), "viewpoint holds a NaN"), (dict(has_viewpoint=1, viewpoint=(NAN, 0.0, 0.0)), "viewpoint holds a NaN"),
])
def test_covariances_refuse_bad_arguments_before_touching_the_gpu(case, text):
    refused(_cov(**case), "dgr_point_covariances", text)


def _step(index=FAKE, N=100, target=FAKE, target_cov=FAKE, S=50, source=OTHER, source_cov=OTHER, transform_in=FAKE, params=True,
          dist_max=0.5, huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6, scratch=FAKE, transform_out=FAKE, quat=FAKE,
          trans=FAKE, stats=FAKE, idx=FAKE, flags=FAKE):
    p = _capi.GicpParams(dist_max, huber_delta, damping, rcond, min_points) if params else None
    return _capi.load().dgr_gicp_step(None, index, N, target, target_cov, S, source, source_cov, transform_in, p, scratch,
                                      transform_out, quat, trans, stats, idx, flags)


@pytest.mark.parametrize("case, text", [
    (dict(N=0), "n_target must be 1 .. 2^24"), (dict(N=(1 << 24) + 1), "n_target must be 1 .. 2^24"), (dict(N=-1), "n_target must be 1 .. 2^24"),
    (dict(S=0), "n_source must be 1 .. 2^24"), (dict(S=(1 << 24) + 1), "n_source must be 1 .. 2^24"),
    (dict(params=False), "params is NULL"),
    (dict(index=None), "target_index is NULL or not 16-byte aligned"), (dict(index=FAKE + 8), "target_index is NULL or not 16-byte aligned"),
    (dict(target=None), "target is NULL"), (dict(source=None), "source is NULL"),
    (dict(target_cov=FAKE + 4), "target_cov is not 16-byte aligned"), (dict(source_cov=OTHER + 8), "source_cov is not 16-byte aligned"),
    (dict(transform_in=None), "transform_in is NULL"),
    (dict(scratch=None), "scratch is NULL or not 16-byte aligned"), (dict(scratch=FAKE + 4), "scratch is NULL or not 16-byte aligned"),
    (dict(transform_out=None), "transform_out is NULL"),
    (dict(stats=None), "stats is NULL or not 8-byte aligned"), (dict(stats=FAKE + 4), "stats is NULL or not 8-byte aligned"),
    (dict(idx=FAKE + 2), "not 4-byte aligned"), (dict(source=OTHER + 1), "not 4-byte aligned"),
    (dict(dist_max=NAN), "dist_max is NaN or negative"), (dict(dist_max=-0.1), "dist_max is NaN or negative"),
    (dict(huber_delta=NAN), "huber_delta is NaN or negative"), (dict(huber_delta=-1.0), "huber_delta is NaN or negative"),
    (dict(damping=NAN), "damping is NaN or negative"), (dict(damping=-1e-3), "damping is NaN or negative"),
    (dict(rcond=NAN), "rcond is NaN or negative"), (dict(rcond=-1e-8), "rcond is NaN or negative"),
    (dict(min_points=0), "min_points must be at least 1"), (dict(min_points=-4), "min_points must be at least 1"),
])
def test_step_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_step(**case), "dgr_gicp_step", text)


def test_python_surface():
    keyword_only(gicp.point_covariances, ["points", "index"],
                 dict(k=10, include_self=True, mode="plane", epsilon=1e-3, min_neighbours=4, viewpoint=None, scale_floor=1e-4,
                      return_normals=False, return_gaussians=False))
    keyword_only(gicp.gicp_align, ["source", "target"],
                 dict(transform=None, source_cov=None, target_cov=None, target_index=None, iterations=15, max_distance=INF,
                      huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6, return_idx=False, return_flags=False))
    keyword_only(gicp.gicp_step, ["source", "target_index", "transform_in"],
                 dict(transform_out=None, source_cov=None, target_cov=None, max_distance=INF, huber_delta=INF, damping=0.0, rcond=1e-8,
                      min_points=6, return_idx=False, return_flags=False, scratch=None))
    assert gicp.PointCovariances._fields == ("cov", "normals", "log_scales", "quats", "flags", "index")
    assert gicp.GicpResult._fields == ("transform", "quat", "trans", "stats", "idx", "flags")
    for name in ("point_covariances", "gicp_step", "gicp_align", "gaussian_covariances", "unproject_depth", "PointCovariances", "GicpResult"):
        assert getattr(slam, name) is getattr(gicp, name), name


def test_python_surface_refuses_what_it_cannot_read():
    """every check runs on the host, the device check last: CPU tensors reach each of them and never the library"""
    p, t = torch.rand(10, 3), torch.rand(12, 3)
    fake = knn.KnnIndex(t, torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8))
    pc = gicp.point_covariances
    with pytest.raises(ValueError, match="GPU tensors"):
        pc(p)
    with pytest.raises(ValueError, match="points must be float32"):
        pc(p.double())
    with pytest.raises(ValueError, match=r"points is \[N,3\]"):
        pc(torch.rand(10, 4))
    with pytest.raises(ValueError, match="index must be what knn_build returned"):
        pc(p, p)
    with pytest.raises(ValueError, match="index was built for 12 points"):
        pc(p, fake)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="k must be 1 .. 16"):
            pc(p, k=bad)
    with pytest.raises(ValueError, match="mode must be 'plane' or 'raw'"):
        pc(p, mode="full")
    for bad in (0.0, 2.0, -1.0):
        with pytest.raises(ValueError, match=r"epsilon must lie in \(0, 1\]"):
            pc(p, epsilon=bad)
    with pytest.raises(ValueError, match="epsilon must not be NaN"):
        pc(p, epsilon=NAN)
    for bad in (2, 11):
        with pytest.raises(ValueError, match="min_neighbours must be 3 .. k"):
            pc(p, min_neighbours=bad)
    with pytest.raises(ValueError, match="scale_floor must not be NaN"):
        pc(p, scale_floor=NAN)
    with pytest.raises(ValueError, match="viewpoint must not be NaN"):
        pc(p, viewpoint=(0.0, NAN, 1.0))
    with pytest.raises(ValueError, match="viewpoint is three numbers"):
        pc(p, viewpoint=(0.0, 1.0))
    ga = gicp.gicp_align
    with pytest.raises(ValueError, match="GPU tensors"):
        ga(p, t)
    with pytest.raises(ValueError, match="GPU tensors"):
        ga(p, t, transform=torch.eye(4), source_cov=torch.zeros(10, 8), target_cov=torch.zeros(12, 8), target_index=fake,
           max_distance=0.5, huber_delta=2.0, damping=1e-3, return_idx=True, return_flags=True)
    with pytest.raises(ValueError, match="source must be float32"):
        ga(p.double(), t)
    with pytest.raises(ValueError, match=r"target is \[N,3\]"):
        ga(p, torch.rand(12, 2))
    with pytest.raises(ValueError, match="target_index was built for 12 points"):
        ga(p, p, target_index=fake)
    with pytest.raises(ValueError, match=r"source_cov must be a contiguous float32 tensor \[10,8\]"):
        ga(p, t, source_cov=torch.zeros(12, 8))
    with pytest.raises(ValueError, match=r"target_cov must be a contiguous float32 tensor \[12,8\]"):
        ga(p, t, target_cov=torch.zeros(12, 6))
    with pytest.raises(ValueError, match=r"transform is \[4,4\]"):
        ga(p, t, transform=torch.eye(3))
    with pytest.raises(ValueError, match="iterations must be at least 1"):
        ga(p, t, iterations=0)
    for name in ("max_distance", "huber_delta", "damping", "rcond"):
        with pytest.raises(ValueError, match=f"{name} must not be NaN"):
            ga(p, t, **{name: NAN})
        with pytest.raises(ValueError, match=f"{name} must not be negative"):
            ga(p, t, **{name: -1.0})
    with pytest.raises(ValueError, match="min_points must be at least 1"):
        ga(p, t, min_points=0)
    gs = gicp.gicp_step
    with pytest.raises(ValueError, match="GPU tensors"):
        gs(p, fake, torch.eye(4))
    with pytest.raises(ValueError, match="target_index must be what knn_build returned"):
        gs(p, t, torch.eye(4))
    with pytest.raises(ValueError, match=r"transform_in is \[4,4\]"):
        gs(p, fake, torch.eye(4).reshape(16))
    with pytest.raises(ValueError, match="GPU tensors"):
        gicp.point_covariances(p, viewpoint=(0, 0, 0), return_normals=True, return_gaussians=True, mode="raw", include_self=False)


def test_the_torch_helpers_on_the_cpu():
    """gaussian_covariances and unproject_depth are torch ops: they run wherever their inputs live"""
    import numpy as np
    import gicp_model as gm
    s = torch.tensor([[0.3, 0.2, 0.1], [1.0, 1.0, 1.0], [float("nan"), 1.0, 1.0]])
    q = torch.tensor([[2.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.5, 0.5], [1.0, 0.0, 0.0, 0.0]])
    rows = gicp.gaussian_covariances(s, q)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (3, 8)
    assert torch.allclose(rows[0], torch.tensor([0.09, 0.0, 0.0, 0.04, 0.0, 0.01, 0.01 / 0.14, 1.0]), atol=1e-7)
    assert torch.allclose(rows[1, :6], torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]), atol=1e-7) and not rows[2].any()
    with pytest.raises(ValueError, match=r"scales is \[N,3\]"):
        gicp.gaussian_covariances(s, q[:, :3])
    depth = torch.rand(7, 9) + 0.5
    depth[2, 4], depth[0, 0] = 0.0, float("nan")
    for stride in (1, 2, 3):
        got = gicp.unproject_depth(depth, 8.0, 7.5, 4.3, 2.9, stride=stride).numpy()
        want = gm.unproject32(depth.numpy(), 8.0, 7.5, 4.3, 2.9, stride=stride)
        assert got.shape == want.shape == (-(-7 // stride) * -(-9 // stride), 3)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[0]).all()
        ok = ~np.isnan(want)
        assert (np.abs(got[ok] - want[ok]) <= 4 * gm.U32 * np.abs(want[ok])).all()  # three rounded operations per coordinate
    with pytest.raises(ValueError, match="depth must be float32"):
        gicp.unproject_depth(depth.double(), 8.0, 7.5, 4.3, 2.9)
    with pytest.raises(ValueError, match="stride must be positive"):
        gicp.unproject_depth(depth, 8.0, 7.5, 4.3, 2.9, stride=0)
