"""The ICP entry points (include/dgr_hip.h: dgr_depth_normals, dgr_icp_scratch_bytes, dgr_icp_step) and their Python surface
without a GPU: declared, exported and bound; the params struct's layout against the header text; the scratch size; every argument
error refused with a message before any device call; the keyword-only arguments and the ValueErrors of the Python side."""
import ctypes as C
import re

import pytest
import torch

from dgr_amd import _capi, icp, slam

from abi_checks import FAKE, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_depth_normals", "dgr_icp_scratch_bytes", "dgr_icp_step")
NAN, INF = float("nan"), float("inf")
FIELDS = [("fx", "float"), ("fy", "float"), ("cx", "float"), ("cy", "float"), ("depth_min", "float"), ("depth_max", "float"),
          ("dist_max", "float"), ("normal_cos_min", "float"), ("huber_delta", "float"), ("damping", "float"), ("rcond", "float"),
          ("min_points", "int"), ("stride", "int")]


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_depth_normals": 14, "dgr_icp_scratch_bytes": 3, "dgr_icp_step": 15})
    assert _capi._SIGS["dgr_icp_scratch_bytes"][0] is C.c_size_t


def test_params_struct_matches_the_header_text():
    body = header_text().split("} dgr_icp_params;")[0].rsplit("typedef struct dgr_icp_params {", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == FIELDS
    P = _capi.IcpParams
    assert [(n, {C.c_float: "float", C.c_int: "int"}[t]) for n, t in P._fields_] == fields
    assert C.sizeof(P) == 52 and [getattr(P, n).offset for n, _ in fields] == list(range(0, 52, 4))  # thirteen four-byte fields


def test_scratch_size():
    f = _capi.load().dgr_icp_scratch_bytes
    for bad in ((0, 8, 1), (8, 0, 1), (-8, 8, 1), (8, -8, 1), (8, 8, 0), (8, 8, -1), (1 << 16, 1 << 15, 1)):
        assert f(*bad) == 0, bad
    assert f(1 << 16, 1 << 15, 2) > 0
    for W, H, s in ((1, 1, 1), (3, 3, 1), (67, 5, 3), (96, 80, 1), (640, 480, 4), (640, 480, 1)):
        S = -(-W // s) * -(-H // s)
        blocks = -(-S // 2048)
        assert f(W, H, s) % 16 == 0 and 16 + 29 * 8 * blocks <= f(W, H, s) <= 256 + 256 * blocks, (W, H, s)
    assert f(640, 480, 4) < f(640, 480, 2) < f(640, 480, 1)  # one allocation for the largest grid serves every stride


def _normals(width=64, height=48, depth=FAKE, mask=None, threshold=0.99, fx=50.0, fy=50.0, cx=31.5, cy=23.5, lo=0.0, hi=INF,
             jump=0.1, vnmap=FAKE):
    return _capi.load().dgr_depth_normals(None, width, height, depth, mask, threshold, fx, fy, cx, cy, lo, hi, jump, vnmap)


@pytest.mark.parametrize("case, text", [
    (dict(width=0), "width and height"), (dict(height=-1), "width and height"),
    (dict(width=1 << 16, height=1 << 15), "2^30 pixels"),
    (dict(depth=None), "depth is NULL"), (dict(vnmap=None), "vnmap is NULL"), (dict(vnmap=FAKE + 8), "16-byte aligned"),
    (dict(fx=NAN), "fx and fy"), (dict(fx=0.0), "fx and fy"), (dict(fy=-50.0), "fx and fy"), (dict(fy=INF), "fx and fy"),
    (dict(cx=NAN), "cx or cy is NaN"), (dict(cy=NAN), "cx or cy is NaN"),
    (dict(lo=NAN), "depth_min or depth_max is NaN"), (dict(hi=NAN), "depth_min or depth_max is NaN"),
    (dict(jump=NAN), "max_jump is NaN or negative"), (dict(jump=-0.1), "max_jump is NaN or negative"),
    (dict(mask=FAKE, threshold=NAN), "mask_threshold is NaN"),
])
def test_depth_normals_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_normals(**case), "dgr_depth_normals", text)


def _step(width=64, height=48, depth_obs=FAKE, vn_obs=None, vn_model=FAKE, model_view=FAKE, view_in=FAKE, params=True, scratch=FAKE,
          view_out=FAKE, quat=None, trans=None, stats=FAKE, flags=None, fx=50.0, fy=50.0, cx=31.5, cy=23.5, lo=0.0, hi=INF,
          dist_max=0.1, cos_min=0.8, huber=INF, damping=0.0, rcond=1e-8, min_points=6, stride=1):
    p = _capi.IcpParams(fx, fy, cx, cy, lo, hi, dist_max, cos_min, huber, damping, rcond, min_points, stride) if params else None
    return _capi.load().dgr_icp_step(None, width, height, depth_obs, vn_obs, vn_model, model_view, view_in, p, scratch, view_out,
                                     quat, trans, stats, flags)


@pytest.mark.parametrize("case, text", [
    (dict(width=0), "width and height"), (dict(height=-1), "width and height"),
    (dict(stride=0), "stride"), (dict(stride=-2), "stride"),
    (dict(width=1 << 16, height=1 << 15), "2^30 candidates"),
    (dict(params=False), "params is NULL"),
    (dict(depth_obs=None), "depth_obs is NULL"),
    (dict(vn_obs=FAKE + 4), "vn_obs is not 16-byte aligned"),
    (dict(vn_model=None), "vn_model is NULL"), (dict(vn_model=FAKE + 8), "16-byte aligned"),
    (dict(model_view=None), "model_viewmatrix is NULL"), (dict(view_in=None), "viewmatrix_in is NULL"),
    (dict(scratch=None), "scratch is NULL"), (dict(scratch=FAKE + 4), "16-byte aligned"),
    (dict(view_out=None), "viewmatrix_out is NULL"),
    (dict(stats=None), "stats is NULL"), (dict(stats=FAKE + 4), "8-byte aligned"),
    (dict(fx=NAN), "fx and fy"), (dict(fx=0.0), "fx and fy"), (dict(fy=-50.0), "fx and fy"), (dict(fy=INF), "fx and fy"),
    (dict(cx=NAN), "cx or cy is NaN"), (dict(cy=NAN), "cx or cy is NaN"),
    (dict(lo=NAN), "depth_min or depth_max is NaN"), (dict(hi=NAN), "depth_min or depth_max is NaN"),
    (dict(dist_max=NAN), "dist_max is NaN or negative"), (dict(dist_max=-0.1), "dist_max is NaN or negative"),
    (dict(cos_min=NAN), "normal_cos_min"), (dict(cos_min=1.5), "normal_cos_min"), (dict(cos_min=-1.01), "normal_cos_min"),
    (dict(huber=NAN), "huber_delta is NaN or negative"), (dict(huber=-1.0), "huber_delta is NaN or negative"),
    (dict(damping=NAN), "damping is NaN or negative"), (dict(damping=-1e-3), "damping is NaN or negative"),
    (dict(rcond=NAN), "rcond is NaN or negative"), (dict(rcond=-1e-8), "rcond is NaN or negative"),
    (dict(min_points=0), "min_points"), (dict(min_points=-3), "min_points"),
    (dict(min_points=0, vn_obs=FAKE, quat=FAKE, trans=FAKE, flags=FAKE), "min_points"),
])
def test_icp_step_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_step(**case), "dgr_icp_step", text)


def test_python_surface():
    keyword_only(slam.depth_normals, ["depth", "fx", "fy", "cx", "cy"],
                 dict(depth_range=(0.0, INF), max_jump=0.1, mask_image=None, mask_threshold=0.99))
    keyword_only(slam.icp_align, ["depth_obs", "model_depth", "viewmatrix", "model_viewmatrix", "fx", "fy", "cx", "cy"],
                 dict(iterations=10, strides=None, opacity_map=None, silhouette_threshold=0.99, depth_range=(0.0, INF), max_jump=0.1,
                      dist_max=0.1, normal_cos_min=0.8, use_obs_normals=True, huber_delta=INF, damping=0.0, rcond=1e-8,
                      min_points=6, return_flags=False))
    assert slam.IcpResult._fields == ("viewmatrix", "quat", "trans", "stats", "flags")
    assert slam.icp_align is icp.icp_align and slam.depth_normals is icp.depth_normals and slam.IcpResult is icp.IcpResult


def test_python_surface_refuses_what_it_cannot_read():
    """Every check runs on the host, the device check last: CPU tensors reach each of them and never the library."""
    d, vm = torch.rand(8, 12) + 1.0, torch.eye(4)
    n = lambda *a, **kw: slam.depth_normals(*a, 10.0, 10.0, 5.5, 3.5, **kw)  # noqa: E731
    f = lambda *a, **kw: slam.icp_align(*a, 10.0, 10.0, 5.5, 3.5, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="GPU tensors"):
        n(d)
    with pytest.raises(ValueError, match="GPU tensors"):
        n(d[None], mask_image=torch.ones(1, 8, 12))
    with pytest.raises(ValueError, match="GPU tensors"):
        f(d, d, None, vm)
    with pytest.raises(ValueError, match="GPU tensors"):
        f(d[None], d[None], vm, vm, opacity_map=torch.ones(8, 12), strides=(2, 1), iterations=2, use_obs_normals=False)
    with pytest.raises(ValueError, match="depth must be float32"):
        n(d.double())
    with pytest.raises(ValueError, match="mask_image .* is not"):
        n(d, mask_image=torch.ones(8, 11))
    with pytest.raises(ValueError, match="depth_obs must be float32"):
        f(d.half(), d, None, vm)
    with pytest.raises(ValueError, match="model_depth must be a tensor"):
        f(d, None, None, vm)
    for bad in (torch.rand(2, 8, 12), torch.rand(96), torch.rand(0, 12)):
        with pytest.raises(ValueError, match="depth_obs is"):
            f(bad, d, None, vm)
    with pytest.raises(ValueError, match="model_depth .* is not"):
        f(d, torch.rand(8, 11), None, vm)
    with pytest.raises(ValueError, match="opacity_map .* is not"):
        f(d, d, None, vm, opacity_map=torch.rand(7, 12))
    with pytest.raises(ValueError, match=r"model_viewmatrix is \[4,4\]"):
        f(d, d, None, torch.rand(16))
    with pytest.raises(ValueError, match=r"viewmatrix is \[4,4\]"):
        f(d, d, torch.rand(3, 4), vm)
    with pytest.raises(ValueError, match="viewmatrix must be float32"):
        f(d, d, vm.double(), vm)
    with pytest.raises(ValueError, match="iterations must be at least 1"):
        f(d, d, None, vm, iterations=0)
    with pytest.raises(ValueError, match="one stride per iteration"):
        f(d, d, None, vm, iterations=3, strides=(2, 1))
    with pytest.raises(ValueError, match="stride must be positive"):
        f(d, d, None, vm, iterations=2, strides=(2, 0))
    with pytest.raises(ValueError, match="min_points must be at least 1"):
        f(d, d, None, vm, min_points=0)
    for kw in (dict(dist_max=NAN), dict(normal_cos_min=NAN), dict(huber_delta=NAN), dict(damping=NAN), dict(rcond=NAN),
               dict(max_jump=NAN), dict(silhouette_threshold=NAN), dict(depth_range=(NAN, 1.0)), dict(depth_range=(0.0, NAN))):
        with pytest.raises(ValueError, match="must not be NaN"):
            f(d, d, None, vm, **kw)
    for kw in (dict(dist_max=-1.0), dict(huber_delta=-0.1), dict(damping=-1e-3), dict(rcond=-1e-9), dict(max_jump=-0.1)):
        with pytest.raises(ValueError, match="must not be negative"):
            f(d, d, None, vm, **kw)
    for bad in (-1.5, 1.5):
        with pytest.raises(ValueError, match="normal_cos_min"):
            f(d, d, None, vm, normal_cos_min=bad)
    for intr in ((0.0, 10.0), (10.0, -1.0), (INF, 10.0)):
        with pytest.raises(ValueError, match="finite and positive"):
            slam.icp_align(d, d, None, vm, *intr, 5.5, 3.5)
        with pytest.raises(ValueError, match="finite and positive"):
            slam.depth_normals(d, *intr, 5.5, 3.5)
    with pytest.raises(ValueError, match="fx must not be NaN"):
        slam.icp_align(d, d, None, vm, NAN, 10.0, 5.5, 3.5)
    with pytest.raises(ValueError, match="max_jump must not be negative"):
        n(d, max_jump=-1.0)
