"""The ray-cast entry points (include/dgr_hip.h: dgr_tsdf_brick_bytes, dgr_tsdf_bricks, dgr_tsdf_raycast) and their Python surface
without a GPU: declared, exported and bound; the descriptor's layout against the header text; every argument error refused with
its message before any device call (FAKE pointers: nothing is dereferenced); the size of the brick map."""
import ctypes as C
import re

import pytest
import torch

from dgr_amd import _capi, fusion, slam

from abi_checks import FAKE, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_tsdf_brick_bytes", "dgr_tsdf_bricks", "dgr_tsdf_raycast")
NAN, INF = float("nan"), float("inf")


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_tsdf_brick_bytes": 1, "dgr_tsdf_bricks": 5, "dgr_tsdf_raycast": 14})
    assert _capi._SIGS["dgr_tsdf_brick_bytes"][0] is C.c_size_t


def test_the_descriptor_matches_the_header_text():
    body = header_text().split("} dgr_raycast_params;")[0].rsplit("typedef struct dgr_raycast_params {", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, names = decl.strip().split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [(n, "float") for n in ("fx", "fy", "cx", "cy", "depth_min", "depth_max", "step", "min_weight")]
    P = _capi.RaycastParams
    assert [(n, "float") for n, t in P._fields_ if t is C.c_float] == fields
    assert C.sizeof(P) == 32 and [getattr(P, n).offset for n, _ in fields] == list(range(0, 32, 4))


def test_the_header_states_the_rule():
    text = header_text()
    doc = text[text.index("Ray-casting the TSDF volume"):text.index("typedef struct dgr_raycast_params")]
    for word in ("R^T (z d_c - t)", "fused multiply-add", "never accumulated", "floor(q)", "0 <= i <= n - 2", ">= min_weight",
                 "smallest k", "flags bit 0", "flags bit 1", "flags bit 2", "F_(k*-1) / (F_(k*-1) - F_k*)", "central", "face the camera",
                 "NOT consulted", "8 x 8 x 8", "ceil((nz-1)/8)", "SAME BITS", "wherever it lies", "hipGraph", "out-of-range read"):
        assert word in doc, word


def _grid(nx=20, ny=12, nz=9, voxel=0.1):
    return _capi.TsdfGrid(nx, ny, nz, (C.c_float * 3)(0.0, 0.0, 0.0), voxel)


def _raycast(grid=True, volume=FAKE, color=FAKE, bricks=FAKE, V=2, W=64, H=48, views=FAKE, params=True, fx=60.0, fy=60.0, lo=0.05,
             hi=INF, step=0.05, min_weight=1.0, depth=FAKE, vnmap=FAKE, color_out=FAKE, flags=FAKE, **g):
    p = _capi.RaycastParams(fx, fy, 31.5, 23.5, lo, hi, step, min_weight) if params else None
    return _capi.load().dgr_tsdf_raycast(None, _grid(**g) if grid else None, volume, color, bricks, V, W, H, views, p, depth, vnmap,
                                         color_out, flags)


@pytest.mark.parametrize("case, text", [
    (dict(grid=False), "grid is NULL"), (dict(params=False), "params is NULL"),
    (dict(volume=None), "volume is NULL"), (dict(views=None), "viewmatrices is NULL"),
    (dict(nx=0), "must be positive"), (dict(nz=-1), "must be positive"), (dict(nx=2048, ny=1024, nz=1024), "fewer than 2^31 samples"),
    (dict(voxel=0.0), "voxel_size must be finite and positive"), (dict(voxel=NAN), "voxel_size must be finite and positive"),
    (dict(voxel=INF), "voxel_size must be finite and positive"),
    (dict(fx=0.0), "fx and fy"), (dict(fy=-1.0), "fx and fy"), (dict(fx=NAN), "fx and fy"), (dict(fy=INF), "fx and fy"),
    (dict(step=0.0), "step must be finite and positive"), (dict(step=-0.1), "step must be finite and positive"),
    (dict(step=NAN), "step must be finite and positive"), (dict(step=INF), "step must be finite and positive"),
    (dict(min_weight=NAN), "min_weight is NaN"),
    (dict(lo=NAN), "depth_min must be finite and depth_max not NaN"), (dict(hi=NAN), "depth_min must be finite and depth_max not NaN"),
    (dict(lo=-INF), "depth_min must be finite and depth_max not NaN"),
    (dict(V=0), "n_views must be at least 1"), (dict(V=-2), "n_views must be at least 1"), (dict(V=65536), "n_views must be at least 1"),
    (dict(W=0), "width and height"), (dict(H=0), "width and height"), (dict(H=-3), "width and height"), (dict(W=1 << 16, H=1 << 15), "width and height"),
    (dict(depth=None, vnmap=None, color_out=None, flags=None), "no output given"),
    (dict(color=None), "color_out asked for of a volume without colour"),
    (dict(vnmap=FAKE + 8), "vnmap is not 16-byte aligned"), (dict(vnmap=FAKE + 4), "vnmap is not 16-byte aligned"),
    (dict(volume=FAKE + 4), "volume is not 8-byte aligned"), (dict(color=FAKE + 8), "color is not 16-byte aligned"),
    (dict(views=FAKE + 2), "not 4-byte aligned"), (dict(depth=FAKE + 1), "not 4-byte aligned"), (dict(color_out=FAKE + 2), "not 4-byte aligned"),
])
def test_raycast_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_raycast(**case), "dgr_tsdf_raycast", text)


def _bricks(grid=True, volume=FAKE, min_weight=1.0, bricks=FAKE, **g):
    return _capi.load().dgr_tsdf_bricks(None, _grid(**g) if grid else None, volume, min_weight, bricks)


@pytest.mark.parametrize("case, text", [
    (dict(grid=False), "grid is NULL"), (dict(ny=0), "must be positive"), (dict(nx=1 << 16, ny=1 << 16, nz=1), "fewer than 2^31 samples"),
    (dict(voxel=-1.0), "voxel_size must be finite and positive"), (dict(volume=None), "volume is NULL"),
    (dict(volume=FAKE + 4), "volume is not 8-byte aligned"), (dict(min_weight=NAN), "min_weight is NaN"), (dict(bricks=None), "bricks is NULL"),
])
def test_bricks_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_bricks(**case), "dgr_tsdf_bricks", text)


def test_brick_bytes_follow_the_formula():
    f = _capi.load().dgr_tsdf_brick_bytes
    assert f(None) == 0 and f(_grid(nx=2048, ny=1024, nz=1024)) == 0 and f(_grid(nx=0)) == 0 and f(_grid(voxel=NAN)) == 0
    for dims in ((1, 1, 1), (2, 2, 2), (9, 9, 9), (10, 9, 9), (17, 10, 9), (40, 36, 28), (256, 256, 256), (257, 258, 3), (5, 1, 7)):
        want = 1
        for n in dims:
            want *= -(-(n - 1) // 8)
        assert f(_grid(*dims)) == want, dims
        assert fusion._brick_shape(dims) == tuple(-(-(n - 1) // 8) for n in reversed(dims))


def test_python_surface():
    keyword_only(slam.tsdf_raycast, ["vol", "viewmatrices", "fx", "fy", "cx", "cy", "H", "W"],
                 dict(depth_range=(0.05, INF), step=None, min_weight=1.0, bricks="build", normals=True, color=None, return_flags=False))
    keyword_only(slam.tsdf_bricks, ["vol"], dict(min_weight=1.0))
    assert slam.TsdfRaycast._fields == ("depth", "vnmap", "color", "flags")
    assert slam.tsdf_raycast is fusion.tsdf_raycast and slam.tsdf_bricks is fusion.tsdf_bricks and slam.TsdfRaycast is fusion.TsdfRaycast


def test_python_surface_refuses_what_it_cannot_read():
    """every check runs on the host, the device check last: CPU tensors reach each of them and never the library"""
    v = slam.TsdfVolume((0, 0, 0), 0.1, (12, 10, 9), device="cpu")
    m = torch.eye(4).repeat(2, 1, 1)
    ok = dict(fx=10.0, fy=10.0, cx=4.0, cy=3.0, H=6, W=8)
    f = slam.tsdf_raycast
    with pytest.raises(ValueError, match="must live on the GPU"):
        f(v, m, **ok)
    with pytest.raises(ValueError, match="must live on the GPU"):
        f(v, m[0], **ok, bricks=None, normals=False, color=False, return_flags=True, step=0.2, depth_range=(0.0, 3.0))
    with pytest.raises(ValueError, match="must live on the GPU"):
        f(v, m, **ok, bricks=torch.zeros((1, 2, 2), dtype=torch.uint8))
    with pytest.raises(ValueError, match="must be a TsdfVolume"):
        f(v.volume, m, **ok)
    with pytest.raises(ValueError, match="viewmatrices must be a tensor"):
        f(v, None, **ok)
    with pytest.raises(ValueError, match=r"viewmatrices must be \[V, 4, 4\]"):
        f(v, torch.eye(4)[None, None], **ok)
    with pytest.raises(ValueError, match="viewmatrices must be float32"):
        f(v, m.double(), **ok)
    with pytest.raises(ValueError, match="viewmatrices must be float32"):
        f(v, m[:, :3], **ok)
    with pytest.raises(ValueError, match="H and W must be positive"):
        f(v, m, 10.0, 10.0, 4.0, 3.0, 0, 8)
    with pytest.raises(ValueError, match="fx and fy"):
        f(v, m, 0.0, 10.0, 4.0, 3.0, 6, 8)
    with pytest.raises(ValueError, match="fx and fy"):
        f(v, m, 10.0, NAN, 4.0, 3.0, 6, 8)
    for bad in (0.0, -0.1, NAN, INF):
        with pytest.raises(ValueError, match="step must be finite and positive"):
            f(v, m, **ok, step=bad)
    for bad in ((NAN, 1.0), (0.0, NAN), (-INF, 1.0)):
        with pytest.raises(ValueError, match="depth_range"):
            f(v, m, **ok, depth_range=bad)
    with pytest.raises(ValueError, match="min_weight must not be NaN"):
        f(v, m, **ok, min_weight=NAN)
    with pytest.raises(ValueError, match="color=False"):
        f(slam.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), color=False, device="cpu"), m, **ok, color=True)
    with pytest.raises(ValueError, match="bricks must be the uint8"):
        f(v, m, **ok, bricks=torch.zeros((2, 2, 2), dtype=torch.uint8))
    with pytest.raises(ValueError, match="bricks must be the uint8"):
        f(v, m, **ok, bricks=torch.zeros((1, 2, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match='bricks must be "build", None or a tensor'):
        f(v, m, **ok, bricks="auto")
    with pytest.raises(ValueError, match="must live on the GPU"):
        slam.tsdf_bricks(v)
    with pytest.raises(ValueError, match="must be a TsdfVolume"):
        slam.tsdf_bricks(v.volume)
    with pytest.raises(ValueError, match="min_weight must not be NaN"):
        slam.tsdf_bricks(v, min_weight=NAN)
