"""The hybrid RGB-D entry points (include/dgr_hip.h: dgr_intensity_map, dgr_frame_halve, dgr_rgbd_scratch_bytes, dgr_rgbd_step) and
their Python surface without a GPU: declared, exported and bound; the params struct's layout against the header text; the scratch
size; every argument error refused with a message before any device call; the keyword-only arguments and the ValueErrors of the
Python side."""
import ctypes as C
import re

import pytest
import torch

from dgr_amd import _capi, rgbd, slam

from abi_checks import FAKE, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_intensity_map", "dgr_frame_halve", "dgr_rgbd_scratch_bytes", "dgr_rgbd_step")
NAN, INF = float("nan"), float("inf")
FIELDS = [("fx", "float"), ("fy", "float"), ("cx", "float"), ("cy", "float"), ("depth_min", "float"), ("depth_max", "float"),
          ("dist_max", "float"), ("normal_cos_min", "float"), ("huber_delta", "float"), ("damping", "float"), ("rcond", "float"),
          ("min_points", "int"), ("stride", "int"), ("geo_weight", "float"), ("photo_weight", "float"), ("photo_max", "float"),
          ("photo_huber", "float")]


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_intensity_map": 9, "dgr_frame_halve": 11, "dgr_rgbd_scratch_bytes": 3, "dgr_rgbd_step": 17})
    assert _capi._SIGS["dgr_rgbd_scratch_bytes"][0] is C.c_size_t


def test_params_struct_matches_the_header_text_and_begins_as_the_icp_one():
    body = header_text().split("} dgr_rgbd_params;")[0].rsplit("typedef struct dgr_rgbd_params {", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == FIELDS
    P = _capi.RgbdParams
    assert [(n, {C.c_float: "float", C.c_int: "int"}[t]) for n, t in P._fields_] == fields
    assert C.sizeof(P) == 68 and [getattr(P, n).offset for n, _ in fields] == list(range(0, 68, 4))  # seventeen four-byte fields
    assert P._fields_[:13] == _capi.IcpParams._fields_


def test_scratch_size_is_the_icp_step_s():
    f, g = _capi.load().dgr_rgbd_scratch_bytes, _capi.load().dgr_icp_scratch_bytes
    for bad in ((0, 8, 1), (8, 0, 1), (-8, 8, 1), (8, 8, 0), (1 << 16, 1 << 15, 1)):
        assert f(*bad) == 0, bad
    for shape in ((1, 1, 1), (3, 3, 1), (67, 5, 3), (96, 80, 1), (640, 480, 4), (640, 480, 1)):
        S = -(-shape[0] // shape[2]) * -(-shape[1] // shape[2])
        assert f(*shape) == g(*shape) and f(*shape) >= 16 + 31 * 8 * -(-S // 2048), shape


def _map(width=64, height=48, channels=3, image=FAKE, mask=None, threshold=0.99, imap=FAKE, intensity=None):
    return _capi.load().dgr_intensity_map(None, width, height, channels, image, mask, threshold, imap, intensity)


@pytest.mark.parametrize("case, text", [
    (dict(width=0), "width and height"), (dict(height=-1), "width and height"),
    (dict(width=1 << 16, height=1 << 15), "2^30 pixels"),
    (dict(channels=2), "channels must be 1 or 3"), (dict(channels=0), "channels must be 1 or 3"), (dict(channels=4), "channels"),
    (dict(image=None), "image is NULL"),
    (dict(imap=None), "imap and intensity are both NULL"), (dict(imap=FAKE + 8), "imap is not 16-byte aligned"),
    (dict(imap=FAKE + 4, intensity=FAKE), "imap is not 16-byte aligned"),
    (dict(mask=FAKE, threshold=NAN), "mask_threshold is NaN"),
])
def test_intensity_map_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_map(**case), "dgr_intensity_map", text)


def _halve(width=64, height=48, n=2, planes=FAKE, depth=FAKE, lo=0.0, hi=INF, jump=0.1, planes_out=FAKE, depth_out=FAKE):
    return _capi.load().dgr_frame_halve(None, width, height, n, planes, depth, lo, hi, jump, planes_out, depth_out)


@pytest.mark.parametrize("case, text", [
    (dict(width=1), "at least 2"), (dict(height=1), "at least 2"), (dict(width=0), "at least 2"), (dict(height=-4), "at least 2"),
    (dict(width=1 << 16, height=1 << 15), "2^30 pixels"),
    (dict(n=-1), "n_planes must be 0 .. 64"), (dict(n=65), "n_planes must be 0 .. 64"),
    (dict(n=0, depth=None), "nothing to halve"),
    (dict(planes=None), "planes or planes_out is NULL"), (dict(planes_out=None), "planes or planes_out is NULL"),
    (dict(depth_out=None), "depth_out is NULL"),
    (dict(lo=NAN), "depth_min or depth_max is NaN"), (dict(hi=NAN), "depth_min or depth_max is NaN"),
    (dict(jump=NAN), "max_jump is NaN or negative"), (dict(jump=-0.1), "max_jump is NaN or negative"),
])
def test_frame_halve_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_halve(**case), "dgr_frame_halve", text)


def _step(width=64, height=48, depth_obs=FAKE, vn_obs=None, vn_model=FAKE, intensity_obs=FAKE, imap_model=FAKE, model_view=FAKE,
          view_in=FAKE, params=True, scratch=FAKE, view_out=FAKE, quat=None, trans=None, stats=FAKE, flags=None, fx=50.0, fy=50.0,
          cx=31.5, cy=23.5, lo=0.0, hi=INF, dist_max=0.1, cos_min=0.8, huber=INF, damping=0.0, rcond=1e-8, min_points=6, stride=1,
          geo=1.0, photo=1.0, photo_max=INF, photo_huber=INF):
    p = _capi.RgbdParams(fx, fy, cx, cy, lo, hi, dist_max, cos_min, huber, damping, rcond, min_points, stride, geo, photo, photo_max,
                         photo_huber) if params else None
    return _capi.load().dgr_rgbd_step(None, width, height, depth_obs, vn_obs, vn_model, intensity_obs, imap_model, model_view, view_in,
                                      p, scratch, view_out, quat, trans, stats, flags)


@pytest.mark.parametrize("case, text", [
    (dict(width=0), "width and height"), (dict(height=-1), "width and height"),
    (dict(stride=0), "stride"), (dict(stride=-2), "stride"),
    (dict(width=1 << 16, height=1 << 15), "2^30 candidates"),
    (dict(params=False), "params is NULL"),
    (dict(depth_obs=None), "depth_obs is NULL"),
    (dict(vn_obs=FAKE + 4), "vn_obs is not 16-byte aligned"),
    (dict(vn_model=None), "vn_model is NULL"), (dict(vn_model=FAKE + 8), "16-byte aligned"),
    (dict(intensity_obs=None), "intensity_obs is NULL"),
    (dict(imap_model=None), "imap_model is NULL"), (dict(imap_model=FAKE + 8), "imap_model is NULL or not 16-byte aligned"),
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
    (dict(geo=NAN), "geo_weight is NaN or negative"), (dict(geo=-1.0), "geo_weight is NaN or negative"),
    (dict(photo=NAN), "photo_weight is NaN or negative"), (dict(photo=-0.5), "photo_weight is NaN or negative"),
    (dict(photo_max=NAN), "photo_max is NaN or negative"), (dict(photo_max=-0.1), "photo_max is NaN or negative"),
    (dict(photo_huber=NAN), "photo_huber is NaN or negative"), (dict(photo_huber=-0.1), "photo_huber is NaN or negative"),
    (dict(photo=-1.0, vn_obs=FAKE, quat=FAKE, trans=FAKE, flags=FAKE), "photo_weight"),
])
def test_rgbd_step_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_step(**case), "dgr_rgbd_step", text)


def test_python_surface():
    keyword_only(slam.intensity_map, ["image"], dict(mask_image=None, mask_threshold=0.99))
    keyword_only(slam.halve_frame, ["planes", "depth"], dict(depth_range=(0.0, INF), max_jump=0.1))
    keyword_only(slam.rgbd_align, ["color_obs", "depth_obs", "model_color", "model_depth", "viewmatrix", "model_viewmatrix", "fx", "fy",
                                   "cx", "cy"],
                 dict(levels=1, iterations=10, strides=None, opacity_map=None, silhouette_threshold=0.99, geo_weight=1.0,
                      photo_weight=1.0, photo_max=INF, photo_huber=INF, depth_range=(0.0, INF), max_jump=0.1, dist_max=0.1,
                      normal_cos_min=0.8, use_obs_normals=True, huber_delta=INF, damping=0.0, rcond=1e-8, min_points=6,
                      return_flags=False))
    keyword_only(rgbd.rgbd_step, ["depth_obs", "vn_obs", "vn_model", "intensity_obs", "imap_model", "model_viewmatrix", "viewmatrix_in",
                                  "fx", "fy", "cx", "cy"],
                 dict(viewmatrix_out=None, stride=1, geo_weight=1.0, photo_weight=1.0, photo_max=INF, photo_huber=INF, scratch=None))
    assert slam.RgbdResult._fields == ("viewmatrix", "quat", "trans", "stats", "flags")
    assert slam.rgbd_align is rgbd.rgbd_align and slam.intensity_map is rgbd.intensity_map and slam.halve_frame is rgbd.halve_frame
    assert slam.level_intrinsics(525.0, 520.0, 319.5, 239.5) == (262.5, 260.0, 159.5, 119.5)
    assert slam.level_intrinsics(525.0, 520.0, 319.5, 239.5, 2) == (131.25, 130.0, 79.5, 59.5)


def test_python_surface_refuses_what_it_cannot_read():
    """Every check runs on the host, the device check last: CPU tensors reach each of them and never the library."""
    c, d, vm = torch.rand(3, 8, 12), torch.rand(8, 12) + 1.0, torch.eye(4)
    f = lambda *a, **kw: slam.rgbd_align(*a, 10.0, 10.0, 5.5, 3.5, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="GPU tensors"):
        slam.intensity_map(c)
    with pytest.raises(ValueError, match="GPU tensors"):
        slam.intensity_map(d, mask_image=torch.ones(1, 8, 12))
    with pytest.raises(ValueError, match="GPU tensors"):
        slam.halve_frame(c, d)
    with pytest.raises(ValueError, match="GPU tensors"):
        f(c, d, c, d, None, vm)
    with pytest.raises(ValueError, match="GPU tensors"):
        f(d, d[None], c[:1], d, vm, vm, levels=2, iterations=(2, 1), strides=(2, 1, 1), opacity_map=torch.ones(8, 12))
    with pytest.raises(ValueError, match="image must be float32"):
        slam.intensity_map(c.double())
    with pytest.raises(ValueError, match="image is"):
        slam.intensity_map(torch.rand(2, 8, 12))
    with pytest.raises(ValueError, match="mask_image .* is not"):
        slam.intensity_map(c, mask_image=torch.ones(8, 11))
    with pytest.raises(ValueError, match="mask_threshold must not be NaN"):
        slam.intensity_map(c, mask_threshold=NAN)
    with pytest.raises(ValueError, match="nothing to halve"):
        slam.halve_frame()
    with pytest.raises(ValueError, match=r"planes must be a float32 tensor \[N,H,W\]"):
        slam.halve_frame(d)
    with pytest.raises(ValueError, match="depth .* is not"):
        slam.halve_frame(c, torch.rand(8, 11))
    with pytest.raises(ValueError, match="cannot be halved"):
        slam.halve_frame(torch.rand(2, 1, 12))
    with pytest.raises(ValueError, match="max_jump"):
        slam.halve_frame(c, d, max_jump=-1.0)
    with pytest.raises(ValueError, match="depth_range must not be NaN"):
        slam.halve_frame(c, d, depth_range=(NAN, 1.0))
    with pytest.raises(ValueError, match="color_obs must be float32"):
        f(c.half(), d, c, d, None, vm)
    with pytest.raises(ValueError, match="model_color must be a tensor"):
        f(c, d, None, d, None, vm)
    with pytest.raises(ValueError, match="model_color .* is not"):
        f(c, d, torch.rand(3, 8, 11), d, None, vm)
    with pytest.raises(ValueError, match="color_obs is"):
        f(torch.rand(2, 8, 12), d, c, d, None, vm)
    with pytest.raises(ValueError, match="model_depth .* is not"):
        f(c, d, c, torch.rand(8, 11), None, vm)
    with pytest.raises(ValueError, match="opacity_map .* is not"):
        f(c, d, c, d, None, vm, opacity_map=torch.rand(7, 12))
    with pytest.raises(ValueError, match=r"model_viewmatrix is \[4,4\]"):
        f(c, d, c, d, None, torch.rand(16))
    with pytest.raises(ValueError, match="levels must be at least 1"):
        f(c, d, c, d, None, vm, levels=0)
    with pytest.raises(ValueError, match="without an interior pixel"):
        f(c, d, c, d, None, vm, levels=3)
    with pytest.raises(ValueError, match="iterations must be at least 1"):
        f(c, d, c, d, None, vm, iterations=0)
    with pytest.raises(ValueError, match="one number or one per level"):
        f(c, d, c, d, None, vm, levels=2, iterations=(3, 2, 1))
    with pytest.raises(ValueError, match="one stride per iteration"):
        f(c, d, c, d, None, vm, levels=2, iterations=2, strides=(2, 1))
    with pytest.raises(ValueError, match="stride must be positive"):
        f(c, d, c, d, None, vm, iterations=2, strides=(2, 0))
    with pytest.raises(ValueError, match="min_points must be at least 1"):
        f(c, d, c, d, None, vm, min_points=0)
    for kw in (dict(geo_weight=NAN), dict(photo_weight=NAN), dict(photo_max=NAN), dict(photo_huber=NAN), dict(dist_max=NAN),
               dict(huber_delta=NAN), dict(max_jump=NAN), dict(silhouette_threshold=NAN), dict(depth_range=(0.0, NAN))):
        with pytest.raises(ValueError, match="must not be NaN"):
            f(c, d, c, d, None, vm, **kw)
    for kw in (dict(geo_weight=-1.0), dict(photo_weight=-0.1), dict(photo_max=-1.0), dict(photo_huber=-1e-3), dict(damping=-1e-3)):
        with pytest.raises(ValueError, match="must not be negative"):
            f(c, d, c, d, None, vm, **kw)
    with pytest.raises(ValueError, match="finite and positive"):
        slam.rgbd_align(c, d, c, d, None, vm, 0.0, 10.0, 5.5, 3.5)
    maps = torch.rand(8, 12, 4)
    with pytest.raises(ValueError, match="imap_model must be a contiguous float32 tensor"):
        rgbd.rgbd_step(d, None, maps, d, torch.rand(8, 12, 3), vm, vm, 10.0, 10.0, 5.5, 3.5)
    with pytest.raises(ValueError, match="intensity_obs .* is not"):
        rgbd.rgbd_step(d, None, maps, torch.rand(8, 11), maps, vm, vm, 10.0, 10.0, 5.5, 3.5)
    with pytest.raises(ValueError, match="GPU tensors"):
        rgbd.rgbd_step(d, None, maps, d, maps, vm, vm, 10.0, 10.0, 5.5, 3.5)
