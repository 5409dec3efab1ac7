"""The keyframe-overlap entry points (include/dgr_hip.h: dgr_keyframe_overlap*) and their Python surface without a GPU: declared,
exported and bound; the params struct's layout against the header text; the scratch size; every argument error refused with a
message before any device call; select_keyframes and the float64 model (tests/overlap_model.py) on spot values."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from dgr_amd import _capi, slam

import overlap_model as M
from abi_checks import FAKE, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_keyframe_overlap_scratch_bytes", "dgr_keyframe_overlap")
NAN, INF = float("nan"), float("inf")


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_keyframe_overlap": 15, "dgr_keyframe_overlap_scratch_bytes": 4})
    assert _capi._SIGS["dgr_keyframe_overlap_scratch_bytes"][0] is C.c_size_t


def test_params_struct_matches_the_header_text():
    body = header_text().split("} dgr_keyframe_overlap_params;")[0].rsplit("typedef struct dgr_keyframe_overlap_params {", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [("fx", "float"), ("fy", "float"), ("cx", "float"), ("cy", "float"), ("depth_min", "float"),
                      ("depth_max", "float"), ("edge", "float"), ("near_z", "float"), ("depth_tolerance", "float"), ("stride", "int")]
    P = _capi.KeyframeOverlapParams
    assert [(n, {C.c_float: "float", C.c_int: "int"}[t]) for n, t in P._fields_] == fields
    assert C.sizeof(P) == 40 and [getattr(P, n).offset for n, _ in fields] == list(range(0, 40, 4))  # ten four-byte fields


def test_scratch_size():
    f = _capi.load().dgr_keyframe_overlap_scratch_bytes
    for bad in ((0, 8, 1, 1), (8, 0, 1, 1), (-8, 8, 1, 1), (8, -8, 1, 1), (8, 8, 0, 1), (8, 8, -1, 1), (8, 8, 1, 0), (8, 8, 1, -1),
                (8, 8, 1, (1 << 20) + 1), (1 << 8, 1 << 8, 1, 1 << 15), (1 << 16, 1 << 15, 1, 1)):
        assert f(*bad) == 0, bad
    assert f(1, 1, 1, 1 << 20) > 0 and f(1 << 8, 1 << 8, 1, (1 << 15) - 1) > 0 and f(1 << 8, 1 << 8, 2, 1 << 15) > 0
    for shape in ((1, 1, 1, 1), (37, 23, 3, 3), (640, 480, 16, 512), (96, 80, 1, 70), (640, 480, 1, 8)):
        W, H, s, K = shape
        S = -(-W // s) * -(-H // s)
        assert f(*shape) % 16 == 0 and 0 < f(*shape) <= 16 + 16 * K * (S // 1024 + 1), shape  # far less than a word per pair


def _call(width=64, height=48, depth_obs=FAKE, viewmatrix=FAKE, K=3, kf_views=FAKE, kf_depths=None, params=True, scratch=FAKE,
          inside=FAKE, visible=FAKE, valid=FAKE, score=FAKE, flags=None, fx=50.0, fy=50.0, cx=31.5, cy=23.5, lo=0.0, hi=INF,
          edge=20.0, near=0.0, tol=0.05, stride=4):
    p = _capi.KeyframeOverlapParams(fx, fy, cx, cy, lo, hi, edge, near, tol, stride) if params else None
    return _capi.load().dgr_keyframe_overlap(None, width, height, depth_obs, viewmatrix, K, kf_views, kf_depths, p, scratch, inside,
                                             visible, valid, score, flags)


@pytest.mark.parametrize("case, text", [
    (dict(width=0), "width and height"),
    (dict(height=-1), "width and height"),
    (dict(stride=0), "stride"),
    (dict(stride=-2), "stride"),
    (dict(K=0), "n_keyframes must be positive"),
    (dict(K=-1), "n_keyframes must be positive"),
    (dict(K=(1 << 20) + 1), "2^20"),
    (dict(width=1 << 8, height=1 << 8, stride=1, K=1 << 15), "below 2^31"),
    (dict(width=1 << 16, height=1 << 15, stride=1, K=1), "below 2^31"),
    (dict(params=False), "params is NULL"),
    (dict(depth_obs=None), "depth_obs is NULL"),
    (dict(viewmatrix=None), "viewmatrix is NULL"),
    (dict(kf_views=None), "keyframe_viewmatrices is NULL"),
    (dict(scratch=None), "scratch is NULL"),
    (dict(scratch=FAKE + 4), "16-byte aligned"),
    (dict(inside=None), "inside, visible, valid or score is NULL"),
    (dict(visible=None), "inside, visible, valid or score is NULL"),
    (dict(valid=None), "inside, visible, valid or score is NULL"),
    (dict(score=None), "inside, visible, valid or score is NULL"),
    (dict(fx=NAN), "fx and fy"),
    (dict(fx=0.0), "fx and fy"),
    (dict(fy=-50.0), "fx and fy"),
    (dict(fy=INF), "fx and fy"),
    (dict(cx=NAN), "cx or cy is NaN"),
    (dict(cy=NAN), "cx or cy is NaN"),
    (dict(lo=NAN), "depth_min or depth_max is NaN"),
    (dict(hi=NAN), "depth_min or depth_max is NaN"),
    (dict(near=NAN), "near_z is NaN"),
    (dict(edge=NAN), "edge is NaN or negative"),
    (dict(edge=-0.5), "edge is NaN or negative"),
    (dict(tol=NAN), "depth_tolerance is NaN or negative"),
    (dict(tol=-0.01), "depth_tolerance is NaN or negative"),
    (dict(tol=-0.01, kf_depths=FAKE, flags=FAKE), "depth_tolerance is NaN or negative"),
], ids=["W=0", "H<0", "stride=0", "stride<0", "K=0", "K<0", "K>2^20", "KS=2^31", "S=2^31", "params-null", "depth_obs-null",
        "viewmatrix-null", "kf-views-null", "scratch-null", "scratch-misaligned", "inside-null", "visible-null", "valid-null",
        "score-null", "fx-nan", "fx=0", "fy<0", "fy-inf", "cx-nan", "cy-nan", "lo-nan", "hi-nan", "near-nan", "edge-nan", "edge<0",
        "tol-nan", "tol<0", "tol<0-with-depths"])
def test_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_call(**case), "dgr_keyframe_overlap", text)


def test_python_surface():
    keyword_only(slam.keyframe_overlap, ["depth_obs", "viewmatrix", "keyframe_viewmatrices", "fx", "fy", "cx", "cy"],
                 dict(stride=16, edge=20.0, near=0.0, depth_range=(0.0, INF), keyframe_depths=None, depth_tolerance=0.05,
                      return_flags=False))
    assert slam.KeyframeOverlap._fields == ("score", "inside", "visible", "valid", "flags")
    keyword_only(slam.select_keyframes, ["score", "k"], dict(min_overlap=0.0, mode="top", generator=None))
    assert "only host" in " ".join(slam.select_keyframes.__doc__.split())


def test_python_surface_refuses_what_it_cannot_read():
    """Every check runs on the host, the device check last: CPU tensors reach each of them and never the library."""
    d, vm, kv = torch.rand(8, 12), torch.eye(4), torch.eye(4).repeat(3, 1, 1)
    f = lambda *a, **kw: slam.keyframe_overlap(*a, 10.0, 10.0, 5.5, 3.5, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="GPU tensors"):
        f(d, vm, kv)
    with pytest.raises(ValueError, match="GPU tensors"):
        f(d[None], vm, kv, keyframe_depths=torch.rand(3, 1, 8, 12), stride=1, return_flags=True)
    with pytest.raises(ValueError, match="depth_obs must be float32"):
        f(d.double(), vm, kv)
    with pytest.raises(ValueError, match="viewmatrix must be float32"):
        f(d, vm.half(), kv)
    with pytest.raises(ValueError, match="keyframe_viewmatrices must be a tensor"):
        f(d, vm, None)
    with pytest.raises(ValueError, match="keyframe_depths must be float32"):
        f(d, vm, kv, keyframe_depths=torch.zeros(3, 8, 12, dtype=torch.int32))
    for bad in (torch.rand(2, 8, 12), torch.rand(96), torch.rand(0, 12)):
        with pytest.raises(ValueError, match="depth_obs is"):
            f(bad, vm, kv)
    with pytest.raises(ValueError, match=r"viewmatrix is \[4,4\]"):
        f(d, torch.rand(16), kv)
    for bad in (torch.rand(4, 4), torch.rand(3, 16), torch.rand(3, 3, 4)):
        with pytest.raises(ValueError, match=r"keyframe_viewmatrices is \[K,4,4\]"):
            f(d, vm, bad)
    for bad in (torch.rand(2, 8, 12), torch.rand(3, 8, 11), torch.rand(8, 12)):
        with pytest.raises(ValueError, match="keyframe_depths .* is not"):
            f(d, vm, kv, keyframe_depths=bad)
    with pytest.raises(ValueError, match="stride must be positive"):
        f(d, vm, kv, stride=0)
    for kw in (dict(edge=NAN), dict(near=NAN), dict(depth_tolerance=NAN), dict(depth_range=(NAN, 1.0)), dict(depth_range=(0.0, NAN))):
        with pytest.raises(ValueError, match="must not be NaN"):
            f(d, vm, kv, **kw)
    for kw in (dict(edge=-1.0), dict(depth_tolerance=-0.1)):
        with pytest.raises(ValueError, match="must not be negative"):
            f(d, vm, kv, **kw)
    for intr in ((0.0, 10.0), (10.0, -1.0), (INF, 10.0)):
        with pytest.raises(ValueError, match="finite and positive"):
            slam.keyframe_overlap(d, vm, kv, *intr, 5.5, 3.5)
    with pytest.raises(ValueError, match="fx must not be NaN"):
        slam.keyframe_overlap(d, vm, kv, NAN, 10.0, 5.5, 3.5)


def test_select_keyframes_on_the_host():
    """The same torch operations run on CPU tensors: order, ties, padding, filtering, the shuffle."""
    s = torch.tensor([0.2, 0.9, 0.0, 0.9, 0.5, 0.1])
    idx, n = slam.select_keyframes(s, 3)
    assert idx.dtype == torch.int64 and idx.tolist() == [1, 3, 4] and int(n) == 3  # the tie goes to the lower index
    idx, n = slam.select_keyframes(s, 8)
    assert idx.tolist() == [1, 3, 4, 0, 5, -1, -1, -1] and int(n) == 5  # a zero overlap is no overlap; k above K pads
    idx, n = slam.select_keyframes(s, 4, min_overlap=0.45)
    assert idx.tolist() == [1, 3, 4, -1] and int(n) == 3
    idx, n = slam.select_keyframes(s, 2, min_overlap=0.95)
    assert idx.tolist() == [-1, -1] and int(n) == 0
    idx, n = slam.select_keyframes(s, 0)
    assert idx.shape == (0,) and int(n) == 0
    idx, n = slam.select_keyframes(torch.zeros(0), 2)
    assert idx.tolist() == [-1, -1] and int(n) == 0
    seen = set()
    for seed in range(8):
        g = torch.Generator().manual_seed(seed)
        idx, n = slam.select_keyframes(s, 4, min_overlap=0.15, mode="random", generator=g)
        again, _ = slam.select_keyframes(s, 4, min_overlap=0.15, mode="random", generator=torch.Generator().manual_seed(seed))
        assert int(n) == 4 and sorted(idx.tolist()) == [0, 1, 3, 4] and idx.tolist() == again.tolist()
        seen.add(tuple(idx.tolist()))
    assert len(seen) > 1
    idx, n = slam.select_keyframes(s, 2, min_overlap=0.15, mode="random", generator=torch.Generator().manual_seed(0))
    assert int(n) == 2 and set(idx.tolist()) < {0, 1, 3, 4}
    for bad in (dict(score=s.view(2, 3), k=1), dict(score=s, k=-1), dict(score=s, k=1, mode="best"), dict(score=[0.5], k=1),
                dict(score=torch.tensor([1, 2]), k=1)):
        with pytest.raises(ValueError, match="select_keyframes"):
            slam.select_keyframes(**bad)


def test_the_model_follows_the_definition():
    """Spot values that follow from the header's definition: identity poses put every candidate back on its own pixel."""
    W, H = 12, 8
    eye = np.eye(4, dtype=np.float32)
    depth = np.full((H, W), 2.0, np.float32)
    depth[0, 0], depth[2, 4], depth[4, 6] = np.nan, 0.0, np.inf
    m = M.overlap_model(depth, eye, eye[None], 10.0, 10.0, 5.5, 3.5, stride=2, edge=1.5)
    x, y = M.candidates(W, H, 2)
    assert m["S"] == 24 == len(x) and (x[:7].tolist(), y[:7].tolist()) == ([0, 2, 4, 6, 8, 10, 0], [0] * 6 + [2])
    valid = np.ones(24, bool)
    valid[[0, 6 + 2, 12 + 3]] = False
    inside = valid & (x > 1.5) & (x < W - 1.5) & (y > 1.5) & (y < H - 1.5)
    assert np.array_equal(m["flags"][0], valid * 1 + inside * 6) and not m["ambiguous"].any()
    assert m["valid"] == 21 and m["inside"].tolist() == m["visible"].tolist() == [int(inside.sum())] == [13]
    assert m["score"].dtype == np.float32 and m["score"][0] == np.float32(13) / np.float32(21)
    assert np.allclose(m["u"][0][valid], x[valid], atol=1e-12) and np.allclose(m["Z"][0][valid], 2.0)
    # a border on a candidate column is ambiguous, nothing else is
    m = M.overlap_model(depth, eye, eye[None], 10.0, 10.0, 5.5, 3.5, stride=2, edge=2.0)
    assert np.array_equal(m["ambiguous"][0], valid & ((x == 2) | (x == 10) | (y == 2) | (y == 6)))
    # keyframe depths: agreeing, halved, a hole; and a keyframe behind the frame sees nothing
    kd = np.stack([depth, depth * 0.5, np.zeros_like(depth)])
    m = M.overlap_model(depth, eye, np.stack([eye] * 3), 10.0, 10.0, 5.5, 3.5, stride=2, edge=1.5, keyframe_depths=kd)
    assert m["inside"].tolist() == [13, 13, 13] and m["visible"].tolist() == [13, 0, 0]
    assert m["score"].tolist() == [float(np.float32(13) / np.float32(21)), 0.0, 0.0]
    back = eye.copy()
    back[0, 0] = back[2, 2] = -1.0  # a half turn about y
    m = M.overlap_model(depth, eye, back[None], 10.0, 10.0, 5.5, 3.5, stride=2, edge=0.0)
    assert m["inside"].tolist() == [0] and m["valid"] == 21
    m = M.overlap_model(np.zeros((H, W), np.float32), eye, eye[None], 10.0, 10.0, 5.5, 3.5, stride=1)
    assert m["valid"] == 0 and m["score"].tolist() == [0.0]
