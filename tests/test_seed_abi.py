"""The map-expansion entry points (include/dgr_hip.h: dgr_seed_*) without a GPU: declared, exported and bound; the descriptor's
layout; every argument error refused with a message before any device call."""
import math

import pytest

from dgr_amd import _capi

from abi_checks import FAKE, assert_descriptor, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_seed_plan_bytes", "dgr_seed_plan", "dgr_seed_apply")
INF = float("inf")
XYZ, LOG_SCALE, RGB_DC, QUAT_IDENTITY, CONST = range(5)


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, dict(zip(NAMES, (3, 15, 17))))


def test_descriptor_matches_the_c_layout():
    # typedef struct { const float* src; float* dst; int k; int mode; float value; } dgr_seed_tensor;
    # (32 bytes: 28 of fields, padded to the pointers' alignment)
    assert_descriptor(_capi.SeedTensor, 32, dict(src=0, dst=8, k=16, mode=20, value=24), "SEED",
                      dict(MAX_TENSORS=24, XYZ=0, LOG_SCALE=1, RGB_DC=2, QUAT_IDENTITY=3, CONST=4))
    for field in ("const float* src;", "float* dst;", "int k;", "int mode;", "float value;"):
        assert field in header_text().split("} dgr_seed_tensor;")[0].rsplit("typedef struct {", 1)[1], field


def test_plan_bytes_hold_a_byte_per_candidate_and_a_record_per_block():
    lib = _capi.load()
    for shape in ((0, 10, 1), (10, 0, 1), (-3, 10, 1), (10, -3, 1), (10, 10, 0), (10, 10, -1), (1 << 16, 1 << 15, 1)):
        assert lib.dgr_seed_plan_bytes(*shape) == 0, shape
    # monotone in the number of candidates: 1, 4 * 2 = 8, 256, 257, 72 * 54 = 3888, 307200, 2073600
    shapes = [(1, 1, 1), (37, 23, 12), (16, 16, 1), (257, 1, 1), (640, 480, 9), (640, 480, 1), (1920, 1080, 1)]
    cands = [math.ceil(w / s) * math.ceil(h / s) for w, h, s in shapes]
    assert cands == sorted(cands) and len(set(cands)) == len(cands)
    sizes = [lib.dgr_seed_plan_bytes(*shape) for shape in shapes]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert all(s % 16 == 0 for s in sizes)
    n = 1920 * 1080
    assert n + 16 * 8100 <= sizes[-1] <= n + 16 * 8100 + 256
    # the stride divides rounding up: 37 x 23 at stride 3 has 13 x 8 candidates, as many bytes as a 13 x 8 frame
    assert lib.dgr_seed_plan_bytes(37, 23, 3) == lib.dgr_seed_plan_bytes(13, 8, 1)


def _plan(width=64, height=48, stride=1, depth_obs=FAKE, rows=10, plan=FAKE, counts=FAKE):
    return _capi.load().dgr_seed_plan(None, width, height, stride, depth_obs, None, None, 0.0, INF, 0.5, INF, None, rows, plan,
                                      counts)


def _apply(tensors, width=64, height=48, stride=1, rows=10, rows_out=12, plan=FAKE, n=None, color_obs=FAKE, depth_obs=FAKE,
           viewmatrix=FAKE, fx=50.0, fy=50.0, src=FAKE, dst=FAKE, descs=True):
    table = (_capi.SeedTensor * max(len(tensors), 1))()
    for d, (k, mode) in zip(table, tensors):
        d.src, d.dst, d.k, d.mode, d.value = src, dst, k, mode, 0.0
    return _capi.load().dgr_seed_apply(None, width, height, stride, rows, rows_out, plan, len(tensors) if n is None else n,
                                       table if descs else None, color_obs, depth_obs, viewmatrix, fx, fy, 31.5, 23.5, 0.02)


@pytest.mark.parametrize("case, text", [
    (dict(plan=None), "plan"),
    (dict(plan=FAKE + 4), "aligned"),
    (dict(depth_obs=None), "depth_obs"),
    (dict(width=0), "width"),
    (dict(height=-1), "height"),
    (dict(stride=0), "stride"),
    (dict(stride=-2), "stride"),
    (dict(rows=-1), "rows"),
    (dict(rows=1 << 30), "rows"),
    (dict(counts=None), "counts"),
], ids=["plan-null", "plan-misaligned", "depth_obs-null", "W=0", "H<0", "stride=0", "stride<0", "rows<0", "rows=2^30", "counts-null"])
def test_plan_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_plan(**case), "dgr_seed_plan", text)


NAN = float("nan")


@pytest.mark.parametrize("case, text", [
    (dict(tensors=[(3, CONST)], plan=None), "plan"),
    (dict(tensors=[(3, CONST)], plan=FAKE + 8), "aligned"),
    (dict(tensors=[(3, CONST)], depth_obs=None), "depth_obs"),
    (dict(tensors=[(3, CONST)], viewmatrix=None), "viewmatrix"),
    (dict(tensors=[(3, CONST)], width=0), "width"),
    (dict(tensors=[(3, CONST)], height=0), "height"),
    (dict(tensors=[(3, CONST)], stride=0), "stride"),
    (dict(tensors=[(3, CONST)], fx=0.0), "fx"),
    (dict(tensors=[(3, CONST)], fx=-50.0), "fx"),
    (dict(tensors=[(3, CONST)], fy=NAN), "fy"),
    (dict(tensors=[(3, CONST)], fy=INF), "fy"),
    (dict(tensors=[(3, CONST)], rows=-1), "rows"),
    (dict(tensors=[(3, CONST)], rows_out=9), "rows_out"),
    (dict(tensors=[(3, CONST)], rows_out=10 + 64 * 48 + 1), "rows_out"),
    (dict(tensors=[(3, CONST)], stride=2, rows_out=10 + 32 * 24 + 1), "rows_out"),
    (dict(tensors=[], n=0), "n must be"),
    (dict(tensors=[(3, CONST)], n=-1), "n must be"),
    (dict(tensors=[(1, CONST)] * 25), "n must be"),
    (dict(tensors=[(3, CONST)], descs=False), "tensors is NULL"),
    (dict(tensors=[(3, XYZ), (0, CONST)]), "k < 1"),
    (dict(tensors=[(-2, CONST)]), "k < 1"),
    (dict(tensors=[(3, 5)]), "unknown mode"),
    (dict(tensors=[(3, -1)]), "unknown mode"),
    (dict(tensors=[(3, XYZ), (4, CONST), (3, XYZ)]), "more than one XYZ"),
    (dict(tensors=[(4, XYZ)]), "k = 3"),
    (dict(tensors=[(2, LOG_SCALE)]), "k = 3 or k = 1"),
    (dict(tensors=[(4, RGB_DC)]), "k = 3"),
    (dict(tensors=[(3, QUAT_IDENTITY)]), "k = 4"),
    (dict(tensors=[(3, RGB_DC)], color_obs=None), "color_obs"),
    (dict(tensors=[(3, CONST)], dst=None), "NULL dst"),
    (dict(tensors=[(3, CONST)], src=None), "NULL src"),
], ids=["plan-null", "plan-misaligned", "depth_obs-null", "viewmatrix-null", "W=0", "H=0", "stride=0", "fx=0", "fx<0", "fy-nan",
        "fy-inf", "rows<0", "rows_out<rows", "rows_out>rows+candidates", "rows_out>rows+candidates-strided", "n=0", "n<0", "n=25",
        "tensors-null", "k=0", "k<0", "mode=5", "mode<0", "two-xyz", "xyz-k4", "log-scale-k2", "rgb-k4", "quat-k3",
        "rgb-without-colour", "dst-null", "src-null-with-rows"])
def test_apply_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_apply(**case), "dgr_seed_apply", text)


def test_constants_are_formed_in_float64():
    from dgr_amd.optim import seed_constants
    c = seed_constants(50.0, 40.0, silhouette_threshold=0.4, depth_error_min=0.05, depth_range=(0.1, 8.0), stride=3,
                       init_opacity=0.7, scale_factor=1.5)
    assert c == (0.1, 8.0, 0.4, 0.05, 1.5 * 3 * 0.5 * (1.0 / 50.0 + 1.0 / 40.0), math.log(0.7 / (1 - 0.7)))
    assert seed_constants(50.0, 50.0)[:4] == (0.0, INF, 0.5, INF) and seed_constants(50.0, 50.0)[5] == 0.0


def test_python_surface():
    from dgr_amd import optim
    keyword_only(optim.seed_from_frame, ["params", "optimizer", "color_obs", "depth_obs", "viewmatrix", "fx", "fy", "cx", "cy"],
                 dict(opacity_map=None, depth=None, silhouette_threshold=0.5, depth_error_min=INF, depth_range=(0.0, INF), stride=1,
                      init_opacity=0.5, scale_factor=1.0, fill=None, roles=None, xyz_gradient_accum=None, denom=None, max_radii2D=None))
    assert optim.SeedCounts._fields == ("rows", "new", "valid", "unseen", "infront")
    assert optim.SEED_ROLES == dict(optim.DEFAULT_ROLES, f_dc="f_dc")
