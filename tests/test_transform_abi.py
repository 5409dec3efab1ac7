"""The map-correction entry points (include/dgr_hip.h: dgr_transform_*) without a GPU: declared, exported and bound; the descriptor's
layout and the mode constants; the scratch size; every argument error refused with a message before any device call; the Python
surface."""
import inspect

import pytest

from dgr_amd import _capi

from abi_checks import FAKE, assert_descriptor, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_transform_scratch_bytes", "dgr_transform_plan", "dgr_transform_apply")
VALUE, MOMENT1, MOMENT2 = range(3)
XYZ, QUAT, LOG_SCALE, SH = 0, 4, 8, 12


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, dict(zip(NAMES, (1, 5, 8))))


def test_descriptor_and_constants_match_the_header():
    # typedef struct { float* data; int k; int mode; int skip; } dgr_transform_tensor;
    assert_descriptor(_capi.TransformTensor, 24, dict(data=0, k=8, mode=12, skip=16), "TRANSFORM",
                      dict(MAX_TENSORS=24, VALUE=0, MOMENT1=1, MOMENT2=2, XYZ=0, QUAT=4, LOG_SCALE=8, SH=12))
    assert "int skip;" in header_text() and "} dgr_transform_tensor;" in header_text()


def test_scratch_bytes():
    lib = _capi.load()
    for K in (0, -1, (1 << 20) + 1, 1 << 40):
        assert lib.dgr_transform_scratch_bytes(K) == 0, K
    sizes = [lib.dgr_transform_scratch_bytes(K) for K in (1, 2, 3, 70, 255, 256, 257, 1 << 20)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    # a record holds A, t, R, three scalars, q and 9 + 25 + 49 matrix values: at least 111 floats, and not more than 128
    assert 111 * 4 <= sizes[1] - sizes[0] <= 128 * 4 and sizes[0] <= 128 * 4 + 64


def _plan(K=3, transforms=FAKE, scratch=FAKE, counts=FAKE):
    return _capi.load().dgr_transform_plan(None, K, transforms, scratch, counts)


@pytest.mark.parametrize("case, text", [
    (dict(K=0), "K must be"), (dict(K=-5), "K must be"), (dict(K=(1 << 20) + 1), "K must be"), (dict(transforms=None), "transforms is NULL"),
    (dict(scratch=None), "scratch"), (dict(scratch=FAKE + 8), "aligned"), (dict(counts=None), "counts4_device"),
], ids=["K=0", "K<0", "K>2^20", "transforms-null", "scratch-null", "scratch-unaligned", "counts-null"])
def test_plan_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_plan(**case), "dgr_transform_plan", text)


def _apply(tensors, P=10, K=3, scratch=FAKE, anchor=None, n=None, data=FAKE, counts=FAKE, descs=True):
    table = (_capi.TransformTensor * max(len(tensors), 1))()
    for d, (k, mode, skip) in zip(table, tensors):
        d.data, d.k, d.mode, d.skip = data, k, mode, skip
    return _capi.load().dgr_transform_apply(None, P, K, scratch, anchor, len(tensors) if n is None else n, table if descs else None,
                                            counts)


ONE = [(3, XYZ, 0)]


@pytest.mark.parametrize("case, text", [
    (dict(tensors=ONE, P=-1), "P must be"),
    (dict(tensors=ONE, P=1 << 30), "P must be"),
    (dict(tensors=ONE, K=0), "K must be"),
    (dict(tensors=ONE, K=(1 << 20) + 1), "K must be"),
    (dict(tensors=ONE, scratch=None), "scratch"),
    (dict(tensors=ONE, scratch=FAKE + 4), "aligned"),
    (dict(tensors=ONE, counts=None), "counts4_device"),
    (dict(tensors=[], n=0), "n must be"),
    (dict(tensors=ONE, n=-1), "n must be"),
    (dict(tensors=[(9, SH, 0)] * 25), "n must be"),
    (dict(tensors=ONE, descs=False), "tensors is NULL"),
    (dict(tensors=[(0, SH, 0)]), "k < 1"),
    (dict(tensors=[(3, 15, 0)]), "unknown mode"),
    (dict(tensors=[(3, -1, 0)]), "unknown mode"),
    (dict(tensors=[(3, XYZ + 3, 0)]), "unknown mode"),
    (dict(tensors=[(3, LOG_SCALE + MOMENT1, 0)]), "unknown mode"),
    (dict(tensors=[(3, LOG_SCALE + MOMENT2, 0)]), "unknown mode"),
    (dict(tensors=ONE, data=None), "NULL data"),
    (dict(tensors=[(4, XYZ, 0)]), "k = 3"),
    (dict(tensors=[(3, XYZ + MOMENT1, 0), (4, XYZ + MOMENT2, 0)]), "XYZ tensor must have k = 3"),
    (dict(tensors=[(3, QUAT, 0)]), "QUAT tensor must have k = 4"),
    (dict(tensors=[(4, LOG_SCALE, 0)]), "LOG_SCALE tensor must have k = 3"),
    (dict(tensors=[(3, XYZ, 3)]), "skip must be 0"),
    (dict(tensors=[(9, SH, 1)]), "skip must be 0 or 3"),
    (dict(tensors=[(10, SH, 0)]), "complete bands"),
    (dict(tensors=[(48, SH + MOMENT1, 0)]), "complete bands"),
    (dict(tensors=[(45, SH, 3)]), "complete bands"),
    (dict(tensors=[(3, SH, 3)]), "complete bands"),
    (dict(tensors=[(3, XYZ, 0), (3, XYZ, 0)]), "more than one XYZ"),
    (dict(tensors=[(4, QUAT, 0), (4, QUAT + MOMENT1, 0), (4, QUAT, 0)]), "more than one QUAT"),
    (dict(tensors=[(3, LOG_SCALE, 0), (3, LOG_SCALE, 0)]), "more than one LOG_SCALE"),
], ids=["P<0", "P=2^30", "K=0", "K>2^20", "scratch-null", "scratch-unaligned", "counts-null", "n=0", "n<0", "n=25", "tensors-null",
        "k=0", "mode=15", "mode<0", "order=3", "scale-moment1", "scale-moment2", "data-null", "xyz-k4", "xyz-moment-k4", "quat-k3",
        "scale-k4", "xyz-skip", "sh-skip1", "sh-k10", "sh-k48-skip0", "sh-k45-skip3", "sh-dc-only", "two-xyz", "two-quat",
        "two-scale"])
def test_apply_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_apply(**case), "dgr_transform_apply", text)


def test_python_surface():
    from dgr_amd import map_steps, optim
    assert optim.transform_map is map_steps.transform_map and optim.pose_corrections is map_steps.pose_corrections
    keyword_only(optim.transform_map, ["params", "optimizer", "transforms"], dict(anchor="anchor", moments="rotate", roles=None))
    assert list(inspect.signature(optim.pose_corrections).parameters) == ["old_viewmatrices", "new_viewmatrices"]
    assert optim.TransformCounts._fields == ("transformed", "unanchored", "invalid_transforms", "anchored_invalid")
    assert optim.TRANSFORM_ROLES["f_rest"] == "f_rest" and optim.TRANSFORM_ROLES["shs"] == "shs"
