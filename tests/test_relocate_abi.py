"""The fixed-size map upkeep entry points (include/dgr_hip.h: dgr_relocate_*, dgr_position_noise) without a GPU: declared, exported
and bound; the descriptor's layout; every argument error refused with a message before any device call."""
import ctypes as C
import inspect
import os

import pytest

from dgr_amd import _capi

from test_capi_symbols import declared_symbols

NAMES = ("dgr_relocate_scratch_bytes", "dgr_relocate_plan", "dgr_relocate_apply", "dgr_position_noise")
FAKE = 1 << 20  # a non-NULL, 16-byte aligned "device" pointer: every call below is refused before anything dereferences it
OTHER = 1 << 21
COPY, OPACITY, LOG_SCALE, ZERO_TOUCHED, ZERO_RELOCATED = range(5)


def test_symbols_are_declared_exported_and_bound():
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert name in declared_symbols(), name
        assert name in _capi.exported_symbols(), name
        assert hasattr(lib, name), name
    assert [len(_capi._SIGS[name][1]) for name in NAMES] == [1, 11, 8, 15]


def test_descriptor_matches_the_c_layout():
    # typedef struct { float* data; int k; int mode; } dgr_relocate_tensor;
    T = _capi.RelocateTensor
    assert C.sizeof(T) == C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_int) == 16
    assert (T.data.offset, T.k.offset, T.mode.offset) == (0, 8, 12)
    assert _capi.RELOCATE_MAX_TENSORS == 24
    assert (_capi.RELOCATE_COPY, _capi.RELOCATE_OPACITY, _capi.RELOCATE_LOG_SCALE, _capi.RELOCATE_ZERO_TOUCHED,
            _capi.RELOCATE_ZERO_RELOCATED) == (0, 1, 2, 3, 4)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dgr_hip.h")).read()
    for name, value in (("MAX_TENSORS", 24), ("COPY", 0), ("OPACITY", 1), ("LOG_SCALE", 2), ("ZERO_TOUCHED", 3), ("ZERO_RELOCATED", 4)):
        assert f"#define DGR_RELOCATE_{name} {value}\n" in header, name


def test_scratch_bytes_grow_with_the_rows():
    lib = _capi.load()
    assert lib.dgr_relocate_scratch_bytes(-1) == 0 and lib.dgr_relocate_scratch_bytes(1 << 30) == 0
    sizes = [lib.dgr_relocate_scratch_bytes(p) for p in (0, 1, 2, 255, 256, 257, 65_537, 2_000_000)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[-2] > sizes[2]
    assert all(s % 16 == 0 for s in sizes)
    # three 4-byte and two 8-byte values per row, a 16-byte record per 256 rows
    assert 28 * 2_000_000 + 16 * 7813 <= sizes[-1] <= 28 * 2_000_000 + 16 * 7813 + 256


def _refused(rc, who, text):
    assert rc == _capi.DGR_ERR_BAD_ARGUMENT and text in _capi.last_error(), (rc, _capi.last_error())
    assert _capi.last_error().startswith(who + ": ")


def _plan(P=10, opacity=FAKE, thr=-5.0, step=0, step_dev=None, scratch=FAKE, counts=FAKE, source=FAKE):
    return _capi.load().dgr_relocate_plan(None, P, opacity, thr, None, 0, step, step_dev, scratch, counts, source)


@pytest.mark.parametrize("case, text", [
    (dict(P=-1), "P must be"), (dict(P=1 << 30), "P must be"), (dict(scratch=None), "scratch"), (dict(scratch=FAKE + 8), "aligned"),
    (dict(counts=None), "counts8_device"), (dict(opacity=None), "opacity_raw is NULL"), (dict(source=None), "source is NULL"),
    (dict(thr=float("nan")), "NaN"), (dict(step=-1), "step is negative"),
], ids=["P<0", "P=2^30", "scratch-null", "scratch-unaligned", "counts-null", "opacity-null", "source-null", "thr-nan", "step<0"])
def test_plan_refuses_bad_arguments_before_touching_the_gpu(case, text):
    _refused(_plan(**case), "dgr_relocate_plan", text)


def _apply(tensors, P=10, scratch=FAKE, n=None, min_opacity=0.005, data=FAKE, scaling=OTHER, opacity=FAKE, descs=True):
    table = (_capi.RelocateTensor * max(len(tensors), 1))()
    for d, (k, mode) in zip(table, tensors):
        d.data, d.k, d.mode = (OTHER if mode == LOG_SCALE and data else data), k, mode
    return _capi.load().dgr_relocate_apply(None, P, scratch, len(tensors) if n is None else n, table if descs else None, scaling,
                                           opacity, min_opacity)


@pytest.mark.parametrize("case, text", [
    (dict(tensors=[(3, COPY)], P=-1), "P must be"),
    (dict(tensors=[(3, COPY)], P=1 << 30), "P must be"),
    (dict(tensors=[(3, COPY)], scratch=None), "scratch"),
    (dict(tensors=[(3, COPY)], scratch=FAKE + 4), "aligned"),
    (dict(tensors=[(3, COPY)], min_opacity=-0.1), "min_opacity"),
    (dict(tensors=[(3, COPY)], min_opacity=1.0), "min_opacity"),
    (dict(tensors=[(3, COPY)], min_opacity=float("nan")), "min_opacity"),
    (dict(tensors=[], n=0), "n must be"),
    (dict(tensors=[(3, COPY)], n=-1), "n must be"),
    (dict(tensors=[(1, COPY)] * 25), "n must be"),
    (dict(tensors=[(3, COPY)], descs=False), "tensors is NULL"),
    (dict(tensors=[(3, COPY), (0, COPY)]), "k < 1"),
    (dict(tensors=[(-2, ZERO_TOUCHED)]), "k < 1"),
    (dict(tensors=[(3, 5)]), "unknown mode"),
    (dict(tensors=[(3, -1)]), "unknown mode"),
    (dict(tensors=[(3, COPY)], data=None), "NULL data"),
    (dict(tensors=[(3, OPACITY)]), "k = 1"),
    (dict(tensors=[(1, OPACITY), (1, OPACITY)]), "more than one OPACITY"),
    (dict(tensors=[(1, OPACITY)], opacity=OTHER), "must be opacity_raw"),
    (dict(tensors=[(3, LOG_SCALE), (3, LOG_SCALE)]), "more than one LOG_SCALE"),
    (dict(tensors=[(3, LOG_SCALE)], scaling=FAKE), "must be scaling_raw"),
], ids=["P<0", "P=2^30", "scratch-null", "scratch-unaligned", "min<0", "min=1", "min-nan", "n=0", "n<0", "n=25", "tensors-null", "k=0",
        "k<0", "mode=5", "mode<0", "data-null", "opacity-k3", "two-opacity", "opacity-elsewhere", "two-scale", "scale-elsewhere"])
def test_apply_refuses_bad_arguments_before_touching_the_gpu(case, text):
    _refused(_apply(**case), "dgr_relocate_apply", text)


def _noise(P=10, xyz=FAKE, scaling=FAKE, rotation=FAKE, opacity=FAKE, step=0, lr=1e-4, lr_dev=None, scale=5e5, k=100.0, x0=0.995):
    return _capi.load().dgr_position_noise(None, P, xyz, scaling, rotation, opacity, None, 0, step, None, lr, lr_dev, scale, k, x0)


@pytest.mark.parametrize("case, text", [
    (dict(P=-1), "P must be"), (dict(P=1 << 30), "P must be"), (dict(xyz=None), "is NULL"), (dict(scaling=None), "is NULL"),
    (dict(rotation=None), "is NULL"), (dict(opacity=None), "is NULL"), (dict(step=-3), "step is negative"),
    (dict(lr=float("inf")), "lr is not finite"), (dict(scale=float("nan")), "not finite"), (dict(k=float("inf")), "not finite"),
    (dict(x0=float("nan")), "not finite"),
], ids=["P<0", "P=2^30", "xyz-null", "scaling-null", "rotation-null", "opacity-null", "step<0", "lr-inf", "scale-nan", "k-inf", "x0-nan"])
def test_position_noise_refuses_bad_arguments_before_touching_the_gpu(case, text):
    _refused(_noise(**case), "dgr_position_noise", text)


def test_python_surface():
    from dgr_amd import optim
    p = inspect.signature(optim.relocate_dead).parameters
    assert list(p)[:2] == ["params", "optimizer"]
    for name, default in (("min_opacity", 0.005), ("draws", None), ("seed", 0), ("step", 0), ("xyz_gradient_accum", None),
                          ("denom", None), ("max_radii2D", None), ("roles", None)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name
    assert optim.RelocateResult._fields == ("counts", "source")
    p = inspect.signature(optim.inject_position_noise).parameters
    assert list(p)[:2] == ["params", "lr"]
    for name, default in (("noise_scale", 5e5), ("gate_k", 100.0), ("gate_x0", 0.995), ("noise", None), ("seed", 0), ("step", 0),
                          ("roles", None)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name

