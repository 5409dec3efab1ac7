"""The densify-and-prune entry points (include/dgr_hip.h: dgr_densify_*) without a GPU: declared, exported and bound; the
descriptor's layout; every argument error refused with a message before any device call."""
import ctypes as C
import inspect
import math
import os

import pytest

from dgr_amd import _capi

from test_capi_symbols import declared_symbols

NAMES = ("dgr_densify_plan_bytes", "dgr_densify_plan", "dgr_densify_apply")
FAKE = 1 << 20  # a non-NULL, 16-byte aligned "device" pointer: every call below is refused before anything dereferences it
INF = float("inf")


def test_symbols_are_declared_exported_and_bound():
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert name in declared_symbols(), name
        assert name in _capi.exported_symbols(), name
        assert hasattr(lib, name), name
    assert len(_capi._SIGS["dgr_densify_plan"][1]) == 14 and len(_capi._SIGS["dgr_densify_apply"][1]) == 10


def test_descriptor_matches_the_c_layout():
    # typedef struct { const float* src; float* dst; int k; int mode; } dgr_densify_tensor;
    T = _capi.DensifyTensor
    assert C.sizeof(T) == 2 * C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_int) == 24
    assert (T.src.offset, T.dst.offset, T.k.offset, T.mode.offset) == (0, 8, 16, 20)
    assert _capi.DENSIFY_MAX_TENSORS == 24
    assert (_capi.DENSIFY_COPY, _capi.DENSIFY_ZERO_NEW, _capi.DENSIFY_ZERO, _capi.DENSIFY_XYZ, _capi.DENSIFY_LOG_SCALE) == (0, 1, 2, 3, 4)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dgr_hip.h")).read()
    for name, value in (("MAX_TENSORS", 24), ("COPY", 0), ("ZERO_NEW", 1), ("ZERO", 2), ("XYZ", 3), ("LOG_SCALE", 4)):
        assert f"#define DGR_DENSIFY_{name} {value}\n" in header, name


def test_plan_bytes_hold_a_byte_per_row_and_a_record_per_block():
    lib = _capi.load()
    assert lib.dgr_densify_plan_bytes(-1) == 0
    sizes = [lib.dgr_densify_plan_bytes(p) for p in (0, 1, 256, 257, 2_000_000)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert all(s % 16 == 0 for s in sizes)
    assert 2_000_000 + 16 * 7813 <= sizes[-1] <= 2_000_000 + 16 * 7813 + 256


def _refused(rc, text):
    assert rc == _capi.DGR_ERR_BAD_ARGUMENT and text in _capi.last_error(), (rc, _capi.last_error())
    assert _capi.last_error().startswith("dgr_densify_")


def _plan(rows=10, plan=FAKE, counts=FAKE, accum=FAKE):
    return _capi.load().dgr_densify_plan(None, rows, accum, FAKE, None, FAKE, FAKE, 2e-4, -5.0, -3.0, INF, INF, plan, counts)


def _apply(tensors, rows=10, rows_out=12, plan=FAKE, n=None):
    descs = (_capi.DensifyTensor * max(len(tensors), 1))()
    for d, (k, mode) in zip(descs, tensors):
        d.src, d.dst, d.k, d.mode = FAKE, FAKE, k, mode
    return _capi.load().dgr_densify_apply(None, rows, rows_out, plan, len(tensors) if n is None else n, descs, FAKE, FAKE, None, 0)


def test_plan_refuses_bad_arguments_before_touching_the_gpu():
    _refused(_plan(rows=-1), "rows")
    _refused(_plan(rows=1 << 30), "rows")
    _refused(_plan(plan=None), "plan")
    _refused(_plan(plan=FAKE + 4), "aligned")
    _refused(_plan(counts=None), "counts")
    _refused(_plan(accum=None), "NULL input")


COPY, ZERO_NEW, ZERO, XYZ, LOG_SCALE = range(5)


@pytest.mark.parametrize("case, text", [
    (dict(tensors=[(3, COPY)], rows=-1), "rows"),
    (dict(tensors=[(3, COPY)], rows_out=-1), "rows_out"),
    (dict(tensors=[(3, COPY)], rows_out=21), "rows_out"),
    (dict(tensors=[(3, COPY)], plan=None), "plan"),
    (dict(tensors=[], n=0), "n must be"),
    (dict(tensors=[(3, COPY)], n=-1), "n must be"),
    (dict(tensors=[(1, COPY)] * 25), "n must be"),
    (dict(tensors=[(3, XYZ), (0, COPY)]), "k < 1"),
    (dict(tensors=[(-2, ZERO)]), "k < 1"),
    (dict(tensors=[(3, 5)]), "unknown mode"),
    (dict(tensors=[(3, -1)]), "unknown mode"),
    (dict(tensors=[(3, XYZ), (4, COPY), (3, XYZ)]), "more than one XYZ"),
    (dict(tensors=[(4, XYZ)]), "k = 3"),
], ids=["rows<0", "rows_out<0", "rows_out>2rows", "plan-null", "n=0", "n<0", "n=25", "k=0", "k<0", "mode=5", "mode<0", "two-xyz",
        "xyz-k4"])
def test_apply_refuses_bad_arguments_before_touching_the_gpu(case, text):
    _refused(_apply(**case), text)


def test_apply_refuses_null_tensors_and_missing_xyz_inputs():
    lib = _capi.load()
    descs = (_capi.DensifyTensor * 1)()
    descs[0].src, descs[0].dst, descs[0].k, descs[0].mode = None, FAKE, 3, COPY
    _refused(lib.dgr_densify_apply(None, 10, 12, FAKE, 1, descs, FAKE, FAKE, None, 0), "NULL src or dst")
    descs[0].src, descs[0].dst, descs[0].mode = None, None, ZERO
    _refused(lib.dgr_densify_apply(None, 10, 12, FAKE, 1, descs, FAKE, FAKE, None, 0), "NULL src or dst")
    descs[0].src, descs[0].dst, descs[0].mode = FAKE, FAKE, XYZ
    _refused(lib.dgr_densify_apply(None, 10, 12, FAKE, 1, descs, None, FAKE, None, 0), "scaling_raw")
    _refused(lib.dgr_densify_apply(None, 10, 12, FAKE, 1, None, FAKE, FAKE, None, 0), "tensors is NULL")


def test_thresholds_are_formed_in_float64():
    from dgr_amd.optim import densify_thresholds
    t = densify_thresholds(2e-4, 5.0, percent_dense=0.01, min_opacity=0.005, max_screen_size=20)
    assert t == (2e-4, math.log(0.005 / 0.995), math.log(0.05), math.log(0.5), 20.0)
    assert densify_thresholds(2e-4, 5.0)[3:] == (INF, INF)


def test_python_surface():
    from dgr_amd import optim
    p = inspect.signature(optim.densify_and_prune).parameters
    assert list(p)[:5] == ["params", "optimizer", "xyz_gradient_accum", "denom", "max_radii2D"]
    for name, default in (("percent_dense", 0.01), ("min_opacity", 0.005), ("max_screen_size", None), ("noise", None),
                          ("seed", 0), ("roles", None)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name
    for name in ("grad_threshold", "extent"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is inspect.Parameter.empty, name
    assert optim.DensifyCounts._fields == ("rows", "survivors", "clones", "children", "split")


def test_replace_params_swaps_tensors_and_keeps_the_step_count():
    import torch
    from dgr_amd.optim import SparseAdam
    a, b, c = torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 4)
    opt = SparseAdam([{"params": [a], "lr": 1e-2}, {"params": [b, c]}])
    opt.state[a] = (torch.ones(4, 3), torch.ones(4, 3))
    opt.state[b] = (torch.ones(4, 1), torch.ones(4, 1))
    opt.steps = 7
    a2, b2 = torch.zeros(6, 3), torch.zeros(6, 1)
    m, v = torch.zeros(6, 3), torch.zeros(6, 3)
    opt.replace_params({a: a2, b: b2}, {a: (m, v)})
    assert opt.param_groups[0]["params"][0] is a2 and opt.param_groups[0]["lr"] == 1e-2
    assert opt.param_groups[1]["params"][0] is b2 and opt.param_groups[1]["params"][1] is c
    assert opt.state[a2][0] is m and opt.state[a2][1] is v
    assert a not in opt.state and b not in opt.state and b2 not in opt.state  # no moments given: no state
    assert opt.steps == 7
    with pytest.raises(RuntimeError):
        opt.replace_params({a2: a}, {a2: (m, v)})
