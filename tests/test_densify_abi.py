"""The densify-and-prune entry points (include/dgr_hip.h: dgr_densify_*) without a GPU: declared, exported and bound; the
descriptor's layout; every argument error refused with a message before any device call."""
import ctypes as C
import math

import pytest

from dgr_amd import _capi

from abi_checks import FAKE, assert_descriptor, assert_entry_points, keyword_only, refused

NAMES = ("dgr_densify_plan_bytes", "dgr_densify_plan", "dgr_densify_apply")
INF = float("inf")


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_densify_plan": 14, "dgr_densify_apply": 10})


def test_descriptor_matches_the_c_layout():
    # typedef struct { const float* src; float* dst; int k; int mode; } dgr_densify_tensor;
    assert 2 * C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_int) == 24
    assert_descriptor(_capi.DensifyTensor, 24, dict(src=0, dst=8, k=16, mode=20), "DENSIFY",
                      dict(MAX_TENSORS=24, COPY=0, ZERO_NEW=1, ZERO=2, XYZ=3, LOG_SCALE=4))


def test_plan_bytes_hold_a_byte_per_row_and_a_record_per_block():
    lib = _capi.load()
    assert lib.dgr_densify_plan_bytes(-1) == 0
    sizes = [lib.dgr_densify_plan_bytes(p) for p in (0, 1, 256, 257, 2_000_000)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert all(s % 16 == 0 for s in sizes)
    assert 2_000_000 + 16 * 7813 <= sizes[-1] <= 2_000_000 + 16 * 7813 + 256


def _plan(rows=10, plan=FAKE, counts=FAKE, accum=FAKE):
    return _capi.load().dgr_densify_plan(None, rows, accum, FAKE, None, FAKE, FAKE, 2e-4, -5.0, -3.0, INF, INF, plan, counts)


def _apply(tensors, rows=10, rows_out=12, plan=FAKE, n=None):
    descs = (_capi.DensifyTensor * max(len(tensors), 1))()
    for d, (k, mode) in zip(descs, tensors):
        d.src, d.dst, d.k, d.mode = FAKE, FAKE, k, mode
    return _capi.load().dgr_densify_apply(None, rows, rows_out, plan, len(tensors) if n is None else n, descs, FAKE, FAKE, None, 0)


def test_plan_refuses_bad_arguments_before_touching_the_gpu():
    for case, text in ((dict(rows=-1), "rows"), (dict(rows=1 << 30), "rows"), (dict(plan=None), "plan"), (dict(plan=FAKE + 4), "aligned"),
                       (dict(counts=None), "counts"), (dict(accum=None), "NULL input")):
        refused(_plan(**case), "dgr_densify_plan", text)


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
    refused(_apply(**case), "dgr_densify_apply", text)


def test_apply_refuses_null_tensors_and_missing_xyz_inputs():
    descs = (_capi.DensifyTensor * 1)()
    apply = lambda table, scaling: _capi.load().dgr_densify_apply(None, 10, 12, FAKE, 1, table, scaling, FAKE, None, 0)  # noqa: E731
    descs[0].src, descs[0].dst, descs[0].k, descs[0].mode = None, FAKE, 3, COPY
    refused(apply(descs, FAKE), "dgr_densify_apply", "NULL src or dst")
    descs[0].src, descs[0].dst, descs[0].mode = None, None, ZERO
    refused(apply(descs, FAKE), "dgr_densify_apply", "NULL src or dst")
    descs[0].src, descs[0].dst, descs[0].mode = FAKE, FAKE, XYZ
    refused(apply(descs, None), "dgr_densify_apply", "scaling_raw")
    refused(apply(None, FAKE), "dgr_densify_apply", "tensors is NULL")


def test_thresholds_are_formed_in_float64():
    from dgr_amd.optim import densify_thresholds
    t = densify_thresholds(2e-4, 5.0, percent_dense=0.01, min_opacity=0.005, max_screen_size=20)
    assert t == (2e-4, math.log(0.005 / 0.995), math.log(0.05), math.log(0.5), 20.0)
    assert densify_thresholds(2e-4, 5.0)[3:] == (INF, INF)


def test_python_surface():
    from dgr_amd import optim
    keyword_only(optim.densify_and_prune, ["params", "optimizer", "xyz_gradient_accum", "denom", "max_radii2D"],
                 dict(percent_dense=0.01, min_opacity=0.005, max_screen_size=None, noise=None, seed=0, roles=None),
                 required=("grad_threshold", "extent"))
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
