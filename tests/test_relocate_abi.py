"""The fixed-size map upkeep entry points (include/dgr_hip.h: dgr_relocate_*, dgr_position_noise) without a GPU: declared, exported
and bound; the descriptor's layout; every argument error refused with a message before any device call."""
import ctypes as C

import pytest

from dgr_amd import _capi

from abi_checks import FAKE, OTHER, assert_descriptor, assert_entry_points, keyword_only, refused

NAMES = ("dgr_relocate_scratch_bytes", "dgr_relocate_plan", "dgr_relocate_apply", "dgr_position_noise")
COPY, OPACITY, LOG_SCALE, ZERO_TOUCHED, ZERO_RELOCATED = range(5)


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, dict(zip(NAMES, (1, 11, 8, 15))))


def test_descriptor_matches_the_c_layout():
    # typedef struct { float* data; int k; int mode; } dgr_relocate_tensor;
    assert C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_int) == 16
    assert_descriptor(_capi.RelocateTensor, 16, dict(data=0, k=8, mode=12), "RELOCATE",
                      dict(MAX_TENSORS=24, COPY=0, OPACITY=1, LOG_SCALE=2, ZERO_TOUCHED=3, ZERO_RELOCATED=4))


def test_scratch_bytes_grow_with_the_rows():
    lib = _capi.load()
    assert lib.dgr_relocate_scratch_bytes(-1) == 0 and lib.dgr_relocate_scratch_bytes(1 << 30) == 0
    sizes = [lib.dgr_relocate_scratch_bytes(p) for p in (0, 1, 2, 255, 256, 257, 65_537, 2_000_000)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[-2] > sizes[2]
    assert all(s % 16 == 0 for s in sizes)
    # three 4-byte and two 8-byte values per row, a 16-byte record per 256 rows
    assert 28 * 2_000_000 + 16 * 7813 <= sizes[-1] <= 28 * 2_000_000 + 16 * 7813 + 256


def _plan(P=10, opacity=FAKE, thr=-5.0, step=0, step_dev=None, scratch=FAKE, counts=FAKE, source=FAKE):
    return _capi.load().dgr_relocate_plan(None, P, opacity, thr, None, 0, step, step_dev, scratch, counts, source)


@pytest.mark.parametrize("case, text", [
    (dict(P=-1), "P must be"), (dict(P=1 << 30), "P must be"), (dict(scratch=None), "scratch"), (dict(scratch=FAKE + 8), "aligned"),
    (dict(counts=None), "counts8_device"), (dict(opacity=None), "opacity_raw is NULL"), (dict(source=None), "source is NULL"),
    (dict(thr=float("nan")), "NaN"), (dict(step=-1), "step is negative"),
], ids=["P<0", "P=2^30", "scratch-null", "scratch-unaligned", "counts-null", "opacity-null", "source-null", "thr-nan", "step<0"])
def test_plan_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_plan(**case), "dgr_relocate_plan", text)


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
    refused(_apply(**case), "dgr_relocate_apply", text)


def _noise(P=10, xyz=FAKE, scaling=FAKE, rotation=FAKE, opacity=FAKE, step=0, lr=1e-4, lr_dev=None, scale=5e5, k=100.0, x0=0.995):
    return _capi.load().dgr_position_noise(None, P, xyz, scaling, rotation, opacity, None, 0, step, None, lr, lr_dev, scale, k, x0)


@pytest.mark.parametrize("case, text", [
    (dict(P=-1), "P must be"), (dict(P=1 << 30), "P must be"), (dict(xyz=None), "is NULL"), (dict(scaling=None), "is NULL"),
    (dict(rotation=None), "is NULL"), (dict(opacity=None), "is NULL"), (dict(step=-3), "step is negative"),
    (dict(lr=float("inf")), "lr is not finite"), (dict(scale=float("nan")), "not finite"), (dict(k=float("inf")), "not finite"),
    (dict(x0=float("nan")), "not finite"),
], ids=["P<0", "P=2^30", "xyz-null", "scaling-null", "rotation-null", "opacity-null", "step<0", "lr-inf", "scale-nan", "k-inf", "x0-nan"])
def test_position_noise_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_noise(**case), "dgr_position_noise", text)


def test_python_surface():
    from dgr_amd import optim
    keyword_only(optim.relocate_dead, ["params", "optimizer"],
                 dict(min_opacity=0.005, draws=None, seed=0, step=0, xyz_gradient_accum=None, denom=None, max_radii2D=None, roles=None))
    assert optim.RelocateResult._fields == ("counts", "source")
    keyword_only(optim.inject_position_noise, ["params", "lr"],
                 dict(noise_scale=5e5, gate_k=100.0, gate_x0=0.995, noise=None, seed=0, step=0, roles=None))
