"""absgrad (include/dgr_hip.h: dgr_*_backward*_absgrad) without a GPU: the four entry points are declared, exported and bound,
the refusals that come before any device call, and the keyword-only `means2D_abs` of the rasterizer modules."""
import ctypes as C
import inspect

import pytest

from dgr_amd import _capi
from dgr_amd import full as F
from dgr_amd import light as L

from abi_checks import FAKE, assert_entry_points, keyword_only, neutral_args, refused

ABS = ("dgr_light_backward_absgrad", "dgr_full_backward_absgrad", "dgr_light_backward_batch_absgrad",
       "dgr_full_backward_batch_absgrad")
WHO = "absgrad"  # its refusals (csrc/api.hip: absgrad_refused) start "absgrad: ", not with the entry point's name


def test_absgrad_symbols_are_declared_exported_and_bound():
    # each takes its namesake's arguments plus one
    assert_entry_points(ABS, {name: len(_capi._SIGS[name.replace("_absgrad", "")][1]) + 1 for name in ABS})
    _capi.load()


@pytest.fixture
def thread_option():
    lib = _capi.load()
    set_ = lambda n, v: lib.dgr_set_thread_option(n.encode(), v)  # noqa: E731
    yield set_
    for n in ("alpha_mode", "deterministic_grads"):
        set_(n, -1)


def _light(abs_ptr, map_off=0, P=10):
    """(every list below: neutral arguments for the namesake with P = 10 on a 64 x 64 frame, then the absgrad output)"""
    args = neutral_args("dgr_light_backward", i1=P, i6=64, i7=64)
    args[-3] = map_off
    return _capi.load().dgr_light_backward_absgrad(*args, abs_ptr)


def _full(abs_ptr, P=10):
    args = neutral_args("dgr_full_backward", i1=P, i6=64, i7=64)
    return _capi.load().dgr_full_backward_absgrad(*args, abs_ptr)


def _light_batch(abs_ptrs, map_off=0):
    views = (_capi.LightViewGrad * 1)()
    args = neutral_args("dgr_light_backward_batch", i1=1, i2=views, i3=10, i7=64, i8=64)
    args[-1] = map_off
    return _capi.load().dgr_light_backward_batch_absgrad(*args, (C.c_void_p * len(abs_ptrs))(*abs_ptrs))


def _full_batch(abs_ptrs):
    views = (_capi.FullViewGrad * 1)()
    args = neutral_args("dgr_full_backward_batch", i1=1, i2=views, i3=10, i7=64, i8=64)
    return _capi.load().dgr_full_backward_batch_absgrad(*args, (C.c_void_p * len(abs_ptrs))(*abs_ptrs))


def test_absgrad_with_map_off_is_refused():
    refused(_light(FAKE, map_off=1), WHO, "map_off")
    refused(_light_batch([FAKE], map_off=1), WHO, "map_off")


def test_absgrad_under_deterministic_grads_is_refused(thread_option):
    assert thread_option("deterministic_grads", 1) == 0
    refused(_light(FAKE), WHO, "deterministic")
    refused(_full(FAKE), WHO, "deterministic")
    refused(_light_batch([FAKE]), WHO, "deterministic")
    refused(_full_batch([FAKE]), WHO, "deterministic")


def test_absgrad_with_the_glibc_alpha_mode_is_refused(thread_option):
    assert thread_option("alpha_mode", 2) == 0
    refused(_light(FAKE), WHO, "alpha_mode")
    refused(_full(FAKE), WHO, "alpha_mode")
    refused(_light_batch([FAKE]), WHO, "alpha_mode")
    refused(_full_batch([FAKE]), WHO, "alpha_mode")


def test_a_null_absgrad_output_is_the_namesakes_behaviour(thread_option):
    # (NULL: nothing is refused for absgrad's sake -- the same "bad sizes" refusal as the namesake, before any device call; the
    # one-view and batch backwards leave these two messages without a prefix)
    assert thread_option("deterministic_grads", 1) == 0
    lib = _capi.load()
    args = neutral_args("dgr_light_backward", i1=-1, i6=64, i7=64)
    refused(lib.dgr_light_backward_absgrad(*args, None), None, "bad sizes")
    refused(lib.dgr_light_backward(*args), None, "bad sizes")
    refused(_light_batch([None]), None, "dL_dview")  # (past the absgrad check: the view has no dL_dview)


@pytest.mark.parametrize("mod", [L, F], ids=["light", "full"])
def test_rasterizer_forward_takes_means2D_abs_as_keyword_only(mod):
    keyword_only(mod.GaussianRasterizer.forward, (), {"means2D_abs": None})


def test_means2D_abs_is_checked():
    import torch
    means3D = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="map_off"):
        L.check_means2D_abs(torch.zeros(5, 3), means3D, True)
    with pytest.raises(ValueError, match="shape"):
        L.check_means2D_abs(torch.zeros(5, 2), means3D, False)
    with pytest.raises(ValueError):
        L.check_means2D_abs(torch.zeros(5, 3, dtype=torch.float64), means3D, False)
    L.check_means2D_abs(torch.zeros(5, 3), means3D, False)


def test_batch_rasterizers_take_means2D_abs_as_keyword_only():
    from dgr_amd import batch as B
    from dgr_amd import batch_full as BF
    for cls in (B.GaussianRasterizerBatch, BF.GaussianRasterizerBatchFull):
        keyword_only(cls.forward, (), {"means2D_abs": None})


def test_batch_means2D_abs_with_map_off_is_refused():
    import torch
    from dgr_amd import batch as B
    rs = B.BatchRasterizationSettings(image_height=8, image_width=8, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                      scale_modifier=1.0, viewmatrices=torch.eye(4)[None].repeat(2, 1, 1),
                                      projmatrices=torch.eye(4)[None].repeat(2, 1, 1), sh_degree=0, campos=torch.zeros(2, 3),
                                      prefiltered=False, debug=False, perspec_matrix=torch.eye(4), track_off=False, map_off=True)
    m = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="map_off"):
        B.GaussianRasterizerBatch(rs)(m, torch.zeros(2, 5, 3), torch.zeros(5, 1), shs=torch.zeros(5, 1, 3),
                                      scales=torch.zeros(5, 3), rotations=torch.zeros(5, 4), means2D_abs=torch.zeros(2, 5, 3))


def test_slam_renders_take_absgrad():
    from dgr_amd import slam
    for fn in (slam.render, slam.render_views, slam.render_batch, slam.render_batch_fused):
        p = inspect.signature(fn).parameters["absgrad"]
        assert p.default is False, fn.__name__
