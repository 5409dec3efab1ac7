"""absgrad (include/dgr_hip.h: dgr_*_backward*_absgrad) without a GPU: the four entry points are declared, exported and bound,
the refusals that come before any device call, and the keyword-only `means2D_abs` of the rasterizer modules."""
import ctypes as C
import inspect

import pytest

from dgr_amd import _capi
from dgr_amd import full as F
from dgr_amd import light as L

from test_capi_symbols import declared_symbols

ABS = ("dgr_light_backward_absgrad", "dgr_full_backward_absgrad", "dgr_light_backward_batch_absgrad",
       "dgr_full_backward_batch_absgrad")
FAKE = 1 << 20  # a non-NULL "device" pointer: every call below is refused before anything dereferences it


def test_absgrad_symbols_are_declared_exported_and_bound():
    lib = _capi.load()
    for name in ABS:
        assert name in declared_symbols(), name
        assert name in _capi.exported_symbols(), name
        assert hasattr(lib, name), name
    # each takes its namesake's arguments plus one
    for name in ABS:
        base = name.replace("_absgrad", "")
        assert len(_capi._SIGS[name][1]) == len(_capi._SIGS[base][1]) + 1, name


@pytest.fixture
def thread_option():
    lib = _capi.load()
    set_ = lambda n, v: lib.dgr_set_thread_option(n.encode(), v)  # noqa: E731
    yield set_
    for n in ("alpha_mode", "deterministic_grads"):
        set_(n, -1)


def _args(name, **at):
    """neutral arguments for `name`'s namesake (NULL pointers, zero ints, unit floats), with P = 10 on a 64 x 64 frame and
    `at` = {index: value} on top"""
    base = _capi._SIGS[name.replace("_absgrad", "")][1]
    out = [None if t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents") or hasattr(t, "_type_") and t._type_ == "P"
           else 1.0 if t is C.c_float else 0 for t in base]
    for i, v in at.items():
        out[int(i[1:])] = v
    return out


def _light(abs_ptr, map_off=0, P=10):
    args = _args("dgr_light_backward", i1=P, i6=64, i7=64)
    args[-3] = map_off
    return _capi.load().dgr_light_backward_absgrad(*args, abs_ptr)


def _full(abs_ptr, P=10):
    args = _args("dgr_full_backward", i1=P, i6=64, i7=64)
    return _capi.load().dgr_full_backward_absgrad(*args, abs_ptr)


def _light_batch(abs_ptrs, map_off=0):
    views = (_capi.LightViewGrad * 1)()
    args = _args("dgr_light_backward_batch", i1=1, i2=views, i3=10, i7=64, i8=64)
    args[-1] = map_off
    return _capi.load().dgr_light_backward_batch_absgrad(*args, (C.c_void_p * len(abs_ptrs))(*abs_ptrs))


def _full_batch(abs_ptrs):
    views = (_capi.FullViewGrad * 1)()
    args = _args("dgr_full_backward_batch", i1=1, i2=views, i3=10, i7=64, i8=64)
    return _capi.load().dgr_full_backward_batch_absgrad(*args, (C.c_void_p * len(abs_ptrs))(*abs_ptrs))


def _refused(rc, text):
    assert rc == _capi.DGR_ERR_BAD_ARGUMENT and text in _capi.last_error(), (rc, _capi.last_error())


def test_absgrad_with_map_off_is_refused():
    _refused(_light(FAKE, map_off=1), "map_off")
    _refused(_light_batch([FAKE], map_off=1), "map_off")


def test_absgrad_under_deterministic_grads_is_refused(thread_option):
    assert thread_option("deterministic_grads", 1) == 0
    _refused(_light(FAKE), "deterministic")
    _refused(_full(FAKE), "deterministic")
    _refused(_light_batch([FAKE]), "deterministic")
    _refused(_full_batch([FAKE]), "deterministic")


def test_absgrad_with_the_glibc_alpha_mode_is_refused(thread_option):
    assert thread_option("alpha_mode", 2) == 0
    _refused(_light(FAKE), "alpha_mode")
    _refused(_full(FAKE), "alpha_mode")
    _refused(_light_batch([FAKE]), "alpha_mode")
    _refused(_full_batch([FAKE]), "alpha_mode")


def test_a_null_absgrad_output_is_the_namesakes_behaviour(thread_option):
    # (NULL: nothing is refused for absgrad's sake -- the same "bad sizes" refusal as the namesake, before any device call)
    assert thread_option("deterministic_grads", 1) == 0
    lib = _capi.load()
    args = _args("dgr_light_backward", i1=-1, i6=64, i7=64)
    _refused(lib.dgr_light_backward_absgrad(*args, None), "bad sizes")
    _refused(lib.dgr_light_backward(*args), "bad sizes")
    _refused(_light_batch([None]), "dL_dview")  # (past the absgrad check: the view has no dL_dview)


@pytest.mark.parametrize("mod", [L, F], ids=["light", "full"])
def test_rasterizer_forward_takes_means2D_abs_as_keyword_only(mod):
    p = inspect.signature(mod.GaussianRasterizer.forward).parameters["means2D_abs"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


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
        p = inspect.signature(cls.forward).parameters["means2D_abs"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, cls


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
