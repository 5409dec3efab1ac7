"""The full variant's batched entry points without a GPU: exported, the ctypes structs laid out as the header's (an offsetof
probe built with the host compiler), arguments refused before anything touches a device, and dgr_amd.batch_full's
documented refusals."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from dgr_amd import _capi

from abi_checks import HEADER, assert_entry_points, header_text, neutral_args


def test_the_full_batch_entry_points_are_exported_and_bound():
    assert_entry_points(("dgr_full_forward_batch", "dgr_full_backward_batch"))
    _capi.load()


def header_fields(struct):
    """field names of `typedef struct <struct> { ... }` in declaration order"""
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\}" % struct, text, flags=re.S).group(1)
    return [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]


@pytest.mark.parametrize("struct,cls", [("dgr_full_view", _capi.FullView), ("dgr_full_view_grad", _capi.FullViewGrad)])
def test_ctypes_structs_match_the_header(struct, cls, tmp_path):
    names = header_fields(struct)
    assert names == [f[0] for f in cls._fields_]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dgr_hip.h"', "int main(void) {",
             f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("%zu\\n", offsetof({struct}, {n}));' for n in names]
    src.write_text("\n".join(lines + ["    return 0;", "}"]) + "\n")
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(cls)
    assert got[1:] == [getattr(cls, n).offset for n in names]


def test_bad_view_counts_are_refused_before_touching_the_gpu():
    lib = _capi.load()
    views = (_capi.FullView * 1)()
    args = (0, 3, 16, None, 64, 48, None, None, None, None, None, 1.0, None, None, 0.6, 0.45, 0)
    for n in (0, _capi.MAX_BATCH_VIEWS + 1):
        assert lib.dgr_full_forward_batch(None, n, views, *args) == _capi.DGR_ERR_BAD_ARGUMENT
        assert b"views per batch" in lib.dgr_last_error()
    grads = (_capi.FullViewGrad * 1)()
    bargs = (0, 3, 16, None, 64, 48, None, None, None, None, 1.0, None, None, 0.6, 0.45, None, None, None, None, None, None, None)
    for n in (0, _capi.MAX_BATCH_VIEWS + 1):
        assert lib.dgr_full_backward_batch(None, n, grads, *bargs) == _capi.DGR_ERR_BAD_ARGUMENT
        assert b"views per batch" in lib.dgr_last_error()
    # a view without its pose-gradient output is refused as well (P == 0 would otherwise clear it)
    assert lib.dgr_full_backward_batch(None, 1, grads, *bargs) == _capi.DGR_ERR_BAD_ARGUMENT
    assert b"dL_dview" in lib.dgr_last_error()


@pytest.mark.parametrize("variant,cls", [("light", _capi.LightViewGrad), ("full", _capi.FullViewGrad)])
def test_batch_backward_refuses_a_view_without_its_binning_buffer(variant, cls):
    """Both variants' batch backward read the view's binning buffer as its sorted list: a view with every other input and a
    NULL binning buffer is refused before anything touches a device (host pointers stand in for device ones)."""
    lib = _capi.load()
    host = torch.zeros(1024, dtype=torch.uint8)
    fake = host.data_ptr()
    grads = (cls * 1)()
    for name, t in cls._fields_:
        setattr(grads[0], name, fake if t is ctypes.c_void_p else 1 << 40 if name == "scratch_bytes" else 100)
    grads[0].binning_buffer = None
    args = neutral_args("dgr_%s_backward_batch" % variant, pointer=fake)
    args[:10] = [None, 1, grads, 10, 3, 16, fake, 64, 48, fake]  # stream, n_views, views, P, D, M, background, W, H, means3D
    assert getattr(lib, "dgr_%s_backward_batch" % variant)(*args) == _capi.DGR_ERR_BAD_ARGUMENT
    assert b"missing state buffer" in lib.dgr_last_error()


def _settings(V, track_off=False, map_off=False):
    from dgr_amd.batch_full import BatchRasterizationSettings
    eye = torch.eye(4).expand(V, 4, 4).contiguous()
    return BatchRasterizationSettings(48, 64, 0.6, 0.45, torch.zeros(3), 1.0, eye, eye, 3, torch.zeros(V, 3), False, False,
                                      torch.eye(4), track_off, map_off)


def _call(V, P=100, **kw):
    from dgr_amd import batch_full as BF
    rs = _settings(V, **kw)
    means = torch.zeros(P, 3)
    return BF.GaussianRasterizerBatchFull(rs)(means, torch.zeros(V, P, 3), torch.ones(P, 1), shs=torch.zeros(P, 16, 3),
                                              scales=torch.ones(P, 3), rotations=torch.zeros(P, 4),
                                              gt_depths=torch.zeros(V, 48, 64))


def test_batch_full_refuses_cpu_tensors_too_many_views_and_the_light_switches():
    from dgr_amd import batch_full as BF
    assert BF.MAX_VIEWS == _capi.MAX_BATCH_VIEWS == 8
    with pytest.raises(RuntimeError, match="GPU only"):
        _call(2)
    with pytest.raises(RuntimeError, match="views per batch"):
        _call(_capi.MAX_BATCH_VIEWS + 1)
    for sw in ("track_off", "map_off"):
        with pytest.raises(ValueError, match="track_off / map_off"):
            _call(2, **{sw: True})


def test_render_views_refuses_the_light_switches_for_the_full_variant():
    from dgr_amd import slam
    with pytest.raises(ValueError, match="track_off / map_off"):
        slam.render_views([dict(viewmatrix=torch.eye(4), fov=(0.6, 0.45), HW=(48, 64))], None, None, torch.zeros(3),
                          track_off=True, variant="full")
    with pytest.raises(ValueError, match="unknown variant"):
        slam.render_views([], None, None, torch.zeros(3), variant="nope")
