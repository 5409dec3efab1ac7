"""What the Python front end hands downward, call by call, against a record made before the four front-end modules were folded.

Two places are hooked: the ctypes functions of the object `_capi.load()` returns whose names begin `dgr_light_` or `dgr_full_`
(plus `dgr_mark_visible`), and the functions of the compiled extension (`light._CompiledC.ext`).  Each call becomes one line: the
name, then every argument -- a scalar by value, a pointer as NULL or not, a tensor by dtype, shape and whether it is empty, a view
struct field by field.  What follows the binning policy's history (capacities, R, num_related, scratch sizes, the opaque uint8
buffers' lengths) is recorded as present only.  The compiled node's backward runs inside the autograd engine, below both hooks:
of a node case only the forward's crossing is seen.  The batches have no node, and the node has no absgrad input: such a case
records whatever ran instead.

Cases: {light, full} x {one view, batch of 2} x {ctypes binding, the Python Function over the compiled `_C`, the compiled node} x
{plain, means2D_abs, option silhouette_grad} x {a loss on every output, on colour only} x {every leaf requires a gradient, only
the view matrix does}, and `markVisible` per one-view variant and binding.  The scene: 48 Gaussians, one of them behind the camera,
32 x 32 pixels (2 x 2 tiles), SH rows [P,16,3] at degree 3.  Each case starts from cleared binning state under DGR_SYNC_MODE=strict.

The expected record, tests/golden/frontend_calls.json, was written by this file's recorder on an MI355X at the commit before the
fold (`python tests/test_hip_frontend_calls.py <path>`); it holds each distinct line once and, per case, the lines' indices.
"""
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_calls.json")
P, H, W, DEG, V = 48, 32, 32, 3, 2
VARIANTS, VIEWS, BINDINGS = ("light", "full"), ("one", "batch"), ("ctypes", "function", "node")
MODES, LOSSES, LEAVES = ("plain", "absgrad", "silhouette"), ("all", "colour"), ("mapping", "tracking")

# arguments that follow the binning policy's history, by position: "present", not their value
_LIB_PRESENT = {"dgr_light_forward_presized": {3}, "dgr_full_forward_presized": {3}, "dgr_light_backward": {4, 48},
                "dgr_full_backward": {4, 51}, "dgr_light_backward_scratch_bytes_r": {3}}
_FIELDS_PRESENT = {"binning_capacity", "scratch_bytes", "num_rendered"}
_EXT_PRESENT = {"light_forward": {20}, "full_forward": {20}, "light_apply": {23}, "full_apply": {23}, "light_forward_batch": {19},
                "full_forward_batch": {19}, "light_backward": {21}, "full_backward": {20, 23}}


def _scalar(v):
    if isinstance(v, bool):
        return str(v)
    return f"{v:.6g}" if isinstance(v, float) else str(int(v))


def _pointer(v):
    return "NULL" if v is None or v == 0 else "ptr"


def _lib_arg(name, i, kind, v, n_views):
    base = name.replace("_absgrad", "").replace("_silhouette", "")
    if i in _LIB_PRESENT.get(base, ()):
        return "present"
    if kind is C.c_void_p:
        return "stream" if i == 0 else _pointer(v)
    if kind in (C.c_int, C.c_float, C.c_size_t):
        return _scalar(v)
    if v is None:
        return "NULL"
    if kind is C.POINTER(C.c_void_p):  # (a batch's absgrad / silhouette images: one pointer per view)
        return "[" + " ".join(_pointer(v[k]) for k in range(n_views)) + "]"
    if isinstance(v, C.Array) and issubclass(v._type_, C.Structure):  # the views of a batch
        views = []
        for k in range(n_views):
            f = [f"{fn}=" + ("present" if fn in _FIELDS_PRESENT else _pointer(getattr(v[k], fn)) if ft is C.c_void_p
                             else _scalar(getattr(v[k], fn))) for fn, ft in v._type_._fields_]
            views.append("{" + " ".join(f) + "}")
        return "[" + " ".join(views) + "]"
    return "callback" if callable(v) else "ref"  # the resize callbacks; a byref() result


def _ext_arg(name, i, v):
    if i in _EXT_PRESENT.get(name, ()):
        return "present"
    if isinstance(v, torch.Tensor):
        if v.dtype is torch.uint8:  # an opaque buffer, carved by capacity
            return "uint8 present"
        return f"{str(v.dtype)[6:]}{list(v.shape)}" + ("" if v.numel() else " empty")
    if isinstance(v, (list, tuple)):
        return f"list[{len(v)}]"
    return "None" if v is None else _scalar(v)


@contextlib.contextmanager
def recording(lines):
    """Hooks both places for the block; every call appends its line to `lines`."""
    from dgr_amd import _capi, light
    lib, ext, saved = _capi.load(), light._CompiledC.ext, []

    def hook(obj, name, describe):
        fn = getattr(obj, name)

        def wrapped(*a):
            lines.append(name + "(" + ", ".join(describe(a)) + ")")
            return fn(*a)
        saved.append((obj, name, fn))
        setattr(obj, name, wrapped)
    for name, (_, kinds) in _capi._SIGS.items():
        if name.startswith(("dgr_light_", "dgr_full_")) or name == "dgr_mark_visible":
            hook(lib, name, lambda a, name=name, kinds=kinds: [
                _lib_arg(name, i, kinds[i], v, a[1] if "_batch" in name else 0) for i, v in enumerate(a)])
    for name in ([] if ext is None else dir(ext)):
        if not name.startswith("_") and callable(getattr(ext, name)):
            hook(ext, name, lambda a, name=name: [_ext_arg(name, i, v) for i, v in enumerate(a)])
    try:
        yield
    finally:
        for obj, name, fn in saved:
            setattr(obj, name, fn)


@contextlib.contextmanager
def bound(binding):
    """The three switch points (light._C, full._C, light._USE_NODE) set for the block."""
    from dgr_amd import full, light
    prev = light._C, full._C, light._USE_NODE
    compiled = binding != "ctypes"
    light._C, full._C = (light._CompiledC, full._CompiledC) if compiled else (light._CtypesC, full._CtypesC)
    light._USE_NODE = binding == "node"
    try:
        yield
    finally:
        light._C, full._C, light._USE_NODE = prev


def _clear_binning_state():
    from dgr_amd import _binning
    _binning.check_async_errors()
    for d in (_binning._capacity_cache, _binning._unsettled, _binning._last_status, _binning._pending_status,
              _binning._capture_keepalive):
        d.clear()


def _scenes():
    from dgr_amd.synth import make_scene
    ss = [make_scene(P, W, H, seed=5, view_index=v) for v in range(V)]
    s = ss[0]
    means = s.means.copy()
    means[0] = (np.array([0.0, 0.0, -2.0]) - s.view[3, :3]) @ s.view[:3, :3].T  # camera space (0, 0, -2): behind the camera
    ss = [x._replace(means=means) for x in ss]
    for x in ss:
        z = (np.concatenate([means, np.ones((P, 1), np.float32)], 1) @ x.view)[:, 2]
        assert z[0] < 0 < z[1:].min()
    return ss


def _rasterizer(variant, views, ss, dev):
    """(the variant's rasterizer module for `views`, the camera keyword arguments of its call)"""
    from dgr_amd import batch, batch_full, full, light
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    s = ss[0]
    if views == "batch":
        rs = batch.BatchRasterizationSettings(H, W, s.tanfovx, s.tanfovy, t(s.bg), 1.0, t(np.stack([x.view for x in ss])),
                                              t(np.stack([x.proj for x in ss])), DEG, t(np.stack([x.campos for x in ss])), False,
                                              False, t(s.persp), False, False)
        cls = batch.GaussianRasterizerBatch if variant == "light" else batch_full.GaussianRasterizerBatchFull
        return cls(rs), dict(viewmatrices=t(np.stack([x.view for x in ss])).requires_grad_(),
                             gt_depths=t(np.stack([x.gt for x in ss])))
    common = dict(image_height=H, image_width=W, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=t(s.bg), scale_modifier=1.0,
                  viewmatrix=t(s.view), projmatrix=t(s.proj), sh_degree=DEG, campos=t(s.campos), prefiltered=False,
                  perspec_matrix=t(s.persp))
    if variant == "light":
        rast = light.GaussianRasterizer(light.GaussianRasterizationSettings(debug=False, track_off=False, map_off=False, **common))
    else:
        rast = full.GaussianRasterizer(full.GaussianRasterizationSettings(**common))
    return rast, dict(viewmatrix=t(s.view).requires_grad_(), gt_depth=t(s.gt))


def record_group(variant, views, binding):
    """{case id: the lines of its calls} of every case of one variant, view count and binding."""
    from dgr_amd import _capi
    dev = torch.device("cuda:0")
    ss = _scenes()
    s = ss[0]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    nv = (V,) if views == "batch" else ()
    gen = torch.Generator(device=dev).manual_seed(1)
    out = {}
    with bound(binding):
        for mode in MODES:
            for loss in LOSSES:
                for leaves in LEAVES:
                    mapping = leaves == "mapping"
                    rast, cam = _rasterizer(variant, views, ss, dev)
                    g = {k: t(a).requires_grad_(mapping) for k, a in (("means3D", s.means), ("shs", s.shs), ("opacities", s.opac),
                                                                       ("scales", s.scales), ("rotations", s.rots))}
                    g["means2D"] = torch.zeros(nv + (P, 3), device=dev, requires_grad=mapping)
                    if mode == "absgrad":
                        g["means2D_abs"] = torch.zeros(nv + (P, 3), device=dev, requires_grad=mapping)
                    _clear_binning_state()
                    lines = []
                    with recording(lines), _capi.thread_options(silhouette_grad=int(mode == "silhouette")):
                        res = rast(**g, **cam)
                        used = [o for o in res if o.is_floating_point() and o.requires_grad][:None if loss == "all" else 1]
                        sum((o * torch.rand(o.shape, generator=gen, device=dev)).sum() for o in used).backward()
                        torch.cuda.synchronize()
                    out[f"{variant}-{views}-{binding}-{mode}-{loss}-{leaves}"] = lines
        if views == "one":
            rast, _ = _rasterizer(variant, views, ss, dev)
            lines = []
            with recording(lines):
                rast.markVisible(t(s.means))
                torch.cuda.synchronize()
            out[f"{variant}-{views}-{binding}-markVisible"] = lines
    _clear_binning_state()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("binding", BINDINGS)
@pytest.mark.parametrize("views", VIEWS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_the_front_end_hands_down_what_it_did_before_the_fold(variant, views, binding, monkeypatch):
    from dgr_amd import light
    if binding != "ctypes" and light._CompiledC.ext is None and os.environ.get("DGR_BINDING") == "ctypes":
        pytest.skip("DGR_BINDING=ctypes: the compiled binding is not loaded")
    assert binding == "ctypes" or light._CompiledC.ext is not None, "the compiled extension is not built"
    monkeypatch.setenv("DGR_SYNC_MODE", "strict")
    monkeypatch.delenv("DGR_FORWARD_MODE", raising=False)
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = record_group(variant, views, binding)
    want = {k: [golden["lines"][i] for i in idx] for k, idx in golden["cases"].items() if k.startswith(f"{variant}-{views}-{binding}-")}
    assert sorted(got) == sorted(want)
    for k in got:
        assert got[k], k  # (every case reaches at least one hook)
        assert got[k] == want[k], k


if __name__ == "__main__":  # writes the record (see the module's docstring)
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd")]
    os.environ["DGR_SYNC_MODE"] = "strict"
    os.environ.pop("DGR_FORWARD_MODE", None)
    lines, cases = [], {}
    for variant in VARIANTS:
        for views in VIEWS:
            for binding in BINDINGS:
                for k, ls in record_group(variant, views, binding).items():
                    for ln in ls:
                        if ln not in lines:
                            lines.append(ln)
                    cases[k] = [lines.index(ln) for ln in ls]
    with open(sys.argv[1], "w") as f:
        json.dump({"lines": lines, "cases": cases}, f, indent=0)
        f.write("\n")
    print(f"{len(cases)} cases, {len(lines)} distinct lines -> {sys.argv[1]}")
