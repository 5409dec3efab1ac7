"""What the four front-end modules share (dgr_amd.light, dgr_amd.full: the mirrors of the reference's two __init__.py;
dgr_amd.batch, dgr_amd.batch_full: their V-camera surfaces): the binding selection, one description per variant (`LIGHT`,
`FULL`), the input checks and coercion, the ctypes marshalling of forward and backward, and the one autograd body.

Three module attributes stay the switch points and are read where they are, at call time: `light._C`, `full._C` and
`light._USE_NODE`.  Nothing here keeps a copy of them.
"""
import ctypes as C
import os
import threading
from typing import NamedTuple

import torch

from . import _binning, _capi
from ._binning import _check

MAX_VIEWS = _capi.MAX_BATCH_VIEWS
_row = _capi.row_ptr

# The compiled torch extension (csrc/torch_ext.cpp -> dgr_amd/_dgr_torch_ext.so), or None: DGR_BINDING=ctypes forces the ctypes
# binding, and DGR_HIP_LIB selects another build of the C ABI for the ctypes loader (the extension is linked against the in-tree one).
ext = None
if os.environ.get("DGR_BINDING", "compiled") != "ctypes" and not os.environ.get("DGR_HIP_LIB"):
    try:
        from . import _dgr_torch_ext as ext
    except ImportError:  # the extension is optional (make -C diff-gaussian-rasterization_amd builds it); ctypes still binds the C ABI
        pass


def _ext():
    """the extension (forward_batch<V> / backward_batch<V>: allocation and marshalling in C++) when `light._C` selects the
    compiled binding, else None: the ctypes code below binds the same C ABI"""
    from . import light  # (at call time: the switch point)
    return ext if light._C is light._CompiledC else None


# What a missing image gradient (an output that took no part in the loss) becomes: a zero image, as the reference's autograd would
# have passed; NULL, the lean blend backward; or NULL only with absgrad.  The lean backward is bit-identical to zero images, so the
# rule changes the speed alone.  The two batch surfaces differ from the one-view ones, and from each other.
ZEROS, NULL, LEAN_WITH_ABSGRAD = "zeros", "null", "null with absgrad"


class Variant(NamedTuple):
    """What the front end knows of a variant.  Outputs are named by their view-struct field (include/dgr_hip.h)."""
    stem: str                  # dgr_<stem>_*, ext.<stem>_*
    full: bool                 # reports num_related
    view: type                 # the view structs of the batched entry points
    view_grad: type
    outputs: tuple             # (output, image channels or 0: per Gaussian, its trailing shape, int32?, zero-filled on the one-view
    #                            surface?) in result order
    forward_order: tuple       # the one-view forward entry points' output arguments (gt_depth, an input, sits among them)
    returns: tuple             # the autograd Functions' outputs, in the reference's order
    non_differentiable: tuple
    saved_outputs: tuple       # outputs the backward reads, beside radii and the three state buffers
    images: tuple              # (output, channels, the missing-image rule one view, batch) in the backward's order
    silhouette: str            # the output whose gradient is the silhouette image under the option "silhouette_grad"
    # derived (_with_positions): a forward's tensors are the outputs with the geometry, binning and image buffers behind "radii"
    results: tuple = ()        # their names
    slots: tuple = ()          # positions in `results` of: radii (the buffers follow), saved_outputs, non_differentiable, returns
    image_slots: tuple = ()    # `images` with the output's position in `returns` for its name
    silhouette_slot: int = 0   # the position of `silhouette` in `returns`


def _with_positions(v):
    results = tuple(k for o in v.outputs for k in ((o[0], "geom", "binning", "img") if o[0] == "radii" else o[:1]))
    at = lambda names: tuple(results.index(k) for k in names)  # noqa: E731
    return v._replace(results=results, slots=(results.index("radii"), at(v.saved_outputs), at(v.non_differentiable), at(v.returns)),
                      image_slots=tuple((v.returns.index(k), *rest) for k, *rest in v.images),
                      silhouette_slot=v.returns.index(v.silhouette))


LIGHT = _with_positions(Variant(
    stem="light", full=False, view=_capi.LightView, view_grad=_capi.LightViewGrad,
    outputs=(("out_color", 3, (), False, False), ("out_depth", 1, (), False, False),
             ("out_median_depth", 1, (), False, False), ("out_depth_var", 1, (), False, False),
             ("out_alpha", 1, (), False, False), ("radii", 0, (), True, False),
             ("gau_uncertainty", 0, (1,), False, False), ("gau_related_pixels", 0, (1,), True, False)),
    forward_order=("out_color", "out_depth", "out_median_depth", "out_alpha", "gt_depth", "out_depth_var", "gau_uncertainty",
                   "gau_related_pixels", "radii"),
    returns=("out_color", "radii", "out_depth", "out_median_depth", "out_depth_var", "out_alpha", "gau_uncertainty",
             "gau_related_pixels"),
    # (gau_uncertainty has no gradient input in the C++ backward either; opacity_map has one with "silhouette_grad")
    non_differentiable=("radii", "gau_related_pixels"),
    saved_outputs=("out_alpha",),
    images=(("out_color", 3, ZEROS, ZEROS), ("out_depth", 1, ZEROS, ZEROS), ("out_median_depth", 1, LEAN_WITH_ABSGRAD, ZEROS),
            ("out_depth_var", 1, LEAN_WITH_ABSGRAD, ZEROS)),
    silhouette="out_alpha"))
FULL = _with_positions(Variant(
    stem="full", full=True, view=_capi.FullView, view_grad=_capi.FullViewGrad,
    outputs=(("out_color", 3, (), False, False), ("out_depth", 1, (), False, False),
             ("out_uncertainty", 1, (), False, False), ("radii", 0, (), True, True)),
    forward_order=("out_color", "out_depth", "gt_depth", "out_uncertainty", "radii"),
    returns=("out_color", "radii", "out_depth", "out_uncertainty"),
    non_differentiable=("radii",),
    saved_outputs=(),
    images=(("out_color", 3, ZEROS, ZEROS), ("out_depth", 1, ZEROS, ZEROS), ("out_uncertainty", 1, LEAN_WITH_ABSGRAD, NULL)),
    # (the uncertainty gradient then is the exact silhouette image, and dL_duncertainties is NULL)
    silhouette="out_uncertainty"))


def _f32c(t, dev):
    """contiguous fp32 tensor on `dev` (L/rasterize_points.cu:101-125 calls .contiguous() on every input)."""
    if t.dtype is torch.float32 and t.is_contiguous() and t.device == dev:
        return t  # the common case, checked first
    if t.device != dev:
        t = t.to(dev)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _coerced(dev, *tensors):
    """The input coercion of every ctypes call, one view and batch: each tensor contiguous fp32 on `dev`."""
    return [_f32c(t, dev) for t in tensors]


# dgr_amd.multiview.ViewStreams.before_backward(): an event the rasterizer backward THAT RUNS ON A GIVEN STREAM makes that
# stream wait for once its kernels are issued -- i.e. before autograd goes on to the activations' backward and to the
# accumulation into the leaves' .grad, the only part of a view's backward that touches state shared with the previous view.
# Keyed by the raw stream handle: the wait is set by the thread that calls loss.backward() and consumed by the autograd
# engine's thread (which runs the node on the forward's stream), and two ViewStreams objects -- or two threads -- never
# see each other's entries.  ViewStreams drops a view's entry when the view's block ends (a backward that never reached
# the rasterizer must not leave a stale wait behind).
_post_backward_waits = {}
_post_backward_lock = threading.Lock()


def _set_post_backward_wait(stream, event):
    with _post_backward_lock:
        _post_backward_waits[int(stream.cuda_stream)] = (stream, event)  # (also keeps both objects alive)
    if ext is not None:  # the compiled autograd node consumes the wait inside the engine, without Python
        ext.set_post_backward_wait(int(stream.cuda_stream), int(event.cuda_event))


def _drop_post_backward_wait(stream):
    # (the C++ table is dropped whether or not the Python table still has the entry: the Python Function's backward may have
    #  consumed it -- debug = True, DGR_AUTOGRAD=python -- and the raw event handle the extension holds must not outlive the Event)
    key = int(stream.cuda_stream)
    if _post_backward_waits:
        with _post_backward_lock:
            _post_backward_waits.pop(key, None)
    if ext is not None:
        ext.drop_post_backward_wait(key)


def _consume_post_backward_wait():
    if not _post_backward_waits:
        return
    key = int(torch.cuda.current_stream().cuda_stream)
    with _post_backward_lock:
        w = _post_backward_waits.pop(key, None)
    if w is not None:
        if ext is not None:  # the extension's copy of the entry goes with it (it holds the event's raw handle)
            ext.drop_post_backward_wait(key)
        w[0].wait_event(w[1])


# The flat gradient arena of a backward is found through the gradients themselves (`p.grad._base`, see
# dgr_amd.multiview.GradientArena): no module-level "last arena" is kept, so nothing outlives the gradients and threads
# cannot see each other's arenas.  SPAN_SEGMENTS names the leading segments that form the all-reduce payload.
SPAN_SEGMENTS = ("means3D", "means2D", "sh", "opacity", "scales", "rotations")


def _grad_arena(P, M, f32, alloc=torch):
    """One flat arena holds every per-Gaussian gradient (returned as views), ordered so that the tensors a
    mapping step all-reduces across GPUs -- means3D, means2D, sh, opacity, scales, rotations -- are one
    contiguous span (dgr_amd.multiview.GradientArena).  Every row is written by the kernels (zeros for
    invisible Gaussians; the library clears dL_dsh itself when M > 16), so the arena is not zero-filled.  `alloc`: the caller's
    `torch` (below)."""
    shapes = [("means3D", (P, 3)), ("means2D", (P, 3)), ("sh", (P, M, 3)), ("opacity", (P, 1)),
              ("scales", (P, 3)), ("rotations", (P, 4)), ("cov3D", (P, 6)), ("colors", (P, 3))]
    offs, o = {}, 0
    for name, shp in shapes:
        n = 1
        for d_ in shp:
            n *= d_
        offs[name] = (o, n, shp)
        o += (n + 63) // 64 * 64  # 256-byte aligned segments (vector stores in the kernels)
    arena = (alloc.empty if P else alloc.zeros)((max(o, 1),), **f32)
    return {name: arena[a:a + n].view(shp) for name, (a, n, shp) in offs.items()}


def set_complete_pose_gradient(on=True):
    """Opt in to the complete pose gradient (include/dgr_hip.h: dgr_set_option "pose_grad"): dL_dview becomes the view-matrix
    counterpart of dL_dmeans3D -- 2D covariance, SH colour (through campos = -Rcam^T t) and every depth term included --
    instead of the reference's mean2D + depth terms.  Process-wide; per thread: `_capi.thread_options(pose_grad=1)`."""
    _capi.set_option("pose_grad", 1 if on else 0)


def set_silhouette_gradient(on=True):
    """Opt in to the exact silhouette gradient (include/dgr_hip.h: dgr_set_option "silhouette_grad"): a loss on `opacity_map`
    (light; the full variant's `uncertainty`, the same sum alpha T) then trains the Gaussians and the pose through
    dA/dalpha_k = T_final / (1 - alpha_k), instead of being dropped (light) or taken as the depth variance (full).  Takes effect
    at the next forward; process-wide; per thread: `_capi.thread_options(silhouette_grad=1)`."""
    _capi.set_option("silhouette_grad", 1 if on else 0)


def set_tight_culling(on=True):
    """Opt in to alpha-aware tile rectangles (include/dgr_hip.h: dgr_set_option "tight_cull"): same images and gradients,
    ~40 % fewer tile instances; `num_rendered` and the opaque state buffers are then not the reference's.  Process-wide."""
    _capi.set_option("tight_cull", 1 if on else 0)


def _device_guarded(arg_index):
    """Runs a `_C` function with its tensors' device current (kernels, events and the stream handle all belong to the
    device of `means3D`, whichever device the caller had selected)."""
    def deco(fn):
        def wrapped(*a, **kw):
            with _capi.on_device(a[arg_index].device):
                return fn(*a, **kw)
        wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
        return staticmethod(wrapped)
    return deco


# ---- the checks of the rasterizer classes

def check_means2D_abs(means2D_abs, means3D, map_off, shape=None):
    """The checks of a `means2D_abs` leaf (GaussianRasterizer.forward and the batch classes): float32, on the Gaussians'
    device, [P,3] (or `shape`), and not with map_off (tracking forms no per-Gaussian gradients)."""
    if map_off:
        raise ValueError("means2D_abs: absgrad is a mapping gradient; not with map_off=True")
    shape = (means3D.size(0), 3) if shape is None else shape
    if means2D_abs.dtype != torch.float32 or tuple(means2D_abs.shape) != tuple(shape) or means2D_abs.device != means3D.device:
        raise ValueError(f"means2D_abs: a float32 tensor of shape {tuple(shape)} on {means3D.device} "
                         f"(got {means2D_abs.dtype} {tuple(means2D_abs.shape)} on {means2D_abs.device})")


_EMPTY = torch.Tensor([])  # stands for "None" at the C++ boundary (L/__init__.py:223-232)


def _checked_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp):
    """The checks of the reference's GaussianRasterizer.forward (L/__init__.py:209-232), shared by both variants' one-view and
    batch rasterizers; a missing input becomes _EMPTY (the reference builds a fresh `torch.Tensor([])` per missing input and
    call; one shared empty tensor says the same).  Returns (shs, colors_precomp, scales, rotations, cov3D_precomp)."""
    if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
    e = _EMPTY
    return (e if shs is None else shs, e if colors_precomp is None else colors_precomp, e if scales is None else scales,
            e if rotations is None else rotations, e if cov3D_precomp is None else cov3D_precomp)


def _rasterizer_inputs(means3D, means2D_abs, map_off, shs, colors_precomp, scales, rotations, cov3D_precomp, abs_shape=None):
    """The body of the rasterizer classes' forward before their dispatch: the `means2D_abs` leaf's checks (absgrad, an extension:
    a float32 [P,3] -- `abs_shape` [V,P,3] for a batch -- leaf whose .grad receives the absolute screen-space gradient
    sum_p |dL/dmean2D contribution of pixel p| per Gaussian; AbsGS; include/dgr_hip.h: dgr_light_backward_absgrad), then
    _checked_inputs.  A `means2D_abs` goes to the Function's `apply`: the compiled node has no such input."""
    if means2D_abs is not None:
        check_means2D_abs(means2D_abs, means3D, map_off, abs_shape)
    return _checked_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)


def _check_batch(means3D, viewmatrices):
    """V of a batch: `viewmatrices` is [V,4,4] with 1 <= V <= MAX_VIEWS (as csrc/torch_ext.cpp: forward_batch has it), checked
    before the device and before anything is allocated -- the ctypes binding forms V row pointers into it."""
    V = viewmatrices.size(0) if viewmatrices.dim() == 3 else 0
    if not 1 <= V <= MAX_VIEWS:
        raise RuntimeError(f"1 .. {MAX_VIEWS} views per batch")
    if means3D.device.type != "cuda":
        raise RuntimeError("dgr_hip runs on the GPU only (no CPU path exists, as in the reference)")
    return V


# ---- the forward: ctypes marshalling (one view, batch) and the compiled binding's one-view call

def _outputs(variant, alloc, lead, P, H, W, f32, i32):
    """A forward's output tensors {output: tensor}, in result order; `lead`: () for one view, (V,) for a batch.  The images are
    written whole; the per-Gaussian ones are written for every Gaussian, or zeroed by the C ABI (stream memsets)."""
    out, per_gaussian = {}, alloc.empty if P else alloc.zeros
    for name, channels, trailing, integer, zeroed_one_view in variant.outputs:
        if channels:
            out[name] = alloc.empty(lead + (channels, H, W), **f32)
        else:
            mk = alloc.zeros if zeroed_one_view and not lead else per_gaussian
            out[name] = mk(lead + (P,) + trailing, **(i32 if integer else f32))
    return out


def _early_status(lib):
    """{num_rendered, -, prefiltered violation, -} of the presized forward just issued (include/dgr_hip.h: early status).
    The buffer is per call: ctypes releases the GIL during the wait, so a shared one could be read by another thread."""
    buf = (C.c_int * 4)()
    _check(lib.dgr_early_status_wait(buf))
    return list(buf)


def _forward_r(variant, alloc, background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
               gt_depth, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug=False):
    """The ctypes binding's one-view forward of both variants (L/rasterize_points.cu:35-129, F/rasterize_points.cu:35-120).
    Returns (R for the backward, num_rendered and num_related (full; None for light) to report, the output tensors, geometry,
    binning and image buffers); the mode and capacity come from dgr_amd._binning.  `alloc`: the calling module's `torch`, through
    which every device buffer of the call is allocated -- the guard-region tests stand in for it there."""
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    lib = _capi.load()
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("dgr_hip runs on the GPU only (no CPU path exists, as in the reference)")
    P, H, W = means3D.size(0), int(image_height), int(image_width)
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    (means3D, background, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, gt_depth, sh) = _coerced(
        dev, means3D, background, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, gt_depth, sh)
    M = sh.size(1) if sh.numel() != 0 else 0
    outputs = _outputs(variant, alloc, (), P, H, W, f32, i32)
    out = tuple(outputs.values())
    outputs["gt_depth"] = gt_depth
    st = _capi.stream_handle(dev.index)
    p = _capi.ptr
    common = (P, int(degree), M, p(background), W, H, p(means3D), p(sh), p(colors), p(opacity), p(scales),
              float(scale_modifier), p(rotations), p(cov3D_precomp), p(viewmatrix), p(projmatrix), p(campos),
              float(tan_fovx), float(tan_fovy), int(bool(prefiltered)), *[p(outputs[k]) for k in variant.forward_order])
    full = variant.full
    presized = lib.dgr_full_forward_presized if full else lib.dgr_light_forward_presized

    key = (dev.index, P, H, W)
    mode, use, cap = _binning._binning_policy(key, P)
    if mode == 0:
        bufs = {k: alloc.empty((0,), **u8) for k in ("geom", "binning", "img")}

        def mk(name):
            def cb(nbytes, _user):
                bufs[name] = alloc.empty((max(int(nbytes), 1),), **u8)
                return bufs[name].data_ptr()
            return _capi.ALLOC_FN(cb)
        cbs = [mk("geom"), mk("binning"), mk("img")]
        ng = C.c_int(0)  # (the full variant's num_related; the light one takes the debug flag in its place)
        forward = lib.dgr_full_forward if full else lib.dgr_light_forward
        rendered = _check(forward(st, cbs[0], cbs[1], cbs[2], None, *common, C.byref(ng) if full else int(bool(debug))))
        return rendered, rendered, ng.value if full else None, out, bufs["geom"], bufs["binning"], bufs["img"]
    geom = alloc.empty((lib.dgr_geometry_bytes(P),), **u8)
    img = alloc.empty((lib.dgr_image_bytes(W, H),), **u8)
    status = alloc.empty((4,), **i32)
    if mode == 2:
        binning = alloc.empty((lib.dgr_binning_bytes(use, W, H),), **u8)
        _check(presized(st, p(geom), p(binning), use, p(img), p(status), *common))
        rendered, related, R = _binning.record(key, 2, cap, use, None, status, related=-1 if full else None)
        return R, rendered, related, out, geom, binning, img

    def attempt(capacity):
        binning = alloc.empty((lib.dgr_binning_bytes(capacity, W, H),), **u8)
        lib.dgr_early_status_arm()
        _check(presized(st, p(geom), p(binning), capacity, p(img), p(status), *common))
        # the one host wait of this forward: until num_rendered is known, a tenth of the way into the forward -- not until the
        # forward has finished
        return [_early_status(lib)], binning
    # num_related (the reference's NG) is produced by the forward blend: the second blocking read of the reference
    # (F/cuda_rasterizer/rasterizer_impl.cu:498); lazy mode reports it one call late instead
    (rendered,), related, binning = _binning.strict_retry(key, cap, use, attempt,
                                                          (lambda: status.tolist()[3]) if full else None)
    if debug:
        torch.cuda.synchronize(dev)
    return rendered, rendered, related, out, geom, binning, img


def _compiled_forward_r(variant, background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                        gt_depth, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered,
                        debug=False):
    """The compiled binding's one-view forward of both variants: tensor allocation, argument marshalling and the C-ABI call
    happen in C++; only the capacity / status policy stays in Python.  Returns (R for the backward, num_rendered and num_related
    to report, the tensors: the variant's results)."""
    P, H, W = means3D.size(0) if means3D.dim() else 0, int(image_height), int(image_width)
    args = (background, means3D, colors, opacity, scales, rotations, float(scale_modifier), cov3D_precomp, viewmatrix, gt_depth,
            projmatrix, float(tan_fovx), float(tan_fovy), H, W, sh, int(degree), campos, bool(prefiltered), bool(debug))
    return _binning.compiled_forward(getattr(ext, variant.stem + "_forward"), args, means3D.device.index, P, H, W, variant.full)


@_device_guarded(0)
def _mark_visible(means3D, viewmatrix, projmatrix):
    # L/rasterize_points.cu:238-256 (the ctypes binding's, of both variants)
    lib = _capi.load()
    dev = means3D.device
    P = means3D.size(0)
    present = torch.zeros((P,), dtype=torch.bool, device=dev)
    if P != 0:
        means3D, viewmatrix, projmatrix = _f32c(means3D, dev), _f32c(viewmatrix, dev), _f32c(projmatrix, dev)
        _check(lib.dgr_mark_visible(_capi.stream_handle(dev.index), P, _capi.ptr(means3D), _capi.ptr(viewmatrix),
                                    _capi.ptr(projmatrix), present.data_ptr()))
    return present


@staticmethod
def _mark_visible_compiled(means3D, viewmatrix, projmatrix):
    return ext.mark_visible(means3D, viewmatrix, projmatrix)


def _forward_views(variant, V, bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                   gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered):
    """The batch forward of both variants: the extension's <stem>_forward_batch when selected (_ext), else
    dgr_<stem>_forward_batch through ctypes; mode, capacity, retries and status words follow dgr_amd._binning.run_batch.
    Returns (per-view R for the backward, the [V,4] status words followed by the variant's results)."""
    ext_ = _ext()
    P = means3D.size(0)

    def attempt(cap, lazy):
        if ext_ is not None:
            return getattr(ext_, f"{variant.stem}_forward_batch")(
                bg, means3D, colors, opacity, scales, rotations, float(scale_modifier), cov3D_precomp, viewmatrices, gt_depths,
                projmatrices, float(tanfovx), float(tanfovy), int(H), int(W), sh, int(degree), campos, bool(prefiltered), cap, lazy)
        return _attempt_ctypes(variant, bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                               viewmatrices, gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered,
                               cap, V), None
    return _binning.run_batch((means3D.device.index, P, H, W), P, V, attempt)


def _attempt_ctypes(variant, bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                    gt_depths, projmatrices, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered, cap, V):
    """One ctypes attempt of _forward_views with binning capacity `cap` per view; returns what the extension returns."""
    lib = _capi.load()
    dev = means3D.device
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    (means3D, bg, colors, opacity, scales, rotations, cov3D_precomp, sh, viewmatrices, projmatrices, campos, gt_depths) = _coerced(
        dev, means3D, bg, colors, opacity, scales, rotations, cov3D_precomp, sh, viewmatrices, projmatrices, campos, gt_depths)
    P = means3D.size(0)
    M = sh.size(1) if sh.numel() != 0 else 0
    out = _outputs(variant, torch, (V,), P, H, W, f32, i32)
    geom = torch.empty((V, max(lib.dgr_geometry_bytes(P), 1)), **u8)
    img = torch.empty((V, max(lib.dgr_image_bytes(W, H), 1)), **u8)
    binning = torch.empty((V, max(lib.dgr_binning_bytes(cap, W, H), 1)), **u8)
    status = torch.zeros((V, 4), **i32)
    views = (variant.view * V)()
    per_view = dict(out, geometry_buffer=geom, binning_buffer=binning, image_buffer=img, status=status, viewmatrix=viewmatrices,
                    projmatrix=projmatrices, cam_pos=campos, gt_depth=gt_depths)
    for v in range(V):
        w = views[v]
        w.binning_capacity = cap
        for k, x in per_view.items():
            setattr(w, k, _row(x, v))
    p = _capi.ptr
    _check(getattr(lib, f"dgr_{variant.stem}_forward_batch")(
        _capi.stream_handle(dev.index), V, views, P, int(degree), M, p(bg), W, H, p(means3D), p(sh), p(colors), p(opacity),
        p(scales), float(scale_modifier), p(rotations), p(cov3D_precomp), float(tanfovx), float(tanfovy), int(bool(prefiltered))))
    results = dict(out, geom=geom, binning=binning, img=img)
    return (status, *(results[k] for k in variant.results))


# ---- the backward: ctypes marshalling (one view, batch)

def _tracking_tail(track_off, map_off, need_gaussian_grads):
    """(track_off, map_off) as the light backward entry points take them.  Tracking -- no Gaussian input requires a gradient --
    needs no per-Gaussian sums: the blend kernels then form the three pose sums only, as with map_off.  Decided here for the
    ctypes binding (csrc/torch_ext.cpp decides it for the compiled one)."""
    return int(bool(track_off)), int(bool(map_off or not need_gaussian_grads))


def _backward_one(variant, alloc, grad_arena, abi_args, dview_shape, R, need_gaussian_grads, absgrad, silhouette, means3D, sh,
                  dL_dout_color, *tensors):
    """The ctypes one-view backward of both variants: dgr_<stem>_backward[_absgrad|_silhouette].  `means3D`, `sh`, the colour
    gradient [3,H,W] and `tensors`: the float inputs and image gradients; `abi_args(st, P, M, W, H, i, g, dview, scratch,
    scratch_bytes)` -> the entry point's arguments in its order, from the device pointers `i` of those tensors, in their order,
    and `g` of the per-Gaussian gradients (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales,
    dL_drotations; NULL without need_gaussian_grads).  Returns those eight (views of one arena, or None each), dL_dview and, with
    absgrad, the absolute screen-space gradient [P,3].  `silhouette`: the silhouette gradient image [1,H,W], or None.  `alloc`,
    `grad_arena(P, M, f32)`: the calling module's `torch` and `_grad_arena`, read there at call time (tests stand in for both)."""
    lib = _capi.load()
    dev = means3D.device
    f32 = dict(dtype=torch.float32, device=dev)
    t = _coerced(dev, means3D, sh, dL_dout_color, *tensors)
    P, sh = means3D.size(0), t[1]
    H, W = dL_dout_color.size(1), dL_dout_color.size(2)
    M = sh.size(1) if sh.numel() != 0 else 0
    if need_gaussian_grads:
        seg = grad_arena(P, M, f32)
        out = (seg["means2D"], seg["colors"], seg["opacity"], seg["means3D"], seg["cov3D"], seg["sh"], seg["scales"], seg["rotations"])
    else:
        out = (None,) * 8
    dL_dview = alloc.empty(dview_shape, **f32)
    # (option "deterministic_grads": + 64 bytes per tile instance; R = num_rendered, or the capacity of a lazy forward)
    scratch = alloc.empty((max(lib.dgr_light_backward_scratch_bytes_r(P, W, H, int(R)), 1),), dtype=torch.uint8, device=dev)
    p = _capi.ptr
    args = abi_args(_capi.stream_handle(dev.index), P, M, W, H, [p(x) for x in t], [p(x) for x in out], p(dL_dview), p(scratch),
                    scratch.numel())
    dL_dmeans2D_abs = alloc.empty((P, 3), **f32) if absgrad else None
    _check(_capi.call_backward(variant.stem, 0, args, dL_dmeans2D_abs, None if silhouette is None else _f32c(silhouette, dev)))
    return out + (dL_dview, dL_dmeans2D_abs) if absgrad else out + (dL_dview,)


def _backward_views(variant, per_view, tail, bg, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                    viewmatrices, projmatrices, tanfovx, tanfovy, gt_depths, sh, degree, campos, geom, binning, img,
                    perspec_matrix, need_gaussian_grads, need_means2D, num_rendered, absgrad, silhouette=None):
    """The ctypes batch backward of both variants: dgr_<stem>_backward_batch[_absgrad|_silhouette] (`silhouette`: every view's
    silhouette gradient image [V,1,H,W], or None).  `per_view`: the variant's own [V, ...] inputs by the view struct's field name
    (None: NULL; "dL_dpix" is the colour gradient [V,3,H,W]); `tail`: the entry point's arguments after the common ones.  Returns
    (dL_dmeans2D [V,P,3] or None, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations,
    dL_dview [V,4,4]) and, with absgrad, every view's absolute screen-space gradient [V,P,3]."""
    lib = _capi.load()
    dev = means3D.device
    V, P = viewmatrices.size(0), means3D.size(0)
    f32 = dict(dtype=torch.float32, device=dev)
    H, W = per_view["dL_dpix"].size(2), per_view["dL_dpix"].size(3)
    (means3D, bg, colors, scales, rotations, cov3D_precomp, sh, viewmatrices, projmatrices, campos, gt_depths,
     perspec_matrix) = _coerced(dev, means3D, bg, colors, scales, rotations, cov3D_precomp, sh, viewmatrices, projmatrices, campos,
                                gt_depths, perspec_matrix)
    own = [None if x is None else _f32c(x, dev) for x in per_view.values()]
    M = sh.size(1) if sh.numel() != 0 else 0
    if need_gaussian_grads:
        seg = _grad_arena(P, M, f32)
        seg["means2D"].zero_()  # the arena's one-view slot: the batch returns means2D gradients per view, beside the arena
        d3, dsh, dop, dsc, drot, dcov, dcol = (seg[k] for k in ("means3D", "sh", "opacity", "scales", "rotations", "cov3D", "colors"))
        d2 = torch.empty((V, P, 3), **f32) if need_means2D else None
    else:
        d3 = dsh = dop = dsc = drot = dcov = dcol = d2 = None
    dview = torch.empty((V, 4, 4), **f32)
    nscr = (max(lib.dgr_light_backward_scratch_bytes_r(P, W, H, max(num_rendered + [0])), 1) + 255) // 256 * 256
    scratch = torch.empty((V, nscr), dtype=torch.uint8, device=dev)
    views = (variant.view_grad * V)()
    rows = dict(zip(per_view, own), viewmatrix=viewmatrices, projmatrix=projmatrices, cam_pos=campos, gt_depth=gt_depths,
                geometry_buffer=geom, binning_buffer=binning, image_buffer=img, radii=radii, dL_dmean2D=d2, dL_dview=dview,
                scratch=scratch)
    if perspec_matrix.dim() == 3:  # one projection per view; else the batch's one
        rows["perspec_matrix"] = perspec_matrix
    pp = _capi.ptr(perspec_matrix)
    for v in range(V):
        w = views[v]
        w.perspec_matrix, w.scratch_bytes, w.num_rendered = pp, nscr, num_rendered[v]
        for k, x in rows.items():
            setattr(w, k, _row(x, v))
    p = _capi.ptr
    args = (_capi.stream_handle(dev.index), V, views, P, int(degree), M, p(bg), W, H, p(means3D), p(sh), p(colors), p(scales),
            float(scale_modifier), p(rotations), p(cov3D_precomp), float(tanfovx), float(tanfovy), p(dop), p(dcol), p(d3), p(dcov),
            p(dsh), p(dsc), p(drot)) + tail
    out = (d2, dcol, dop, d3, dcov, dsh, dsc, drot, dview)
    dabs = torch.empty((V, P, 3), **f32) if absgrad else None
    _check(_capi.call_backward(variant.stem, V, args, dabs, None if silhouette is None else _f32c(silhouette, dev)))
    return out + (dabs,) if absgrad else out


# ---- the autograd body of the four Functions

def _record_forward(ctx, variant, raster_settings, R, means2D_abs, colors_precomp, means3D, scales, rotations, cov3Ds_precomp,
                    viewmatrix, sh, gt_depth, results):
    """What every Function's forward leaves for its backward; `results`: the forward's tensors, `variant.results`.  Returns the
    Function's outputs.  (R: the backward's num_rendered -- the capacity of a lazy forward, which never learns its own count.)"""
    radii_slot, saved, non_differentiable, returns = variant.slots
    radii, geom, binning, img = results[radii_slot:radii_slot + 4]
    ctx.raster_settings = raster_settings
    ctx.num_rendered = R
    ctx.absgrad = means2D_abs is not None
    ctx.dgr_options = _capi.load().dgr_thread_options_effective()  # the backward runs under the forward's options
    ctx.silhouette = _capi.silhouette_on(ctx.dgr_options)
    ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrix, radii, sh, geom, binning, img,
                          *[results[i] for i in saved], gt_depth)
    # Outputs without a gradient input in the C++ backward: autograd would still zero-fill a gradient tensor for each of them on
    # every backward.
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(*[results[i] for i in non_differentiable])
    return tuple([results[i] for i in returns])


def _run_backward(ctx, variant, batch, grad_outputs, call):
    """Every Function's backward.  Replaces the image gradients that did not arrive (gradients are not materialised) by the
    variant's rule for the surface; `call(saved tensors, images, need_gaussian_grads, silhouette)` -- `images` in
    `variant.images` order -- runs the surface's backward (under the tensors' device: the `_C` functions and the batches' `call`
    see to that) and returns (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations,
    dL_dview[, the absgrad]); it runs here under the forward's options.  Returns the gradients in the Functions' input order."""
    saved = ctx.saved_tensors  # (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrix, radii, sh, geom, ...)
    absgrad = ctx.absgrad
    null = None if batch else _EMPTY  # NULL: as the batch entry points and the `_C` mirrors take it
    silhouette = grad_outputs[variant.silhouette_slot] if ctx.silhouette else None
    images = []
    for slot, channels, *rules in variant.image_slots:
        image = grad_outputs[slot]
        if ctx.silhouette and slot == variant.silhouette_slot:  # (it went to the silhouette argument)
            image = null
        elif image is None:
            rule = rules[batch]
            if rule is ZEROS or (rule is LEAN_WITH_ABSGRAD and not absgrad):
                rs = ctx.raster_settings
                image = torch.zeros(((saved[5].size(0),) if batch else ()) + (channels, int(rs.image_height), int(rs.image_width)),
                                    dtype=torch.float32, device=saved[1].device)
            else:
                image = null
        images.append(image)
    with _capi.under_options(ctx.dgr_options):  # (the autograd engine may run this on a thread of its own)
        # (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp): tracking needs none
        out = call(saved, images, absgrad or any(ctx.needs_input_grad[:8]), silhouette)
    if not batch:
        # One view: dL_dcolors / dL_dcov3D are handed on only for a colors_precomp / cov3Ds_precomp leaf that needs a gradient
        # (inputs 3 and 7), the compiled node's rule (csrc/torch_ext.cpp: Node::backward, which does not even have the library
        # write them).  The `_C` mirrors of the reference binding keep returning all eight, and what this binding hands the C ABI
        # is on record (tests/golden/frontend_calls.json): here the two are only not passed on to autograd, which dropped them anyway.
        keep = {1: ctx.needs_input_grad[3] and saved[0] is not None and saved[0].numel() != 0,
                4: ctx.needs_input_grad[7] and saved[4] is not None and saved[4].numel() != 0}
        out = tuple(x if keep.get(i, True) else None for i, x in enumerate(out))
    (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales, grad_rotations,
     grad_viewmatrix) = out[:9]
    _consume_post_backward_wait()  # (dgr_amd.multiview.ViewStreams.before_backward)
    return (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales, grad_rotations,
            grad_cov3Ds_precomp, grad_viewmatrix, None, None, out[9] if absgrad else None)
