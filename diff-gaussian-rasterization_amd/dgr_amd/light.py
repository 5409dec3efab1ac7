"""Host-side mirror of diff-gaussian-rasterization-light/diff_gaussian_rasterization/__init__.py.

Same names, argument order, return arity and error behaviour as the reference module
(`GaussianRasterizationSettings`, `GaussianRasterizer`, `rasterize_gaussians`, `_RasterizeGaussians`),
with `_C.*` replaced by calls into the gfx950 C ABI (include/dgr_hip.h).  Differences, all invisible
to a caller of the autograd surface:
  * the per-pixel [H*W,4,4] pose-gradient buffer and its torch.sum (reference __init__.py:160-161)
    do not exist; the C ABI returns the reduced [4,4];
  * forward runs without a mid-pipeline host sync when a binning capacity is known from an earlier
    call of the same shape (one status read at the end instead); DGR_FORWARD_MODE=callback selects the
    strict mirror with allocation callbacks and the reference's blocking read;
  * the debug path's NameError (`deoth_var`, reference __init__.py:93) is not reproduced.
"""
import ctypes as C
import os
from typing import NamedTuple

import threading

import torch
import torch.nn as nn

from . import _binning, _capi
# The binning status policy and its state live in dgr_amd._binning; the names outside code reads are the same objects here
# (mutated in place there, never rebound).  The lazy depth is reached through lazy_depth() / set_lazy_depth() only.
from ._binning import (_capacity_cache, _capture_keepalive, _check, _check_oldest, _last_status, _pending_status,  # noqa: F401
                       _unsettled, check_async_errors, check_captured_status, lazy_depth, set_lazy_depth)


def cpu_deep_copy_tuple(input_tuple):
    copied_tensors = [item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple]
    return tuple(copied_tensors)


def _f32c(t, dev):
    """contiguous fp32 tensor on `dev` (L/rasterize_points.cu:101-125 calls .contiguous() on every input)."""
    if t.dtype is torch.float32 and t.is_contiguous() and t.device == dev:
        return t  # the common case, checked first
    if t.device != dev:
        t = t.to(dev)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


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
    if _CompiledC.ext is not None:  # the compiled autograd node consumes the wait inside the engine, without Python
        _CompiledC.ext.set_post_backward_wait(int(stream.cuda_stream), int(event.cuda_event))


def _drop_post_backward_wait(stream):
    # (the C++ table is dropped whether or not the Python table still has the entry: the Python Function's backward may have
    #  consumed it -- debug = True, DGR_AUTOGRAD=python -- and the raw event handle the extension holds must not outlive the Event)
    key = int(stream.cuda_stream)
    if _post_backward_waits:
        with _post_backward_lock:
            _post_backward_waits.pop(key, None)
    if _CompiledC.ext is not None:
        _CompiledC.ext.drop_post_backward_wait(key)


def _consume_post_backward_wait():
    if not _post_backward_waits:
        return
    key = int(torch.cuda.current_stream().cuda_stream)
    with _post_backward_lock:
        w = _post_backward_waits.pop(key, None)
    if w is not None:
        if _CompiledC.ext is not None:  # the extension's copy of the entry goes with it (it holds the event's raw handle)
            _CompiledC.ext.drop_post_backward_wait(key)
        w[0].wait_event(w[1])


# The flat gradient arena of a backward is found through the gradients themselves (`p.grad._base`, see
# dgr_amd.multiview.GradientArena): no module-level "last arena" is kept, so nothing outlives the gradients and threads
# cannot see each other's arenas.  SPAN_SEGMENTS names the leading segments that form the all-reduce payload.
SPAN_SEGMENTS = ("means3D", "means2D", "sh", "opacity", "scales", "rotations")


def _grad_arena(P, M, f32):
    """One flat arena holds every per-Gaussian gradient (returned as views), ordered so that the tensors a
    mapping step all-reduces across GPUs -- means3D, means2D, sh, opacity, scales, rotations -- are one
    contiguous span (dgr_amd.multiview.GradientArena).  Every row is written by the kernels (zeros for
    invisible Gaussians; the library clears dL_dsh itself when M > 16), so the arena is not zero-filled."""
    shapes = [("means3D", (P, 3)), ("means2D", (P, 3)), ("sh", (P, M, 3)), ("opacity", (P, 1)),
              ("scales", (P, 3)), ("rotations", (P, 4)), ("cov3D", (P, 6)), ("colors", (P, 3))]
    offs, o = {}, 0
    for name, shp in shapes:
        n = 1
        for d_ in shp:
            n *= d_
        offs[name] = (o, n, shp)
        o += (n + 63) // 64 * 64  # 256-byte aligned segments (vector stores in the kernels)
    arena = (torch.empty if P else torch.zeros)((max(o, 1),), **f32)
    return {name: arena[a:a + n].view(shp) for name, (a, n, shp) in offs.items()}


def _early_status(lib):
    """{num_rendered, -, prefiltered violation, -} of the presized forward just issued (include/dgr_hip.h: early status).
    The buffer is per call: ctypes releases the GIL during the wait, so a shared one could be read by another thread."""
    buf = (C.c_int * 4)()
    _check(lib.dgr_early_status_wait(buf))
    return list(buf)


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


def _light_outputs(P, H, W, gt_depth, f32, i32):
    """The light forward's output tensors, and their pointers in the order of its entry points' output arguments."""
    color = torch.empty((3, H, W), **f32)
    depth, median, var, alpha = (torch.empty((1, H, W), **f32) for _ in range(4))
    # radii is written for every Gaussian and the two median statistics are zeroed by the C ABI (stream memsets)
    mk = torch.empty if P else torch.zeros
    radii, unc, px = mk((P,), **i32), mk((P, 1), **f32), mk((P, 1), **i32)
    p = _capi.ptr
    return ((color, depth, median, var, alpha, radii, unc, px),
            (p(color), p(depth), p(median), p(alpha), p(gt_depth), p(var), p(unc), p(px), p(radii)))


def _forward_r(full, outputs, background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
               gt_depth, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug=False):
    """The ctypes binding's one-view forward of both variants (L/rasterize_points.cu:35-129, F/rasterize_points.cu:35-120):
    `full` picks the entry points, `outputs(P, H, W, gt_depth, f32, i32)` -> (the variant's output tensors, their pointers).
    Returns (R for the backward, num_rendered and num_related (full; None for light) to report, the output tensors, geometry,
    binning and image buffers); the mode and capacity come from dgr_amd._binning."""
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
    means3D = _f32c(means3D, dev)
    background, colors, opacity = _f32c(background, dev), _f32c(colors, dev), _f32c(opacity, dev)
    scales, rotations, cov3D_precomp = _f32c(scales, dev), _f32c(rotations, dev), _f32c(cov3D_precomp, dev)
    viewmatrix, projmatrix, campos = _f32c(viewmatrix, dev), _f32c(projmatrix, dev), _f32c(campos, dev)
    gt_depth, sh = _f32c(gt_depth, dev), _f32c(sh, dev)
    M = sh.size(1) if sh.numel() != 0 else 0
    out, out_ptrs = outputs(P, H, W, gt_depth, f32, i32)
    st = _capi.stream_handle(dev.index)
    p = _capi.ptr
    common = (P, int(degree), M, p(background), W, H, p(means3D), p(sh), p(colors), p(opacity), p(scales),
              float(scale_modifier), p(rotations), p(cov3D_precomp), p(viewmatrix), p(projmatrix), p(campos),
              float(tan_fovx), float(tan_fovy), int(bool(prefiltered))) + out_ptrs
    forward, presized = ((lib.dgr_full_forward, lib.dgr_full_forward_presized) if full else
                         (lib.dgr_light_forward, lib.dgr_light_forward_presized))

    key = (dev.index, P, H, W)
    mode, use, cap = _binning._binning_policy(key, P)
    if mode == 0:
        bufs = {k: torch.empty((0,), **u8) for k in ("geom", "binning", "img")}

        def mk(name):
            def cb(nbytes, _user):
                bufs[name] = torch.empty((max(int(nbytes), 1),), **u8)
                return bufs[name].data_ptr()
            return _capi.ALLOC_FN(cb)
        cbs = [mk("geom"), mk("binning"), mk("img")]
        ng = C.c_int(0)  # (the full variant's num_related; the light one takes the debug flag in its place)
        rendered = _check(forward(st, cbs[0], cbs[1], cbs[2], None, *common, C.byref(ng) if full else int(bool(debug))))
        return rendered, rendered, ng.value if full else None, out, bufs["geom"], bufs["binning"], bufs["img"]
    geom = torch.empty((lib.dgr_geometry_bytes(P),), **u8)
    img = torch.empty((lib.dgr_image_bytes(W, H),), **u8)
    status = torch.empty((4,), **i32)
    if mode == 2:
        binning = torch.empty((lib.dgr_binning_bytes(use, W, H),), **u8)
        _check(presized(st, p(geom), p(binning), use, p(img), p(status), *common))
        rendered, related, R = _binning.record(key, 2, cap, use, None, status, related=-1 if full else None)
        return R, rendered, related, out, geom, binning, img

    def attempt(capacity):
        binning = torch.empty((lib.dgr_binning_bytes(capacity, W, H),), **u8)
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


class _C:
    """Functions with the signatures of the reference's pybind11 module `_C` (L/ext.cpp:15-19)."""

    @staticmethod
    def rasterize_gaussians(*args):
        # L/rasterize_points.cu:35-129.  The tuple's num_rendered is the count last read for the shape (a lazy forward's own
        # count is read one call late); the autograd Function takes its backward's R from rasterize_gaussians_r.
        return _CtypesC.rasterize_gaussians_r(*args)[1]

    @_device_guarded(1)
    def rasterize_gaussians_r(background, means3D, colors, opacity, scales, rotations, scale_modifier,
                              cov3D_precomp, viewmatrix, gt_depth, projmatrix, tan_fovx, tan_fovy,
                              image_height, image_width, sh, degree, campos, prefiltered, debug):
        """(R for the backward, the `rasterize_gaussians` tuple).  R is the exact count of a strict forward and the capacity
        the binning buffer was carved with of a lazy one (dgr_amd._binning.record)."""
        R, rendered, _, out, geom, binning, img = _forward_r(
            False, _light_outputs, background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
            viewmatrix, gt_depth, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered,
            debug)
        color, depth, median, var, alpha, radii, unc, px = out
        return R, (rendered, color, depth, median, var, alpha, radii, geom, binning, img, unc, px)

    @_device_guarded(1)
    def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                     cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                     dL_dout_depth, dL_dout_median_depth, dL_dout_depth_var, gt_depth, sh, degree,
                                     campos, geomBuffer, R, binningBuffer, imageBuffer, alphas, debug,
                                     perspec_matrix, track_off, map_off, need_gaussian_grads=True, absgrad=False,
                                     silhouette=None):
        # L/rasterize_points.cu:131-236.  `need_gaussian_grads=False` (an extension: the autograd Function passes it when
        # no Gaussian input requires a gradient, i.e. tracking) returns None for the eight per-Gaussian gradients and lets
        # the library skip their dense rows; the pose gradient is the same.  `absgrad=True` (dgr_light_backward_absgrad)
        # appends a tenth result, the absolute screen-space gradient [P,3].  `silhouette` (dgr_light_backward_silhouette):
        # the opacity_map gradient [1,H,W], or None (no image).
        lib = _capi.load()
        dev = means3D.device
        P = means3D.size(0)
        H, W = dL_dout_color.size(1), dL_dout_color.size(2)
        f32 = dict(dtype=torch.float32, device=dev)
        means3D = _f32c(means3D, dev)
        background, colors = _f32c(background, dev), _f32c(colors, dev)
        scales, rotations, cov3D_precomp = _f32c(scales, dev), _f32c(rotations, dev), _f32c(cov3D_precomp, dev)
        viewmatrix, projmatrix, campos = _f32c(viewmatrix, dev), _f32c(projmatrix, dev), _f32c(campos, dev)
        gt_depth, sh, alphas = _f32c(gt_depth, dev), _f32c(sh, dev), _f32c(alphas, dev)
        perspec_matrix = _f32c(perspec_matrix, dev)
        gC, gD = _f32c(dL_dout_color, dev), _f32c(dL_dout_depth, dev)
        gM, gV = _f32c(dL_dout_median_depth, dev), _f32c(dL_dout_depth_var, dev)
        M = sh.size(1) if sh.numel() != 0 else 0
        if need_gaussian_grads:
            seg = _grad_arena(P, M, f32)
            dL_dmeans3D, dL_dmeans2D, dL_dsh, dL_dopacity = seg["means3D"], seg["means2D"], seg["sh"], seg["opacity"]
            dL_dscales, dL_drotations, dL_dcov3D, dL_dcolors = seg["scales"], seg["rotations"], seg["cov3D"], seg["colors"]
        else:
            dL_dmeans3D = dL_dmeans2D = dL_dsh = dL_dopacity = dL_dscales = dL_drotations = dL_dcov3D = dL_dcolors = None
            map_off = True  # nobody reads the per-Gaussian sums: the blend kernel forms the three pose sums only
        # [1,4,4]: the reference binding returns the per-pixel [H*W,4,4] buffer and its __init__.py sums dim 0
        # (L/rasterize_points.cu:186,235, L/__init__.py:160-161); one already-reduced "pixel" keeps that code working
        dL_dview = torch.empty((1, 4, 4), **f32)
        # (option "deterministic_grads": + 64 bytes per tile instance; R = num_rendered, or the capacity of a lazy forward)
        scratch = torch.empty((max(lib.dgr_light_backward_scratch_bytes_r(P, W, H, int(R)), 1),), dtype=torch.uint8, device=dev)
        p = _capi.ptr
        args = (_capi.stream_handle(dev.index), P, int(degree), M, int(R), p(background), W, H, p(means3D), p(sh), p(colors),
                p(alphas), p(scales), float(scale_modifier), p(rotations), p(cov3D_precomp), p(viewmatrix),
                p(projmatrix), p(campos), float(tan_fovx), float(tan_fovy), p(radii), p(geomBuffer), p(binningBuffer),
                p(imageBuffer), p(gC), p(gD), p(gM), p(gV), p(dL_dmeans2D), None, p(dL_dopacity), p(dL_dcolors), None,
                p(dL_dmeans3D), p(dL_dcov3D), p(dL_dsh), p(dL_dscales), p(dL_drotations), int(bool(debug)), None,
                p(perspec_matrix), p(dL_dview), None, p(gt_depth), int(bool(track_off)), int(bool(map_off)),
                p(scratch), scratch.numel())
        out = (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dL_dview)
        dL_dmeans2D_abs = torch.empty((P, 3), **f32) if absgrad else None
        _check(_capi.call_backward("light", 0, args, dL_dmeans2D_abs, None if silhouette is None else _f32c(silhouette, dev)))
        return out + (dL_dmeans2D_abs,) if absgrad else out

    @_device_guarded(0)
    def mark_visible(means3D, viewmatrix, projmatrix):
        # L/rasterize_points.cu:238-256
        lib = _capi.load()
        dev = means3D.device
        P = means3D.size(0)
        present = torch.zeros((P,), dtype=torch.bool, device=dev)
        if P != 0:
            means3D, viewmatrix, projmatrix = _f32c(means3D, dev), _f32c(viewmatrix, dev), _f32c(projmatrix, dev)
            _check(lib.dgr_mark_visible(_capi.stream_handle(dev.index), P, _capi.ptr(means3D), _capi.ptr(viewmatrix),
                                        _capi.ptr(projmatrix), present.data_ptr()))
        return present


class _CompiledC:
    """The same three functions over the compiled torch extension (csrc/torch_ext.cpp -> dgr_amd/_dgr_torch_ext.so), the
    counterpart of the reference's pybind11 `_C` (L/ext.cpp:15-19): tensor allocation, argument marshalling and the C-ABI
    call happen in C++; only the capacity / status policy above stays in Python.  Selected when the extension is built
    (DGR_BINDING=ctypes forces the ctypes class)."""

    ext = None

    @staticmethod
    def rasterize_gaussians(*args):
        return _CompiledC.rasterize_gaussians_r(*args)[1]

    @staticmethod
    def rasterize_gaussians_r(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                              viewmatrix, gt_depth, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree,
                              campos, prefiltered, debug):
        """(R for the backward, the `rasterize_gaussians` tuple): see _C.rasterize_gaussians_r."""
        P, H, W = means3D.size(0) if means3D.dim() else 0, int(image_height), int(image_width)
        args = (background, means3D, colors, opacity, scales, rotations, float(scale_modifier), cov3D_precomp, viewmatrix, gt_depth,
                projmatrix, float(tan_fovx), float(tan_fovy), H, W, sh, int(degree), campos, bool(prefiltered), bool(debug))
        # tensors: color, depth, median, var, alpha, radii, geom, binning, img, unc, px
        R, rendered, _, tensors = _binning.compiled_forward(_CompiledC.ext.light_forward, args, means3D.device.index, P, H, W, False)
        return R, (rendered, *tensors)

    @staticmethod
    def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                     viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_depth,
                                     dL_dout_median_depth, dL_dout_depth_var, gt_depth, sh, degree, campos, geomBuffer, R,
                                     binningBuffer, imageBuffer, alphas, debug, perspec_matrix, track_off, map_off,
                                     need_gaussian_grads=True, absgrad=False, silhouette=None):
        args = (background, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp, viewmatrix,
                projmatrix, float(tan_fovx), float(tan_fovy), dL_dout_color, dL_dout_depth, dL_dout_median_depth,
                dL_dout_depth_var, gt_depth, sh, int(degree), campos, geomBuffer, int(R), binningBuffer, imageBuffer, alphas,
                bool(debug), perspec_matrix, bool(track_off), bool(map_off), bool(need_gaussian_grads),
                _EMPTY if silhouette is None else silhouette, bool(absgrad))
        return tuple(_CompiledC.ext.light_backward(*args))

    @staticmethod
    def mark_visible(means3D, viewmatrix, projmatrix):
        return _CompiledC.ext.mark_visible(means3D, viewmatrix, projmatrix)


# DGR_AUTOGRAD=python keeps the Python autograd.Function over the compiled `_C` (the A/B for profiles/host_breakdown.py)
_USE_NODE = os.environ.get("DGR_AUTOGRAD", "compiled") != "python"
_CtypesC = _C
# (DGR_HIP_LIB selects another build of the C ABI for the ctypes loader; the extension is linked against the in-tree one)
if os.environ.get("DGR_BINDING", "compiled") != "ctypes" and not os.environ.get("DGR_HIP_LIB"):
    try:
        from . import _dgr_torch_ext as _ext
        _CompiledC.ext = _ext
        _C = _CompiledC
    except ImportError:  # the extension is optional (make -C diff-gaussian-rasterization_amd builds it); ctypes still binds the C ABI
        pass


def _rasterize_compiled(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix,
                        gt_depth, rs):
    """`_RasterizeGaussians.apply` through the autograd node compiled into the extension (csrc/torch_ext.cpp: Node<Light>):
    one Python -> C++ crossing per forward, the backward runs inside the autograd engine without the interpreter.  Same
    inputs, outputs, saved state and gradients as the Python Function below, which stays for the debug path and the ctypes
    binding."""
    P, H, W = (means3D.size(0) if means3D.dim() == 2 else 0), rs.image_height, rs.image_width
    args = (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, gt_depth, rs.bg,
            rs.projmatrix, rs.campos, rs.perspec_matrix, rs.scale_modifier, rs.tanfovx, rs.tanfovy, H, W, rs.sh_degree,
            rs.prefiltered, rs.track_off, rs.map_off)
    return tuple(_binning.compiled_forward(_CompiledC.ext.light_apply, args, means3D.device.index, P, H, W, False)[3])


def rasterize_gaussians(
    means3D,
    means2D,
    sh,
    colors_precomp,
    opacities,
    scales,
    rotations,
    cov3Ds_precomp,
    viewmatrix,
    gt_depth,
    raster_settings,
):
    if _C is _CompiledC and not raster_settings.debug and _USE_NODE:
        return _rasterize_compiled(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                   viewmatrix, gt_depth, raster_settings)
    return _RasterizeGaussians.apply(
        means3D,
        means2D,
        sh,
        colors_precomp,
        opacities,
        scales,
        rotations,
        cov3Ds_precomp,
        viewmatrix,
        gt_depth,
        raster_settings,
    )


class _RasterizeGaussians(torch.autograd.Function):
    """`means2D_abs` (absgrad, an extension): one more leaf [P,3] whose gradient is the absolute screen-space gradient
    (include/dgr_hip.h: dgr_light_backward_absgrad); None when absent.  Over either binding's forward and backward: the compiled
    compiled node has no such input.  With the option "silhouette_grad" on at the forward, the opacity_map gradient goes to the
    backward as the silhouette image (dgr_light_backward_silhouette); without it, it is dropped, as the reference does."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                viewmatrix, gt_depth, raster_settings, means2D_abs=None):
        # argument packing of L/diff_gaussian_rasterization/__init__.py:66-87
        args = (
            raster_settings.bg,
            means3D,
            colors_precomp,
            opacities,
            scales,
            rotations,
            raster_settings.scale_modifier,
            cov3Ds_precomp,
            viewmatrix,
            gt_depth,
            raster_settings.projmatrix,
            raster_settings.tanfovx,
            raster_settings.tanfovy,
            raster_settings.image_height,
            raster_settings.image_width,
            sh,
            raster_settings.sh_degree,
            raster_settings.campos,
            raster_settings.prefiltered,
            raster_settings.debug,
        )
        # (R: the backward's num_rendered -- the capacity of a lazy forward, which never learns its own count)
        if raster_settings.debug:
            cpu_args = cpu_deep_copy_tuple(args)
            try:
                R, out = _C.rasterize_gaussians_r(*args)
            except Exception as ex:
                torch.save(cpu_args, "snapshot_fw.dump")
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
                raise ex
        else:
            R, out = _C.rasterize_gaussians_r(*args)
        (_, color, depth, depth_median, depth_var, opacity_map, radii, geomBuffer, binningBuffer,
         imgBuffer, gau_uncertainty, gau_related_pixels) = out

        ctx.raster_settings = raster_settings
        ctx.num_rendered = R
        ctx.absgrad = means2D_abs is not None
        ctx.dgr_options = _capi.load().dgr_thread_options_effective()  # the backward runs under the forward's options
        ctx.silhouette = _capi.silhouette_on(ctx.dgr_options)
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrix, radii, sh,
                              geomBuffer, binningBuffer, imgBuffer, opacity_map, gt_depth)
        # Four of the eight outputs (radii, opacity_map, gau_uncertainty, gau_related_pixels) have no gradient input in
        # the C++ backward (opacity_map has one with "silhouette_grad"); autograd would still zero-fill a gradient tensor for
        # each of them on every backward.
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii, gau_related_pixels)
        return color, radii, depth, depth_median, depth_var, opacity_map, gau_uncertainty, gau_related_pixels

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_depth_median, grad_depth_var, grad_alpha,
                 grad_gau_uncertainty, grad_gau_realted_pixels):
        num_rendered = ctx.num_rendered
        raster_settings = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, viewmatrix, radii, sh, geomBuffer,
         binningBuffer, imgBuffer, opacity_map, gt_depth) = ctx.saved_tensors
        # an output that did not take part in the loss arrives as None (gradients are not materialised): zeros, as the
        # reference's autograd would have passed
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        zeros = lambda c: torch.zeros((c, H, W), dtype=torch.float32, device=means3D.device)  # noqa: E731
        absgrad = ctx.absgrad
        grad_color = zeros(3) if grad_color is None else grad_color
        grad_depth = zeros(1) if grad_depth is None else grad_depth
        if absgrad:  # an unused median / variance output: NULL, the lean blend backward (bit-identical to zero images)
            grad_depth_median = _EMPTY if grad_depth_median is None else grad_depth_median
            grad_depth_var = _EMPTY if grad_depth_var is None else grad_depth_var
        grad_depth_median = zeros(1) if grad_depth_median is None else grad_depth_median
        grad_depth_var = zeros(1) if grad_depth_var is None else grad_depth_var

        # argument packing of L/diff_gaussian_rasterization/__init__.py:116-146
        args = (raster_settings.bg,
                means3D,
                radii,
                colors_precomp,
                scales,
                rotations,
                raster_settings.scale_modifier,
                cov3Ds_precomp,
                viewmatrix,
                raster_settings.projmatrix,
                raster_settings.tanfovx,
                raster_settings.tanfovy,
                grad_color,
                grad_depth,
                grad_depth_median,
                grad_depth_var,
                gt_depth,
                sh,
                raster_settings.sh_degree,
                raster_settings.campos,
                geomBuffer,
                num_rendered,
                binningBuffer,
                imgBuffer,
                opacity_map,
                raster_settings.debug,
                raster_settings.perspec_matrix,
                raster_settings.track_off,
                raster_settings.map_off)

        # (option "silhouette_grad" at the forward: the opacity_map gradient is the silhouette image; an unused one is NULL)
        debug = raster_settings.debug
        cpu_args = cpu_deep_copy_tuple(args) if debug else None
        with _capi.under_options(ctx.dgr_options):  # (the autograd engine may run this on a thread of its own)
            try:
                # (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp): tracking needs none
                out = _C.rasterize_gaussians_backward(
                    *args, need_gaussian_grads=debug or absgrad or any(ctx.needs_input_grad[:8]), absgrad=absgrad,
                    silhouette=grad_alpha if ctx.silhouette else None)
            except Exception:
                if debug:
                    torch.save(cpu_args, "snapshot_bw.dump")
                    print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
                raise
        grad_means2D_abs = out[9] if absgrad else None
        out = out[:9]
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_rotations, grad_viewmatrix) = out
        # reference: torch.sum(grad_viewmatrix, dim=0) over a [H*W,4,4] buffer (__init__.py:160-161);
        # here the buffer is [1,4,4], already reduced: a view instead of a reduction kernel.
        grad_viewmatrix = grad_viewmatrix.view(4, 4)
        _consume_post_backward_wait()

        grads = (
            grad_means3D,
            grad_means2D,
            grad_sh,
            grad_colors_precomp,
            grad_opacities,
            grad_scales,
            grad_rotations,
            grad_cov3Ds_precomp,
            grad_viewmatrix,
            None,
            None,
            grad_means2D_abs,
        )
        return grads


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


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    perspec_matrix: torch.Tensor
    track_off: bool
    map_off: bool


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        # Mark visible points (based on frustum culling for camera) with a boolean
        with torch.no_grad():
            raster_settings = self.raster_settings
            visible = _C.mark_visible(
                positions,
                raster_settings.viewmatrix,
                raster_settings.projmatrix)
        return visible

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, viewmatrix=None, gt_depth=None, *, means2D_abs=None):
        # means2D_abs (absgrad, an extension): a float32 [P,3] leaf whose .grad receives the absolute screen-space gradient
        # sum_p |dL/dmean2D contribution of pixel p| per Gaussian (AbsGS; include/dgr_hip.h: dgr_light_backward_absgrad)
        raster_settings = self.raster_settings
        if means2D_abs is not None:
            check_means2D_abs(means2D_abs, means3D, raster_settings.map_off)
        shs, colors_precomp, scales, rotations, cov3D_precomp = _checked_inputs(shs, colors_precomp, scales, rotations,
                                                                                cov3D_precomp)
        if means2D_abs is not None:
            return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                             cov3D_precomp, viewmatrix, gt_depth, raster_settings, means2D_abs)
        return rasterize_gaussians(
            means3D,
            means2D,
            shs,
            colors_precomp,
            opacities,
            scales,
            rotations,
            cov3D_precomp,
            viewmatrix,
            gt_depth,
            raster_settings,
        )
