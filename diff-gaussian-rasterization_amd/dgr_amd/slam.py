"""The caller's side of the rasterizer: CG-SLAM's `render()` and the camera tensors a tracking or
mapping step feeds it.

The reference repository documents this call but does not contain it (README.md:33-47, 71-96: `render(viewpoint_cam,
gaussians, pipe, background, viewmatrix=w2cT, fov=(tanfovx, tanfovy), HW=(H, W), gt_depth=..., track_off=...,
map_off=...)` returning a dict); it lives in CG-SLAM and follows the 3DGS `gaussian_renderer.render`.  This module
restates it over `dgr_amd.light` / `dgr_amd.full`, duck-typed on the 3DGS `GaussianModel` accessors, and adds the
differentiable pose -> matrices helpers, so that a whole tracking iteration (pose parameters -> viewmatrix -> render ->
loss -> backward -> pose update) can run without leaving the GPU.

Matrix convention (cuda_rasterizer/auxiliary.h:58-77 reads 16 floats column-major): the rasterizer takes W2C^T,
(Proj W2C)^T and Proj^T.  The analytic pose gradient is returned w.r.t. the `viewmatrix` tensor only; `projmatrix` and
`campos` are recomputed from the same pose but enter as constants, exactly as in the reference (its backward adds their
dependence inside the kernels: L/cuda_rasterizer/backward.cu:633-651, 683-751).
"""
import contextlib as _contextlib
from collections.abc import Mapping as _Mapping
from typing import NamedTuple as _NamedTuple

import torch

from . import full as _full
from . import light as _light


_proj_cache = {}


def projection_matrix(tanfovx, tanfovy, znear=0.01, zfar=100.0, device=None, dtype=torch.float32):
    """Proj (row-major math, z forward, as 3DGS `getProjectionMatrix` with symmetric frustum).  Cached per argument set
    (treat the result as read-only): building it copies host scalars to the device, which a hipGraph capture forbids,
    so a captured step finds the matrix its eager warm-up made."""
    key = (float(tanfovx), float(tanfovy), float(znear), float(zfar), str(device), dtype)
    P = _proj_cache.get(key)
    if P is None:
        P = torch.zeros((4, 4), dtype=dtype)
        P[0, 0] = 1.0 / tanfovx
        P[1, 1] = 1.0 / tanfovy
        P[2, 2] = zfar / (zfar - znear)
        P[2, 3] = -(zfar * znear) / (zfar - znear)
        P[3, 2] = 1.0
        P = _proj_cache[key] = P.to(device) if device is not None else P
    return P


_const_cache = {}


def _constants(device, dtype):
    """(identity, Levi-Civita tensor, bottom row) on `device`, built once (host -> device copies are not capturable)."""
    key = (str(device), dtype)
    c = _const_cache.get(key)
    if c is None:
        eps = torch.zeros((3, 3, 3), dtype=dtype)
        for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            eps[i, j, k], eps[i, k, j] = 1.0, -1.0
        c = _const_cache[key] = (torch.eye(3, dtype=dtype).to(device), eps.to(device),
                                 torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=dtype).to(device))
    return c


def quat_to_rotmat(q):
    """Unit quaternion (r, x, y, z) -> 3x3 rotation, differentiable (q is normalised here).
    R = (r^2 - |v|^2) I + 2 v v^T + 2 r [v]x in a dozen tensor operations (a tracking loop is launch-bound)."""
    eye, eps, _ = _constants(q.device, q.dtype)
    q = q / q.norm()
    r, v = q[0], q[1:]
    cross = -(eps * v).sum(-1)  # [v]x: cross[i][j] = -eps[i][j][k] v[k]
    return (r * r - (v * v).sum()) * eye + 2.0 * v.unsqueeze(1) * v.unsqueeze(0) + (2.0 * r) * cross


def w2c_from_quat_trans(q, t):
    """World-to-camera 4x4 from a quaternion and a translation (both differentiable leaves of a tracking step)."""
    top = torch.cat([quat_to_rotmat(q), t.reshape(3, 1)], dim=1)
    return torch.cat([top, _constants(q.device, q.dtype)[2]], dim=0)


def _small_matmul(a, b):
    """a @ b for 3x3 / 4x4 operands as one broadcast multiply and one sum: a BLAS call for sixteen numbers costs more
    host time on ROCm (≈1.5 ms: handle and heuristics) than the whole render."""
    return (a.unsqueeze(-1) * b.unsqueeze(-3)).sum(-2)


def camera_tensors(w2c, tanfovx, tanfovy, znear=0.01, zfar=100.0):
    """(viewmatrix, projmatrix, perspec_matrix, campos) for the rasterizer from a world-to-camera matrix.
    `viewmatrix` stays attached to `w2c`'s graph; the other three are detached (see the module docstring)."""
    P = projection_matrix(tanfovx, tanfovy, znear, zfar, device=w2c.device, dtype=w2c.dtype)
    viewmatrix = w2c.transpose(0, 1).contiguous()
    with torch.no_grad():
        perspec = P.transpose(0, 1).contiguous()
        projmatrix = _small_matmul(w2c.transpose(0, 1), P.transpose(0, 1)).contiguous()
        campos = (-(w2c[:3, :3] * w2c[:3, 3:4]).sum(0)).contiguous()  # -(R^T t)
    return viewmatrix, projmatrix, perspec, campos


class _PoseToCamera(torch.autograd.Function):
    """(quaternion, translation) -> (viewmatrix, projmatrix, campos) in one launch, dL/dviewmatrix -> (dL/dq, dL/dt) in
    another (C ABI: dgr_pose_forward / dgr_pose_backward).  Same function as
    `camera_tensors(w2c_from_quat_trans(q, t), ...)`: only `viewmatrix` carries a gradient."""

    @staticmethod
    def forward(ctx, q, t, perspec):
        from . import _capi
        lib = _capi.load()
        q, t, perspec = q.contiguous(), t.contiguous(), perspec.contiguous()
        out = torch.empty((35,), dtype=torch.float32, device=q.device)
        view, proj, campos = out[:16].view(4, 4), out[16:32].view(4, 4), out[32:35]
        if lib.dgr_pose_forward(_capi.stream_handle(), q.data_ptr(), t.data_ptr(), perspec.data_ptr(), view.data_ptr(),
                                proj.data_ptr(), campos.data_ptr()):
            raise RuntimeError(_capi.last_error())
        ctx.save_for_backward(q)
        ctx.mark_non_differentiable(proj, campos)
        return view, proj, campos

    @staticmethod
    def backward(ctx, dview, _dproj, _dcampos):
        from . import _capi
        lib = _capi.load()
        (q,) = ctx.saved_tensors
        grads = torch.empty((7,), dtype=torch.float32, device=q.device)
        dview = dview.contiguous()
        if lib.dgr_pose_backward(_capi.stream_handle(), q.data_ptr(), dview.data_ptr(), grads.data_ptr(),
                                 grads[4:].data_ptr()):
            raise RuntimeError(_capi.last_error())
        return grads[:4], grads[4:], None


# ---- tensors kept between calls (the caches below) are made by kernels of whichever stream was current at their first use.  A
# later call on ANOTHER stream (dgr_amd.multiview.ViewStreams: a stream per view) must not read them before those kernels have
# finished: every cache entry carries a stamp -- the creating stream and an event recorded behind the kernels that wrote the
# tensors -- and a consumer on a different stream waits for that event once (per stream).  While a hipGraph is being recorded
# nothing is cached.  The keys are (id, _version) of the source tensors: an in-place `viewmatrix.data = ...` swap changes
# neither and is NOT supported for cached poses -- assign a new tensor, or update it in place with copy_().
class _Stamp:
    __slots__ = ("stream", "event", "seen")

    def __init__(self, device):
        st = torch.cuda.current_stream(device)
        self.stream = int(st.cuda_stream)
        self.event = torch.cuda.Event()
        self.event.record(st)
        self.seen = {self.stream}

    def order(self, device):
        # (the raw handle first: building a Stream object per call costs more than the tensors the cache saves)
        h = torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())
        if h not in self.seen:
            torch.cuda.current_stream(device).wait_event(self.event)
            if len(self.seen) < 64:
                self.seen.add(h)


def _stamp(device):
    dev = torch.device(device)
    return _Stamp(dev) if dev.type == "cuda" else None


_PERSPEC = {}  # (tanfovx, tanfovy, znear, zfar, device) -> (Proj^T, stamp): a constant of the sensor, built once


def _perspec_cached(tanfovx, tanfovy, znear, zfar, device):
    key = (float(tanfovx), float(tanfovy), float(znear), float(zfar), device)
    hit = _PERSPEC.get(key)
    if hit is None:
        if len(_PERSPEC) > 32:
            _PERSPEC.clear()
        m = projection_matrix(tanfovx, tanfovy, znear, zfar, device=device).transpose(0, 1).contiguous()
        if m.is_cuda and torch.cuda.is_current_stream_capturing():
            return m
        hit = _PERSPEC[key] = (m, _stamp(m.device))
    if hit[1] is not None:
        hit[1].order(hit[0].device)
    return hit[0]


def pose_to_camera(q, t, tanfovx, tanfovy, znear=0.01, zfar=100.0):
    """(viewmatrix, projmatrix, perspec_matrix, campos) from a quaternion (r, x, y, z) and a translation, float32 GPU
    tensors: the fused form of `camera_tensors(w2c_from_quat_trans(q, t), tanfovx, tanfovy)` (2 launches for forward +
    backward instead of ~40 elementwise torch kernels).  The perspec_matrix is a symmetric frustum's (principal point at the
    image centre); an off-centre camera goes through `render(viewpoint_camera=...)` with its own `projection_matrix`."""
    for x, n, name in ((q, 4, "q"), (t, 3, "t")):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.numel() != n:
            raise ValueError(f"pose_to_camera: {name} must be a float32 tensor of {n} elements")
    if not q.is_cuda or t.device != q.device:
        raise ValueError("pose_to_camera: q and t must be on one GPU (there is no CPU fallback)")
    perspec = _perspec_cached(tanfovx, tanfovy, znear, zfar, q.device)
    view, proj, campos = _PoseToCamera.apply(q, t, perspec)
    return view, proj, perspec, campos


class _L1Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, depth, color_obs, depth_obs, w_color, w_depth):
        from . import _capi
        lib = _capi.load()
        color, depth, color_obs, depth_obs = (x.contiguous() for x in (color, depth, color_obs, depth_obs))
        buf = torch.empty((lib.dgr_l1_loss_scratch_floats() + 1,), dtype=torch.float32, device=color.device)
        if lib.dgr_l1_loss_forward(_capi.stream_handle(), color.numel(), color.data_ptr(), color_obs.data_ptr(), depth.numel(),
                                   depth.data_ptr(), depth_obs.data_ptr(), float(w_color), float(w_depth), buf[1:].data_ptr(),
                                   buf.data_ptr()):
            raise RuntimeError(_capi.last_error())
        ctx.save_for_backward(color, depth, color_obs, depth_obs)
        ctx.weights = (float(w_color), float(w_depth))
        return buf[0]

    @staticmethod
    def backward(ctx, upstream):
        from . import _capi
        lib = _capi.load()
        color, depth, color_obs, depth_obs = ctx.saved_tensors
        dc, dd = torch.empty_like(color), torch.empty_like(depth)
        upstream = upstream.contiguous()
        if lib.dgr_l1_loss_backward(_capi.stream_handle(), color.numel(), color.data_ptr(), color_obs.data_ptr(), depth.numel(),
                                    depth.data_ptr(), depth_obs.data_ptr(), ctx.weights[0], ctx.weights[1],
                                    upstream.data_ptr(), dc.data_ptr(), dd.data_ptr()):
            raise RuntimeError(_capi.last_error())
        return dc, dd, None, None, None, None


def l1_loss(color, depth, color_obs, depth_obs, w_color=1.0, w_depth=0.5):
    """w_color * mean|color - color_obs| + w_depth * mean|depth - depth_obs| as one fused reduction, with both gradient
    images written by one launch in the backward (float32 GPU tensors, each image of its observation's shape; the observations
    carry no gradient)."""
    _check_pair("color", color, color_obs, "l1_loss")
    _check_pair("depth", depth, depth_obs, "l1_loss")
    _check_gpu("l1_loss", color, color_obs, depth, depth_obs)
    return _L1Loss.apply(color, depth, color_obs, depth_obs, w_color, w_depth)


def _check_pair(name, a, b, what):
    """ValueError unless `a`, `b` are float32 tensors of one shape (with _check_gpu: all on the host, before any device call)."""
    for t, n in ((a, name), (b, name + "_obs")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {n} must be a tensor, not {type(t).__name__}")
    if a.shape != b.shape:
        raise ValueError(f"{what}: {name} {tuple(a.shape)} and {name}_obs {tuple(b.shape)} differ in shape")
    for t, n in ((a, name), (b, name + "_obs")):
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {n} must be float32, not {t.dtype}")


def _check_gpu(what, *tensors):
    if any(not t.is_cuda for t in tensors):
        raise ValueError(f"{what}: the images must be GPU tensors (there is no CPU fallback)")
    if any(t.device != tensors[0].device for t in tensors):
        raise ValueError(f"{what}: the images are on different devices")


def _image_stack(img, what):
    """(V, C, H, W) of a [C,H,W] or [V,C,H,W] image tensor the SSIM kernels can read."""
    if img.dim() not in (3, 4):
        raise ValueError(f"{what}: images are [C,H,W] or [V,C,H,W], not {tuple(img.shape)}")
    V, (C, H, W) = (img.shape[0] if img.dim() == 4 else 1), img.shape[-3:]
    if min(V, C, H, W) < 1 or V * C > 65535:
        raise ValueError(f"{what}: cannot read a stack of shape {tuple(img.shape)} (empty, or more than 65535 image planes)")
    return V, C, H, W


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class _SsimLoss(torch.autograd.Function):
    """w_l1 mean|img - ref| + w_ssim (1 - SSIM(img, ref)) + w_depth mean|depth - depth_obs| (C ABI: dgr_ssim_loss_forward /
    _backward; csrc/ssim.hip).  `depth` / `depth_obs` may be None.  `want_ssim`: return the mean SSIM the forward leaves in its
    scratch header instead of the loss (with weights (0, -1, 0) the loss is SSIM - 1, whose gradient is SSIM's).  `want_maps`:
    whether a backward will follow (the forward then writes the three derivative maps it needs)."""

    @staticmethod
    def forward(ctx, img, depth, ref, depth_obs, shape, w_l1, w_ssim, w_depth, want_maps, want_ssim):
        from . import _capi
        lib = _capi.load()
        img, ref = img.contiguous(), ref.contiguous()
        if depth is not None:
            depth, depth_obs = depth.contiguous(), depth_obs.contiguous()
        n_depth = depth.numel() if depth is not None else 0
        floats = lib.dgr_ssim_scratch_floats(*shape)
        if not want_maps:  # the inference form: the scratch ends where the derivative maps would begin
            floats -= 3 * img.numel()
        buf = torch.empty((floats + 4,), dtype=torch.float32, device=img.device)
        weights = (float(w_l1), float(w_ssim), float(w_depth))
        with _capi.on_device(img.device):
            if lib.dgr_ssim_loss_forward(_capi.stream_handle(img.device.index), *shape, img.data_ptr(), ref.data_ptr(), n_depth,
                                         _capi.ptr(depth), _capi.ptr(depth_obs), *weights, buf.data_ptr(), int(want_maps),
                                         buf[floats:].data_ptr()):
                raise RuntimeError(_capi.last_error())
        ctx.save_for_backward(img, ref, depth, depth_obs, buf)
        ctx.call = (shape, n_depth, weights)
        return buf[0] if want_ssim else buf[floats]

    @staticmethod
    def backward(ctx, upstream):
        from . import _capi
        lib = _capi.load()
        img, ref, depth, depth_obs, buf = ctx.saved_tensors
        shape, n_depth, weights = ctx.call
        dimg = torch.empty_like(img)
        ddepth = torch.empty_like(depth) if n_depth else None
        upstream = upstream.contiguous()
        with _capi.on_device(img.device):
            if lib.dgr_ssim_loss_backward(_capi.stream_handle(img.device.index), *shape, img.data_ptr(), ref.data_ptr(), n_depth,
                                          _capi.ptr(depth), _capi.ptr(depth_obs), *weights, buf.data_ptr(), upstream.data_ptr(),
                                          dimg.data_ptr(), _capi.ptr(ddepth)):
                raise RuntimeError(_capi.last_error())
        return dimg, ddepth, None, None, None, None, None, None, None, None


def ssim(img, ref):
    """Mean SSIM of `img` against `ref` as 3DGS's `ssim(img1, img2, window_size=11, size_average=True)` computes it (11 x 11
    Gaussian window of sigma 1.5 over the zero-padded images, per channel and per image), as a scalar differentiable with respect
    to `img`: one tiled kernel each way instead of five depthwise convolutions and their elementwise trail.  float32 GPU tensors
    [C,H,W] or [V,C,H,W] of one shape; `ref` carries no gradient."""
    _check_pair("img", img, ref, "ssim")
    shape = _image_stack(img, "ssim")
    _check_gpu("ssim", img, ref)
    return _SsimLoss.apply(img, None, ref, None, shape, 0.0, -1.0, 0.0, _wants_grad(img), True)


def l1_ssim_loss(color, depth, color_obs, depth_obs, w_color=1.0, w_depth=0.5, lambda_dssim=0.2):
    """The mapping loss of 3DGS and the SLAM systems built on it,
        w_color * ((1 - lambda) * mean|color - color_obs| + lambda * (1 - SSIM(color, color_obs))) + w_depth * mean|depth - depth_obs|,
    in at most three launches, with both gradient images written by at most two in the backward, none of them with atomics: the
    same bits on every run, and capturable into a hipGraph.  `color` is [C,H,W] or a stack [V,C,H,W] (then the loss is the mean over
    the stack: multiply the weights by V for a sum over keyframes); `depth` and `depth_obs` may both be None.  float32 GPU tensors;
    the observations carry no gradient.  When no input requires a gradient the forward skips the derivative maps."""
    _check_pair("color", color, color_obs, "l1_ssim_loss")
    shape = _image_stack(color, "l1_ssim_loss")
    if (depth is None) != (depth_obs is None):
        raise ValueError("l1_ssim_loss: depth and depth_obs are given together or both None")
    if depth is not None:
        _check_pair("depth", depth, depth_obs, "l1_ssim_loss")
    _check_gpu("l1_ssim_loss", *(t for t in (color, color_obs, depth, depth_obs) if t is not None))
    if depth is not None and depth.numel() == 0:
        depth = depth_obs = None
    lam = float(lambda_dssim)
    return _SsimLoss.apply(color, depth, color_obs, depth_obs, shape, float(w_color) * (1.0 - lam), float(w_color) * lam,
                           float(w_depth) if depth is not None else 0.0, _wants_grad(color, depth), False)


class MaskedLossStats(_NamedTuple):
    """What `masked_l1_loss(..., return_stats=True)` leaves on the device (views into the call's scratch, nothing read on the host):
    `mask` bool [V,H,W] -- the kept set K; `median` float32 [V] -- the lower median of |depth - depth_obs| over each view's base
    set (0 for an empty one, NaN when rejection is off); `base`, `kept` int32 [V] -- |B_v| and |K_v|.  `median[v:v + 1] * 50` is a
    valid device-tensor `depth_error_min` for `optim.seed_from_frame`."""
    mask: torch.Tensor
    median: torch.Tensor
    base: torch.Tensor
    kept: torch.Tensor


def _round16(n):
    return (n + 15) & ~15


class _MaskedL1Loss(torch.autograd.Function):
    """C ABI: dgr_masked_loss_forward / _backward (csrc/masked_loss.hip).  Returns (loss, scratch): the scratch (uint8, the layout
    include/dgr_hip.h documents) holds the statistics and the mask bytes the backward reads."""

    @staticmethod
    def forward(ctx, color, depth, color_obs, depth_obs, opacity_map, mask, shape, params):
        from . import _capi
        lib = _capi.load()
        color, depth, color_obs, depth_obs = (x.contiguous() for x in (color, depth, color_obs, depth_obs))
        if opacity_map is not None:
            opacity_map = opacity_map.detach().contiguous()
        if mask is not None:
            mask = mask.contiguous()
        V, C, H, W = shape
        scratch = torch.empty((lib.dgr_masked_loss_scratch_bytes(V, H, W),), dtype=torch.uint8, device=color.device)
        loss = scratch[8:12].view(torch.float32)  # (a free word of the stats header)
        with _capi.on_device(color.device):
            if lib.dgr_masked_loss_forward(_capi.stream_handle(color.device.index), V, C, H, W, color.data_ptr(),
                                           color_obs.data_ptr(), depth.data_ptr(), depth_obs.data_ptr(), _capi.ptr(opacity_map),
                                           _capi.ptr(mask), params, scratch.data_ptr(), loss.data_ptr()):
                raise RuntimeError(_capi.last_error())
        ctx.save_for_backward(color, depth, color_obs, depth_obs, opacity_map, mask, scratch)
        ctx.call = (shape, params)
        ctx.mark_non_differentiable(scratch)
        return loss[0], scratch

    @staticmethod
    def backward(ctx, upstream, _dscratch):
        from . import _capi
        lib = _capi.load()
        color, depth, color_obs, depth_obs, opacity_map, mask, scratch = ctx.saved_tensors
        (V, C, H, W), params = ctx.call
        dcolor = torch.empty_like(color) if ctx.needs_input_grad[0] else None
        ddepth = torch.empty_like(depth) if ctx.needs_input_grad[1] else None
        if dcolor is None and ddepth is None:
            return (None,) * 8
        upstream = upstream.contiguous()
        with _capi.on_device(color.device):
            if lib.dgr_masked_loss_backward(_capi.stream_handle(color.device.index), V, C, H, W, color.data_ptr(),
                                            color_obs.data_ptr(), depth.data_ptr(), depth_obs.data_ptr(), _capi.ptr(opacity_map),
                                            _capi.ptr(mask), params, scratch.data_ptr(), upstream.data_ptr(),
                                            _capi.ptr(dcolor), _capi.ptr(ddepth)):
                raise RuntimeError(_capi.last_error())
        return dcolor, ddepth, None, None, None, None, None, None


def masked_l1_loss(color, depth, color_obs, depth_obs, opacity_map=None, mask=None, *, silhouette_threshold=0.99,
                   depth_range=(0.0, float("inf")), outlier_factor=10.0, mask_color=True, w_color=1.0, w_depth=0.5,
                   reduction="sum", return_stats=False):
    """The masked L1 loss of the RGB-D SLAM systems (SplaTAM's `get_loss`, CG-SLAM's tracking), fused: at most six launches
    forward, one backward, no host read, the same bits on every run, capturable into a hipGraph.  Per pixel of every view of the
    stack, in single fp32 operations:
        e = |depth - depth_obs|
        B = lo < depth_obs < hi  and  e finite  [and opacity_map > silhouette_threshold]  [and mask != 0]
        K = B and e <= outlier_factor * median_v         median_v: the exact lower median of e over B of view v (torch.median's,
                                                          by a radix select on the device; 0 for an empty B)
        loss = w_depth * sum_K e / N_d + w_color * sum |color - color_obs| / N_c
    The colour sum runs over the channels and over K, or over every pixel with `mask_color=False` (the mapping form).
    `reduction="sum"` (SplaTAM's): N_d = N_c = 1; `"mean"`: N_d = |K| over the whole stack, N_c = C |K| (or C H W V unmasked),
    the counts read on the device; a zero count gives a zero term.  `outlier_factor=None` turns the rejection off (K = B; no
    median is computed).  The comparison is `<=`: a perfectly fitted frame (median 0) keeps its pixels.  NaN in any image drops
    the pixel.  Gradients go to `color` and `depth` (sign(.) on their set, zero outside); the mask is piecewise constant, so
    `opacity_map`, the observations and the median receive none.
    `color`, `color_obs`: [V,C,H,W] or [C,H,W]; `depth`, `depth_obs`, `opacity_map`: [V,1,H,W], [1,H,W] or [H,W]; `mask`: uint8 or
    bool of the depth's pixel shape.  float32 GPU tensors.
    `return_stats=True`: returns (loss, MaskedLossStats(mask, median, base, kept)), device tensors; `stats.median * 50` (one view)
    is a valid device-tensor `depth_error_min` for `optim.seed_from_frame`."""
    what = "masked_l1_loss"
    _check_pair("color", color, color_obs, what)
    _check_pair("depth", depth, depth_obs, what)
    V, C, H, W = _image_stack(color, what)
    pixels = {(V, 1, H, W)} if color.dim() == 4 else {(1, H, W), (H, W)}
    if tuple(depth.shape) not in pixels:
        raise ValueError(f"{what}: depth {tuple(depth.shape)} does not match color {tuple(color.shape)} "
                         "([V,1,H,W] beside [V,C,H,W]; [1,H,W] or [H,W] beside [C,H,W])")
    if opacity_map is not None:
        if not isinstance(opacity_map, torch.Tensor) or opacity_map.dtype != torch.float32:
            raise ValueError(f"{what}: opacity_map must be a float32 tensor")
        if tuple(opacity_map.shape) not in pixels:
            raise ValueError(f"{what}: opacity_map {tuple(opacity_map.shape)} does not have the depth's shape {tuple(depth.shape)}")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"{what}: mask must be a uint8 or bool tensor")
        if tuple(mask.shape) not in pixels and tuple(mask.shape) != (V, H, W):
            raise ValueError(f"{what}: mask {tuple(mask.shape)} does not have the depth's pixel shape {tuple(depth.shape)}")
    if reduction not in ("sum", "mean"):
        raise ValueError(f"{what}: reduction must be 'sum' or 'mean', not {reduction!r}")
    lo, hi = (float(x) for x in depth_range)
    factor = 0.0 if outlier_factor is None else float(outlier_factor)
    if any(x != x for x in (lo, hi, float(silhouette_threshold), factor)) or factor < 0.0:
        raise ValueError(f"{what}: depth_range, silhouette_threshold and outlier_factor must not be NaN, outlier_factor not negative")
    _check_gpu(what, *(t for t in (color, color_obs, depth, depth_obs, opacity_map, mask) if t is not None))
    from . import _capi
    if _capi.load().dgr_masked_loss_scratch_bytes(V, H, W) == 0:
        raise ValueError(f"{what}: cannot read a stack of shape {tuple(color.shape)} (more than 2^30 pixels per view)")
    params = _capi.MaskedLossParams(lo, hi, float(silhouette_threshold), factor, int(outlier_factor is not None), int(bool(mask_color)),
                                    _capi.MASKED_LOSS_MEAN if reduction == "mean" else _capi.MASKED_LOSS_SUM, float(w_color),
                                    float(w_depth))
    if mask is not None and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    loss, scratch = _MaskedL1Loss.apply(color, depth, color_obs, depth_obs, opacity_map, mask, (V, C, H, W), params)
    if not return_stats:
        return loss
    pad, n = _round16(4 * V), V * H * W  # (the scratch layout of include/dgr_hip.h)
    end = scratch.numel() - _round16(n)
    return loss, MaskedLossStats(scratch[end:end + n].view(torch.bool).view(V, H, W),
                                 scratch[64:64 + 4 * V].view(torch.float32), scratch[64 + pad:64 + pad + 4 * V].view(torch.int32),
                                 scratch[64 + 2 * pad:64 + 2 * pad + 4 * V].view(torch.int32))


class KeyframeOverlap(_NamedTuple):
    """What `keyframe_overlap` leaves on the device: `score` float32 [K] = visible / valid (0 for a frame without a valid pixel);
    `inside`, `visible` int32 [K]; `valid` int32 [1]; `flags` uint8 [K, S] (bit 0 valid, bit 1 inside, bit 2 visible) or None."""
    score: torch.Tensor
    inside: torch.Tensor
    visible: torch.Tensor
    valid: torch.Tensor
    flags: torch.Tensor


def keyframe_overlap(depth_obs, viewmatrix, keyframe_viewmatrices, fx, fy, cx, cy, *, stride=16, edge=20.0, near=0.0,
                     depth_range=(0.0, float("inf")), keyframe_depths=None, depth_tolerance=0.05, return_flags=False):
    """Overlap of the current frame with K stored keyframes, the score CG-SLAM, SplaTAM (`keyframe_selection_overlap`) and the
    NICE-SLAM family rank their mapping window by, and MonoGS's keyframe test at K = 1: every `stride`-th pixel of every
    `stride`-th row of `depth_obs` (the candidate grid of `optim.seed_from_frame`, S of them; no random sampling) with a depth in
    `depth_range` (exclusive) is unprojected, taken into every keyframe and counted where it lands more than `edge` pixels inside
    the image in front of `near`; `score[k]` is that count over the number of valid candidates.  With `keyframe_depths` [K,H,W] a
    point also has to agree with keyframe k's depth at the pixel it lands on, to `depth_tolerance` (relative), to count.
    One call, at most two launches, nothing read on the host, the same bits on every run, capturable into a hipGraph
    (include/dgr_hip.h: dgr_keyframe_overlap).  `depth_obs`: [H,W] or [1,H,W]; `viewmatrix` [4,4] and `keyframe_viewmatrices`
    [K,4,4] hold W2C^T, the rasterizer's convention; float32 GPU tensors.  The keyframes share the frame's size and intrinsics
    (pixel (x, y) at depth d is ((x - cx) / fx d, (y - cy) / fy d, d)).  K = 0 returns empty tensors.
    Returns KeyframeOverlap(score, inside, visible, valid, flags); `flags` is None unless `return_flags`."""
    what = "keyframe_overlap"
    named = [("depth_obs", depth_obs), ("viewmatrix", viewmatrix), ("keyframe_viewmatrices", keyframe_viewmatrices)]
    if keyframe_depths is not None:
        named.append(("keyframe_depths", keyframe_depths))
    for n, t in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {n} must be a tensor, not {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {n} must be float32, not {t.dtype}")
    if depth_obs.dim() == 3 and depth_obs.shape[0] == 1:
        depth_obs = depth_obs[0]
    if depth_obs.dim() != 2 or depth_obs.numel() == 0:
        raise ValueError(f"{what}: depth_obs is [H,W] or [1,H,W], not {tuple(depth_obs.shape)}")
    H, W = depth_obs.shape
    if tuple(viewmatrix.shape) != (4, 4):
        raise ValueError(f"{what}: viewmatrix is [4,4] (W2C^T), not {tuple(viewmatrix.shape)}")
    if keyframe_viewmatrices.dim() != 3 or tuple(keyframe_viewmatrices.shape[1:]) != (4, 4):
        raise ValueError(f"{what}: keyframe_viewmatrices is [K,4,4], not {tuple(keyframe_viewmatrices.shape)}")
    K = keyframe_viewmatrices.shape[0]
    if keyframe_depths is not None:
        if keyframe_depths.dim() == 4 and keyframe_depths.shape[1] == 1:
            keyframe_depths = keyframe_depths[:, 0]
        if tuple(keyframe_depths.shape) != (K, H, W):
            raise ValueError(f"{what}: keyframe_depths {tuple(keyframe_depths.shape)} is not [K,H,W] = {(K, H, W)}")
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"{what}: stride must be positive, not {stride}")
    lo, hi = (float(x) for x in depth_range)
    scalars = dict(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), edge=float(edge), near=float(near),
                   depth_tolerance=float(depth_tolerance))
    for n, v in list(scalars.items()) + [("depth_range", lo), ("depth_range", hi)]:
        if v != v:
            raise ValueError(f"{what}: {n} must not be NaN")
    for n in ("fx", "fy"):
        if not 0.0 < scalars[n] < float("inf"):
            raise ValueError(f"{what}: {n} must be finite and positive, not {scalars[n]}")
    for n in ("edge", "depth_tolerance"):
        if scalars[n] < 0.0:
            raise ValueError(f"{what}: {n} must not be negative, not {scalars[n]}")
    _check_gpu(what, *(t for _, t in named))
    dev = depth_obs.device
    S = -(-W // stride) * -(-H // stride)
    buf = torch.empty((3 * K + 1,), dtype=torch.int32, device=dev)
    flags = torch.empty((K, S), dtype=torch.uint8, device=dev) if return_flags else None
    out = KeyframeOverlap(buf[2 * K:3 * K].view(torch.float32), buf[:K], buf[K:2 * K], buf[3 * K:], flags)
    if K == 0:
        out.valid.zero_()
        return out
    from . import _capi
    lib = _capi.load()
    nbytes = lib.dgr_keyframe_overlap_scratch_bytes(W, H, stride, K)
    if nbytes == 0:
        raise ValueError(f"{what}: cannot take {K} keyframes of {S} candidates each (at most 2^20 keyframes, K * S below 2^31)")
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    depth_obs, viewmatrix, keyframe_viewmatrices = (t.detach().contiguous() for t in (depth_obs, viewmatrix, keyframe_viewmatrices))
    if keyframe_depths is not None:
        keyframe_depths = keyframe_depths.detach().contiguous()
    params = _capi.KeyframeOverlapParams(scalars["fx"], scalars["fy"], scalars["cx"], scalars["cy"], lo, hi, scalars["edge"],
                                         scalars["near"], scalars["depth_tolerance"], stride)
    with _capi.on_device(dev):
        if lib.dgr_keyframe_overlap(_capi.stream_handle(dev.index), W, H, depth_obs.data_ptr(), viewmatrix.data_ptr(), K,
                                    keyframe_viewmatrices.data_ptr(), _capi.ptr(keyframe_depths), params, scratch.data_ptr(),
                                    out.inside.data_ptr(), out.visible.data_ptr(), out.valid.data_ptr(), out.score.data_ptr(),
                                    _capi.ptr(flags)):
            raise RuntimeError(_capi.last_error())
    return out


def select_keyframes(score, k, *, min_overlap=0.0, mode="top", generator=None):
    """The mapping window from `keyframe_overlap`'s scores: up to `k` of the keyframes with `score > min_overlap`.
    `mode="top"`: the best scores first, ties to the lower index; `mode="random"`: a uniform shuffle of the overlapping keyframes
    (SplaTAM's choice), drawn from `generator` (a generator of the scores' device, or None for the default one).
    Returns (indices int64 [k], count): both on the device, entries past `count` (a 0-dim int64 tensor) are -1.  A few torch
    operations, none of which reads the device: the caller's one read of the k indices, once per mapping phase, is the only host
    synchronisation of the whole selection step."""
    if not isinstance(score, torch.Tensor) or score.dim() != 1 or not score.is_floating_point():
        raise ValueError("select_keyframes: score must be a 1-D floating-point tensor")
    k = int(k)
    if k < 0:
        raise ValueError(f"select_keyframes: k must not be negative, not {k}")
    if mode not in ("top", "random"):
        raise ValueError(f"select_keyframes: mode must be 'top' or 'random', not {mode!r}")
    ok = score > min_overlap
    keys = score if mode == "top" else torch.rand(score.shape, dtype=score.dtype, device=score.device, generator=generator)
    # (a stable descending sort: equal keys keep their index order, which topk does not promise)
    order = torch.sort(torch.where(ok, keys, torch.full_like(keys, float("-inf"))), descending=True, stable=True).indices[:k]
    count = ok.sum().clamp(max=k)
    indices = torch.full((k,), -1, dtype=torch.int64, device=score.device)
    n = order.numel()
    indices[:n] = torch.where(torch.arange(n, device=score.device) < count, order, indices[:n])
    return indices, count


def _get(obj, name, default=None):
    v = getattr(obj, name, default)
    return v() if callable(v) and not isinstance(v, torch.Tensor) else v


def _matmul_fixed_order(a, b):
    """a @ b for [..., n, 4] @ [4, m] with the four products of every entry added in index order by elementwise kernels
    (see _campos: the result must not depend on whether `a` is one matrix or a slice of a stack).  Four launches."""
    r = a[..., :, 0:1] * b[0]
    for k in (1, 2, 3):
        r = torch.addcmul(r, a[..., :, k:k + 1], b[k])
    return r


def _campos(vm):
    """Camera centre -(R^T t) from viewmatrix = W2C^T ([4,4] or [V,4,4]), with the three products added in a fixed order
    by elementwise kernels: a `sum()` reduction picks its summation order from the tensor's layout and alignment, so the
    same pose gave cameras one ulp apart as a [4,4] tensor and as a slice of a [V,4,4] one.  Three launches."""
    nt = -vm[..., 3, 0:3]
    r = vm[..., :3, 0] * nt[..., 0:1]
    r = torch.addcmul(r, vm[..., :3, 1], nt[..., 1:2])
    return torch.addcmul(r, vm[..., :3, 2], nt[..., 2:3]).contiguous()


_VIEWS_CACHE = {}   # render_views: camera tensors of the last few keyframe batches (see there)
_VIEW_CACHE = {}    # render: the same for single fixed poses
_ZERO_POINTS = {}  # (device, P) -> a [P, 3] zero tensor for calls whose screen-space gradient nobody reads (tracking)


def render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None, viewmatrix=None, fov=None,
           HW=None, gt_depth=None, track_off=False, map_off=False, variant="light", pose_tensors=None, absgrad=False,
           complete_pose=False, silhouette_grad=False):
    """CG-SLAM's `render()` (reference README.md:33,71).

    `pc`: anything with the 3DGS GaussianModel accessors `get_xyz`, `get_opacity`, `get_scaling`, `get_rotation`,
    `get_features` ([P, M, 3]) and `active_sh_degree`.  `viewmatrix` is W2C^T (differentiable for tracking); `fov` the
    two half-angle tangents; `HW` = (H, W).  `viewpoint_camera` may carry `projection_matrix` (Proj^T), `znear`, `zfar`;
    without it a symmetric frustum with znear 0.01 / zfar 100 is used.  `pipe.debug` is honoured.
    `pose_tensors` = what `pose_to_camera(q, t, ...)` returned for this `viewmatrix` -- (viewmatrix, projmatrix, perspec_matrix,
    campos): the projection, the full projection and the camera centre are then taken from there instead of being formed again
    from `viewmatrix` with a dozen small torch kernels (a 640x480 tracking iteration is bound by exactly those).
    Returns the reference's dict (light: render, depth, depth_median, opacity_map, depth_var, gau_uncertainty,
    num_related_pixels; full: render, depth, opacity_map) plus the 3DGS bookkeeping entries viewspace_points,
    visibility_filter, radii.  `absgrad=True` (AbsGS densification, a mapping render) adds `viewspace_points_abs`, a zero leaf
    shaped like `viewspace_points` whose `.grad` receives the absolute screen-space gradient (GaussianRasterizer.forward's
    `means2D_abs`): feed it to `optim.add_densification_stats` in place of `viewspace_points.grad`.
    `complete_pose=True`: the backward returns the complete pose gradient (library option "pose_grad" = 1: the view-matrix
    counterpart of the Gaussians' dL_dmeans3D, with the 2D-covariance, colour and depth terms the reference leaves out) instead
    of the reference's; the forward runs under it and its backward follows.  The campos used is the one formed from
    `viewmatrix` here (or `pose_tensors`), which is what makes the colour term exact.
    `silhouette_grad=True`: `res["opacity_map"]` carries the exact gradient of the silhouette sum alpha T in both variants
    (library option "silhouette_grad" = 1): a mask or opacity loss on it trains the Gaussians and the pose, instead of being
    dropped (light) or taken as the full variant's depth variance.  The full variant's pose gradient receives it only
    together with `complete_pose=True` (include/dgr_hip.h)."""
    if viewmatrix is None or fov is None or HW is None:
        raise ValueError("render() needs viewmatrix=W2C^T, fov=(tanfovx, tanfovy) and HW=(H, W)")
    mod = _light if variant == "light" else _full
    H, W = int(HW[0]), int(HW[1])
    tanfovx, tanfovy = float(fov[0]), float(fov[1])
    dev = viewmatrix.device
    znear = float(_get(viewpoint_camera, "znear", 0.01)) if viewpoint_camera is not None else 0.01
    zfar = float(_get(viewpoint_camera, "zfar", 100.0)) if viewpoint_camera is not None else 100.0
    if pose_tensors is not None:
        vm = viewmatrix.detach()
        projmatrix, perspec, campos = pose_tensors[1].detach(), pose_tensors[2], pose_tensors[3].detach()
    else:
        perspec_src = _get(viewpoint_camera, "projection_matrix") if viewpoint_camera is not None else None
        # a fixed keyframe pose (mapping) is rendered again and again: its derived tensors are kept while `viewmatrix` is the
        # same object at the same version (render_views does the same for a batch); a pose under optimisation is a new
        # tensor every iteration and is not kept; never while a hipGraph is being recorded (a replay re-derives them)
        keep = (not viewmatrix.requires_grad and viewmatrix.is_cuda and not torch.cuda.is_current_stream_capturing())
        key = (id(viewmatrix), viewmatrix._version, id(perspec_src), getattr(perspec_src, "_version", 0), tanfovx, tanfovy,
               znear, zfar) if keep else None
        hit = _VIEW_CACHE.get(key) if keep else None
        if hit is None:
            with torch.no_grad():
                perspec = perspec_src
                if perspec is None:
                    perspec = _perspec_cached(tanfovx, tanfovy, znear, zfar, dev)
                perspec = perspec.to(dev, torch.float32)
                vm = viewmatrix.detach()
                projmatrix = _matmul_fixed_order(vm, perspec).contiguous()
                campos = _campos(vm)
            # (the sources too: ids are unique among live objects; the stamp: see _Stamp)
            hit = (perspec, vm, projmatrix, campos, viewmatrix, perspec_src, _stamp(dev) if keep else None)
            if keep:
                if len(_VIEW_CACHE) >= 16:
                    _VIEW_CACHE.pop(next(iter(_VIEW_CACHE)))
                _VIEW_CACHE[key] = hit
        elif hit[6] is not None:
            hit[6].order(dev)
        perspec, vm, projmatrix, campos = hit[:4]

    means3D = pc.get_xyz
    # 3DGS keeps a zero tensor whose .grad receives the screen-space gradient (densification statistics).  A tracking
    # step (map_off, or a map that carries no gradients) has no use for it, and without it the backward can skip every
    # per-Gaussian gradient row (dgr_amd.light: need_gaussian_grads).
    shs_or_colors = override_color if override_color is not None else pc.get_features
    opacity, scaling, rotation = pc.get_opacity, pc.get_scaling, pc.get_rotation
    mapping = (variant != "light" or not map_off) and any(
        t.requires_grad for t in (means3D, shs_or_colors, opacity, scaling, rotation))
    if mapping:
        screenspace_points = torch.zeros_like(means3D, requires_grad=True)
    else:  # never read, never written: one shared zero tensor per size instead of a fill per call
        key = (means3D.device, means3D.shape[0])
        zp = _ZERO_POINTS.get(key)
        if zp is None:
            if len(_ZERO_POINTS) > 16:
                _ZERO_POINTS.clear()
            z = torch.zeros_like(means3D)
            zp = (z, _stamp(z.device))
            if not (z.is_cuda and torch.cuda.is_current_stream_capturing()):
                _ZERO_POINTS[key] = zp
        elif zp[1] is not None:
            zp[1].order(zp[0].device)
        screenspace_points = zp[0]
    debug = bool(getattr(pipe, "debug", False)) if pipe is not None else False
    common = dict(image_height=H, image_width=W, tanfovx=tanfovx, tanfovy=tanfovy, bg=bg_color,
                  scale_modifier=scaling_modifier, viewmatrix=vm, projmatrix=projmatrix,
                  sh_degree=int(pc.active_sh_degree), campos=campos, prefiltered=False)
    if variant == "light":
        settings = mod.GaussianRasterizationSettings(**common, debug=debug, perspec_matrix=perspec, track_off=track_off,
                                                     map_off=map_off)
    else:
        settings = mod.GaussianRasterizationSettings(**common, perspec_matrix=perspec)
    rasterizer = mod.GaussianRasterizer(raster_settings=settings)
    shs, colors = (None, override_color) if override_color is not None else (shs_or_colors, None)
    with _pose_mode(complete_pose, silhouette_grad):
        if absgrad:
            abs_points = torch.zeros_like(means3D, requires_grad=True)
            out = rasterizer(means3D=means3D, means2D=screenspace_points, opacities=opacity, shs=shs,
                             colors_precomp=colors, scales=scaling, rotations=rotation, cov3D_precomp=None,
                             viewmatrix=viewmatrix, gt_depth=gt_depth, means2D_abs=abs_points)
        else:
            out = rasterizer(means3D=means3D, means2D=screenspace_points, opacities=opacity, shs=shs,
                             colors_precomp=colors, scales=scaling, rotations=rotation, cov3D_precomp=None,
                             viewmatrix=viewmatrix, gt_depth=gt_depth)
    if variant == "light":
        color, radii, depth, depth_median, depth_var, opacity_map, gau_uncertainty, gau_related_pixels = out
        res = {"render": color, "depth": depth, "depth_median": depth_median, "opacity_map": opacity_map,
               "depth_var": depth_var, "gau_uncertainty": gau_uncertainty, "num_related_pixels": gau_related_pixels}
    else:
        color, radii, depth, uncertainty = out
        res = {"render": color, "depth": depth, "opacity_map": uncertainty}
    res.update(viewspace_points=screenspace_points, visibility_filter=radii > 0, radii=radii)
    if absgrad:
        res["viewspace_points_abs"] = abs_points
    return res


def _pose_mode(complete_pose, silhouette_grad=False):
    """The block's rasterizer calls under pose_grad = 1 and / or silhouette_grad = 1 (their backwards follow through the
    forward's options snapshot)."""
    modes = dict(pose_grad=1) if complete_pose else {}
    if silhouette_grad:
        modes["silhouette_grad"] = 1
    if not modes:
        return _contextlib.nullcontext()
    from . import _capi
    return _capi.thread_options(**modes)


def render_views(cameras, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None, track_off=False, map_off=False,
                 variant="light", absgrad=False, complete_pose=False, silhouette_grad=False):
    """`render()` for the V cameras of a keyframe batch in ONE call of the batched entry points (`dgr_amd.batch`, SURVEY.md
    s8(f) item 2; `variant="full"`: `dgr_amd.batch_full`): the cameras share `fov` and `HW` (one sensor, V poses), every
    per-view entry of `render()`'s dict comes back with a leading view dimension, and one backward through it yields the
    Gaussians' gradients already summed over the views, the pose gradient per `viewmatrix` and `viewspace_points.grad`
    ([V,P,3]) per view.  `cameras`: sequence of dicts with `viewmatrix` (W2C^T), `fov`, `HW`, `gt_depth` and optionally
    `viewpoint_camera`.  The full variant has no track_off / map_off.  `absgrad=True`: as in `render()`, with
    `viewspace_points_abs` [V,P,3].  `complete_pose=True`: every view's pose gradient is the complete one, as in `render()`.
    `silhouette_grad=True`: every view's `opacity_map` carries the exact silhouette gradient, as in `render()`."""
    from . import batch as _batch
    if variant not in ("light", "full"):
        raise ValueError(f"unknown variant {variant!r}")
    if variant == "full" and (track_off or map_off):
        raise ValueError("the full variant has no track_off / map_off")
    cameras = list(cameras)
    if not 1 <= len(cameras) <= _batch.MAX_VIEWS:
        raise ValueError(f"1 .. {_batch.MAX_VIEWS} cameras per call")
    c0 = cameras[0]
    H, W = int(c0["HW"][0]), int(c0["HW"][1])
    tanfovx, tanfovy = float(c0["fov"][0]), float(c0["fov"][1])
    for c in cameras[1:]:
        if (int(c["HW"][0]), int(c["HW"][1])) != (H, W) or (float(c["fov"][0]), float(c["fov"][1])) != (tanfovx, tanfovy):
            raise ValueError("the cameras of a batch share fov and HW")
    cam0 = c0.get("viewpoint_camera")
    znear = float(_get(cam0, "znear", 0.01)) if cam0 is not None else 0.01
    zfar = float(_get(cam0, "zfar", 100.0)) if cam0 is not None else 100.0
    gts = [c.get("gt_depth") for c in cameras]
    if any(g is None for g in gts):
        raise ValueError(f"the {variant} variant's batch needs gt_depth for every camera")
    vms = [c["viewmatrix"] for c in cameras]
    perspec_src = _get(cam0, "projection_matrix") if cam0 is not None else None
    # A mapping loop renders the same keyframes iteration after iteration: the camera tensors derived from the poses (a dozen
    # small launches) are kept while the tensors they were made from are the same objects at the same version -- an optimiser
    # step on a pose, or a new depth image, changes the key.
    key = (H, W, tanfovx, tanfovy, znear, zfar, id(perspec_src), getattr(perspec_src, "_version", 0),
           tuple((id(v), v._version, id(g), g._version) for v, g in zip(vms, gts)))
    # (never while a hipGraph is being recorded: a replay must re-derive the cameras from whatever the poses hold then)
    capturing = vms[0].is_cuda and torch.cuda.is_current_stream_capturing()
    hit = None if capturing else _VIEWS_CACHE.get(key)
    if hit is None:
        dev = vms[0].device
        with torch.no_grad():
            perspec = perspec_src
            if perspec is None:
                perspec = _perspec_cached(tanfovx, tanfovy, znear, zfar, dev)
            perspec = perspec.to(dev, torch.float32)
            vm = torch.stack([v.detach() for v in vms])
            # (the operations of render(), in a fixed order: the cameras -- hence the images -- are those of the one-view
            #  path bit for bit)
            projmatrices = _matmul_fixed_order(vm, perspec).contiguous()
            campos = _campos(vm)
            gt_depths = torch.stack([g.reshape(H, W) for g in gts])
        # (the sources are held too: an id() is only unique among live objects)
        hit = (perspec, vm, projmatrices, campos, gt_depths, list(vms), list(gts), perspec_src, None if capturing else _stamp(dev))
        if not capturing:
            if len(_VIEWS_CACHE) >= 4:
                _VIEWS_CACHE.pop(next(iter(_VIEWS_CACHE)))
            _VIEWS_CACHE[key] = hit
    elif hit[8] is not None:
        hit[8].order(hit[1].device)
    perspec, vm, projmatrices, campos, gt_depths = hit[:5]
    dev = vm.device
    # (differentiable where a pose is a leaf: every pose keeps its gradient)
    viewmatrices = torch.stack(vms) if any(v.requires_grad for v in vms) else vm
    means3D = pc.get_xyz
    shs_or_colors = override_color if override_color is not None else pc.get_features
    opacity, scaling, rotation = pc.get_opacity, pc.get_scaling, pc.get_rotation
    mapping = not map_off and any(t.requires_grad for t in (means3D, shs_or_colors, opacity, scaling, rotation))
    screenspace_points = torch.zeros((len(cameras),) + tuple(means3D.shape), dtype=means3D.dtype, device=dev, requires_grad=mapping)
    # (absgrad: a [V,P,3] leaf of its own; None leaves the calls below as they are)
    abs_points = torch.zeros_like(screenspace_points, requires_grad=True) if absgrad else None
    debug = bool(getattr(pipe, "debug", False)) if pipe is not None else False
    settings = _batch.BatchRasterizationSettings(
        image_height=H, image_width=W, tanfovx=tanfovx, tanfovy=tanfovy, bg=bg_color, scale_modifier=scaling_modifier,
        viewmatrices=vm, projmatrices=projmatrices, sh_degree=int(pc.active_sh_degree), campos=campos, prefiltered=False,
        debug=debug, perspec_matrix=perspec, track_off=track_off, map_off=map_off)
    shs, colors = (None, override_color) if override_color is not None else (shs_or_colors, None)
    if variant == "full":
        from .batch_full import GaussianRasterizerBatchFull
        with _pose_mode(complete_pose, silhouette_grad):
            color, radii, depth, uncertainty = GaussianRasterizerBatchFull(settings)(
                means3D, screenspace_points, opacity, shs=shs, colors_precomp=colors, scales=scaling, rotations=rotation,
                viewmatrices=viewmatrices, gt_depths=gt_depths, means2D_abs=abs_points)
        res = {"render": color, "depth": depth, "opacity_map": uncertainty, "viewspace_points": screenspace_points,
               "visibility_filter": radii > 0, "radii": radii}
        if absgrad:
            res["viewspace_points_abs"] = abs_points
        return res
    with _pose_mode(complete_pose, silhouette_grad):
        color, radii, depth, depth_median, depth_var, opacity_map, gau_uncertainty, gau_related_pixels = \
            _batch.GaussianRasterizerBatch(settings)(means3D, screenspace_points, opacity, shs=shs, colors_precomp=colors,
                                                     scales=scaling, rotations=rotation, viewmatrices=viewmatrices,
                                                     gt_depths=gt_depths, means2D_abs=abs_points)
    res = {"render": color, "depth": depth, "depth_median": depth_median, "opacity_map": opacity_map, "depth_var": depth_var,
           "gau_uncertainty": gau_uncertainty, "num_related_pixels": gau_related_pixels,
           "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii}
    if absgrad:
        res["viewspace_points_abs"] = abs_points
    return res


class _ViewOf(_Mapping):
    """View k of `render_views`' dict: entry n is `out[n][k]`, sliced when it is first asked for (a loss reads two or three
    of the ten; every slice is an autograd node and a launch-free but not cost-free call) -- except `viewspace_points` (and
    `viewspace_points_abs`, with absgrad), which stays the whole [V,P,3] tensor: one backward fills every view's slice."""
    _NAMES = ("render", "depth", "depth_median", "opacity_map", "depth_var", "gau_uncertainty", "num_related_pixels",
              "visibility_filter", "radii", "viewspace_points")
    _FULL_NAMES = ("render", "depth", "opacity_map", "visibility_filter", "radii", "viewspace_points")  # (variant="full")

    def __init__(self, out, k):
        self._out, self._k, self._got = out, k, {}
        self._names = self._NAMES if "depth_median" in out else self._FULL_NAMES
        if "viewspace_points_abs" in out:
            self._names = self._names + ("viewspace_points_abs",)

    def __getitem__(self, n):
        v = self._got.get(n)
        if v is None:
            if n not in self._names:
                raise KeyError(n)
            whole = n == "viewspace_points" or n == "viewspace_points_abs"
            v = self._got[n] = self._out[n] if whole else self._out[n][self._k]
        return v

    def __iter__(self):
        return iter(self._names)

    def __len__(self):
        return len(self._names)


def render_batch_fused(cameras, pc, pipe, bg_color, loss_fn, batch_loss_fn=None, absgrad=False, silhouette_grad=False,
                       **render_kwargs):
    """`render_batch` through ONE batched forward and ONE batched backward (`render_views`): `loss_fn(out_k, k)` sees the
    dict of view k (slices of the batched outputs), the losses are summed and back-propagated once.  Same gradients as
    `render_batch` -- the sum over the keyframes in the Gaussians' `.grad`, one pose gradient per `viewmatrix` -- without V - 1
    accumulation passes over the dense gradient rows and with the camera-independent per-Gaussian work done once.
    `batch_loss_fn(out)`, if given, replaces the V calls of `loss_fn`: it sees the batched dict and returns the SUM of the
    views' losses as one scalar (then the returned list holds that one value).  `variant="full"` (a render_kwargs entry) renders
    through the full variant's batch.  `absgrad=True`: the returned dict carries `viewspace_points_abs` (render_views).
    `complete_pose=True` (a render_kwargs entry) passes through to `render_views`: complete pose gradients.
    `silhouette_grad=True`: the exact silhouette gradient of every view's `opacity_map` (render_views)."""
    if silhouette_grad:
        render_kwargs["silhouette_grad"] = True
    if absgrad:
        render_kwargs["absgrad"] = True
    out = render_views(cameras, pc, pipe, bg_color, **render_kwargs)
    if batch_loss_fn is not None:
        # ONE loss over the stacked outputs ([V,3,H,W], [V,1,H,W], ...): no per-view slice in the graph -- each is a node whose
        # backward zero-fills a tensor of the whole stack's size -- and one reduction instead of V
        total = batch_loss_fn(out)
        total.backward()
        return [total.detach()], out
    losses = [loss_fn(_ViewOf(out, k), k) for k in range(out["render"].size(0))]
    torch.stack(losses).sum().backward()
    return [l_.detach() for l_ in losses], out


def render_batch(cameras, pc, pipe, bg_color, loss_fn, views_in_flight=3, absgrad=False, silhouette_grad=False,
                 **render_kwargs):
    """One mapping step over a batch of keyframes: every camera is rendered, `loss_fn(out, k)`
    is evaluated on its output dict and back-propagated, each view's forward + loss + backward on its own HIP stream
    (`dgr_amd.multiview.ViewStreams`) so that the views overlap on the GPU; gradients accumulate in the `.grad` of the
    Gaussian parameters as usual.  Accumulation into a shared `.grad` from several streams needs an explicit order
    (PyTorch gives none): every view's backward waits for the end of the previous view (`views.before_backward()`), its
    forward and loss still overlap the previous view's backward.  `cameras`: sequence of dicts with `viewmatrix`
    (W2C^T), `fov`, `HW` and optionally `gt_depth`, `viewpoint_camera`.  Returns the list of detached loss values
    (device tensors); the caller's stream is ordered after all views on return.  `absgrad=True`: every view's dict carries
    `viewspace_points_abs` (render()), which `loss_fn` may keep for the densification statistics.  `silhouette_grad=True`: every
    view's `opacity_map` carries the exact silhouette gradient (render())."""
    if absgrad:
        render_kwargs["absgrad"] = True
    if silhouette_grad:
        render_kwargs["silhouette_grad"] = True
    from .multiview import ViewStreams
    cameras = list(cameras)
    if not cameras:
        return []
    views = ViewStreams(min(max(1, views_in_flight), len(cameras)), cameras[0]["viewmatrix"].device)

    def one_view(k, cam):  # (a function: no autograd graph of one view is kept alive into the next)
        out = render(cam.get("viewpoint_camera"), pc, pipe, bg_color, viewmatrix=cam["viewmatrix"], fov=cam["fov"],
                     HW=cam["HW"], gt_depth=cam.get("gt_depth"), **render_kwargs)
        loss = loss_fn(out, k)
        views.before_backward()
        loss.backward()
        return loss.detach()

    losses = []
    for k, cam in enumerate(cameras):
        with views.next():
            losses.append(one_view(k, cam))
    views.join()
    return losses
