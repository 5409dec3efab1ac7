"""Per-Gaussian contribution statistics of a rendered view (C ABI: dgr_contribution_stats): which Gaussians the pixels of a
finished forward actually blended, and how much -- the signal MonoGS (`n_touched`), RTG-SLAM, LightGaussian and Mini-Splatting
key their map hygiene on, which `radii > 0` (a frustum and rectangle test) and `gau_related_pixels` (median pixels, light
only) do not give."""
from typing import NamedTuple as _NamedTuple

import torch

from . import _capi
from ._frontend import _EMPTY

_Q32 = 2.0 ** -32


class ContributionStats(_NamedTuple):
    """One view's statistics, on the device: `n_touched` int32 [P] = blended (pixel, Gaussian) pairs; `max_weight` float32 [P] =
    largest blend weight alpha T (0 if none); `sum_weight` int64 [P] = sum of floor(alpha T 2^32) (Q32 fixed point: an integer
    sum has the same bits on every run); `counts` int32 [4] = {Gaussians touched, Gaussians observed (min_pixels / weight_min),
    1 if the frame's binning had overflowed, 0}."""
    n_touched: torch.Tensor
    max_weight: torch.Tensor
    sum_weight: torch.Tensor
    counts: torch.Tensor

    def sum_weight_float(self):
        """the accumulated blend weight per Gaussian, float64 [P]"""
        return self.sum_weight.to(torch.float64) * _Q32


class ContributionAccumulator:
    """The running statistics of a map of P Gaussians over the views folded into it (`into=` of `contribution_stats` and
    `render_contributions`): `touched_total` int64, `max_weight_total` float32, `sum_weight_total` int64 (Q32), `views` int32 =
    views that observed the Gaussian, `last_seen` int32 = frame_id of the last one (-1: never), all [P] on `device`."""

    def __init__(self, P, device):
        P = int(P)
        if P < 0:
            raise ValueError(f"ContributionAccumulator: P must not be negative, not {P}")
        self.P, self.device = P, torch.device(device)
        self.touched_total = torch.zeros((P,), dtype=torch.int64, device=self.device)
        self.max_weight_total = torch.zeros((P,), dtype=torch.float32, device=self.device)
        self.sum_weight_total = torch.zeros((P,), dtype=torch.int64, device=self.device)
        self.views = torch.zeros((P,), dtype=torch.int32, device=self.device)
        self.last_seen = torch.full((P,), -1, dtype=torch.int32, device=self.device)

    def tensors(self):
        return (self.touched_total, self.max_weight_total, self.sum_weight_total, self.views, self.last_seen)

    def reset(self):
        """back to "no view folded" (in place: a captured graph keeps pointing at the same tensors)"""
        for t in self.tensors()[:4]:
            t.zero_()
        self.last_seen.fill_(-1)

    def observed(self, min_views=1):
        """device mask [P]: the Gaussians at least `min_views` of the folded views observed"""
        return self.views >= int(min_views)

    def sum_weight_float(self):
        return self.sum_weight_total.to(torch.float64) * _Q32


def contribution_stats(geomBuffer, binningBuffer, imageBuffer, P, H, W, R, *, into=None, min_pixels=1, weight_min=0.0, frame_id=0):
    """The statistics of the view whose forward left the three state buffers -- what the reference-shaped
    `_C.rasterize_gaussians` of either variant returns as geomBuffer, binningBuffer, imgBuffer, with its num_rendered as `R` -- for
    a map of `P` Gaussians rendered at `H` x `W`.  A pair (pixel, list entry) counts iff the forward blended it; its weight is the
    forward's alpha T, bit for bit (include/dgr_hip.h: dgr_contribution_stats).  Call it under the forward's alpha_mode, on the
    forward's stream, before another forward reuses the buffers.
    `into`: a ContributionAccumulator that receives the view; a Gaussian is OBSERVED by the view when n_touched >= `min_pixels` and
    max_weight >= `weight_min`, and then gets views += 1 and last_seen = `frame_id`.  A frame whose binning overflowed is not folded.
    At most three launches, nothing read on the host, the same bits on every run, capturable into a hipGraph.
    Returns ContributionStats."""
    what = "contribution_stats"
    bufs = (("geomBuffer", geomBuffer), ("binningBuffer", binningBuffer), ("imageBuffer", imageBuffer))
    for n, t in bufs:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {n} must be a tensor, not {type(t).__name__}")
        if t.dtype != torch.uint8 or t.dim() != 1:
            raise ValueError(f"{what}: {n} must be a 1-D uint8 tensor (a forward's state buffer), not {t.dtype} {tuple(t.shape)}")
    P, H, W, R, min_pixels, frame_id, weight_min = int(P), int(H), int(W), int(R), int(min_pixels), int(frame_id), float(weight_min)
    if P < 0 or P >= 1 << 28:
        raise ValueError(f"{what}: P must be 0 .. 2^28 - 1, not {P}")
    if H <= 0 or W <= 0:
        raise ValueError(f"{what}: H and W must be positive, not {(H, W)}")
    if R < 0:
        raise ValueError(f"{what}: R must not be negative, not {R}")
    if min_pixels < 0:
        raise ValueError(f"{what}: min_pixels must not be negative, not {min_pixels}")
    if weight_min != weight_min:
        raise ValueError(f"{what}: weight_min must not be NaN")
    if weight_min < 0.0:
        raise ValueError(f"{what}: weight_min must not be negative, not {weight_min}")
    if into is not None:
        if not isinstance(into, ContributionAccumulator):
            raise ValueError(f"{what}: into must be a ContributionAccumulator, not {type(into).__name__}")
        if into.P != P:
            raise ValueError(f"{what}: into holds {into.P} Gaussians, not P = {P}")
    if any(not t.is_cuda for _, t in bufs):
        raise ValueError(f"{what}: the state buffers must be GPU tensors (there is no CPU fallback)")
    dev = geomBuffer.device
    if any(t.device != dev for _, t in bufs) or (into is not None and into.device != dev):
        raise ValueError(f"{what}: the state buffers and the accumulator are on different devices")
    lib = _capi.load()
    if P > 0:
        need = (("geomBuffer", geomBuffer, lib.dgr_geometry_bytes(P)), ("imageBuffer", imageBuffer, lib.dgr_image_bytes(W, H)))
        for n, t, nbytes in need:
            if t.numel() < nbytes:
                raise ValueError(f"{what}: {n} has {t.numel()} bytes, a forward of P = {P} at {H} x {W} leaves {nbytes}")
    # one allocation: n_touched | max_weight | counts (int32 words), and the 8-byte sums
    words = torch.empty((2 * P + 4,), dtype=torch.int32, device=dev)
    out = ContributionStats(words[:P], words[P:2 * P].view(torch.float32), torch.empty((P,), dtype=torch.int64, device=dev),
                            words[2 * P:])
    acc = into.tensors() if into is not None else (None,) * 5
    p = _capi.ptr
    _capi.call("dgr_contribution_stats", dev, P, W, H, R, p(geomBuffer), p(binningBuffer), p(imageBuffer),
               _capi.ContributionParams(min_pixels, weight_min, frame_id), None, p(out.n_touched), p(out.max_weight),
               p(out.sum_weight), *(p(t) for t in acc), out.counts.data_ptr())
    return out


def render_contributions(viewpoint_camera, pc, pipe, bg_color, *, viewmatrix, fov, HW, scaling_modifier=1.0, override_color=None,
                         gt_depth=None, variant="light", into=None, min_pixels=1, weight_min=0.0, frame_id=0):
    """`slam.render()` without gradients, and the view's contribution statistics with it: one no-grad forward of `variant`
    ("light" or "full") through the selected binding's `_C.rasterize_gaussians`, then `contribution_stats` on the same stream over
    the state it left.  The rendered images are the ordinary ones, bit for bit those of `slam.render` (a keyframe insertion can
    feed them to `seed_from_frame`); `viewspace_points` is None (nothing is differentiated).  `into`, `min_pixels`, `weight_min`,
    `frame_id`: see `contribution_stats`.  A window of keyframes is a loop over them into one accumulator.
    Returns (the dict of `slam.render`, ContributionStats)."""
    from . import slam as _slam
    from .pose import _cameras_of
    if variant not in ("light", "full"):
        raise ValueError(f"render_contributions: unknown variant {variant!r}")
    mod = _slam._light if variant == "light" else _slam._full
    H, W = int(HW[0]), int(HW[1])
    tanfovx, tanfovy = float(fov[0]), float(fov[1])
    get = _slam._get
    znear = float(get(viewpoint_camera, "znear", 0.01)) if viewpoint_camera is not None else 0.01
    zfar = float(get(viewpoint_camera, "zfar", 100.0)) if viewpoint_camera is not None else 100.0
    perspec_src = get(viewpoint_camera, "projection_matrix") if viewpoint_camera is not None else None
    empty = _EMPTY
    with torch.no_grad():
        # (the camera tensors as render() forms them: the same operations, hence the same images)
        _, vm, projmatrix, campos = _cameras_of(viewmatrix.detach(), perspec_src, tanfovx, tanfovy, znear, zfar)[:4]
        means3D = pc.get_xyz.detach()
        P = means3D.size(0)
        shs, colors = (empty, override_color) if override_color is not None else (pc.get_features, empty)
        if gt_depth is None:
            gt_depth = torch.zeros((1, H, W), dtype=torch.float32, device=means3D.device)
        args = (bg_color, means3D, colors, pc.get_opacity, pc.get_scaling, pc.get_rotation, scaling_modifier, empty, vm, gt_depth,
                projmatrix, tanfovx, tanfovy, H, W, shs, int(pc.active_sh_degree), campos, False)
        if variant == "light":
            debug = bool(getattr(pipe, "debug", False)) if pipe is not None else False
            R, (_, color, depth, median, var, alpha, radii, geom, binning, img, unc, px) = mod._C.rasterize_gaussians_r(*args, debug)
            res = _slam._result((color, radii, depth, median, var, alpha, unc, px), None, None)
        else:
            R, (_, _, color, depth, unc, radii, geom, binning, img) = mod._C.rasterize_gaussians_r(*args)
            res = _slam._result((color, radii, depth, unc), None, None)
        with _capi.on_device(means3D.device):
            stats = contribution_stats(geom, binning, img, P, H, W, R, into=into, min_pixels=min_pixels, weight_min=weight_min,
                                       frame_id=frame_id)
    return res, stats
