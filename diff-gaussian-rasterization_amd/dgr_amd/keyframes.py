"""Keyframe overlap scores on the device and the covisibility selection built on them (C ABI: dgr_keyframe_overlap)."""
from typing import NamedTuple as _NamedTuple

import torch

from . import _capi
from .losses import _check_gpu


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
    nbytes = _capi.load().dgr_keyframe_overlap_scratch_bytes(W, H, stride, K)
    if nbytes == 0:
        raise ValueError(f"{what}: cannot take {K} keyframes of {S} candidates each (at most 2^20 keyframes, K * S below 2^31)")
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    depth_obs, viewmatrix, keyframe_viewmatrices = (t.detach().contiguous() for t in (depth_obs, viewmatrix, keyframe_viewmatrices))
    if keyframe_depths is not None:
        keyframe_depths = keyframe_depths.detach().contiguous()
    params = _capi.KeyframeOverlapParams(scalars["fx"], scalars["fy"], scalars["cx"], scalars["cy"], lo, hi, scalars["edge"],
                                         scalars["near"], scalars["depth_tolerance"], stride)
    _capi.call("dgr_keyframe_overlap", dev, W, H, depth_obs.data_ptr(), viewmatrix.data_ptr(), K, keyframe_viewmatrices.data_ptr(),
               _capi.ptr(keyframe_depths), params, scratch.data_ptr(), out.inside.data_ptr(), out.visible.data_ptr(),
               out.valid.data_ptr(), out.score.data_ptr(), _capi.ptr(flags))
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
