"""The CPU model of `slam.masked_l1_loss` (include/dgr_hip.h: dgr_masked_loss_*) and the inputs its tests share.

Masks, medians and counts are computed in float32 with single operations and `torch.median` (the lower median), exactly as the
header defines them, so the GPU's must EQUAL them; the sums are taken in float64."""
import functools

import torch

INF = float("inf")
SHAPES = [(1, 3, 1, 1), (1, 3, 1, 2), (1, 1, 7, 5), (1, 3, 37, 53), (3, 3, 33, 65), (1, 3, 480, 640)]  # (V, C, H, W)
FAMILIES = ("dyadic", "random")
NAN_BITS = 0x7FC00000  # the median stored when rejection is off


@functools.lru_cache(maxsize=None)
def inputs(family, shape):
    """dict(color, depth, color_obs, depth_obs, opacity_map, mask) of float32 CPU tensors ([V,C,H,W] / [V,1,H,W]; mask uint8),
    made once per (family, shape): treat them as read-only.
    dyadic: everything a multiple of 1/4 (depth_obs in [0.5, 4] with 30 % holes, depth = depth_obs + k/4, k in -4..4, 5 % outliers
            at +10, colours in [0, 1]): nine distinct errors, so the select is all ties, and every sum is exact in fp32 and fp64.
    random: continuous values, errors ~ rand^3 (nearly all keys distinct), the same holes and outliers, a few NaN / inf depths.
    The silhouette is 1.0 on about 80 % of the pixels and uniform below that.  In the (3, 3, 33, 65) stack view 1 has no valid
    depth at all; the one pixel of (1, 3, 1, 1) is forced valid."""
    V, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(family) + SHAPES.index(shape))
    r = lambda *s: torch.rand(*s, generator=g)
    pix = (V, 1, H, W)
    if family == "dyadic":
        depth_obs = torch.randint(2, 17, pix, generator=g).float() / 4
        depth = depth_obs + torch.randint(-4, 5, pix, generator=g).float() / 4
        color_obs = torch.randint(0, 5, (V, C, H, W), generator=g).float() / 4
        color = torch.randint(0, 5, (V, C, H, W), generator=g).float() / 4
    else:
        depth_obs = 0.5 + 3.5 * r(pix)
        depth = depth_obs + (r(pix) ** 3) * torch.where(r(pix) < 0.5, -1.0, 1.0)
        color_obs, color = r(V, C, H, W), r(V, C, H, W)
    outlier = r(pix) < 0.05
    depth = torch.where(outlier, depth_obs + 10.0, depth)
    hole = r(pix) < 0.30
    depth_obs = torch.where(hole, torch.zeros(()), depth_obs)
    opacity_map = torch.where(r(pix) < 0.8, torch.ones(()), r(pix))
    mask = (r(pix) < 0.7).to(torch.uint8)
    if shape == (1, 3, 1, 1):
        depth_obs[...] = 1.0
        depth[...] = 1.25
        opacity_map[...] = 1.0
        mask[...] = 1
    if shape == (3, 3, 33, 65):
        depth_obs[1] = 0.0
    if family == "random" and H * W >= 35:
        flat = depth.view(V, -1)
        flat[:, 3] = float("nan")
        flat[:, 17] = INF
        flat[:, 29] = -INF
        depth_obs.view(V, -1)[:, 3] = 2.0  # (so that the NaN meets a valid observation)
    return dict(color=color, depth=depth, color_obs=color_obs, depth_obs=depth_obs, opacity_map=opacity_map, mask=mask)


def model(color, depth, color_obs, depth_obs, opacity_map=None, mask=None, *, silhouette_threshold=0.99, depth_range=(0.0, INF),
          outlier_factor=10.0, mask_color=True, w_color=1.0, w_depth=0.5, reduction="sum"):
    """dict(mask [V,H,W] bool, median [V] f32, base, kept [V] int32, loss (float64 scalar), n_terms, dcolor, ddepth (float64, for
    upstream 1)) of float32 CPU inputs."""
    V, C, H, W = color.shape
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    d, dobs = depth.reshape(V, H, W), depth_obs.reshape(V, H, W)
    e = (d - dobs).abs()
    B = (f32(depth_range[0]) < dobs) & (dobs < f32(depth_range[1])) & torch.isfinite(e)
    if opacity_map is not None:
        B = B & (opacity_map.reshape(V, H, W) > f32(silhouette_threshold))
    if mask is not None:
        B = B & (mask.reshape(V, H, W) != 0)
    if outlier_factor is None:
        median = torch.full((V,), float("nan")).view(torch.int32).fill_(NAN_BITS).view(torch.float32)
        K = B
    else:
        median = torch.stack([torch.median(e[v][B[v]]) if bool(B[v].any()) else torch.zeros(()) for v in range(V)])
        K = B & (e <= (f32(outlier_factor) * median).view(V, 1, 1))
    S_d = e[K].double().sum()
    diff = (color - color_obs).abs()
    sel = K.view(V, 1, H, W).expand(V, C, H, W) if mask_color else torch.ones((V, C, H, W), dtype=torch.bool)
    S_c = diff[sel].double().sum()
    n_k = int(K.sum())
    N_d = (n_k if reduction == "mean" else 1)
    N_c = ((C * n_k if mask_color else C * H * W * V) if reduction == "mean" else 1)
    k_d = w_depth / N_d if N_d else 0.0
    k_c = w_color / N_c if N_c else 0.0
    loss = k_d * S_d + k_c * S_c
    ddepth = torch.where(K, torch.sign(d - dobs).double() * k_d, torch.zeros((), dtype=torch.float64)).view(depth.shape)
    dcolor = torch.where(sel, torch.sign(color - color_obs).double() * k_c, torch.zeros((), dtype=torch.float64))
    return dict(mask=K, median=median, base=B.view(V, -1).sum(1).int(), kept=K.view(V, -1).sum(1).int(), loss=loss,
                n_terms=n_k + int(sel.sum()), dcolor=dcolor, ddepth=ddepth, k_d=k_d, k_c=k_c)


def autograd_grads(color, depth, color_obs, depth_obs, K, *, mask_color=True, w_color=1.0, w_depth=0.5, reduction="sum"):
    """(dcolor, ddepth) by float64 autograd of the model's loss with the mask K [V,H,W] held fixed."""
    V, C, H, W = color.shape
    c, d = color.double().requires_grad_(), depth.double().requires_grad_()
    sel = K.view(V, 1, H, W).expand(V, C, H, W) if mask_color else torch.ones((V, C, H, W), dtype=torch.bool)
    e = (d.reshape(V, H, W) - depth_obs.double().reshape(V, H, W)).abs()
    S_d = torch.where(K, e, torch.zeros((), dtype=torch.float64)).sum()
    S_c = torch.where(sel, (c - color_obs.double()).abs(), torch.zeros((), dtype=torch.float64)).sum()
    n_k = int(K.sum())
    N_d = (n_k if reduction == "mean" else 1)
    N_c = ((C * n_k if mask_color else C * H * W * V) if reduction == "mean" else 1)
    loss = (w_depth / N_d if N_d else 0.0) * S_d + (w_color / N_c if N_c else 0.0) * S_c
    loss.backward()
    return c.grad, d.grad
