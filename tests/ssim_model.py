"""The SSIM / L1 + D-SSIM loss the HIP kernels implement (csrc/ssim.hip), restated in torch on the CPU.  Not a test.

    window   g[i] ~ exp(-(i - 5)^2 / (2 1.5^2)), i = 0..10, normalised to sum 1 in double and rounded once to float; 2D: g g^T
    moments  mu1 = w*x, mu2 = w*y, s1 = w*x^2 - mu1^2, s2 = w*y^2 - mu2^2, s12 = w*xy - mu1 mu2   (zero padding 5, per channel)
    map      m = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),  C1 = 0.01^2, C2 = 0.03^2
    SSIM     mean of m over every element of the [V, C, H, W] stack
    loss     w_l1 mean|x - y| + w_ssim (1 - SSIM) + w_depth mean|d - d_obs|

`model(..., dtype=torch.float64)` is the model the tests measure distances from; the same lines in float32 (the 121-tap window
applied directly by `F.conv2d`) are the YARDSTICK: how far a float32 evaluation of this loss lies from the model.
`maps` are the three derivative maps the forward kernel leaves in its scratch and `analytic_grad` the form of dSSIM/dx the
backward kernel evaluates from them.  The edge cases of tests/test_hip_ssim_edges.py are defined at the end."""
import math

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window_1d():
    """The eleven taps as the kernels hold them: normalised in double, rounded once to float (returned as float32)."""
    e = [math.exp(-((i - 5) ** 2) / (2.0 * 1.5 ** 2)) for i in range(11)]
    s = sum(e)
    return torch.tensor([v / s for v in e], dtype=torch.float64).to(torch.float32)


def _window_2d(channels, dtype):
    g = window_1d().to(dtype)  # (the float taps; their outer product in `dtype`)
    return (g[:, None] * g[None, :]).expand(channels, 1, 11, 11).contiguous()


def _conv(t, w):
    return F.conv2d(t, w, padding=5, groups=t.shape[1])


def _moments(x, y):
    w = _window_2d(x.shape[1], x.dtype)
    mu1, mu2 = _conv(x, w), _conv(y, w)
    s1, s2, s12 = _conv(x * x, w) - mu1 * mu1, _conv(y * y, w) - mu2 * mu2, _conv(x * y, w) - mu1 * mu2
    return w, mu1, mu2, s1, s2, s12


def ssim_map(x, y):
    """m for [V, C, H, W] tensors, in their dtype."""
    _, mu1, mu2, s1, s2, s12 = _moments(x, y)
    return (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def _as_stack(t, dtype):
    t = t.detach().cpu().to(dtype)
    return t[None] if t.dim() == 3 else t


def model(x, y, depth=None, depth_obs=None, w_l1=0.0, w_ssim=-1.0, w_depth=0.0, dtype=torch.float64):
    """dict(loss, ssim, grad, grad_depth, m) of the loss above evaluated in `dtype` on the CPU, the gradients by autograd.
    The default weights give loss = SSIM - 1, i.e. grad = dSSIM/dx."""
    x, y = _as_stack(x, dtype).requires_grad_(), _as_stack(y, dtype)
    m = ssim_map(x, y)
    ssim = m.mean()
    loss = w_l1 * (x - y).abs().mean() + w_ssim * (1 - ssim)
    d = None
    if depth is not None:
        d, do = depth.detach().cpu().to(dtype).requires_grad_(), depth_obs.detach().cpu().to(dtype)
        loss = loss + w_depth * (d - do).abs().mean()
    loss.backward()
    return dict(loss=loss.detach(), ssim=ssim.detach(), grad=x.grad, grad_depth=None if d is None else d.grad, m=m.detach())


def maps(x, y, dtype=torch.float64):
    """The three derivative maps the forward kernel leaves for the backward, (dm/dmu1, dm/ds1, dm/ds12), each [V, C, H, W] in
    `dtype`: with A, B the numerator and Cc, D the denominator factors of m,
        dm/ds1 = -m / D,  dm/ds12 = 2A / (Cc D),  dm/dmu1 = 2 mu2 B / (Cc D) - 2 mu1 m / Cc - 2 mu1 dm/ds1 - mu2 dm/ds12"""
    x, y = _as_stack(x, dtype), _as_stack(y, dtype)
    _, mu1, mu2, s1, s2, s12 = _moments(x, y)
    A, B, Cc, D = 2 * mu1 * mu2 + C1, 2 * s12 + C2, mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    m = A * B / (Cc * D)
    dm_ds1 = -m / D
    dm_ds12 = 2 * A / (Cc * D)
    dm_dmu1 = 2 * mu2 * B / (Cc * D) - 2 * mu1 * m / Cc - 2 * mu1 * dm_ds1 - mu2 * dm_ds12
    return dm_dmu1, dm_ds1, dm_ds12


def grad_from_maps(x, y, three, dtype=torch.float64):
    """dSSIM/dx = [w*(dm/dmu1) + 2x w*(dm/ds1) + y w*(dm/ds12)] / N from the three maps (the window is symmetric: the same
    zero-padded correlation serves forward and backward)."""
    x, y = _as_stack(x, dtype), _as_stack(y, dtype)
    w = _window_2d(x.shape[1], dtype)
    dm_dmu1, dm_ds1, dm_ds12 = (t.to(dtype) for t in three)
    return (_conv(dm_dmu1, w) + 2 * x * _conv(dm_ds1, w) + y * _conv(dm_ds12, w)) / x.numel()


def analytic_grad(x, y, dtype=torch.float64):
    """dSSIM/dx in the three-map form the backward kernel evaluates: `maps` recombined by `grad_from_maps`."""
    return grad_from_maps(x, y, maps(x, y, dtype), dtype)


def placed(canvas_hw, patch, oy, ox, background=(0.5, 0.4)):
    """(img, ref) float32 [1, 1, H, W]: constant canvases of `background` with the patch pair `patch` = (px, py), two [h, w]
    tensors, written at rows oy .. oy + h, columns ox .. ox + w."""
    out = []
    for p, level in zip(patch, background):
        canvas = torch.full((1, 1) + tuple(canvas_hw), level, dtype=torch.float32)
        canvas[0, 0, oy:oy + p.shape[0], ox:ox + p.shape[1]] = p
        out.append(canvas)
    return tuple(out)


def tiles_of(shape):
    """workgroups of the tile kernels for a (V, C, H, W) stack: one per 32 x 16 tile of every plane"""
    V, C, H, W = shape
    return V * C * ((H + 15) // 16) * ((W + 31) // 32)


SHAPES = ((1, 3, 7, 9), (1, 1, 16, 16), (2, 3, 17, 33), (1, 3, 37, 53), (4, 3, 48, 64), (1, 3, 144, 192))
KINDS = ("rand", "smooth", "flatbright")

# ---- the edge cases of tests/test_hip_ssim_edges.py (their defining conditions are asserted in tests/test_ssim_abi.py) ----
# one tile exactly, one over in each direction, a single pixel / row / column, images smaller than the window, an odd height
EDGE_SHAPES = ((1, 1, 16, 32), (1, 1, 17, 32), (1, 1, 16, 33), (1, 1, 1, 1), (1, 2, 1, 45), (2, 1, 45, 1), (1, 3, 5, 11),
               (1, 3, 11, 5), (2, 2, 37, 53))
# "same": ref == img (gradient 0 analytically); "const": constant planes (sigma = 0, D = C2 away from the border)
EDGE_KINDS = KINDS + ("same", "const")
# the one-workgroup sum adds the tiles' slots 256 at a time: tile counts below, at and past one trip
TILE_SHAPES = ((255, 1, 3, 3), (256, 1, 3, 3), (257, 1, 3, 3), (65, 4, 1, 1), (3, 3, 97, 161))
FINAL_THREADS = 256
# the depth term's sum is a grid-stride loop over 128 x 256 threads
DEPTH_COUNTS = (32767, 32768, 32769, 65537)
DEPTH_THREADS = 128 * 256
# the largest shapes dgr_ssim_scratch_floats accepts
LIMIT_SHAPES = ((65535, 1, 1, 1), (1, 1, 1 << 20, 1), (1, 1, 1, 1 << 20))
# the tile-phase scene: a 13 x 19 patch pair on a constant canvas, its corner at (20 + dy, 20 + dx)
CANVAS_HW, PATCH_HW, PATCH_ORIGIN, MARGIN = (68, 90), (13, 19), (20, 20), 10
PHASES = ([(0, dx) for dx in range(32)] + [(dy, 0) for dy in range(1, 16)]
          + [(1, 1), (15, 31), (7, 13), (8, 16), (15, 1), (1, 31), (11, 29), (5, 22)])


def edge_inputs(kind, shape, seed=0):
    """(x, y) for EDGE_KINDS: `inputs` for the model's three kinds; "same": y is x; "const": one level per plane and image."""
    if kind in KINDS:
        return inputs(kind, shape, seed)
    g = torch.Generator().manual_seed(5000 + 7 * sum(shape) + seed)
    if kind == "same":
        x = torch.rand(shape, generator=g, dtype=torch.float32)
        return x, x.clone()
    if kind == "const":
        a = 0.2 + 0.7 * torch.rand(shape[:2] + (1, 1), generator=g, dtype=torch.float32)
        b = 0.2 + 0.7 * torch.rand(shape[:2] + (1, 1), generator=g, dtype=torch.float32)
        return a.expand(shape).contiguous(), b.expand(shape).contiguous()
    raise ValueError(kind)


def patch_pair(seed=0):
    g = torch.Generator().manual_seed(7000 + seed)
    return torch.rand(PATCH_HW, generator=g, dtype=torch.float32), torch.rand(PATCH_HW, generator=g, dtype=torch.float32)


def depth_pair(n_depth, variant, seed=0):
    """(d, d_obs, special) float32 [n_depth]: |d - d_obs| below 0.5 everywhere but at `special` = the indices DEPTH_THREADS - 1,
    DEPTH_THREADS (where they exist) and n_depth - 1, the last element of the loop's first trip, the first of its second and the
    last of all.  variant "ties": d == d_obs there; "peaks": d - d_obs = +-8 there, so that one dropped or doubled element
    moves the mean by 8 / n_depth."""
    g = torch.Generator().manual_seed(9000 + n_depth + seed)
    d_obs = 1.0 + torch.rand(n_depth, generator=g, dtype=torch.float32)
    d = d_obs + (torch.rand(n_depth, generator=g, dtype=torch.float32) - 0.5)
    special = sorted({i for i in (DEPTH_THREADS - 1, DEPTH_THREADS, n_depth - 1) if i < n_depth})
    for k, i in enumerate(special):
        d_obs[i] = 1.5  # (so that d - d_obs is 8 exactly)
        d[i] = d_obs[i] if variant == "ties" else d_obs[i] + (8.0 if k % 2 == 0 else -8.0)
    return d, d_obs, special


def inputs(kind, shape, seed=0):
    """(x, y) float32 CPU tensors of `shape` = (V, C, H, W), fixed by (kind, shape, seed)."""
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + 7 * sum(shape) + seed)
    u = lambda: torch.rand(shape, generator=g, dtype=torch.float32)  # noqa: E731
    if kind == "rand":
        return u(), u()
    if kind == "smooth":
        col = torch.arange(shape[3], dtype=torch.float32)[None, None, None, :]
        row = torch.arange(shape[2], dtype=torch.float32)[None, None, :, None]
        x = (0.5 + 0.3 * torch.sin(col / 7) * torch.cos(row / 5)).expand(shape).contiguous()
        return x, x + 0.02 * (u() - 0.5)
    if kind == "flatbright":
        return 0.95 + 0.001 * (u() - 0.5), 0.9 + 0.001 * (u() - 0.5)
    raise ValueError(kind)
