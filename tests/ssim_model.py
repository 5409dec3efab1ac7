"""The SSIM / L1 + D-SSIM loss the HIP kernels implement (csrc/ssim.hip), restated in torch on the CPU.  Not a test.

    window   g[i] ~ exp(-(i - 5)^2 / (2 1.5^2)), i = 0..10, normalised to sum 1 in double and rounded once to float; 2D: g g^T
    moments  mu1 = w*x, mu2 = w*y, s1 = w*x^2 - mu1^2, s2 = w*y^2 - mu2^2, s12 = w*xy - mu1 mu2   (zero padding 5, per channel)
    map      m = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),  C1 = 0.01^2, C2 = 0.03^2
    SSIM     mean of m over every element of the [V, C, H, W] stack
    loss     w_l1 mean|x - y| + w_ssim (1 - SSIM) + w_depth mean|d - d_obs|

`model(..., dtype=torch.float64)` is the model the tests measure distances from; the same lines in float32 (the 121-tap window
applied directly by `F.conv2d`) are the YARDSTICK: how far a float32 evaluation of this loss lies from the model.
`analytic_grad` is the three-map form of dSSIM/dx the backward kernel evaluates."""
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


def analytic_grad(x, y, dtype=torch.float64):
    """dSSIM/dx in the three-map form: with A, B the numerator and Cc, D the denominator factors of m,
        dm/ds1 = -m / D,  dm/ds12 = 2A / (Cc D),  dm/dmu1 = 2 mu2 B / (Cc D) - 2 mu1 m / Cc - 2 mu1 dm/ds1 - mu2 dm/ds12
        dSSIM/dx = [w*(dm/dmu1) + 2x w*(dm/ds1) + y w*(dm/ds12)] / N
    (the window is symmetric: the same zero-padded correlation serves forward and backward)."""
    x, y = _as_stack(x, dtype), _as_stack(y, dtype)
    w, mu1, mu2, s1, s2, s12 = _moments(x, y)
    A, B, Cc, D = 2 * mu1 * mu2 + C1, 2 * s12 + C2, mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    m = A * B / (Cc * D)
    dm_ds1 = -m / D
    dm_ds12 = 2 * A / (Cc * D)
    dm_dmu1 = 2 * mu2 * B / (Cc * D) - 2 * mu1 * m / Cc - 2 * mu1 * dm_ds1 - mu2 * dm_ds12
    return (_conv(dm_dmu1, w) + 2 * x * _conv(dm_ds1, w) + y * _conv(dm_ds12, w)) / x.numel()


SHAPES = ((1, 3, 7, 9), (1, 1, 16, 16), (2, 3, 17, 33), (1, 3, 37, 53), (4, 3, 48, 64), (1, 3, 144, 192))
KINDS = ("rand", "smooth", "flatbright")


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
