"""The float64 model of the per-Gaussian contribution statistics (include/dgr_hip.h: dgr_contribution_stats), on the per-tile
building blocks of tests/fp64_model.py (tiles, alpha_of, valid_pairs, blend_weights).  Like the entry point it models, it works on
the state of a finished forward: the hard decisions (`point_list`, `ranges`, `n_contrib`) AND the render records the forward left
(screen-space means, conic, opacity: fp32 values, taken to float64 exactly -- `records()`), from a HIP forward's exported state or
from the CPU oracle's.  What it checks is therefore the replay -- which pairs count, in which order T runs down, the max and the
sum -- evaluated independently in float64 from the replay's own inputs.

A pair (pixel, 1-based list position k) is blended iff k <= n_contrib[pixel], power <= 0 and alpha >= 15/255 -- for the light
forward (which does not blend the entry that ends a pixel: it lies behind n_contrib) and the full one (which does: it is
n_contrib) alike.  Its weight is alpha T, T the product of (1 - alpha) over the pixel's earlier blended pairs.

`stats()` returns, per Gaussian [P]: count, max and sum of the weights in float64; `ambiguous` = its pairs inside n_contrib whose
decision a float32 evaluation may take the other way (|alpha - 15/255| <= 1e-6 or |power| <= 1e-6); `tainted` = it blends at or
behind an ambiguous pair of the same pixel (its T there may be another); and `max32` / `sum32`, the same weights replayed in NumPy
float32 in list order (power, exp, clamp and the running product, under the float64 decisions): the distance of that replay from
the float64 values is the model's own distance from a float32 evaluation, which a test doubles for its tolerance."""
from types import SimpleNamespace

import numpy as np
import torch

import fp64_model as fm

ALPHA_MIN = 15.0 / 255.0
AMBIGUOUS = 1e-6


def records(means2D, conic_opacity):
    """the geometry of `stats` from a forward's exported records: means2D [P,2] and conic_opacity [P,4] = (a, b, c, opacity), fp32"""
    m, c = fm.f64(np.asarray(means2D).reshape(-1, 2)), fm.f64(np.asarray(conic_opacity).reshape(-1, 4))
    return m, (c[:, 0], c[:, 1], c[:, 2]), c[:, 3]


def tile_weights(tl, pix, con, opac, g32):
    """One tile: (valid [n,npix], ambiguous [n,npix], float64 weights, float32-replay weights); g32 = the geometry as float32 tensors"""
    power, alpha = fm.alpha_of(tl, fm.tile_xy(pix, tl), con, opac)
    valid = fm.valid_pairs(tl, power, alpha)
    amb = (tl.pos < tl.ncp) & (((alpha - ALPHA_MIN).abs() <= AMBIGUOUS) | (power.abs() <= AMBIGUOUS))
    w, _, _ = fm.blend_weights(torch.where(valid, alpha, torch.zeros_like(alpha)))
    # the float32 replay: every operation in float32, in list order, under the model's float64 decisions
    f32 = lambda x: x.numpy().astype(np.float32)  # noqa: E731
    ids = tl.ids
    pix, con, opac = g32
    dx = f32(pix[ids, 0:1]) - f32(tl.pxs[None])
    dy = f32(pix[ids, 1:2]) - f32(tl.pys[None])
    a, b, c = (f32(k[ids, None]) for k in con)
    p32 = np.float32(-0.5) * (a * dx * dx + c * dy * dy) - b * dx * dy
    a32 = np.minimum(np.float32(0.99), f32(opac[ids, None]) * np.exp(p32, dtype=np.float32))
    a32 = np.where(valid.numpy(), a32, np.float32(0.0)).astype(np.float32)
    T32 = np.cumprod(np.float32(1.0) - a32, axis=0, dtype=np.float32)
    T32 = np.concatenate([np.ones((1, a32.shape[1]), np.float32), T32[:-1]], 0)
    return valid.numpy(), amb.numpy(), w.numpy(), (a32 * T32).astype(np.float32)


def stats(s, geom, point_list, ranges, n_contrib):
    """`s`: anything with P, W, H; `geom`: (pixel means [P,2], conic (a, b, c), opacity [P]) as float64 tensors, a row per Gaussian
    (`records()`; rows of Gaussians that are in no list are never read)"""
    P = s.P
    vis, idx, (pix, con, opac) = np.ones(P, bool), np.arange(P), geom
    g32 = (pix.float(), tuple(c.float() for c in con), opac.float())  # (exact: the records are fp32 values)
    out = SimpleNamespace(count=np.zeros(P, np.int64), max=np.zeros(P), sum=np.zeros(P), ambiguous=np.zeros(P, np.int64),
                          tainted=np.zeros(P, bool), max32=np.zeros(P, np.float32), sum32=np.zeros(P), n_pairs=0)
    for tl in fm.tiles(s, vis, point_list, ranges, n_contrib):
        valid, amb, w, w32 = tile_weights(tl, pix, con, opac, g32)
        g = idx[tl.ids.numpy()]
        behind = np.cumsum(amb, axis=0) > 0  # at or behind an ambiguous pair of the same pixel
        np.add.at(out.count, g, valid.sum(1))
        np.maximum.at(out.max, g, np.where(valid, w, 0.0).max(1))
        np.add.at(out.sum, g, w.sum(1))
        np.add.at(out.ambiguous, g, amb.sum(1))
        np.logical_or.at(out.tainted, g, (valid & behind).any(1) | amb.any(1))
        np.maximum.at(out.max32, g, w32.max(1))
        np.add.at(out.sum32, g, w32.astype(np.float64).sum(1))  # (the float32 weights, summed without further rounding)
        out.n_pairs += int(valid.sum())
    return out


def tolerances(m):
    """per Gaussian: (max_weight, sum_weight) tolerance = max(2 |float32 replay - float64|, floor), floors 1e-6 and 1e-6 n_touched"""
    return (np.maximum(2.0 * np.abs(m.max32.astype(np.float64) - m.max), 1e-6),
            np.maximum(2.0 * np.abs(m.sum32 - m.sum), 1e-6 * m.count))


def conditions(m):
    """(share of the touched Gaussians with an ambiguous pair, share left out of the weight checks)"""
    touched = m.count > 0
    n = max(int(touched.sum()), 1)
    return float(((m.ambiguous > 0) & touched).sum()) / n, float((m.tainted & touched).sum()) / n
