"""Keyframe overlap as include/dgr_hip.h defines it (dgr_keyframe_overlap), restated in float64 numpy on the CPU.  Written from
that text, not from the kernel.  Per (keyframe, candidate) it returns the three decisions and an *ambiguous* mark: the pair sits so
close to one of the thresholds that the kernel's fp32 evaluation may decide either way.

The band is derived, not tuned.  The fp32 chain -- unprojection, one rigid transform whose twelve entries the kernel forms in
double and rounds once, one division, one multiply-add -- evaluated at frames up to 640 px wide stays within about 2e-3 px of
float64 even far outside the frame and within 5e-4 px near the borders (a CPU simulation at 640x480 stride 16, 96x80 stride 1 and
37x23 stride 3: zero decision mismatches outside the band, at most 7 ambiguous pairs of 7680), so a pair is ambiguous when
  u or v lies within 0.01 px of a border it is tested against;
  |Z - near| < 1e-4 max(1, |Z|);
  with keyframe depths, u + 0.5 or v + 0.5 lies within 0.01 of an integer (the pixel looked up may differ), or
  |Z - d_k| - tol d_k lies within 1e-4 d_k of zero.
A slip in a convention (transpose, half-pixel, stride, row / column) moves every point by at least 0.5 px."""
import numpy as np

VALID, INSIDE, VISIBLE = 1, 2, 4
PX_BAND, Z_BAND = 0.01, 1e-4


def f32(x):
    """a parameter: formed in float64, rounded once to fp32 (what the C ABI receives), carried on as float64"""
    return float(np.float32(x))


def candidates(W, H, stride):
    """(x [S], y [S]) of the candidate pixels, row-major"""
    xs, ys = np.arange(0, W, stride), np.arange(0, H, stride)
    return np.tile(xs, len(ys)), np.repeat(ys, len(xs))


def overlap_model(depth_obs, viewmatrix, keyframe_viewmatrices, fx, fy, cx, cy, *, stride=16, edge=20.0, near=0.0,
                  depth_range=(0.0, float("inf")), keyframe_depths=None, depth_tolerance=0.05):
    """depth_obs [H,W], viewmatrix [4,4] and keyframe_viewmatrices [K,4,4] (W2C^T), keyframe_depths [K,H,W] or None: float32 numpy
    arrays.  Returns a dict: flags uint8 [K,S] (bit 0 valid, bit 1 inside, bit 2 visible), ambiguous bool [K,S] (never set where the
    candidate is not valid: valid is a raw fp32 comparison, decided exactly), inside / visible int [K], valid int, score float32 [K],
    u, v, Z float64 [K,S]."""
    depth_obs = np.asarray(depth_obs, np.float32)
    H, W = depth_obs.shape
    fx, fy, cx, cy, edge, near, tol = (f32(t) for t in (fx, fy, cx, cy, edge, near, depth_tolerance))
    lo, hi = np.float32(depth_range[0]), np.float32(depth_range[1])
    x, y = candidates(W, H, stride)
    d32 = depth_obs[y, x]
    with np.errstate(invalid="ignore"):
        valid = (d32 > lo) & (d32 < hi)  # raw fp32 comparisons; NaN fails
    d = np.where(valid, d32, 1.0).astype(np.float64)
    p = np.stack([(x - cx) / fx * d, (y - cy) / fy * d, d], 1)  # [S,3] in the current camera
    view = np.asarray(viewmatrix, np.float64).reshape(4, 4)
    world = (p - view[3, :3]) @ view[:3, :3].T  # world_i = sum_j view[i][j] (p_j - view[3][j])
    kv = np.asarray(keyframe_viewmatrices, np.float64).reshape(-1, 4, 4)
    K, S = kv.shape[0], len(x)
    cam = np.einsum("si,kij->ksj", world, kv[:, :3, :3]) + kv[:, None, 3, :3]  # X_j = sum_i world_i view_k[i][j] + view_k[3][j]
    X, Y, Z = cam[..., 0], cam[..., 1], cam[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = fx * X / Z + cx, fy * Y / Z + cy
        front = Z > near
        inside = valid[None] & front & (u > edge) & (u < W - edge) & (v > edge) & (v < H - edge)
        near_border = ((np.abs(u - edge) < PX_BAND) | (np.abs(u - (W - edge)) < PX_BAND) | (np.abs(v - edge) < PX_BAND) |
                       (np.abs(v - (H - edge)) < PX_BAND))
        # a border test matters only where every other test of `inside` could pass: keep it simple and mark wherever it is close
        ambiguous = near_border | (np.abs(Z - near) < Z_BAND * np.maximum(1.0, np.abs(Z)))
    ambiguous &= valid[None]
    visible = inside.copy()
    if keyframe_depths is not None:
        kd = np.asarray(keyframe_depths, np.float32).reshape(K, H, W)
        uh, vh = u + 0.5, v + 0.5
        with np.errstate(invalid="ignore"):
            px = np.where(inside, np.floor(uh), 0).astype(np.int64)
            py = np.where(inside, np.floor(vh), 0).astype(np.int64)
            in_image = (px < W) & (py < H)
            dk32 = kd[np.arange(K)[:, None], np.minimum(py, H - 1), np.minimum(px, W - 1)]
            ok = (dk32 > lo) & (dk32 < hi)
            dk = np.where(ok, dk32, 1.0).astype(np.float64)
            margin = np.abs(Z - dk) - tol * dk
            visible = inside & in_image & ok & (margin <= 0.0)
            on_pixel_edge = (np.abs(uh - np.rint(uh)) < PX_BAND) | (np.abs(vh - np.rint(vh)) < PX_BAND)
            ambiguous |= inside & (on_pixel_edge | (ok & (np.abs(margin) < Z_BAND * dk)))
    flags = (valid[None] * VALID + inside * INSIDE + visible * VISIBLE).astype(np.uint8) * np.ones((K, 1), np.uint8)
    n_valid = int(valid.sum())
    n_visible = visible.sum(1)
    score = (n_visible.astype(np.float32) / np.float32(n_valid)) if n_valid else np.zeros(K, np.float32)
    return dict(flags=flags, ambiguous=ambiguous, inside=inside.sum(1), visible=n_visible, valid=n_valid, score=score.astype(np.float32),
                u=u, v=v, Z=Z, S=S)
