"""Map expansion from an RGB-D keyframe as include/dgr_hip.h defines it (dgr_seed_plan / dgr_seed_apply), in plain torch ops on
the CPU.  Written from that text, not from the kernel: masks as fp32 comparisons, `nonzero` in row-major order, `torch.cat`.  The
new rows' positions and log-scales are carried in float64, so that they are the reference values of the kernel's fp32 ones."""
import math

import torch

INV_C0 = 1.0 / 0.28209479177387814


def f32(value):
    """a threshold: formed in float64, rounded once to fp32"""
    return torch.tensor(value, dtype=torch.float64).to(torch.float32)


def seed_masks(depth_obs, opacity_map=None, depth=None, *, silhouette_threshold=0.5, depth_error_min=float("inf"),
               depth_range=(0.0, float("inf")), stride=1):
    """(select, valid, unseen, infront) as [H, W] bool masks over the whole frame, False off the candidate grid"""
    H, W = depth_obs.shape
    cand = torch.zeros((H, W), dtype=torch.bool)
    cand[::stride, ::stride] = True
    valid = (depth_obs > f32(depth_range[0])) & (depth_obs < f32(depth_range[1]))
    unseen = torch.zeros_like(valid) if opacity_map is None else opacity_map.reshape(H, W) < f32(silhouette_threshold)
    if depth is None:
        infront = torch.zeros_like(valid)
    else:
        d = depth.reshape(H, W)
        infront = (d > depth_obs) & ((d - depth_obs) > f32(depth_error_min))  # (d - depth_obs: one fp32 subtraction)
    select = valid & (unseen | infront) if (opacity_map is not None or depth is not None) else valid
    return select & cand, valid & cand, valid & unseen & cand, valid & infront & cand


def seed_model(leaves, moments, accumulators, color_obs, depth_obs, viewmatrix, fx, fy, cx, cy, *, opacity_map=None, depth=None,
               silhouette_threshold=0.5, depth_error_min=float("inf"), depth_range=(0.0, float("inf")), stride=1,
               init_opacity=0.5, scale_factor=1.0, fill=None):
    """leaves: dict with "xyz", "scaling", "rotation", "opacity", optionally "f_dc", and any further [P, ...] tensors; moments:
    dict name -> (exp_avg, exp_avg_sq); accumulators: dict name -> tensor or None; viewmatrix: [4, 4] holding W2C^T.  Returns a dict:
      leaves (the new rows of xyz and scaling in float64: "xyz_new", "scaling_new"; their old rows under the leaf's name),
      moments, accumulators, counts (rows, new, valid, unseen, infront), pixels [n, 2] (x, y of every new row, in order),
      xyz_scale [n]: |p_cam| + |campos|, what the positions' tolerance is relative to."""
    fill = fill or {}
    P = leaves["xyz"].shape[0]
    select, valid, unseen, infront = seed_masks(depth_obs, opacity_map, depth, silhouette_threshold=silhouette_threshold,
                                                depth_error_min=depth_error_min, depth_range=depth_range, stride=stride)
    yx = torch.nonzero(select)  # row-major: y, then x
    y, x = yx[:, 0], yx[:, 1]
    n = yx.shape[0]
    d = depth_obs[y, x].double()
    p = torch.stack([(x.double() - cx) / fx * d, (y.double() - cy) / fy * d, d], dim=1)
    view = viewmatrix.double().reshape(4, 4)
    world = (p - view[3, :3]) @ view[:3, :3].T            # world_i = sum_j view[i][j] (p_j - view[3][j])
    campos = -(view[:3, :3] @ view[3, :3])
    pix = float(scale_factor) * stride * 0.5 * (1.0 / fx + 1.0 / fy)
    log_scale = torch.log(d * pix)
    out = {}
    for name, t in leaves.items():
        shape = (n,) + tuple(t.shape[1:])
        if name in ("xyz", "scaling"):
            out[name] = t
            continue
        if name == "rotation":
            fresh = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n, 1)
        elif name == "opacity":
            fresh = f32(math.log(init_opacity / (1.0 - init_opacity))).expand(shape)
        elif name == "f_dc":
            rgb = color_obs[:, y, x].T                     # [n, 3]
            fresh = ((rgb - torch.tensor(0.5)) * f32(INV_C0)).reshape(shape)
        else:
            fresh = f32(float(fill.get(name, 0.0))).expand(shape)
        out[name] = torch.cat([t, fresh.to(torch.float32)])
    out["xyz_new"], out["scaling_new"] = world, log_scale.unsqueeze(1).expand(n, 3)
    grow = lambda t: torch.cat([t, t.new_zeros((n,) + tuple(t.shape[1:]))])  # noqa: E731
    mom = {name: (grow(m), grow(v)) for name, (m, v) in moments.items()}
    acc = {name: None if t is None else grow(t) for name, t in accumulators.items()}
    counts = (P + n, n, int(valid.sum()), int(unseen.sum()), int(infront.sum()))
    return dict(leaves=out, moments=mom, accumulators=acc, counts=counts, pixels=torch.stack([x, y], dim=1),
                xyz_scale=p.norm(dim=1) + campos.norm())
