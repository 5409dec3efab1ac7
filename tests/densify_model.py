"""3DGS's densify-and-prune as the SEQUENCE include/dgr_hip.h defines the fused step by, in plain torch ops on whatever
device the tensors live on: clone, split, remove the split originals, prune, with `max_radii2D` carried to the prune.
Written from that text, not from the kernel: masks, `torch.cat` and boolean indexing, as 3DGS's GaussianModel does it.  The
positions (xyz) are carried in float64, so that the children's are the reference values of the kernel's fp32 ones."""
import math

import torch

LOG_1P6 = math.log(1.6)  # rounded to fp32 where it is used: one fp32 subtraction from scaling_raw


def f32(value, dev):
    """a threshold: formed in float64, rounded once to fp32"""
    return torch.tensor(value, dtype=torch.float64).to(torch.float32).to(dev)


def build_rotation64(q):
    q = q.double()
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.empty((q.shape[0], 3, 3), dtype=torch.float64, device=q.device)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def densify_model(leaves, moments, accum, denom, max_radii2D, noise, *, grad_threshold, extent, percent_dense=0.01,
                  min_opacity=0.005, max_screen_size=None):
    """leaves: dict with "xyz", "scaling", "rotation", "opacity" and any further [P, ...] tensors; moments: dict name ->
    (exp_avg, exp_avg_sq) for some of them; noise [P, 2, 3].  Returns a dict:
      leaves (xyz in float64), moments, counts (rows, survivors, clones kept, children kept, split),
      origin [P'] (the original row of every output row), fresh [P'] (True for clones and children),
      xyz_slack [P', 3]: 0 for survivors and clones, |xyz_c| + sum_k exp(scaling_raw_k) |n_k| for children (the smaller of the
      parent's and the child's |xyz_c|)."""
    xyz, scaling, rotation = leaves["xyz"], leaves["scaling"], leaves["rotation"]
    P, dev = xyz.shape[0], xyz.device
    a, d = accum.reshape(P), denom.reshape(P)
    hot = (d > 0) & (a >= f32(grad_threshold, dev) * d)
    m = scaling.max(dim=1).values if P else scaling.new_zeros(0)
    split = hot & (m > f32(math.log(percent_dense * extent), dev))
    clone = hot & ~split
    n_clone, n_split = int(clone.sum()), int(split.sum())
    rows = torch.arange(P, device=dev)

    # 1. clones, 2. children (sample 0 of all split rows, then sample 1)
    R = build_rotation64(rotation[split])
    spread = torch.exp(scaling[split].double())
    kids, slack = [], []
    for s in (0, 1):
        n = noise[split, s].double()
        kids.append(xyz[split].double() + torch.bmm(R, (spread * n).unsqueeze(-1)).squeeze(-1))
        slack.append(torch.minimum(xyz[split].double().abs(), kids[-1].abs()) + (spread * n.abs()).sum(dim=1, keepdim=True))
    out = {}
    for name, t in leaves.items():
        if name == "xyz":
            out[name] = torch.cat([t.double(), t[clone].double()] + kids)
        elif name == "scaling":
            child = t[split] - f32(LOG_1P6, dev)
            out[name] = torch.cat([t, t[clone], child, child])
        else:
            out[name] = torch.cat([t, t[clone], t[split], t[split]])
    n_new = n_clone + 2 * n_split
    mom = {name: tuple(torch.cat([x, x.new_zeros((n_new,) + tuple(x.shape[1:]))]) for x in mv) for name, mv in moments.items()}
    radii = max_radii2D.reshape(P) if max_radii2D is not None else xyz.new_zeros(P)
    radii = torch.cat([radii, radii.new_zeros(n_new)])
    origin = torch.cat([rows, rows[clone], rows[split], rows[split]])
    fresh = torch.cat([torch.zeros(P, dtype=torch.bool, device=dev), torch.ones(n_new, dtype=torch.bool, device=dev)])
    group = torch.cat([torch.zeros(P, dtype=torch.long, device=dev), torch.ones(n_clone, dtype=torch.long, device=dev),
                       torch.full((2 * n_split,), 2, dtype=torch.long, device=dev)])
    xyz_slack = torch.cat([torch.zeros((P + n_clone, 3), dtype=torch.float64, device=dev)] + slack)

    # 3. the split originals go, 4. the prune over everything that is left
    keep = ~torch.cat([split, torch.zeros(n_new, dtype=torch.bool, device=dev)])
    prune = out["opacity"].reshape(-1) < f32(math.log(min_opacity / (1.0 - min_opacity)), dev)
    if max_screen_size is not None:
        prune = prune | (radii > f32(max_screen_size, dev))
        prune = prune | (out["scaling"].max(dim=1).values > f32(math.log(0.1 * extent), dev))
    keep = keep & ~prune
    out = {name: t[keep] for name, t in out.items()}
    mom = {name: tuple(x[keep] for x in mv) for name, mv in mom.items()}
    group = group[keep]
    counts = (int(keep.sum()), int((group == 0).sum()), int((group == 1).sum()), int((group == 2).sum()), n_split)
    return dict(leaves=out, moments=mom, counts=counts, origin=origin[keep], fresh=fresh[keep], xyz_slack=xyz_slack[keep])
