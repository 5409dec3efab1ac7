#!/usr/bin/env python3
"""Host cost of the step functions' Python side: every call at a size whose kernels take a few microseconds, so that the wall
time per call is the host's (argument checks, allocations, the way into the C ABI, the kept-tensor lookups of render()), which is
where a change to dgr_amd/_capi.py or to the caches of dgr_amd/slam.py could cost.  BATCHES batches of CALLS calls each, one
synchronize per batch; per step the median and the minimum over the batches, microseconds per call, as one JSON line.

    python profiles/loss_steps/host_calls.py [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd")]
os.environ.setdefault("DGR_SYNC_MODE", "lazy")

import numpy as np  # noqa: E402
import torch  # noqa: E402

BATCHES, CALLS = 15, 200


class Model:
    """the accessors of 3DGS's GaussianModel that slam.render() reads"""

    def __init__(self, s, dev):
        for name, a in (("get_xyz", s.means), ("get_opacity", s.opac), ("get_scaling", s.scales), ("get_rotation", s.rots),
                        ("get_features", s.shs)):
            setattr(self, name, torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        self.active_sh_degree = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from dgr_amd import slam
    from dgr_amd.synth import make_scene
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(s, generator=g).to(dev)  # noqa: E731
    c, d, co, do = r(3, 24, 32).requires_grad_(), r(1, 24, 32).requires_grad_(), r(3, 24, 32), r(1, 24, 32) + 0.5
    q, t = (r(4) + 0.5).requires_grad_(), r(3).requires_grad_()
    weight = r(4, 4)
    kvm = torch.eye(4, device=dev).repeat(8, 1, 1)
    W, H = 64, 64
    scenes = [make_scene(2000, W, H, 3, view_index=k) for k in range(2)]
    s = scenes[0]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    pc, bg, gt = Model(s, dev), T(s.bg), T(s.gt)
    cams = [dict(viewmatrix=T(x.view), fov=(x.tanfovx, x.tanfovy), HW=(H, W), gt_depth=gt) for x in scenes]

    def pose():
        q.grad = t.grad = None
        (slam.pose_to_camera(q, t, 0.6, 0.45)[0] * weight).sum().backward()

    def l1():
        c.grad = d.grad = None
        slam.l1_loss(c, d, co, do).backward()

    def l1_ssim():
        c.grad = d.grad = None
        slam.l1_ssim_loss(c, d, co, do).backward()

    def masked():
        c.grad = d.grad = None
        slam.masked_l1_loss(c, d, co, do).backward()

    def overlap():
        slam.keyframe_overlap(do, kvm[0], kvm, 40.0, 40.0, 16.0, 12.0, stride=4, edge=1.0)

    def render_fixed_pose():  # (a kept pose: the lookup, the stamp's order, the result dict)
        with torch.no_grad():
            slam.render(None, pc, None, bg, viewmatrix=cams[0]["viewmatrix"], fov=cams[0]["fov"], HW=(H, W), gt_depth=gt)

    def render_views_fixed_poses():
        with torch.no_grad():
            slam.render_views(cams, pc, None, bg)

    res = {}
    for name, fn in (("pose_to_camera fwd+bwd", pose), ("l1_loss fwd+bwd", l1), ("l1_ssim_loss fwd+bwd", l1_ssim),
                     ("masked_l1_loss fwd+bwd", masked), ("keyframe_overlap", overlap), ("render, kept pose", render_fixed_pose),
                     ("render_views, kept poses", render_views_fixed_poses)):
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        per = []
        for _ in range(BATCHES):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) / CALLS * 1e6)
        res[name] = dict(median_us=round(statistics.median(per), 2), min_us=round(min(per), 2))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
