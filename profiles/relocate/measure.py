#!/usr/bin/env python3
"""Times the fixed-size map upkeep at the mapping benchmark's size (P = 500 000, one [P, 16, 3] feature tensor, all five leaves
with Adam moments, three accumulators; 1 % of the rows dead): relocate_dead and inject_position_noise, and the relocation written
with torch ops on the GPU as a caller of gsplat's MCMCStrategy would write it (multinomial, bincount, indexed writes, one host read
of the dead count).  Both relocations work in place, so the opacity and scale are put back before every call, outside the timed
region; the two are timed alternately, call by call, with device events.

  python profiles/relocate/measure.py [--rows 500000] [--calls 30] [--count-launches] [--out profiles/relocate/measure.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "diff-gaussian-rasterization_amd")]

import torch  # noqa: E402

from dgr_amd.optim import SparseAdam, inject_position_noise, relocate_dead  # noqa: E402

NAMES = ("xyz", "features", "opacity", "scaling", "rotation")
MIN_OPACITY = 0.005


def make(P, dev, dead=0.01, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = {"xyz": 3.0 * torch.randn((P, 3), generator=g), "features": torch.randn((P, 16, 3), generator=g),
         "opacity": (2.0 * torch.randn((P, 1), generator=g)).clamp_min(-4.5),
         "scaling": 0.7 * torch.randn((P, 3), generator=g) - 3.0, "rotation": torch.randn((P, 4), generator=g)}
    L["opacity"] = torch.where(torch.rand((P, 1), generator=g) < dead, torch.full((P, 1), -8.0), L["opacity"])
    L = {n: t.to(dev) for n, t in L.items()}
    M = {n: (torch.randn_like(t), torch.rand_like(t)) for n, t in L.items()}
    A = {"xyz_gradient_accum": torch.rand((P, 1), device=dev), "denom": torch.ones((P, 1), device=dev),
         "max_radii2D": torch.rand(P, device=dev)}
    return L, M, A


def torch_relocate(L, M, A, min_opacity=MIN_OPACITY):
    """the same step in torch ops: fp32 sampling weights, the new opacity and scale in float64"""
    op = L["opacity"].reshape(-1)
    dead = op < math.log(min_opacity / (1.0 - min_opacity))
    n_dead = int(dead.sum())  # the host read
    if n_dead == 0:
        return 0
    dead_idx, live_idx = dead.nonzero().squeeze(1), (~dead).nonzero().squeeze(1)
    src = live_idx[torch.multinomial(torch.sigmoid(op[live_idx]), n_dead, replacement=True)]
    hits = torch.bincount(src, minlength=op.shape[0])
    hit_idx = hits.nonzero().squeeze(1)
    N = (hits[hit_idx] + 1).clamp_max(51)
    o = torch.sigmoid(op[hit_idx].double())
    o1 = 1.0 - (1.0 - o) ** (1.0 / N.double())
    D = torch.zeros_like(o)
    for m in range(1, int(N.max()) + 1):  # (a second host read: how far the table goes)
        inner = sum(math.comb(m - 1, k) * (-1.0) ** k / math.sqrt(k + 1) * o1 ** (k + 1) for k in range(m))
        D += torch.where(N >= m, inner, torch.zeros_like(inner))
    o1c = o1.clamp(min_opacity, 1.0 - 2.0 ** -23)
    L["opacity"].reshape(-1)[hit_idx] = torch.log(o1c / (1.0 - o1c)).float()
    L["scaling"][hit_idx] = (L["scaling"][hit_idx].double() + torch.log(o / D).unsqueeze(1)).float()
    for name, t in L.items():
        t[dead_idx] = t[src]
        for mom in M[name]:
            mom[dead_idx] = 0.0
            mom[hit_idx] = 0.0
    for t in A.values():
        t.reshape(-1)[dead_idx] = 0.0
    return n_dead


def count_launches(fn):
    """GPU kernels one call launches (torch.profiler); None where the profiler is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0)) > 0)
    except Exception as e:  # noqa: BLE001
        print("count_launches:", e, file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--count-launches", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P = args.rows
    L, M, A = make(P, dev)
    saved = {n: L[n].clone() for n in ("opacity", "scaling")}
    opt = SparseAdam(list(L.values()))
    opt.state = {L[n]: M[n] for n in NAMES}
    step = [0]

    def restore():
        for n, t in saved.items():
            L[n].copy_(t)

    def fused():
        step[0] += 1
        return relocate_dead(L, opt, min_opacity=MIN_OPACITY, seed=1, step=step[0], **A)

    def noise():
        inject_position_noise(L, 1.6e-4, seed=2, step=step[0])

    def torch_ops():
        return torch_relocate(L, M, A)

    restore()
    counts = fused().counts.tolist()
    restore()
    assert torch_ops() == counts[0] == counts[2], counts
    res = dict(rows=P, tensors=len(NAMES) * 3 + len(A), counts=counts[:5])
    times = {"relocate_dead": [], "torch_restatement": [], "inject_position_noise": []}
    for call in range(5 + args.calls):
        for name, fn in (("relocate_dead", fused), ("torch_restatement", torch_ops), ("inject_position_noise", noise)):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if call >= 5:
                times[name].append(e0.elapsed_time(e1))
    for name, ms in times.items():
        res[name] = dict(median_us=1e3 * statistics.median(ms), min_us=1e3 * min(ms), max_us=1e3 * max(ms), calls=len(ms))
    res["torch_over_fused"] = res["torch_restatement"]["median_us"] / res["relocate_dead"]["median_us"]
    if args.count_launches:
        for name, fn in (("relocate_dead", fused), ("torch_restatement", torch_ops), ("inject_position_noise", noise)):
            restore()
            res[name]["launches"] = count_launches(fn)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
