#!/usr/bin/env python3
"""Hashes of every output of the map steps and the optimiser on seeded inputs: run on the parent and on the change, the two files
must be identical (no tolerance: the steps promise the same bits).  One line per step and case with the number of outputs under
it; --full: one line per output, to find the one that differs.
  densify_and_prune        P = 66003, Philox noise and given noise         leaves, moments, accumulators, counts
  seed_from_frame          300 x 220 at stride 1 and 3 onto P = 1000       leaves, moments, accumulators, counts
  relocate_dead            P = 0 / 1 / 257 / 300 / 549 / 65537, Philox draws and given draws
                                                                           leaves, moments, accumulators, counts, source
  inject_position_noise    the same P, Philox noise and given noise        xyz
  SparseAdam.step          P = 300 and 65537, plain / visible / capturable, two steps
                                                                           parameters, moments
  add_densification_stats  P = 300 and 66003                               the three accumulators

    python profiles/map_steps/bits.py --out FILE [--full]
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "diff-gaussian-rasterization_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

NAMES = ("xyz", "features", "opacity", "scaling", "rotation", "f_dc")
SHAPES = {"xyz": (3,), "features": (5, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,), "f_dc": (1, 3)}


def model(P, dev, seed, dead=0.05):
    """leaves (a twentieth of the opacities far below the threshold), an optimiser that has moments, the three accumulators"""
    from dgr_amd.optim import SparseAdam
    g = torch.Generator().manual_seed(seed)
    L = {n: torch.randn((P,) + SHAPES[n], generator=g) for n in NAMES}
    L["scaling"] = 0.7 * L["scaling"] - 3.0
    L["opacity"] = torch.where(torch.rand((P, 1), generator=g) < dead, torch.full((P, 1), -8.0), 2.0 * L["opacity"])
    L = {n: t.to(dev).requires_grad_(n != "f_dc") for n, t in L.items()}
    adam = SparseAdam(list(L.values()), lr=0.01)
    adam.state = {t: (torch.randn(t.shape, generator=g).to(dev), torch.rand(t.shape, generator=g).to(dev)) for t in L.values()}
    adam.steps = 3
    A = [torch.rand((P, 1), generator=g).to(dev) * 0.01, torch.randint(0, 3, (P, 1), generator=g).float().to(dev),
         (40.0 * torch.rand(P, generator=g)).to(dev)]
    return L, adam, A, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--full", action="store_true")
    args = ap.parse_args()
    from dgr_amd import optim
    dev = torch.device("cuda:0")
    lines = []

    def put(name, t):
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        lines.append(f"{name} {a.dtype} {list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()[:24]}")

    def put_model(tag, L, adam, A):
        for n, t in L.items():
            put(f"{tag}/{n}", t)
            for k, m in enumerate(adam.state.get(t, ())):
                put(f"{tag}/{n}.moment{k}", m)
        for k, t in enumerate(A):
            if t is not None:
                put(f"{tag}/accumulator{k}", t)

    P = 66003
    for given in (False, True):
        L, adam, A, g = model(P, dev, 1)
        noise = torch.randn((P, 2, 3), generator=g).to(dev) if given else None
        L, a0, a1, a2, counts = optim.densify_and_prune(L, adam, *A, grad_threshold=0.004, extent=4.0, percent_dense=0.01,
                                                        min_opacity=0.005, max_screen_size=38.0, noise=noise, seed=7)
        tag = f"densify_and_prune/P{P}_{'given' if given else 'philox'}"
        put_model(tag, L, adam, (a0, a1, a2))
        put(f"{tag}/counts", torch.tensor(list(counts)))

    W, H = 300, 220
    for stride in (1, 3):
        L, adam, A, g = model(1000, dev, 2)
        depth_obs = torch.rand((H, W), generator=g) * 4.0
        depth_obs[torch.rand((H, W), generator=g) < 0.1] = 0.0
        viewmatrix = torch.eye(4)
        viewmatrix[3, :3] = torch.tensor([0.1, -0.2, 0.3])
        L, a0, a1, a2, counts = optim.seed_from_frame(
            L, adam, torch.rand((3, H, W), generator=g).to(dev), depth_obs.to(dev), viewmatrix.to(dev), 250.0, 240.0, 149.5, 109.5,
            opacity_map=torch.rand((H, W), generator=g).to(dev), depth=(torch.rand((H, W), generator=g) * 4.0).to(dev),
            silhouette_threshold=0.5, depth_error_min=0.6, depth_range=(0.2, 3.8), stride=stride, fill={"features": 0.25},
            xyz_gradient_accum=A[0], denom=A[1], max_radii2D=A[2])
        tag = f"seed_from_frame/{W}x{H}_stride{stride}"
        put_model(tag, L, adam, (a0, a1, a2))
        put(f"{tag}/counts", torch.tensor(list(counts)))

    for P in (0, 1, 257, 300, 549, 65537):
        for given in (False, True):
            L, adam, A, g = model(P, dev, 3 + P)
            draws = torch.randint(0, 2 ** 32, (P,), generator=g, dtype=torch.int64).to(dev) if given else None
            res = optim.relocate_dead(L, adam, min_opacity=0.005, draws=draws, seed=11, step=2, xyz_gradient_accum=A[0], denom=A[1],
                                      max_radii2D=A[2])
            tag = f"relocate_dead/P{P}_{'given' if given else 'philox'}"
            put_model(tag, L, adam, A)
            put(f"{tag}/counts", res.counts)
            put(f"{tag}/source", res.source)
            noise = torch.randn((P, 3), generator=g).to(dev) if given else None
            optim.inject_position_noise(L, 1.6e-4, noise=noise, seed=13, step=5)
            put(f"inject_position_noise/P{P}_{'given' if given else 'philox'}/xyz", L["xyz"])

    for P in (300, 65537, 66003):
        g = torch.Generator().manual_seed(P)
        radii = torch.randint(-1, 4, (P,), generator=g, dtype=torch.int32).to(dev)
        if P != 66003:
            for form in ("plain", "visible", "capturable"):
                params = [torch.randn((P, 3), generator=g).to(dev).requires_grad_(), torch.randn((P, 1), generator=g).to(dev).requires_grad_()]
                adam = optim.SparseAdam(params, lr=0.01, capturable=form == "capturable")
                for _ in range(2):
                    for p in params:
                        p.grad = torch.randn(p.shape, generator=g).to(dev)
                    adam.step(visible=None if form == "plain" else radii)
                for k, p in enumerate(params):
                    put(f"SparseAdam.step/P{P}_{form}/param{k}", p)
                    put(f"SparseAdam.step/P{P}_{form}/param{k}.moment0", adam.state[p][0])
                    put(f"SparseAdam.step/P{P}_{form}/param{k}.moment1", adam.state[p][1])
        if P != 65537:
            acc = [torch.rand((P, 1), generator=g).to(dev), torch.rand((P, 1), generator=g).to(dev), torch.rand(P, generator=g).to(dev)]
            optim.add_densification_stats((torch.randn((P, 3), generator=g)).to(dev), radii, *acc)
            for k, t in enumerate(acc):
                put(f"add_densification_stats/P{P}/accumulator{k}", t)

    torch.cuda.synchronize()
    n_outputs = len(lines)
    if not args.full:  # step/case -> the hash of its outputs' lines
        groups = {}
        for l in lines:
            groups.setdefault("/".join(l.split("/")[:2]), []).append(l)
        lines = [f"{k} {len(v)} outputs {hashlib.sha256(chr(10).join(v).encode()).hexdigest()[:24]}" for k, v in groups.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{n_outputs} outputs, {len(lines)} lines -> {args.out}")


if __name__ == "__main__":
    main()
