#!/usr/bin/env python3
"""Host cost of the map steps' Python side: every call at a size whose kernels take a few microseconds (P = 2000 rows), so that
the wall time per call is the host's (the checks of the model, the table of tensors, the way into the C ABI), which is where a
change to dgr_amd/_capi.py, dgr_amd/optim.py or dgr_amd/map_steps.py could cost.  BATCHES batches of CALLS calls each, one
synchronize per batch; per step the median and the minimum over the batches, microseconds per call, as one JSON line.

    python profiles/map_steps/host_calls.py [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "diff-gaussian-rasterization_amd")]

import torch  # noqa: E402

BATCHES, CALLS = 15, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from dgr_amd import optim
    dev, P = torch.device("cuda:0"), 2000
    g = torch.Generator().manual_seed(0)
    shapes = {"xyz": (3,), "features": (16, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
    L = {n: torch.randn((P,) + s, generator=g).to(dev).requires_grad_() for n, s in shapes.items()}
    for t in L.values():
        t.grad = torch.randn_like(t) * 0.01
    radii = torch.randint(-1, 4, (P,), generator=g, dtype=torch.int32).to(dev)
    dmeans2D = torch.randn((P, 3), generator=g).to(dev)
    acc = [torch.zeros((P, 1), device=dev), torch.zeros((P, 1), device=dev), torch.zeros(P, device=dev)]
    adam = optim.SparseAdam(list(L.values()), lr=1e-4)
    adam_capturable = optim.SparseAdam(list(L.values()), lr=1e-4, capturable=True)

    steps = (("SparseAdam.step, 5 tensors", lambda: adam.step()),
             ("SparseAdam.step, visible", lambda: adam.step(visible=radii)),
             ("SparseAdam.step, capturable", lambda: adam_capturable.step()),
             ("add_densification_stats", lambda: optim.add_densification_stats(dmeans2D, radii, *acc)),
             ("relocate_dead, 5 leaves + moments + 3 accumulators",
              lambda: optim.relocate_dead(L, adam, xyz_gradient_accum=acc[0], denom=acc[1], max_radii2D=acc[2])),
             ("inject_position_noise", lambda: optim.inject_position_noise(L, 1.6e-6)))
    res = {}
    for name, fn in steps:
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
