#!/usr/bin/env python3
"""Times the map correction at the mapping benchmark's size: P = 500 000 Gaussians of degree 3 (xyz, scaling, rotation, opacity,
f_dc, f_rest [P, 15, 3], anchor), all with Adam moments, K = 200 rigid transforms.  transform_map is recorded into a hipGraph (plan,
counts and apply: four launches; the plan alone is timed as well, the apply is the difference) and the replays are timed with device events, a window of `--replays` replays at a time; once with
the anchors in runs (a keyframe's rows lie together, as seeding leaves them: the wave-uniform path) and once with the anchors
shuffled (every lane its own record).  The step works in place, so a replay transforms what the last one left: the transforms are
rigid, which keeps every value bounded.  The algorithmic bytes are one read and one write of every tensor in the table plus one
read of the anchors: P x (159 x 8 + 4).

The baseline is the same per-row work written in torch ops, as a user without the step would write it: gather the row's record,
einsum the positions, the quaternion product, the three SH bands and the moments.  The per-transform part (scale, quaternion, the
band matrices) is taken from the float64 model on the host and NOT timed, which favours the baseline.

  python profiles/transform/measure.py [--rows 500000] [--transforms 200] [--windows 9] [--replays 20] [--out measure.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import transform_model as tm  # noqa: E402
from dgr_amd import _capi  # noqa: E402
from dgr_amd.optim import SparseAdam, transform_map  # noqa: E402

FLOATS_PER_ROW = 3 * 3 + 3 * 4 + 3 + 3 * 45  # xyz, rotation (value + two moments each), scaling, f_rest (value + two moments)


def make(P, K, dev, runs, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = {"xyz": 3.0 * torch.randn((P, 3), generator=g), "scaling": 0.7 * torch.randn((P, 3), generator=g) - 3.0,
         "rotation": torch.randn((P, 4), generator=g), "opacity": torch.randn((P, 1), generator=g),
         "f_dc": torch.randn((P, 1, 3), generator=g), "f_rest": 0.1 * torch.randn((P, 15, 3), generator=g)}
    anchor = torch.arange(P) * K // P if runs else torch.randint(0, K, (P,), generator=g)
    L["anchor"] = anchor.float()
    L = {n: t.to(dev) for n, t in L.items()}
    M = {n: (torch.randn_like(t), torch.rand_like(t)) for n, t in L.items() if n != "anchor"}
    rng = np.random.RandomState(seed)
    transforms = np.stack([tm.random_sim3(rng, 1.0, 0.01) for _ in range(K)])
    return L, M, transforms


def torch_records(transforms, dev):
    plans = [tm.plan_model(T) for T in transforms]
    f = lambda a: torch.from_numpy(np.stack(a).astype(np.float32)).to(dev)  # noqa: E731
    return dict(A=f([p["A"] for p in plans]), t=f([p["t"] for p in plans]), R=f([p["R"] for p in plans]),
                L=f([tm.quat_left(p["q"]) for p in plans]), inv_s=f([1.0 / p["s"] for p in plans]), log_s=f([p["log_s"] for p in plans]),
                M={l: f([p["M"][l] for p in plans]) for l in (1, 2, 3)})


def torch_transform(L, M, rec):
    idx = L["anchor"].long()
    A, R, Lq, inv_s = rec["A"][idx], rec["R"][idx], rec["L"][idx], rec["inv_s"][idx].unsqueeze(1)
    L["xyz"].copy_(torch.einsum("pij,pj->pi", A, L["xyz"]) + rec["t"][idx])
    M["xyz"][0].copy_(torch.einsum("pij,pj->pi", R, M["xyz"][0]) * inv_s)
    M["xyz"][1].copy_(torch.einsum("pij,pj->pi", R * R, M["xyz"][1]) * inv_s * inv_s)
    L["rotation"].copy_(torch.einsum("pij,pj->pi", Lq, L["rotation"]))
    M["rotation"][0].copy_(torch.einsum("pij,pj->pi", Lq, M["rotation"][0]))
    M["rotation"][1].copy_(torch.einsum("pij,pj->pi", Lq * Lq, M["rotation"][1]))
    L["scaling"].add_(rec["log_s"][idx].unsqueeze(1))
    for l, lo, hi in ((1, 0, 3), (2, 3, 8), (3, 8, 15)):
        W = rec["M"][l][idx]
        for t, w in ((L["f_rest"], W), (M["f_rest"][0], W), (M["f_rest"][1], W * W)):
            t[:, lo:hi] = torch.einsum("pij,pjc->pic", w, t[:, lo:hi])


def recorded(dev, fn):
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    return graph


def windows(fn, n_windows, per_window):
    ms = []
    for w in range(n_windows + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_window):
            fn()
        e1.record()
        e1.synchronize()
        if w >= 2:  # (two windows of warm-up)
            ms.append(e0.elapsed_time(e1) / per_window)
    return dict(median_us=1e3 * statistics.median(ms), min_us=1e3 * min(ms), max_us=1e3 * max(ms), windows=len(ms), per_window=per_window)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500000)
    ap.add_argument("--transforms", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P, K = args.rows, args.transforms
    nbytes = P * (FLOATS_PER_ROW * 8 + 4)
    res = dict(rows=P, transforms=K, algorithmic_bytes=nbytes, peak_TBps=8.0)
    for label, runs in (("anchors_in_runs", True), ("anchors_shuffled", False)):
        L, M, transforms = make(P, K, dev, runs)
        opt = SparseAdam([{"params": [t], "lr": 1e-3} for n, t in L.items() if n != "anchor"])
        opt.state = {L[n]: M[n] for n in M}
        T = torch.from_numpy(transforms).to(dev)
        counts = transform_map(L, opt, T)
        assert counts.tolist() == [P, 0, 0, 0], counts.tolist()
        graph = recorded(dev, lambda: transform_map(L, opt, T))
        r = windows(graph.replay, args.windows, args.replays)
        r["TBps"] = nbytes / (r["median_us"] * 1e-6) / 1e12
        r["share_of_peak"] = r["TBps"] / res["peak_TBps"]
        res[label] = r
        rec = torch_records(transforms, dev)
        torch_transform(L, M, rec)
        res[label + "_torch_ops"] = windows(lambda: torch_transform(L, M, rec), max(args.windows // 3, 3), max(args.replays // 4, 2))
        res[label + "_torch_over_fused"] = res[label + "_torch_ops"]["median_us"] / r["median_us"]
        del graph
    # the plan alone (the transforms' launch and the one-workgroup count): what of a call is not the apply
    scratch = torch.empty(_capi.load().dgr_transform_scratch_bytes(K), dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    plan = lambda: _capi.call("dgr_transform_plan", dev, K, T.data_ptr(), scratch.data_ptr(), counts.data_ptr())  # noqa: E731
    plan()
    graph = recorded(dev, plan)
    res["plan_only"] = windows(graph.replay, args.windows, args.replays)
    for label in ("anchors_in_runs", "anchors_shuffled"):
        apply_us = res[label]["median_us"] - res["plan_only"]["median_us"]
        res[label]["apply_us"] = apply_us
        res[label]["apply_TBps"] = nbytes / (apply_us * 1e-6) / 1e12
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
