#!/usr/bin/env python3
"""Times densify_and_prune at the mapping benchmark's size (config 3: P = 500 000, one [P, 16, 3] feature tensor, all five
leaves with Adam moments; about 30 % of the rows hot, 5 % pruned): the fused call, its apply kernel alone, and the same step
written with torch masks, `cat` and boolean indexing on the GPU.  Device events around each call, after warm-up.

  python profiles/densify/measure.py [--rows 500000] [--calls 30] [--out profiles/densify/measure.json]
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

from dgr_amd import _capi  # noqa: E402
from dgr_amd.optim import SparseAdam, densify_and_prune, densify_thresholds  # noqa: E402

NAMES = ("xyz", "features", "opacity", "scaling", "rotation")


def make(P, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = {"xyz": 3.0 * torch.randn((P, 3), generator=g), "features": torch.randn((P, 16, 3), generator=g),
         "opacity": 2.0 * torch.randn((P, 1), generator=g).abs(),
         "scaling": 0.7 * torch.randn((P, 3), generator=g) - 3.0, "rotation": torch.randn((P, 4), generator=g)}
    # 5 % of the rows below logit(0.005) = -5.3; about 40 % of the hot rows are larger than log(0.01 * 10) = -2.3 and split
    L["opacity"] = torch.where(torch.rand((P, 1), generator=g) < 0.05, torch.full((P, 1), -8.0), L["opacity"])
    denom = torch.randint(1, 5, (P, 1), generator=g).float()
    accum = torch.where(torch.rand((P, 1), generator=g) < 0.30, 1e-3 * denom, 1e-5 * denom)  # 30 % hot at 2e-4
    maxr = torch.floor(torch.rand(P, generator=g) * 15.0)
    L = {n: t.to(dev) for n, t in L.items()}
    M = {n: (torch.randn_like(t), torch.rand_like(t)) for n, t in L.items()}
    return L, M, accum.to(dev), denom.to(dev), maxr.to(dev)


def torch_densify(L, M, accum, denom, maxr, noise, thr):
    """the sequence in torch, fp32, as a caller of 3DGS's GaussianModel would write it (moments rebuilt tensor by tensor)"""
    grad_thr, op_min, ls_split, ls_prune, mss = (torch.tensor(v, dtype=torch.float32, device=accum.device) for v in thr)
    P = accum.shape[0]
    a, d = accum.reshape(P), denom.reshape(P)
    hot = (d > 0) & (a >= grad_thr * d)
    m = L["scaling"].max(dim=1).values
    split = hot & (m > ls_split)
    clone = hot & ~split
    q = torch.nn.functional.normalize(L["rotation"][split])
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z),
                     1 - 2 * (x * x + z * z), 2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x),
                     1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    spread = torch.exp(L["scaling"][split])
    kids = [L["xyz"][split] + torch.bmm(R, (spread * noise[split, s]).unsqueeze(-1)).squeeze(-1) for s in (0, 1)]
    n_new = int(clone.sum()) + 2 * int(split.sum())
    out = {}
    for name, t in L.items():
        if name == "xyz":
            out[name] = torch.cat([t, t[clone]] + kids)
        elif name == "scaling":
            child = t[split] - math.log(1.6)
            out[name] = torch.cat([t, t[clone], child, child])
        else:
            out[name] = torch.cat([t, t[clone], t[split], t[split]])
    radii = torch.cat([maxr, maxr.new_zeros(n_new)])
    keep = ~torch.cat([split, split.new_zeros(n_new)])
    keep &= ~((out["opacity"].reshape(-1) < op_min) | (radii > mss) | (out["scaling"].max(dim=1).values > ls_prune))
    out = {name: t[keep] for name, t in out.items()}
    mom = {name: tuple(torch.cat([x, x.new_zeros((n_new,) + tuple(x.shape[1:]))])[keep] for x in mv) for name, mv in M.items()}
    P_new = out["xyz"].shape[0]
    zeros = [torch.zeros((P_new, 1), device=a.device), torch.zeros((P_new, 1), device=a.device), torch.zeros(P_new, device=a.device)]
    masks = dict(survive=keep[:P], clone=clone, split=split)
    return out, mom, zeros, masks


def timed(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), calls=calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P = args.rows
    L, M, accum, denom, maxr = make(P, dev)
    noise = torch.randn((P, 2, 3), device=dev)
    kw = dict(grad_threshold=2e-4, extent=10.0, percent_dense=0.01, min_opacity=0.005, max_screen_size=20.0)
    thr = densify_thresholds(**kw)

    def fused():
        params = {n: t for n, t in L.items()}
        opt = SparseAdam(list(params.values()))
        opt.state = {params[n]: M[n] for n in NAMES}
        return densify_and_prune(params, opt, accum, denom, maxr, noise=noise, **kw)

    out, _, _, _, counts = fused()
    ref, ref_mom, _, masks = torch_densify(L, M, accum, denom, maxr, noise, thr)
    assert counts.rows == ref["xyz"].shape[0], (counts, ref["xyz"].shape)
    for n in NAMES:
        if n != "xyz":
            assert torch.equal(out[n], ref[n]), n
    assert torch.allclose(out["xyz"], ref["xyz"], rtol=1e-5, atol=1e-5)

    # the apply kernel alone: the same 18-tensor table (5 leaves, 10 moments, 3 accumulators) on a plan made once
    lib, st = _capi.load(), _capi.stream_handle()
    plan = torch.empty(lib.dgr_densify_plan_bytes(P), dtype=torch.uint8, device=dev)
    cdev = torch.empty(8, dtype=torch.int32, device=dev)

    def plan_only():
        rc = lib.dgr_densify_plan(st, P, accum.data_ptr(), denom.data_ptr(), maxr.data_ptr(), L["opacity"].data_ptr(),
                                  L["scaling"].data_ptr(), *thr, plan.data_ptr(), cdev.data_ptr())
        assert rc == 0, _capi.last_error()

    plan_only()
    P_new = int(cdev[0])
    table, keepalive = [], []
    mode_of = {"xyz": _capi.DENSIFY_XYZ, "scaling": _capi.DENSIFY_LOG_SCALE}
    for n in NAMES:
        k = L[n].numel() // P
        for src, mode in ((L[n], mode_of.get(n, _capi.DENSIFY_COPY)), (M[n][0], _capi.DENSIFY_ZERO_NEW), (M[n][1], _capi.DENSIFY_ZERO_NEW)):
            dst = torch.empty((P_new, k), device=dev)
            keepalive.append(dst)
            table.append((src.data_ptr(), dst.data_ptr(), k, mode))
    for _ in range(3):
        dst = torch.empty((P_new, 1), device=dev)
        keepalive.append(dst)
        table.append((None, dst.data_ptr(), 1, _capi.DENSIFY_ZERO))
    descs = (_capi.DensifyTensor * len(table))()
    for d, (s, t, k, mode) in zip(descs, table):
        d.src, d.dst, d.k, d.mode = s, t, k, mode

    def apply_only():
        rc = lib.dgr_densify_apply(st, P, P_new, plan.data_ptr(), len(table), descs, L["scaling"].data_ptr(),
                                   L["rotation"].data_ptr(), noise.data_ptr(), 0)
        assert rc == 0, _capi.last_error()

    # algorithmic bytes of the apply: every source row that is emitted read once (moments: surviving rows only), every
    # destination element written once, the XYZ inputs of the split rows whose children stay, one plan byte per row
    s_, c_, sp_ = masks["survive"], masks["clone"], masks["split"]
    pairs = counts.children // 2
    emitted = int((s_ | c_).sum()) + pairs  # rows with a survivor or a kept clone, + split rows with kept children
    n_surv = counts.survivors
    alg = P + P // 16
    for s, t, k, mode in table:
        reads = 0 if mode == _capi.DENSIFY_ZERO else n_surv if mode == _capi.DENSIFY_ZERO_NEW else emitted
        alg += 4 * k * (reads + P_new)
    alg += pairs * 4 * (3 + 4 + 6)

    res = dict(rows=P, rows_out=P_new, counts=counts._asdict(), hot_fraction=float((c_ | sp_).float().mean()),
               pruned_fraction=1.0 - (counts.survivors + int(sp_.sum())) / P, tensors=len(table),
               apply_algorithmic_bytes=alg, apply_algorithmic_bytes_per_row=alg / P)
    res["fused_call"] = timed(fused, args.calls)
    res["plan_kernels"] = timed(plan_only, args.calls)
    res["apply_kernel"] = timed(apply_only, args.calls)
    res["torch_restatement"] = timed(lambda: torch_densify(L, M, accum, denom, maxr, noise, thr), args.calls)
    res["apply_TB_per_s"] = alg / (res["apply_kernel"]["median_ms"] * 1e-3) / 1e12
    res["apply_TB_per_s_best"] = alg / (res["apply_kernel"]["min_ms"] * 1e-3) / 1e12
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
