#!/usr/bin/env python3
"""Times seed_from_frame at two keyframe sizes -- 640 x 480 onto P = 100 000 and 1920 x 1080 onto P = 500 000, six leaves
(xyz, f_dc, f_rest, opacity, scaling, rotation) with their Adam moments = 18 tensors, about 20 % of the pixels selected by the
silhouette: the fused call, its decide + scan and its apply kernel alone, and the same step written with torch masks, `nonzero`,
elementwise ops and `cat` on the GPU.  Device events around each call, the median of --calls after warm-up, each variant in a
timed run of its own.

  python profiles/seed/measure.py [--calls 30] [--out profiles/seed/measure.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "diff-gaussian-rasterization_amd")]

import torch  # noqa: E402

from dgr_amd import _capi  # noqa: E402
from dgr_amd.optim import SparseAdam, seed_constants, seed_from_frame  # noqa: E402

SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
WORKLOADS = {"640x480_onto_100k": (640, 480, 100_000), "1920x1080_onto_500k": (1920, 1080, 500_000)}
THRESHOLD = 0.2  # of a uniform silhouette: 20 % of the pixels are unseen
INV_C0 = 1.0 / 0.28209479177387814


def make(W, H, P, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = {n: torch.randn((P,) + shape, generator=g).to(dev) for n, shape in SHAPES.items()}
    M = {n: (torch.randn_like(t), torch.rand_like(t)) for n, t in L.items()}
    frame = dict(color_obs=torch.rand((3, H, W), generator=g).to(dev), depth_obs=(1.0 + 2.0 * torch.rand((H, W), generator=g)).to(dev),
                 opacity_map=torch.rand((H, W), generator=g).to(dev))
    view = torch.eye(4)
    view[3, :3] = torch.tensor([0.05, -0.02, 0.10])
    c, s = 0.9553365, 0.2955202  # a rotation by 0.3 rad about y
    view[0, 0], view[0, 2], view[2, 0], view[2, 2] = c, -s, s, c
    K = (0.9 * W, 0.8 * W, (W - 1) / 2 + 3.0, (H - 1) / 2 - 2.0)
    return L, M, frame, view.to(dev), K


def torch_seed(L, M, frame, view, K, consts):
    """the step in torch, fp32, as a caller would write it (masks, nonzero, elementwise ops, one cat per leaf and per moment)"""
    fx, fy, cx, cy = K
    depth_min, depth_max, threshold, _, pix, opacity_raw = consts
    depth_obs, dev = frame["depth_obs"], frame["depth_obs"].device
    select = (depth_obs > depth_min) & (depth_obs < depth_max) & (frame["opacity_map"] < threshold)
    yx = torch.nonzero(select)
    y, x = yx[:, 0], yx[:, 1]
    n = yx.shape[0]
    d = depth_obs[y, x]
    p = torch.stack([(x.float() - cx) / fx * d, (y.float() - cy) / fy * d, d], dim=1)
    new = {"xyz": (p - view[3, :3]) @ view[:3, :3].T, "scaling": torch.log(d * pix).unsqueeze(1).expand(n, 3),
           "rotation": torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).expand(n, 4),
           "opacity": torch.full((n, 1), opacity_raw, device=dev),
           "f_dc": ((frame["color_obs"][:, y, x].T - 0.5) * INV_C0).reshape(n, 1, 3), "f_rest": torch.zeros((n, 15, 3), device=dev)}
    out = {name: torch.cat([t, new[name]]) for name, t in L.items()}
    mom = {name: tuple(torch.cat([m, m.new_zeros((n,) + tuple(m.shape[1:]))]) for m in mv) for name, mv in M.items()}
    return out, mom


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


def measure(W, H, P, calls, dev):
    L, M, frame, view, K = make(W, H, P, dev)
    consts = seed_constants(K[0], K[1], silhouette_threshold=THRESHOLD)
    kw = dict(opacity_map=frame["opacity_map"], silhouette_threshold=THRESHOLD)

    def fused():
        opt = SparseAdam(list(L.values()))
        opt.state = {L[n]: M[n] for n in L}
        return seed_from_frame(L, opt, frame["color_obs"], frame["depth_obs"], view, *K, **kw), opt

    (out, _, _, _, counts), opt = fused()
    ref, ref_mom = torch_seed(L, M, frame, view, K, consts)
    assert counts.rows == ref["xyz"].shape[0], (counts, ref["xyz"].shape)
    for n in L:
        if n in ("xyz", "scaling"):
            assert torch.allclose(out[n], ref[n], rtol=1e-5, atol=1e-5), n
        else:
            assert torch.equal(out[n], ref[n]), n
        assert torch.equal(opt.state[out[n]][0], ref_mom[n][0]) and torch.equal(opt.state[out[n]][1], ref_mom[n][1]), n

    # the kernels alone: the same 18-tensor table on a plan made once
    lib, st = _capi.load(), _capi.stream_handle()
    plan = torch.empty(lib.dgr_seed_plan_bytes(W, H, 1), dtype=torch.uint8, device=dev)
    cdev = torch.empty(8, dtype=torch.int32, device=dev)

    def plan_only():
        rc = lib.dgr_seed_plan(st, W, H, 1, frame["depth_obs"].data_ptr(), frame["opacity_map"].data_ptr(), None, consts[0], consts[1],
                               consts[2], consts[3], None, P, plan.data_ptr(), cdev.data_ptr())
        assert rc == 0, _capi.last_error()

    plan_only()
    P_new = int(cdev[0])
    assert P_new == counts.rows
    mode_of = {"xyz": (_capi.SEED_XYZ, 0.0), "scaling": (_capi.SEED_LOG_SCALE, 0.0), "rotation": (_capi.SEED_QUAT_IDENTITY, 0.0),
               "opacity": (_capi.SEED_CONST, consts[5]), "f_dc": (_capi.SEED_RGB_DC, 0.0)}
    table, keepalive = [], []
    for n, t in L.items():
        k = t.numel() // P
        for src, (mode, value) in ((t, mode_of.get(n, (_capi.SEED_CONST, 0.0))), (M[n][0], (_capi.SEED_CONST, 0.0)),
                                   (M[n][1], (_capi.SEED_CONST, 0.0))):
            dst = torch.empty((P_new, k), device=dev)
            keepalive.append(dst)
            table.append((src.data_ptr(), dst.data_ptr(), k, mode, value))
    descs = (_capi.SeedTensor * len(table))()
    for d, (s, t, k, mode, value) in zip(descs, table):
        d.src, d.dst, d.k, d.mode, d.value = s, t, k, mode, value

    def apply_only():
        rc = lib.dgr_seed_apply(st, W, H, 1, P, P_new, plan.data_ptr(), len(table), descs, frame["color_obs"].data_ptr(),
                                frame["depth_obs"].data_ptr(), view.data_ptr(), *K, consts[4])
        assert rc == 0, _capi.last_error()

    # algorithmic bytes of the apply: every old row read once and every destination element written once; one flag byte per
    # candidate and one 16-byte record per 256 of them; per new row its observed depth (4 B) and colour (12 B)
    cands, n_new = W * H, counts.new
    copy_bytes = sum(4 * k * 2 * P for _, _, k, _, _ in table)
    new_bytes = sum(4 * k * n_new for _, _, k, _, _ in table) + cands + cands // 16 + 16 * n_new
    alg = copy_bytes + new_bytes
    res = dict(width=W, height=H, rows=P, rows_out=P_new, counts=counts._asdict(), selected_fraction=n_new / cands, tensors=len(table),
               apply_algorithmic_bytes=alg, apply_copy_bytes=copy_bytes, apply_new_row_bytes=new_bytes)
    res["fused_call"] = timed(lambda: fused(), calls)
    res["plan_kernels"] = timed(plan_only, calls)
    res["apply_kernel"] = timed(apply_only, calls)
    res["torch_restatement"] = timed(lambda: torch_seed(L, M, frame, view, K, consts), calls)
    res["apply_TB_per_s"] = alg / (res["apply_kernel"]["median_ms"] * 1e-3) / 1e12
    res["apply_TB_per_s_best"] = alg / (res["apply_kernel"]["min_ms"] * 1e-3) / 1e12
    res["fused_over_torch"] = res["fused_call"]["median_ms"] / res["torch_restatement"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {name: measure(W, H, P, args.calls, dev) for name, (W, H, P) in WORKLOADS.items()}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for name, r in res.items():
        assert r["fused_over_torch"] <= 1.0, f"{name}: the fused call is slower than the torch restatement"


if __name__ == "__main__":
    main()
