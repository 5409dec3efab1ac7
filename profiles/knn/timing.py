"""Timing of dgr_knn_build and dgr_knn_search (self mode, k = 3, the mean_dist2 output: distCUDA2) from hipGraph replays, beside the
same result from torch ops on the same GPU (a chunked cdist + topk), for P = 100 k and 500 k on three point sets: uniform random
points, a surface-like set (a synthetic depth frame unprojected) and that set with one outlier 1000 extents away.  Also, from
the index and the answer: the share of the leaves a wave cannot skip -- the leaves whose bound is not above the FINAL k-th
distance of at least one of its 64 queries, a lower bound of the leaves the sweep visits (it prunes with the current k-th
distance, which is larger early on).  The kernel times are medians of the replays; the torch-ops time is ONE eager run after one
warm-up run (it takes 0.1 - 3 s), so the ratio column compares a median with a single sample.

  python profiles/knn/timing.py [--replays 20] [--sizes 100000 500000]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "diff-gaussian-rasterization_amd"))
from dgr_amd import _capi, knn  # noqa: E402


def uniform(P, dev):
    g = torch.Generator(device="cpu").manual_seed(P)
    return torch.rand((P, 3), generator=g).to(dev)


def surface(P, dev):
    """a 4:3 depth frame of about P pixels: a wavy wall with a step, unprojected through a pinhole"""
    H = int(math.sqrt(P * 3 / 4))
    W = -(-P // H)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = 2.0 + 0.3 * torch.sin(x / W * 9.0) * torch.cos(y / H * 7.0) + (x > 0.6 * W).float() * 0.8
    f = 0.9 * W
    pts = torch.stack([(x - W / 2) / f * z, (y - H / 2) / f * z, z], dim=-1).reshape(-1, 3)[:P]
    return pts.contiguous().to(dev)


def with_outlier(pts):
    pts = pts.clone()
    extent = float((pts.max(dim=0).values - pts.min(dim=0).values).max())
    pts[len(pts) // 2] = pts[len(pts) // 2] + 1000.0 * extent
    return pts


KEEP = []  # the graphs stay alive: what a captured call returned lives in their memory pools


def replay_time(fn, replays):
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = fn()
    KEEP.append(graph)
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return out, float(np.median(times)), float(np.min(times))


def torch_ops(pts, chunk=4096):
    out = torch.empty(len(pts), device=pts.device)
    for a in range(0, len(pts), chunk):
        d = torch.cdist(pts[a:a + chunk], pts)
        out[a:a + chunk] = (d.topk(4, dim=1, largest=False).values[:, 1:] ** 2).mean(dim=1)
    return out


def sample_check(pts, values, n=400):
    """largest relative error of `values` on n sampled rows against float64 brute force (the row itself left out by index)"""
    rows = torch.linspace(0, len(pts) - 1, n, device=pts.device).long()
    p64 = pts.double()
    d2 = ((p64[rows][:, None, :] - p64[None, :, :]) ** 2).sum(dim=-1)
    d2[torch.arange(n, device=pts.device), rows] = float("inf")
    want = d2.topk(3, dim=1, largest=False).values.mean(dim=1)
    return float(((values[rows].double() - want).abs() / want).max())


def index_layout(P):
    """csrc/knn.hip's layout of the opaque index, in one place: a 64-byte header (n_valid: the int at byte 24), P float4 records,
    then two tables of one float4 per 256-record leaf (lo, hi); the total is checked against dgr_knn_index_bytes"""
    B = -(-P // 256)
    lay = dict(n_valid=24, records=64, leaf_lo=64 + 16 * P, leaf_hi=64 + 16 * P + 16 * B, end=64 + 16 * P + 32 * B, leaves=B)
    assert lay["end"] == _capi.load().dgr_knn_index_bytes(P), "the index's layout has changed: update index_layout"
    return lay


def unskippable_share(index, kth, chunk=256):
    """per wave of 64 sorted queries: leaves with bound <= the final k-th distance for at least one lane, over the live leaves"""
    P = index.points.shape[0]
    lay, raw = index_layout(P), index.index
    assert raw.numel() == lay["end"]
    B = lay["leaves"]
    n_valid = int(raw[lay["n_valid"]:lay["n_valid"] + 4].view(torch.int32).item())
    assert 0 <= n_valid <= P
    recs = raw[lay["records"]:lay["leaf_lo"]].view(torch.float32).view(P, 4)
    lo = raw[lay["leaf_lo"]:lay["leaf_hi"]].view(torch.float32).view(B, 4)[:, :3]
    hi = raw[lay["leaf_hi"]:lay["end"]].view(torch.float32).view(B, 4)[:, :3]
    live = -(-n_valid // 256)
    lo, hi = lo[:live], hi[:live]
    q = recs[:n_valid - n_valid % 64, :3].view(-1, 64, 3)
    rows = recs[:n_valid - n_valid % 64, 3].view(torch.int32).long().view(-1, 64)
    assert int(rows.min()) >= 0 and int(rows.max()) < P
    lim = kth[rows]
    total = 0
    for a in range(0, len(q), chunk):
        qq = q[a:a + chunk, :, None, :]
        gap = torch.clamp(torch.maximum(lo - qq, qq - hi), min=0.0)
        need = ((gap * gap).sum(dim=-1) <= lim[a:a + chunk, :, None]).any(dim=1)
        total += int(need.sum())
    return total / (len(q) * live), live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 500000])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops baseline")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"{'set':<18}{'P':>8} {'build us':>10} {'search us':>10} {'(min)':>9} {'torch ops us':>13} {'ratio':>7} {'unskippable leaves':>19}")
    for P in args.sizes:
        for name, pts in (("uniform", uniform(P, dev)), ("surface", surface(P, dev)), ("surface+outlier", with_outlier(surface(P, dev)))):
            index, t_build, _ = replay_time(lambda: knn.knn_build(pts), args.replays)
            mean = torch.empty(P, device=dev)
            kth = torch.empty((P, 3), device=dev)

            def search():
                _capi.call("dgr_knn_search", dev, index.index.data_ptr(), P, pts.data_ptr(), P, None, _capi.KnnParams(3, 1, float("inf")),
                           index.scratch.data_ptr(), None, None, None, mean.data_ptr())
            _, t_search, t_min = replay_time(search, args.replays)
            _capi.call("dgr_knn_search", dev, index.index.data_ptr(), P, pts.data_ptr(), P, None, _capi.KnnParams(3, 1, float("inf")),
                       index.scratch.data_ptr(), kth.data_ptr(), None, None, None)
            share, live = unskippable_share(index, kth[:, 2].contiguous())
            t_torch, checks = float("nan"), ""
            if not args.no_torch:
                ref = torch_ops(pts)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ref = torch_ops(pts)
                b.record()
                b.synchronize()
                t_torch = a.elapsed_time(b) * 1e3
                checks = f"  [sample of 400 against float64: kernel {sample_check(pts, mean):.1e}, torch ops {sample_check(pts, ref):.1e}]"
            print(f"{name:<18}{P:>8} {t_build:>10.1f} {t_search:>10.1f} {t_min:>9.1f} {t_torch:>13.1f} {t_torch / (t_build + t_search):>7.1f} "
                  f"{share:>12.4f} of {live}{checks}", flush=True)


if __name__ == "__main__":
    main()
