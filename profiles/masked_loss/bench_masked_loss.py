#!/usr/bin/env python3
"""Times slam.masked_l1_loss (csrc/masked_loss.hip) against the only way to get this loss without it: the torch-op composition of
the same loss on the same machine (elementwise ops + torch.median per view; a sort per view where a hipGraph must record it).  Forward + backward, eagerly and through a hipGraph
replay, the two alternating round by round on one device, ROUNDS x CALLS calls each after a warm-up; one line per round and the
ranges at the end.  Two frames per shape: continuous errors (nearly all keys distinct) and ALL-EQUAL errors (every key of a wave
falls into one histogram bin: the worst case for the select's LDS atomics).

    python profiles/masked_loss/bench_masked_loss.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

ROUNDS, CALLS = 6, 20
SIZES = ((1, 3, 480, 640), (4, 3, 480, 640), (1, 3, 1080, 1920), (4, 3, 1080, 1920))


def torch_loss(c, d, co, do, opa, capturable=False, w_color=1.0, w_depth=0.5, factor=10.0, threshold=0.99):
    """slam.masked_l1_loss(reduction="sum") from torch ops: the mask is a constant of the graph.  The median of a view's base set
    is torch.median over a boolean selection (a host read: the selection's size); `capturable`: no host read -- the errors outside
    the base set become inf, every view is sorted and the element of rank (n - 1) / 2 gathered, which a hipGraph can record."""
    with torch.no_grad():
        e = (d - do).abs()
        B = (do > 0) & torch.isfinite(e) & (opa > threshold)
        V = e.shape[0]
        if capturable:
            ranked = torch.where(B, e, torch.full_like(e, float("inf"))).view(V, -1).sort(dim=1).values
            n = B.view(V, -1).sum(1, keepdim=True)
            median = torch.where(n > 0, ranked.gather(1, (n - 1).clamp(min=0) // 2), torch.zeros_like(ranked[:, :1]))
        else:
            median = torch.stack([torch.median(e[v][B[v]]) for v in range(V)])
        K = B & (e <= (factor * median).view(V, 1, 1, 1))
    return w_depth * ((d - do).abs() * K).sum() + w_color * ((c - co).abs() * K).sum()


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # microseconds per call


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from dgr_amd import slam
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    say(f"# {torch.cuda.get_device_name(0)}; forward + backward of masked_l1_loss(opacity_map, factor 10, sum), microseconds per call,")
    say(f"# {ROUNDS} rounds x {CALLS} calls each, fused and torch-op alternating round by round; 30 % holes, 5 % outliers")
    for shape in SIZES:
        V, C, H, W = shape
        for frame in ("continuous", "all-equal"):
            g = torch.Generator().manual_seed(0)
            r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
            pix = (V, 1, H, W)
            co, c = r(shape).to(dev), r(shape).to(dev).requires_grad_()
            do = 0.5 + 3.5 * r(pix)
            err = r(pix) ** 3 if frame == "continuous" else torch.full(pix, 0.25)
            d = torch.where(r(pix) < 0.05, do + 10.0, do + err)
            do = torch.where(r(pix) < 0.30, torch.zeros(()), do)
            if frame == "all-equal":  # (no outliers, and observations whose sum with 0.25 is exact: one key in the whole frame)
                do = torch.where(do > 0, torch.full(pix, 2.0), do)
                d = do + 0.25
            opa = torch.where(r(pix) < 0.8, torch.ones(()), r(pix)).to(dev)
            d, do = d.to(dev).requires_grad_(), do.to(dev)

            def fused():
                c.grad = d.grad = None
                slam.masked_l1_loss(c, d, co, do, opa).backward()

            def torch_ops():
                c.grad = d.grad = None
                torch_loss(c, d, co, do, opa).backward()

            def torch_ops_capturable():
                c.grad = d.grad = None
                torch_loss(c, d, co, do, opa, capturable=True).backward()

            torch_ops()
            ga, la = d.grad.clone(), float(torch_loss(c, d, co, do, opa).detach())
            fused()
            lb = float(slam.masked_l1_loss(c, d, co, do, opa).detach())
            say(f"{shape} {frame}: loss fused {lb!r} torch-op {la!r}; ddepth equal: {bool(torch.equal(d.grad, ga))}")
            for mode in ("eager", "hipGraph replay"):
                # (the replayed composition is the sort form: torch.median over a selection reads its size on the host)
                fa, fb = (fused, torch_ops) if mode == "eager" else (captured(fused), captured(torch_ops_capturable))
                for fn in (fa, fb):
                    timed(fn, 10)
                tf, tt = [], []
                for k in range(ROUNDS):
                    tf.append(timed(fa, CALLS))
                    tt.append(timed(fb, CALLS))
                    say(f"{shape} {frame} {mode} round {k}: fused {tf[-1]:9.1f} us   torch-op {tt[-1]:9.1f} us")
                apart = max(tf) < min(tt) or max(tt) < min(tf)
                say(f"{shape} {frame} {mode}: fused {min(tf):.1f} .. {max(tf):.1f} us, torch-op {min(tt):.1f} .. {max(tt):.1f} us: "
                    f"ranges {'apart' if apart else 'TOUCH'}, torch-op / fused = {min(tt) / max(tf):.1f} .. {max(tt) / min(tf):.1f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
