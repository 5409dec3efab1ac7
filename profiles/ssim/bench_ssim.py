#!/usr/bin/env python3
"""Times slam.l1_ssim_loss (csrc/ssim.hip) against the only way to get this loss without it: the torch-op formulation
(depthwise F.conv2d on the GPU, autograd backward).  Forward + backward, the two alternating on one device, ROUNDS x CALLS calls
each after a warm-up; one line per round and the ranges at the end.  Also the two entry points on their own (colour only, so the
forward is the tile kernel plus the one-workgroup sum), as a fraction of the bytes they must move at 8 TB/s.

    python profiles/ssim/bench_ssim.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ROUNDS, CALLS = 8, 20
SIZES = ((4, 3, 480, 640), (1, 3, 1080, 1920))
HBM = 8e12  # bytes / s


def torch_loss(c, d, co, do, window, w_color=1.0, w_depth=0.5, lam=0.2):
    conv = lambda t: F.conv2d(t, window, padding=5, groups=t.shape[1])  # noqa: E731
    mu1, mu2 = conv(c), conv(co)
    s1, s2, s12 = conv(c * c) - mu1 * mu1, conv(co * co) - mu2 * mu2, conv(c * co) - mu1 * mu2
    m = (2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return w_color * ((1 - lam) * (c - co).abs().mean() + lam * (1 - m.mean())) + w_depth * (d - do).abs().mean()


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from dgr_amd import _capi, slam
    from ssim_model import window_1d
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    say(f"# {torch.cuda.get_device_name(0)}; forward + backward of l1_ssim_loss(w_color 1, w_depth 0.5, lambda 0.2), microseconds per call,")
    say(f"# {ROUNDS} rounds x {CALLS} calls each, fused and torch-op alternating round by round")
    for shape in SIZES:
        V, C, H, W = shape
        g = torch.Generator().manual_seed(0)
        c = torch.rand(shape, generator=g).to(dev).requires_grad_()
        co = torch.rand(shape, generator=g).to(dev)
        d = torch.rand((V, 1, H, W), generator=g).to(dev).requires_grad_()
        do = torch.rand((V, 1, H, W), generator=g).to(dev)
        g1 = window_1d().to(dev)
        window = (g1[:, None] * g1[None, :]).expand(C, 1, 11, 11).contiguous()

        def fused():
            c.grad = d.grad = None
            slam.l1_ssim_loss(c, d, co, do, 1.0, 0.5, 0.2).backward()

        def torch_ops():
            c.grad = d.grad = None
            torch_loss(c, d, co, do, window).backward()

        fused(), torch_ops()
        ga, gb = c.grad.clone(), None
        fused()
        gb = c.grad.clone()
        say(f"{shape}: max|dfused - dtorch| / max|dtorch| = {float((gb - ga).abs().max() / ga.abs().max()):.2e}")
        for fn in (fused, torch_ops):
            timed(fn, 10)
        tf, tt = [], []
        for r in range(ROUNDS):
            tf.append(timed(fused, CALLS))
            tt.append(timed(torch_ops, CALLS))
            say(f"{shape} round {r}: fused {tf[-1]:9.1f} us   torch-op {tt[-1]:9.1f} us")
        apart = max(tf) < min(tt)
        say(f"{shape}: fused {min(tf):.1f} .. {max(tf):.1f} us, torch-op {min(tt):.1f} .. {max(tt):.1f} us: ranges "
            f"{'apart' if apart else 'TOUCH'}, factor {min(tt) / max(tf):.1f} .. {max(tt) / min(tf):.1f}")

        # the two entry points on their own (colour only): the tile kernels, against the bytes they must move
        lib = _capi.load()
        n = c.numel()
        floats = lib.dgr_ssim_scratch_floats(*shape)
        buf = torch.empty(floats + 4, device=dev)
        dimg = torch.empty_like(c)
        st = _capi.stream_handle(0)
        x, y = c.detach(), co

        def fwd():
            assert lib.dgr_ssim_loss_forward(st, *shape, x.data_ptr(), y.data_ptr(), 0, None, None, 0.8, 0.2, 0.0, buf.data_ptr(), 1,
                                             buf[floats:].data_ptr()) == 0

        def fwd_inference():
            assert lib.dgr_ssim_loss_forward(st, *shape, x.data_ptr(), y.data_ptr(), 0, None, None, 0.8, 0.2, 0.0, buf.data_ptr(), 0,
                                             buf[floats:].data_ptr()) == 0

        def bwd():
            assert lib.dgr_ssim_loss_backward(st, *shape, x.data_ptr(), y.data_ptr(), 0, None, None, 0.8, 0.2, 0.0, buf.data_ptr(),
                                              None, dimg.data_ptr(), None) == 0

        for name, fn, nbytes in (("forward, maps (tile kernel + final sum)", fwd, 20 * n), ("backward", bwd, 24 * n),
                                 ("forward, want_maps = 0", fwd_inference, 8 * n)):
            if fn is bwd:
                fwd()
            timed(fn, 10)
            ts = [timed(fn, CALLS) for _ in range(ROUNDS)]
            floor = nbytes / HBM * 1e6
            say(f"{shape} {name}: {min(ts):.1f} .. {max(ts):.1f} us; {nbytes / 1e6:.1f} MB at 8 TB/s = {floor:.1f} us = "
                f"{floor / max(ts) * 100:.0f} .. {floor / min(ts) * 100:.0f} % of the time")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
