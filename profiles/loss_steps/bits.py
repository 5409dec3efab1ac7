#!/usr/bin/env python3
"""Hashes of every output of the loss and keyframe steps on seeded inputs: run on the parent and on the change, the two files
must be identical (no tolerance: the steps promise the same bits, so their summation order must have survived).  One line per
step and input family with the number of outputs under it; --full: one line per output, to find the one that differs.
  l1_loss          step_model.L1_SHAPES x L1_FAMILIES                 loss, dcolor, ddepth
  l1_ssim_loss     ssim_model.SHAPES x KINDS, with a depth image       loss, scratch header, dcolor, ddepth
  ssim             the same                                            value, dimg
  masked_l1_loss   masked_loss_model.SHAPES x FAMILIES, rejection on and off, sum and mean
                                                                       loss, mask, median, base, kept, dcolor, ddepth
  keyframe_overlap 640 x 480 stride 16 (one workgroup per keyframe) and 96 x 80 stride 1 (four), with keyframe depths
                                                                       score, inside, visible, valid, flags

    python profiles/loss_steps/bits.py --out FILE [--full]
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--full", action="store_true")
    args = ap.parse_args()
    import masked_loss_model as mm
    import ssim_model
    import step_model as sm
    from dgr_amd import slam
    dev = torch.device("cuda:0")
    lines = []

    def put(name, t):
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        lines.append(f"{name} {a.dtype} {list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()[:24]}")

    def leaf(a):
        return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to(dev).clone().requires_grad_()

    for family in sm.L1_FAMILIES:
        for k, shapes in enumerate(sm.L1_SHAPES):
            inp = sm.l1_inputs(family, shapes)
            c, d = leaf(inp["color"]), leaf(inp["depth"])
            loss = slam.l1_loss(c, d, torch.from_numpy(inp["color_obs"]).to(dev), torch.from_numpy(inp["depth_obs"]).to(dev),
                                float(inp["w_color"]), float(inp["w_depth"]))
            (loss * sm.L1_UPSTREAM).backward()
            for n, t in (("loss", loss), ("dcolor", c.grad), ("ddepth", d.grad)):
                put(f"l1_loss/{family}/{k}/{n}", t)

    for kind in ssim_model.KINDS:
        for shape in ssim_model.SHAPES:
            x, y = ssim_model.inputs(kind, shape)
            dx, dy = ssim_model.inputs("rand", (shape[0], 1) + shape[2:], seed=3)
            c, d = leaf(x), leaf(dx)
            loss = slam.l1_ssim_loss(c, d, y.to(dev), dy.to(dev), 1.0, 0.5, 0.2)
            header = loss.grad_fn.saved_tensors[-1][:4].clone()  # (the call's scratch: mean SSIM, mean|c - c_obs|, mean|d - d_obs|, maps flag)
            loss.backward()
            tag = f"l1_ssim_loss/{kind}/{'x'.join(map(str, shape))}"
            for n, t in (("loss", loss), ("header", header), ("dcolor", c.grad), ("ddepth", d.grad)):
                put(f"{tag}/{n}", t)
            c = leaf(x)
            value = slam.ssim(c, y.to(dev))
            value.backward()
            put(f"ssim/{kind}/{'x'.join(map(str, shape))}/value", value)
            put(f"ssim/{kind}/{'x'.join(map(str, shape))}/dimg", c.grad)

    for family in mm.FAMILIES:
        for shape in mm.SHAPES:
            inp = mm.inputs(family, shape)
            for factor in (10.0, None):
                for reduction in ("sum", "mean"):
                    c, d = leaf(inp["color"]), leaf(inp["depth"])
                    loss, stats = slam.masked_l1_loss(c, d, inp["color_obs"].to(dev), inp["depth_obs"].to(dev),
                                                      inp["opacity_map"].to(dev), inp["mask"].to(dev), outlier_factor=factor,
                                                      reduction=reduction, return_stats=True)
                    loss.backward()
                    tag = f"masked_l1_loss/{family}/{'x'.join(map(str, shape))}/factor_{factor}/{reduction}"
                    for n, t in (("loss", loss), ("mask", stats.mask), ("median", stats.median.view(torch.int32)),
                                 ("base", stats.base), ("kept", stats.kept), ("dcolor", c.grad), ("ddepth", d.grad)):
                        put(f"{tag}/{n}", t)

    for W, H, stride, K in ((640, 480, 16, 9), (96, 80, 1, 5)):
        rng = np.random.default_rng(11 + W)
        depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
        depth[rng.random((H, W)) < 0.1] = 0.0

        def pose():  # W2C^T of a small random rotation and translation
            w = rng.normal(size=3) * 0.15
            th = np.linalg.norm(w)
            Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
            m = np.eye(4)
            m[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
            m[:3, 3] = rng.uniform(-0.3, 0.3, 3)
            return m.T.astype(np.float32)

        vm, kvm = pose(), np.stack([pose() for _ in range(K)])
        kd = rng.uniform(0.5, 4.0, (K, H, W)).astype(np.float32)
        for with_depths in (False, True):
            out = slam.keyframe_overlap(torch.from_numpy(depth).to(dev), torch.from_numpy(vm).to(dev), torch.from_numpy(kvm).to(dev),
                                        0.8 * W, 0.8 * W, W / 2 - 0.5, H / 2 - 0.5, stride=stride, edge=3.0, depth_range=(0.0, 10.0),
                                        keyframe_depths=torch.from_numpy(kd).to(dev) if with_depths else None, depth_tolerance=0.3,
                                        return_flags=True)
            for n, t in zip(out._fields, out):
                put(f"keyframe_overlap/{W}x{H}_stride{stride}/depths_{int(with_depths)}/{n}", t.view(torch.int32) if n == "score" else t)

    torch.cuda.synchronize()
    if not args.full:  # step/family -> the hash of its outputs' lines
        groups = {}
        for l in lines:
            groups.setdefault("/".join(l.split("/")[:2]), []).append(l)
        lines = [f"{k} {len(v)} outputs {hashlib.sha256(chr(10).join(v).encode()).hexdigest()[:24]}" for k, v in groups.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {args.out}")


if __name__ == "__main__":
    main()
