"""Runs the mapping blend backward of one BASELINE config, with or without absgrad, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python profiles/absgrad/absgrad_cost.py light 3 0 1

args: variant (light | full), config (2 | 3), lane lists (0: quadrant, 1: half-wave / paired, 2: per frame), absgrad (0 | 1).
Ten warm-up and fifty timed forward + backward pairs; the forward is the same in both runs.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import hip_helpers as hh  # noqa: E402
from dgr_amd import _capi  # noqa: E402
from dgr_amd import full as F  # noqa: E402
from dgr_amd import light as L  # noqa: E402
from dgr_amd.synth import make_scene  # noqa: E402

CONFIGS = {2: (100000, 640, 480), 3: (500000, 1920, 1080)}


def main():
    variant, cfg, lists, absgrad = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), bool(int(sys.argv[4]))
    P, W, H = CONFIGS[cfg]
    _capi.set_option("lane_lists", lists)
    s = make_scene(P, W, H, 5)
    T, E = hh.T, hh.E
    if variant == "light":
        out, _ = hh.hip_forward(s, 3)
        (R, color, depth, median, var, alpha, radii, geom, binning, img, _, _) = out
        args = (T(s.bg), T(s.means), radii, E(), T(s.scales), T(s.rots), 1.0, E(), T(s.view), T(s.proj), s.tanfovx, s.tanfovy,
                T(s.gC), T(s.gD[None]), T(s.gM[None]), T(s.gV[None]), T(s.gt), T(s.shs), 3, T(s.campos), geom, R, binning, img,
                alpha, False, T(s.persp), False, False)
        step = lambda: L._C.rasterize_gaussians_backward(*args, absgrad=absgrad)  # noqa: E731
    else:
        out, _ = hh.hip_full_forward(s, 3)
        (R, NG, color, depth, unc, radii, geom, binning, img) = out
        args = (T(s.bg), T(s.means), radii, E(), T(s.scales), T(s.rots), 1.0, E(), T(s.view), T(s.gt), T(s.proj), s.tanfovx,
                s.tanfovy, T(s.gC), T(s.gD[None]), T(s.gV[None]), T(s.shs), 3, T(s.campos), geom, R, binning, img, NG,
                T(s.persp))
        step = lambda: F._C.rasterize_gaussians_backward(*args, absgrad=absgrad)  # noqa: E731
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(50):
        step()
    ev[1].record()
    torch.cuda.synchronize()
    print(f"{variant} config {cfg} lane_lists {lists} absgrad {int(absgrad)}: {ev[0].elapsed_time(ev[1]) / 50:.4f} ms per backward")


if __name__ == "__main__":
    main()
