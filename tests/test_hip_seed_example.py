"""examples/mapping.py --seed: the map starts empty, is seeded from the keyframes as they join the window, and the mapping loop
goes on with the leaves, moments and accumulators seed_from_frame hands back."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_mapping_loop_seeds_an_empty_map_and_goes_on():
    from mapping import mapping_loop
    lines = []
    (l0, l1), pc, _ = mapping_loop(torch.device("cuda:0"), 6000, 96, 64, 3, 20, views_in_flight=1, log=lines.append, seed=True)
    print("\n".join(lines), f"\nloss {l0:.4e} -> {l1:.4e}")
    assert math.isfinite(l0) and math.isfinite(l1) and l1 < l0
    steps = [ln for ln in lines if ln.startswith("seed: keyframe ")]
    assert len(steps) == 3 and steps[0].startswith("seed: keyframe 0: P 0 -> ")
    sizes = [int(ln.split("->")[1].split()[0]) for ln in steps]
    assert 0 < sizes[0] <= sizes[1] <= sizes[2] and sizes[0] > 96 * 64 // 2
    rows = pc.get_xyz.shape[0]
    assert rows == sizes[-1]
    for t in (pc._f_dc, pc._f_rest, pc._opacity, pc._scaling, pc._rotation, pc.xyz_gradient_accum, pc.denom, pc.max_radii2D):
        assert t.shape[0] == rows
    assert pc._xyz.requires_grad and pc._xyz.grad is not None and pc._xyz.grad.shape[0] == rows
    assert float(pc.denom.sum()) > 0  # the statistics of the rows that stayed were kept across the seeds
