"""examples/mapping.py --densify-every: the mapping loop goes on with the leaves, moments and accumulators densify_and_prune
hands back."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_mapping_loop_densifies_and_goes_on():
    from mapping import mapping_loop
    lines = []
    P = 6000
    (l0, l1), pc, _ = mapping_loop(torch.device("cuda:0"), P, 160, 120, 2, 11, views_in_flight=1, log=lines.append, densify_every=4)
    assert math.isfinite(l0) and math.isfinite(l1)
    steps = [ln for ln in lines if ln.startswith("densify: P ")]
    assert len(steps) == 2 and steps[0].startswith(f"densify: P {P} -> ")
    rows = pc.get_xyz.shape[0]
    assert steps[-1].split("->")[1].split()[0] == str(rows)
    for t in (pc._features, pc._opacity, pc._scaling, pc._rotation, pc.xyz_gradient_accum, pc.denom, pc.max_radii2D):
        assert t.shape[0] == rows
    assert pc._xyz.requires_grad and pc._xyz.grad is not None and pc._xyz.grad.shape[0] == rows
