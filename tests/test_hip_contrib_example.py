"""examples/mapping.py --seed --densify-every 5 --prune-unseen 5 at a small size: the window's keyframes go through
slam.render_contributions into one accumulator, the Gaussians no keyframe blends (here: those whose opacity the optimiser has
pushed below the blend threshold, which opacity pruning at 0.005 keeps) are marked and that iteration's densify_and_prune
removes them.  The step reports a nonzero count."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

# (60 iterations: long enough for the optimiser to push some opacities below the blend threshold, 15/255 -- the Gaussians no
#  pixel blends any more; measured on the MI355X: 0 unseen up to iteration 35, then 1, 26 and 76 of about 12 000)
P, W, H, KEYFRAMES, ITERS = 2000, 64, 48, 2, 60


def test_prune_unseen_reports_what_no_keyframe_blends(monkeypatch):
    from mapping import mapping_loop
    monkeypatch.setenv("DGR_SYNC_MODE", "strict")
    lines = []
    (first, last), pc, _ = mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, seed=True, densify_every=5, prune_unseen=5,
                                        views_in_flight=1, log=lines.append)
    assert math.isfinite(first) and math.isfinite(last) and last < first
    steps = pc.unseen
    print("prune-unseen steps [Gaussians, unseen]:", steps)
    assert len(steps) == len([i for i in range(ITERS - 3) if (i + 4) % 5 == 0]) and all(0 <= u <= n for n, u in steps)
    assert sum(u for _, u in steps) > 0
    marked = [ln for ln in lines if ln.startswith("prune-unseen:")]
    densified = [ln for ln in lines if ln.startswith("densify:")]
    assert len(marked) == len(steps) == len(densified)
    # the marked Gaussians leave with that iteration's densify_and_prune: it keeps no more than the seen ones
    for (n, u), ln in zip(steps, densified):
        assert f"P {n} -> " in ln and int(ln.split("(")[1].split()[0]) <= n - u, (n, u, ln)


def test_the_flag_needs_a_step_that_removes_and_no_graph():
    from mapping import mapping_loop
    with pytest.raises(ValueError, match="prune_unseen"):
        mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, prune_unseen=5)
    with pytest.raises(ValueError, match="prune_unseen"):
        mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, relocate_every=5, prune_unseen=5, graph=True)
