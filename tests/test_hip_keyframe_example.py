"""examples/mapping.py --select: the mapping window is chosen from the keyframe pool by overlap with the newest keyframe
(slam.keyframe_overlap + slam.select_keyframes) and the loop runs to the end against it."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_mapping_loop_selects_its_window_by_overlap():
    from mapping import mapping_loop
    lines = []
    (l0, l1), pc, _ = mapping_loop(torch.device("cuda:0"), 4000, 64, 48, 4, 12, views_in_flight=1, log=lines.append, select=2)
    print("\n".join(lines), f"\nloss {l0:.4e} -> {l1:.4e}")
    assert math.isfinite(l0) and math.isfinite(l1) and l1 < l0
    chosen = [ln for ln in lines if ln.startswith("select: ")]
    assert len(chosen) == 1
    scores = [float(x) for x in chosen[0].split(": ", 2)[2].split(" -> ")[0].split(", ")]
    assert len(scores) == 3 and scores[1] == 0.0 and scores[0] > 0.3 and scores[2] > 0.3  # the pool's keyframe 1 looks away
    best = max((0, 2), key=lambda k: (scores[k], -k))
    assert pc.window == [best, 3]  # the newest keyframe and the one that overlaps it most; never the one that looks away
    assert pc.get_xyz.grad is not None and float(pc.denom.sum()) > 0
