"""examples/mapping.py --loop-close-at: after a pose-graph update the map follows its keyframes (pose_corrections + transform_map)
and the mapping loop goes on as if nothing had happened, eagerly and between the replays of a recorded, batched iteration.

The yardstick is the loop itself: the same run with no pose change at all (`loop_close_scale=0`: the corrections are identities up to
rounding) under two seeds.  Its spread is the largest change of the loss from iteration N to N + 1 in those runs -- what one more
Adam step does -- plus the two runs' difference at iteration N.  The corrected run's loss after the update lies within that spread
of its loss before it; with the poses changed and the map left where it was, the loss jumps by more than ten times the spread."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

P, W, H, KEYFRAMES, ITERS, AT = 2000, 64, 48, 2, 20, 10


def run(mp, recorded, **kw):
    from mapping import mapping_loop
    mp.setenv("DGR_SYNC_MODE", "lazy" if recorded else "strict")
    lines = []
    (first, last), pc, _ = mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, seed=True, loop_close_at=AT, graph=recorded,
                                        fused=recorded, views_in_flight=1, log=None if recorded else lines.append, **kw)
    assert math.isfinite(first) and math.isfinite(last) and (last < first or not kw.get("loop_close_moves_map", True))
    return pc, lines


@pytest.fixture(scope="module", params=[False, True], ids=["eager", "graph-fused"])
def runs(request):
    with pytest.MonkeyPatch.context() as mp:
        out = {"control_a": run(mp, request.param, loop_close_scale=0.0, loop_close_seed=1),
               "control_b": run(mp, request.param, loop_close_scale=0.0, loop_close_seed=2),
               "corrected": run(mp, request.param, loop_close_seed=1),
               "unmoved": run(mp, request.param, loop_close_seed=1, loop_close_moves_map=False)}
    return out


def test_the_map_follows_the_corrected_poses(runs):
    closure = {name: pc.loop_closure for name, (pc, _) in runs.items()}
    step = {name: c["after"] - c["before"] for name, c in closure.items()}
    spread = max(abs(step["control_a"]), abs(step["control_b"])) + abs(closure["control_a"]["before"] - closure["control_b"]["before"])
    print("loss before -> after the update: " + "; ".join(f"{n} {c['before']:.5e} -> {c['after']:.5e}" for n, c in closure.items()) +
          f"; spread {spread:.3e}")
    assert spread > 0.0
    assert abs(step["corrected"]) <= spread
    assert step["unmoved"] > 10.0 * spread
    pc, lines = runs["corrected"]
    rows = pc.get_xyz.shape[0]
    assert closure["corrected"]["counts"] == [rows, 0, 0, 0] and closure["unmoved"]["counts"] is None
    anchors = pc.leaves()["anchor"]
    assert anchors.shape == (rows,) and not anchors.requires_grad and sorted(set(anchors.tolist())) == [0.0, 1.0]
    assert not lines or any(line.startswith("loop closure after iteration 10") for line in lines)


def test_the_model_stays_in_place(runs):
    """the leaves after the update are the optimiser's leaves: the step did not re-point anything"""
    pc, _ = runs["corrected"]
    assert all(t.is_leaf and t.requires_grad == (name != "anchor") for name, t in pc.leaves().items())
