"""examples/mapping.py --loop-close-at N --pgo: the poses the map follows after the update are solved for on the device
(slam.pose_graph_optimize over chain edges and a loop edge measured on the drawn poses), eagerly and between the replays of a
recorded, batched iteration, at the sizes of test_hip_transform_example.py.  The solved poses are the drawn ones, and the loss
after the update lies within that file's control spread: what one more Adam step does in the same run with no pose change."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

P, W, H, KEYFRAMES, ITERS, AT = 2000, 64, 48, 2, 20, 10
# |solved - drawn|, element-wise: twice the worst measured on the MI355X (5.96e-8 in both modes, half an fp32 ulp of this scene's
# largest pose entry, 1.0: the graph is consistent, so the optimum is the drawn poses up to the rounding of relative_pose's fp32
# measurements and of the output); profiles/pgo/measured.txt; the issue's cap is 2e-4
POSE_TOL = 1.2e-7


def run(mp, recorded, **kw):
    from mapping import mapping_loop
    mp.setenv("DGR_SYNC_MODE", "lazy" if recorded else "strict")
    (first, last), pc, _ = mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, seed=True, loop_close_at=AT, graph=recorded,
                                        fused=recorded, views_in_flight=1, log=None, **kw)
    assert math.isfinite(first) and math.isfinite(last) and last < first
    return pc


@pytest.fixture(scope="module", params=[False, True], ids=["eager", "graph-fused"])
def runs(request):
    with pytest.MonkeyPatch.context() as mp:
        out = {"control_a": run(mp, request.param, loop_close_scale=0.0, loop_close_seed=1),
               "control_b": run(mp, request.param, loop_close_scale=0.0, loop_close_seed=2),
               "drawn": run(mp, request.param, loop_close_seed=1),
               "solved": run(mp, request.param, loop_close_seed=1, loop_close_pgo=True)}
    return out


def test_the_solved_poses_are_the_drawn_ones(runs):
    c = runs["solved"].loop_closure
    solved, truth = c["solved"].cpu(), c["truth"].cpu()
    diff = float((solved - truth).abs().max())
    names = ("initial", "final", "ok", "run", "accepted", "rejected", "cg")
    print(f"pgo-figure example: |solved - drawn| {diff:.3e}, largest entry {float(truth.abs().max()):.3f}; " +
          ", ".join(f"{n} {v:.4g}" for n, v in zip(names, c["pgo_stats"])))
    assert solved.shape == (KEYFRAMES, 4, 4) and torch.equal(solved[0], truth[0])  # (the fixed keyframe's bits)
    assert c["pgo_stats"][2] == 1 and c["pgo_stats"][4] >= 1 and c["pgo_stats"][0] > 1e-3 > c["pgo_stats"][1]
    assert diff <= POSE_TOL
    assert "solved" not in runs["drawn"].loop_closure


def test_the_map_follows_the_solved_poses(runs):
    closure = {name: pc.loop_closure for name, pc in runs.items()}
    step = {name: c["after"] - c["before"] for name, c in closure.items()}
    spread = max(abs(step["control_a"]), abs(step["control_b"])) + abs(closure["control_a"]["before"] - closure["control_b"]["before"])
    print("loss before -> after the update: " + "; ".join(f"{n} {c['before']:.5e} -> {c['after']:.5e}" for n, c in closure.items()) +
          f"; spread {spread:.3e}")
    assert spread > 0.0
    assert abs(step["solved"]) <= spread
    rows = runs["solved"].get_xyz.shape[0]
    assert closure["solved"]["counts"] == [rows, 0, 0, 0]
