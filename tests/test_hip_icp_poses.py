"""The ICP step (dgr_icp_step) and the hybrid RGB-D step (dgr_rgbd_step) on the GPU at general poses, gates and block edges, against
the float64 models: every branch of the finisher's rotation_to_quat on the accepted and the refused path (the world frames of
icp_model.WORLD_FRAMES), se3_exp on both sides of its series switch and at large angles, each per-candidate gate away from its
default, frames whose last block and whose 64th and 65th scratch rows carry data, the aligners end to end at poses far from
the world axes, and the hand-off of (quat, trans) to the tracker's pose_to_camera.  tests/test_icp_poses_model.py shows on the CPU
that these inputs reach what they are meant to reach and that wrong finishers fail on them."""
import numpy as np
import pytest
import torch

from dgr_amd import icp, slam

import icp_model as M
import rgbd_model as R
import step_model
import test_hip_rgbd as hybrid
from test_hip_icp import DEV, ULP, T, check_step, intr, refused_keeps_the_input, run_step, same_bits
from test_icp_poses_model import (COND_CAP, EDGE_FRAMES, ICP_GATES, RGBD_GATES, SERIES_SIDE, TWISTS, edge_step, gate_id, gate_step, moved_corner_frame,
                                  moved_frame, moved_plane_scene, moved_step, size_of, start_frame, twist_step)
from test_rgbd_model import corner_frame
from test_rgbd_model import step as rgbd_model_step

pytestmark = pytest.mark.gpu
INF = float("inf")
DIAGONAL = ("half_x", "half_y", "half_z")  # one refusal of the hybrid step per diagonal branch


# ------------------------------------------------------------------------------------------------------------ world frames
@pytest.mark.parametrize("name", M.WORLD_FRAMES)
def test_step_at_every_world_frame(name):
    s = moved_frame(name, *size_of(name))
    _, want = check_step(run_step(s, 1, True, INF), moved_step(name), s, f"{name} {s['W']}x{s['H']}")
    branches = [M.quat_branch(M.pose_of(s[k])[0]) for k in ("model_view", "view_in")] + [want["branch"]]
    print(f"{name}: branches (model, in, out) {branches}")
    assert want["ok"]


@pytest.mark.parametrize("name", M.NAMED_FRAMES)
def test_refusal_at_every_named_world_frame(name):
    s = moved_frame(name)
    count = int(moved_step(name)["associated"].sum()) + int(moved_step(name)["ambiguous"].sum())
    out = run_step(s, 1, True, INF, min_points=count + 1)
    print(f"{name}: branch of the input's rotation {M.quat_branch(M.pose_of(s['view_in'])[0])}")
    stats = refused_keeps_the_input(out, s["view_in"], f"{name}, min_points above the count")
    assert 0 < stats[28] <= count


@pytest.mark.parametrize("name", M.NAMED_FRAMES)
def test_hybrid_step_at_every_named_world_frame(name):
    s = moved_corner_frame(name)
    m = rgbd_model_step(s, 1)
    _, want = hybrid.check_step(hybrid.run_step(s, 1), m, s, f"hybrid {name} 96x80")
    print(f"hybrid {name}: branch of the output's rotation {want['branch']}")
    assert want["ok"]
    if name in DIAGONAL:
        count = int(m["geometric"].sum() + m["photometric"].sum()) + 2 * int(m["ambiguous"].sum())
        out = hybrid.run_step(s, 1, min_points=count + 1)
        as_icp = type(out)(out.viewmatrix, out.quat, out.trans, torch.cat([out.stats[:, :29], out.stats[:, 31:34]], 1), out.flags)
        refused_keeps_the_input(as_icp, s["view_in"], f"hybrid {name}, min_points above both counts together")


# ------------------------------------------------------------------------------------------------------------------ twists
@pytest.mark.parametrize("k", TWISTS, ids=[f"{k}xTWIST" for k in TWISTS])
def test_one_step_at_every_twist_magnitude(k):
    s = start_frame(96, 80, k)
    stats, want = check_step(run_step(s, 1, True, INF, **TWISTS[k]), twist_step(k), s, f"{k} TWIST")
    print(f"{k} TWIST: theta^2 solved on the device {stats[30] ** 2:.3g} (model {want['omega'] ** 2:.3g})")
    assert want["ok"] and (stats[30] ** 2 < 1e-6) == SERIES_SIDE[k]


# ------------------------------------------------------------------------------------------------------------------- gates
@pytest.mark.parametrize("gate", ICP_GATES, ids=gate_id)
def test_each_gate_of_the_icp_step(gate):
    s = moved_frame("identity")
    default = run_step(s, 1, True, INF).stats.cpu().numpy()[0]
    stats, want = check_step(run_step(s, 1, True, INF, **gate), gate_step(gate_id(gate)), s, f"{gate}",
                             conditioned=gate_id(gate) not in COND_CAP)
    assert want["cond"] <= COND_CAP.get(gate_id(gate), 1e3)
    print(f"{gate}: associated {int(stats[28])} (default {int(default[28])})")
    assert want["ok"] and 0 < stats[28] < default[28]


@pytest.mark.parametrize("gate", RGBD_GATES, ids=gate_id)
def test_each_gate_of_the_hybrid_step(gate):
    s = corner_frame(96, 80)
    default = hybrid.run_step(s, 1).stats.cpu().numpy()[0]
    stats, want = hybrid.check_step(hybrid.run_step(s, 1, **gate), gate_step(gate_id(gate), True), s, f"{gate}")
    print(f"{gate}: photometric {int(stats[30])} (default {int(default[30])}), geometric {int(stats[28])} (default {int(default[28])})")
    assert want["ok"] and 0 < stats[30] < default[30] and stats[28] == default[28]


# ------------------------------------------------------------------------------------------------- block and chunk edges
@pytest.mark.parametrize("W,H", EDGE_FRAMES, ids=[f"{w}x{h}" for w, h in EDGE_FRAMES])
def test_step_at_the_block_and_chunk_edges(W, H):
    s, m = start_frame(W, H), edge_step(W, H)
    out = run_step(s, 1, True, INF)
    check_step(out, m, s, f"{W}x{H}, {-(-W * H // M.BLOCK)} blocks")
    last = np.arange(W * H) >= (-(-W * H // M.BLOCK) - 1) * M.BLOCK
    in_last = int((((out.flags.cpu().numpy() & 4) != 0) & last).sum())
    print(f"{W}x{H}: associated in the last block {in_last}")
    assert in_last > 0


def test_one_scratch_serves_65_then_5_then_65_blocks():
    """the finisher's second trip (one row) and then a grid shorter than one trip on the same scratch: nothing of the longer
    run's rows is read again, and the ticket is left at zero"""
    s = start_frame(256, 520)
    scratch = torch.zeros(icp._capi.load().dgr_icp_scratch_bytes(256, 520, 1), dtype=torch.uint8, device=DEV)
    for stride in (1, 4, 1):
        fresh, reused = run_step(s, stride, True, INF), run_step(s, stride, True, INF, scratch=scratch)
        blocks = -(-(-(-256 // stride) * -(-520 // stride)) // M.BLOCK)
        print(f"256x520/{stride}: {blocks} blocks, count {int(fresh.stats[0, 28])}, same bits {same_bits(fresh, reused)}, ticket "
              f"{int(scratch[:4].view(torch.int32)[0])}")
        assert blocks == {1: 65, 4: 5}[stride] and float(fresh.stats[0, 29]) == 1.0
        assert same_bits(fresh, reused)
        assert not scratch[:16].any()


# -------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", ["half_y", "near_z", "perm120", "far"])
def test_icp_align_at_a_world_frame_converges_as_the_model_does(name):
    s = moved_frame(name)
    out = slam.icp_align(T(s["depth_obs"]), T(s["model_depth"]), None, T(s["model_view"]), *intr(s), iterations=10, return_flags=True)
    want = M.icp_align_model(s["depth_obs"], s["model_depth"], None, s["model_view"], *intr(s), iterations=10)
    e_start, e_gpu, e_model = (M.pose_error(v, s["true_view"]) for v in (s["model_view"], out.viewmatrix.cpu().numpy(), want["viewmatrix"]))
    stats = out.stats.cpu().numpy()
    slack = 1e-5 * float(s["depth_obs"].max())
    print(f"{name}: pose error (rad, m) start {e_start[0]:.3e} {e_start[1]:.3e}  gpu {e_gpu[0]:.3e} {e_gpu[1]:.3e}  model "
          f"{e_model[0]:.3e} {e_model[1]:.3e}  slack {slack:.1e}; counts gpu {stats[:, 28].astype(int).tolist()} model {want['count']} "
          f"marked {want['marked']}; branch {M.quat_branch(M.pose_of(out.viewmatrix.cpu().numpy())[0])}")
    assert stats.shape == (10, 32)
    assert e_gpu[0] <= 2 * e_model[0] + slack and e_gpu[1] <= 2 * e_model[1] + slack
    assert e_gpu[0] < 0.05 * e_start[0] and e_gpu[1] < 0.05 * e_start[1]
    for k in range(10):
        assert stats[k, 29] == (1.0 if want["ok"][k] else 0.0) and abs(stats[k, 28] - want["count"][k]) <= want["marked"][k], k
    view, quat, trans = out.viewmatrix.cpu().numpy(), out.quat.cpu().numpy(), out.trans.cpu().numpy()
    assert np.array_equal(trans, view[3, :3]) and np.abs(M.quat_to_rotation(quat.astype(np.float64)) - view[:3, :3].T).max() <= 4 * ULP
    assert quat[0] >= 0


def test_rgbd_align_at_a_half_turn_converges_as_the_model_does():
    s = moved_plane_scene("half_x")
    out = hybrid.align(s, iterations=3, return_flags=True)
    want = R.rgbd_align_model(s["color_obs"], s["depth_obs"], s["model_color"], s["model_depth"], None, s["model_view"], *intr(s),
                              iterations=3)
    e_start, e_gpu, e_model = (M.pose_error(v, s["true_view"]) for v in (s["model_view"], out.viewmatrix.cpu().numpy(), want["viewmatrix"]))
    print(f"textured plane at half_x: pose error (rad, m) start {e_start[0]:.3e} {e_start[1]:.3e}  gpu {e_gpu[0]:.3e} {e_gpu[1]:.3e}  "
          f"model {e_model[0]:.3e} {e_model[1]:.3e}; branch {M.quat_branch(M.pose_of(out.viewmatrix.cpu().numpy())[0])}")
    hybrid.follows_the_model(out, want["rows"], "textured plane at half_x")
    assert all(r["ok"] for r in want["rows"]) and M.quat_branch(M.pose_of(want["viewmatrix"])[0]) == "x"
    assert e_gpu[0] <= max(2 * e_model[0], 1e-5) and e_gpu[1] <= max(2 * e_model[1], 1e-5)
    view, quat, trans = out.viewmatrix.cpu().numpy(), out.quat.cpu().numpy(), out.trans.cpu().numpy()
    assert np.array_equal(trans, view[3, :3]) and np.abs(M.quat_to_rotation(quat.astype(np.float64)) - view[:3, :3].T).max() <= 4 * ULP
    assert quat[0] >= 0


# ----------------------------------------------------------------------------------------------------------------- hand-off
def fp32_rotation_error():
    """the fp32 evaluation error of R(q) at |q| = 1: the largest distance between the fp32 replica of pose_forward_kernel
    (step_model.pose_closed_form) and the float64 model of the same view over step_model.pose_cases()"""
    c, P, exact = step_model.pose_cases(), step_model.pose_perspec(), step_model.pose_model64()["view"]
    worst = 0.0
    for i, label in enumerate(c["label"]):
        if label.endswith("at |q| = 1"):
            view = step_model.pose_closed_form(c["q"][i], c["t"][i], P, c["dview"][i], F=np.float32)[0]
            worst = max(worst, float(np.abs(view.astype(np.float64)[:3, :3] - exact[i][:3, :3]).max()))
    return worst


def test_the_tracker_rebuilds_the_step_s_view_from_its_quaternion_and_translation():
    """slam.pose_to_camera(quat, trans) against viewmatrix_out: the translation row bit for bit; the rotation block within the
    4 ulp of 1 that check_pose allows between the float64 R(quat) and the view, plus the fp32 evaluation error of R(q)"""
    evaluation = fp32_rotation_error()
    allowed = 4 * ULP + evaluation
    print(f"fp32 evaluation error of R(q) over the pose cases at |q| = 1: {evaluation:.3g} ({evaluation / ULP:.3g} ulp of 1); allowed "
          f"distance {allowed:.3g}")
    assert 0 < evaluation < 16 * ULP
    for name in M.NAMED_FRAMES:
        s = moved_frame(name)
        out = run_step(s, 1, True, INF)
        view = slam.pose_to_camera(out.quat, out.trans, 0.6, 0.45)[0].detach().cpu().numpy()
        ours = out.viewmatrix.cpu().numpy()
        distance = float(np.abs(view.astype(np.float64)[:3, :3] - ours.astype(np.float64)[:3, :3]).max())
        print(f"{name}: rotation block differs by at most {distance:.3g} ({distance / ULP:.3g} ulp of 1)")
        assert float(out.stats[0, 29]) == 1.0
        assert np.array_equal(view[3].view(np.uint32), ours[3].view(np.uint32)) and view[:, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
        assert distance <= allowed
