"""slam.depth_normals / slam.icp_align and the single step (dgr_amd.icp.icp_step) on the GPU against the float64 model
(tests/icp_model.py): the normal map at every pixel the model does not mark ambiguous, the step's flags bit for bit at unmarked
candidates, its 28 sums within the model's rounding bound evaluated over the kernel's own associated set, the solve and update
against the model's fed with the kernel's own sums, the refusals, convergence on the room-corner scene, determinism and hipGraph
replay.  Shapes are the smallest at which the kernels can go wrong: one interior pixel, a partial last row and column of the
stride grid, four blocks of candidates (block-order addition and the finisher), the workload's 640 x 480."""
import functools

import numpy as np
import pytest
import torch

from dgr_amd import icp, slam

import icp_model as M
from test_hip_guarded_buffers import GuardedTorch
from test_hip_keyframe_overlap import special_values
from test_icp_model import frame, max_jump_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
ULP = 2.0 ** -23  # of 1.0


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def intr(s):
    return s["fx"], s["fy"], s["cx"], s["cy"]


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- normals
def check_normals(depth, s, label, **kw):
    """runs slam.depth_normals on `depth` and compares with the model; prints the figures first"""
    gkw = dict(kw)
    if gkw.get("mask_image") is not None:
        gkw["mask_image"] = T(gkw["mask_image"])
    got = slam.depth_normals(T(depth), *intr(s), **gkw).cpu().numpy()
    m = M.depth_normals_model(depth, *intr(s), **kw)
    H, W = depth.shape
    assert got.shape == (H, W, 4) and got.dtype == np.float32
    usable = got[..., 3] != 0
    free = ~m["ambiguous"]
    both = usable & m["usable"] & free
    err = np.abs(got[..., :3] - m["vnmap"][..., :3]).max(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(both, err / m["bound"], 0.0)
    print(f"{label}: usable {int(usable.sum())} of {H * W}, marked {int(m['ambiguous'].sum())}, usable differs at unmarked "
          f"{int(((usable != m['usable']) & free).sum())}, largest |n - model| {err[both].max() if both.any() else 0:.3g}, "
          f"largest error / bound {ratio.max():.3g}")
    with np.errstate(invalid="ignore"):
        assert m["ambiguous"].sum() <= 0.01 * max(1, int((depth > 0).sum()))
    assert np.array_equal(usable[free], m["usable"][free])
    assert (ratio <= 1.0).all()
    assert np.array_equal(got[usable][:, 3].view(np.uint32), depth[usable].view(np.uint32))  # d: the input's bits
    assert not got[~usable].any()                                                            # unusable: four zeros (+0)
    assert np.all(np.abs(np.linalg.norm(got[usable][:, :3].astype(np.float64), axis=1) - 1.0) < 4 * ULP)
    yy, xx = np.mgrid[0:H, 0:W]
    rays = np.stack([(xx - s["cx"]) / s["fx"], (yy - s["cy"]) / s["fy"], np.ones((H, W))], -1)
    assert (np.sum(got[..., :3] * rays, -1)[usable & free] <= 0).all()  # facing the camera
    assert not usable[0].any() and not usable[-1].any() and not usable[:, 0].any() and not usable[:, -1].any()
    return got, m


NORMAL_FRAMES = [(3, 3, False), (3, 3, True), (67, 5, False), (67, 5, True), (24, 18, False), (24, 18, True), (96, 80, False),
                 (96, 80, True), (640, 480, True)]


@pytest.mark.parametrize("W,H,masked", NORMAL_FRAMES, ids=[f"{w}x{h}{'-mask' if m else ''}" for w, h, m in NORMAL_FRAMES])
def test_normals_against_the_model(monkeypatch, W, H, masked):
    guarded = GuardedTorch()
    monkeypatch.setattr(icp, "torch", guarded)
    s = frame(W, H)
    rng = np.random.default_rng(100 + W)
    clean = s["model_depth"]
    mask = rng.uniform(0.97, 1.0, (H, W)).astype(np.float32) if masked else None  # two thirds below the threshold
    got, m = check_normals(clean, s, f"{W}x{H} clean", max_jump=max_jump_of(W), mask_image=mask)
    assert guarded.check() == 1
    if not masked:
        interior = (H - 2) * (W - 2)
        assert m["usable"].sum() > 0.8 * interior if W >= 24 else m["usable"].sum() >= 1
    holes = special_values(rng, clean, share=0.08)
    if W == 3:
        holes[0, 1] = np.nan  # (nine pixels: the scatter alone rarely hits one)
    got, m = check_normals(holes, s, f"{W}x{H} special values", max_jump=max_jump_of(W), mask_image=mask)
    assert guarded.check() == 1
    if W >= 24:
        assert 0 < m["usable"].sum() < (H - 2) * (W - 2)
    else:
        assert W != 3 or not got.any()
    if W == 24:
        got, m = check_normals(holes, s, "depth range", max_jump=0.1, mask_image=mask, depth_range=(2.0, 3.2))
        assert 0 < m["usable"].sum() < (H - 2) * (W - 2)


def test_normals_of_a_constant_depth_and_a_depth_step():
    s = frame(24, 18)
    flat = np.full((18, 24), 2.5, np.float32)
    got, _ = check_normals(flat, s, "constant depth")
    assert np.all(got[1:-1, 1:-1, :2] == 0.0) and np.all(got[1:-1, 1:-1, 2] == -1.0) and np.all(got[1:-1, 1:-1, 3] == 2.5)
    step = flat.copy()
    step[:, 12:] = 2.5 * 1.08  # a step of 8 %: inside max_jump = 0.1 from the near side, 7.4 % from the far side
    got, m = check_normals(step, s, "8 % step, max_jump 0.1", max_jump=0.1)
    assert m["usable"][1:-1, 1:-1].all()
    got, m = check_normals(step, s, "8 % step, max_jump 0.075", max_jump=0.075)
    assert not got[1:-1, 11].any() and got[1:-1, 12, 3].all() and got[1:-1, 10, 3].all()  # only the near side sees a jump
    got, m = check_normals(step, s, "8 % step, max_jump 0.05", max_jump=0.05)
    assert not got[1:-1, 11:13].any() and got[1:-1, 13, 3].all()


# -------------------------------------------------------------------------------------------------------------------- step
@functools.lru_cache(maxsize=None)
def step_model(W, H, stride, with_obs, huber):
    s = frame(W, H)
    return M.icp_step_model(s["depth_obs"], s["vn_obs"] if with_obs else None, s["vn_model"], s["model_view"], s["view_in"], *intr(s),
                            stride=stride, huber_delta=huber)


def run_step(s, stride, with_obs, huber, **kw):
    return icp.icp_step(T(s["depth_obs"]), T(s["vn_obs"]) if with_obs else None, T(s["vn_model"]), T(s["model_view"]),
                        T(s["view_in"]), *intr(s), stride=stride, huber_delta=huber, return_flags=True, **kw)


STEP_CASES = ([(W, H, st, o, h) for W, H, st in ((3, 3, 1), (67, 5, 1), (67, 5, 3), (96, 80, 1), (640, 480, 4))
               for o in (True, False) for h in (INF, 0.01)] + [(640, 480, 1, True, INF)])


def check_step(out, m, s, label, conditioned=True, **solve):
    """A step's result `out` on the frame `s` against the model's step `m` of the same arguments: the flags bit for bit at
    unmarked candidates, the 28 sums within the model's bound over the kernel's own associated set, the solve and the update
    against the model's (with `solve`'s arguments) fed with the kernel's own sums.  Prints the figures first; returns (stats, want)."""
    flags, stats = out.flags.cpu().numpy(), out.stats.cpu().numpy()[0]
    amb = m["ambiguous"]
    differ = flags != m["flags"]
    associated = (flags & 4) != 0
    S29, B, mag = m["sums"](associated)
    allowed = B + 2.0 ** -50 * mag
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(allowed > 0, np.abs(stats[:28] - S29[:28]) / allowed, np.where(stats[:28] == S29[:28], 0.0, INF))
    print(f"{label}: S {m['S']} valid {m['valid']} associated {int(associated.sum())} "
          f"(model {int(m['associated'].sum())}) marked {int(amb.sum())} flags differ outside the marks {int((differ & ~amb).sum())} "
          f"inside {int((differ & amb).sum())}; largest |sum - model| / bound {ratio.max():.3g}; bound / sum |term| at most "
          f"{(B / (mag + 1e-300)).max():.3g}")
    assert flags.shape == (m["S"],) and amb.sum() <= 0.01 * m["valid"]
    assert not (differ & ~amb).any()
    assert ((flags & 1) == (m["flags"] & 1)).all()  # valid is a raw fp32 comparison: never ambiguous
    assert not (flags & ~np.uint8(7)).any() and not ((flags & 2) > (flags & 1) * 2).any() and not ((flags & 4) > (flags & 2) * 2).any()
    assert stats[28] == associated.sum() > 0
    assert (ratio <= 1.0).all()
    # the solve and the update: the model's, fed with the kernel's own sums
    want = M.solve_update(stats[:29], s["model_view"], s["view_in"], **solve)
    assert want["cond"] <= 1e3 or not conditioned
    check_pose(out, want, stats, label)
    return stats, want


@pytest.mark.parametrize("W,H,stride,with_obs,huber", STEP_CASES,
                         ids=[f"{w}x{h}-stride{st}{'-vn_obs' if o else ''}-huber{hu}" for w, h, st, o, hu in STEP_CASES])
def test_step_flags_sums_solve_and_update(W, H, stride, with_obs, huber):
    s = frame(W, H)
    out = run_step(s, stride, with_obs, huber)
    # (the two tiny frames are there for the sums, not for the solve)
    check_step(out, step_model(W, H, stride, with_obs, huber), s, f"{W}x{H}/{stride} vn_obs {with_obs} huber {huber}",
               conditioned=(W, H) not in ((3, 3), (67, 5)))


def check_pose(out, want, stats, label):
    """The kernel's pose against the model's solve and update of the kernel's own sums, by icp_model.pose_figures' standard
    (shared with the model's own tests): the viewmatrix within 2 ulp (and the solve's rounding) of the model's, R(quat) within
    4 ulp of 1 of the viewmatrix's rotation, |quat| within 2 ulp of 1, quat[0] >= 0, trans the viewmatrix's bits.  A refused step
    carries the input's bits: no tolerance."""
    fig = M.pose_figures(out.viewmatrix.cpu().numpy(), out.quat.cpu().numpy(), out.trans.cpu().numpy(), want)
    relative = max(1e-9, 16.0 * want["cond_solved"] * 2.0 ** -53) if want["ok"] else 0.0
    print(f"{label}: ok {stats[29]} (model {want['ok']}) cond {want['cond']:.3g} |omega| {stats[30]:.3g} |v| {stats[31]:.3g}; "
          f"viewmatrix_out differs by at most {fig['ulps'].max():.3g} ulp (allowed {fig['allowed']:.3g}); R(quat) - R "
          f"{fig['rot'] / ULP:.3g} ulp of 1; |quat| - 1 {(fig['norm'] - 1) / ULP:.3g} ulp; branch {want['branch']}")
    assert stats[29] == (1.0 if want["ok"] else 0.0)
    assert (fig["ulps"] <= fig["allowed"]).all()
    assert abs(stats[30] - want["omega"]) <= relative * max(want["omega"], 1e-3) and abs(stats[31] - want["v"]) <= relative * max(want["v"], 1e-3)
    assert fig["last_column"]
    assert fig["rot"] <= 4 * ULP and abs(fig["norm"] - 1.0) <= 2 * ULP and fig["r"] >= 0
    assert fig["trans_bits"]
    assert M.pose_holds(fig)


def test_aliased_in_and_out_give_the_bits_of_separate_buffers():
    s = frame(96, 80)
    separate = run_step(s, 1, True, INF)
    pose = T(s["view_in"])
    aliased = icp.icp_step(T(s["depth_obs"]), T(s["vn_obs"]), T(s["vn_model"]), T(s["model_view"]), pose, *intr(s),
                           viewmatrix_out=pose, return_flags=True)
    assert aliased.viewmatrix.data_ptr() == pose.data_ptr() and same_bits(separate, aliased)
    assert not np.array_equal(pose.cpu().numpy(), s["view_in"])  # (the step moved the pose)


def test_one_scratch_serves_every_stride_in_stream_order():
    """the ticket is left at zero: the steps of several strides run back to back on one zero-filled scratch"""
    s = frame(96, 80)
    scratch = torch.zeros(icp._capi.load().dgr_icp_scratch_bytes(96, 80, 1), dtype=torch.uint8, device=DEV)
    for stride in (1, 3, 1, 2, 1):
        fresh, reused = run_step(s, stride, True, INF), run_step(s, stride, True, INF, scratch=scratch)
        assert same_bits(fresh, reused)
    assert not scratch[:16].any()


# --------------------------------------------------------------------------------------------------------------- refusals
def refused_keeps_the_input(out, view_in, label):
    stats = out.stats.cpu().numpy()[0]
    view, quat, trans = out.viewmatrix.cpu().numpy(), out.quat.cpu().numpy(), out.trans.cpu().numpy()
    print(f"{label}: ok {stats[29]} count {stats[28]}")
    assert stats[29] == 0.0 and stats[30] == 0.0 and stats[31] == 0.0
    assert np.array_equal(view.view(np.uint32), view_in.view(np.uint32))
    assert np.array_equal(trans.view(np.uint32), view_in[3, :3].view(np.uint32))
    R, _ = M.pose_of(view_in)
    assert np.abs(M.quat_to_rotation(quat.astype(np.float64)) - R).max() <= 4 * ULP and quat[0] >= 0
    return stats


def test_refusals_on_the_device():
    s = frame(24, 18)
    args = lambda depth: (T(depth), T(s["vn_obs"]), T(s["vn_model"]), T(s["model_view"]), T(s["view_in"]), *intr(s))  # noqa: E731
    for fill in (0.0, np.nan, -1.0):
        stats = refused_keeps_the_input(icp.icp_step(*args(np.full((18, 24), fill, np.float32))), s["view_in"], f"all {fill}")
        assert stats[28] == 0 and not stats[:28].any()
    good = icp.icp_step(*args(s["depth_obs"]))
    count = int(good.stats[0, 28])
    assert float(good.stats[0, 29]) == 1.0 and count > 100
    refused_keeps_the_input(icp.icp_step(*args(s["depth_obs"]), min_points=count + 1), s["view_in"], "count below min_points")
    assert float(icp.icp_step(*args(s["depth_obs"]), min_points=count).stats[0, 29]) == 1.0
    refused_keeps_the_input(icp.icp_step(*args(s["depth_obs"]), rcond=0.5), s["view_in"], "rcond 0.5")


def test_the_fronto_parallel_plane_is_refused_and_solves_under_damping():
    p = M.fronto_parallel_scene(24, 18)
    eye = p["model_view"]
    vn = M.depth_normals_model(p["model_depth"], *intr(p))["vnmap"].astype(np.float32)
    nearer = np.full((18, 24), 1.99, np.float32)  # the observation: the same plane 1 cm nearer
    vn_obs = M.depth_normals_model(nearer, *intr(p))["vnmap"].astype(np.float32)
    args = (T(nearer), T(vn_obs), T(vn), T(eye), T(eye), *intr(p))
    stats = refused_keeps_the_input(icp.icp_step(*args), eye, "fronto-parallel plane")
    A, b, _, count = M.unpack(stats[:29])
    assert count == 22 * 16 and b[5] != 0.0
    for k in (2, 3, 4):  # omega_z, v_x, v_y: exactly zero rows
        assert not A[k].any() and not A[:, k].any() and b[k] == 0.0
    out = icp.icp_step(*args, damping=1e-3)
    stats = out.stats.cpu().numpy()[0]
    want = M.solve_update(stats[:29], eye, eye, damping=1e-3)
    assert want["ok"] and np.all(want["xi"][[2, 3, 4]] == 0.0) and np.all(want["xi"][[0, 1, 5]] != 0.0)
    check_pose(out, want, stats, "fronto-parallel plane, damping 1e-3")
    view = out.viewmatrix.cpu().numpy().astype(np.float64)
    assert abs(view[0, 1]) < 1e-6 and abs(view[1, 0]) < 1e-6  # no rotation about z (second order in omega_x omega_y only)
    assert -0.011 < view[3, 2] < -0.009 and abs(view[3, 0]) < 1e-4 and abs(view[3, 1]) < 1e-4  # the camera stands 1 cm nearer


# -------------------------------------------------------------------------------------------------------------- end to end
ALIGN = [(96, 80, (1,) * 10), (640, 480, (4,) * 10)]


def align_args(s):
    return (T(s["depth_obs"]), T(s["model_depth"]), None, T(s["model_view"]), *intr(s))


@functools.lru_cache(maxsize=None)
def align_model(W, H, strides):
    s = frame(W, H)
    return M.icp_align_model(s["depth_obs"], s["model_depth"], None, s["model_view"], *intr(s), iterations=len(strides), strides=strides)


@pytest.mark.parametrize("W,H,strides", ALIGN, ids=["96x80-stride1", "640x480-stride4"])
def test_icp_align_converges_as_the_model_does(W, H, strides):
    s = frame(W, H)
    out = slam.icp_align(*align_args(s), iterations=len(strides), strides=strides, return_flags=True)
    want = align_model(W, H, strides)
    e_start, e_gpu, e_model = (M.pose_error(v, s["true_view"]) for v in (s["model_view"], out.viewmatrix.cpu().numpy(), want["viewmatrix"]))
    stats = out.stats.cpu().numpy()
    slack = 1e-5 * float(s["depth_obs"].max())
    print(f"{W}x{H} strides {strides[0]}: pose error (rad, m) start {e_start[0]:.3e} {e_start[1]:.3e}  gpu {e_gpu[0]:.3e} {e_gpu[1]:.3e}  "
          f"model {e_model[0]:.3e} {e_model[1]:.3e}  slack {slack:.1e}; counts gpu {stats[:, 28].astype(int).tolist()} model "
          f"{want['count']} marked {want['marked']}")
    assert stats.shape == (len(strides), 32) and out.stats.dtype == torch.float64
    assert e_gpu[0] <= 2 * e_model[0] + slack and e_gpu[1] <= 2 * e_model[1] + slack
    assert e_gpu[0] < 0.05 * e_start[0] and e_gpu[1] < 0.05 * e_start[1]
    for k in range(len(strides)):
        assert stats[k, 29] == (1.0 if want["ok"][k] else 0.0) and abs(stats[k, 28] - want["count"][k]) <= want["marked"][k], k
    flags = out.flags.cpu().numpy()
    assert flags.shape == (-(-W // strides[-1]) * -(-H // strides[-1]),) and int(((flags >> 2) & 1).sum()) == stats[-1, 28]
    view, quat, trans = out.viewmatrix.cpu().numpy(), out.quat.cpu().numpy(), out.trans.cpu().numpy()
    assert np.array_equal(trans, view[3, :3]) and np.abs(M.quat_to_rotation(quat.astype(np.float64)) - view[:3, :3].T).max() <= 4 * ULP


def test_icp_align_without_observation_normals_from_a_given_estimate_and_with_a_silhouette():
    s = frame(96, 80)
    opacity = np.ones((80, 96), np.float32)
    opacity[:, :20] = 0.5  # the model is trusted on the right part of the image only
    out = slam.icp_align(T(s["depth_obs"]), T(s["model_depth"])[None], T(s["view_in"]), T(s["model_view"]), *intr(s), iterations=6,
                         strides=(2, 2, 2, 1, 1, 1), use_obs_normals=False, opacity_map=T(opacity)[None], huber_delta=0.02)
    want = M.icp_align_model(s["depth_obs"], s["model_depth"], s["view_in"], s["model_view"], *intr(s), iterations=6,
                             strides=(2, 2, 2, 1, 1, 1), use_obs_normals=False, opacity_map=opacity, huber_delta=0.02)
    stats = out.stats.cpu().numpy()
    e_gpu, e_model = M.pose_error(out.viewmatrix.cpu().numpy(), s["true_view"]), M.pose_error(want["viewmatrix"], s["true_view"])
    print("silhouette, no vn_obs: gpu", e_gpu, "model", e_model, stats[:, 28].tolist(), want["count"], want["marked"])
    assert out.flags is None and stats[:, 29].tolist() == [1.0] * 6
    slack = 1e-5 * float(s["depth_obs"].max())
    assert e_gpu[0] <= 2 * e_model[0] + slack and e_gpu[1] <= 2 * e_model[1] + slack
    for k in range(6):
        assert abs(stats[k, 28] - want["count"][k]) <= want["marked"][k], k
    assert stats[3, 28] > 3 * stats[2, 28]  # stride 2 -> 1


# ---------------------------------------------------------------------------------------------------- run to run and replay
def test_two_runs_give_the_same_bits():
    s = frame(96, 80)
    a = slam.icp_align(*align_args(s), iterations=4, return_flags=True)
    b = slam.icp_align(*align_args(s), iterations=4, return_flags=True)
    assert same_bits(a, b)
    d = T(special_values(np.random.default_rng(5), s["model_depth"]))
    assert torch.equal(bits(slam.depth_normals(d, *intr(s))), bits(slam.depth_normals(d, *intr(s))))


def test_replayed_from_a_hipgraph():
    """captured once, replayed on another frame's depths written into the same buffers: that frame's eager bits"""
    old, new = frame(96, 80), M.corner_scene(96, 80, twist=-0.6 * M.TWIST)
    held = {n: T(old[n]) for n in ("depth_obs", "model_depth", "model_view")}

    def run(t):
        return slam.icp_align(t["depth_obs"], t["model_depth"], None, t["model_view"], *intr(old), iterations=4,
                              strides=(2, 2, 1, 1), return_flags=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run(held)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(held)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, run(held))
    for n in ("depth_obs", "model_depth"):
        held[n].copy_(T(new[n]))
    graph.replay()
    torch.cuda.synchronize()
    eager = run({n: T(new[n]) for n in ("depth_obs", "model_depth", "model_view")})
    assert same_bits(out, eager)
    assert float(eager.stats[-1, 29]) == 1.0 and not torch.equal(eager.viewmatrix, T(old["model_view"]))
    e = M.pose_error(eager.viewmatrix.cpu().numpy(), new["true_view"])
    assert e[0] < 2e-3 and e[1] < 2e-3


def test_nothing_is_written_outside_the_buffers_of_icp_align(monkeypatch):
    guarded = GuardedTorch()
    monkeypatch.setattr(icp, "torch", guarded)
    s = frame(67, 5)
    out = slam.icp_align(*align_args(s), iterations=3, strides=(3, 2, 1), max_jump=max_jump_of(67), return_flags=True)
    assert guarded.check() == 6  # the maps, the pose, quat + trans, the stats, the flags, the scratch
    assert out.flags.shape == (67 * 5,) and out.stats.shape == (3, 32)
