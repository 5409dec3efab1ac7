"""slam.intensity_map / slam.halve_frame / slam.rgbd_align and the single hybrid step (dgr_amd.rgbd.rgbd_step) on the GPU against
the float64 model (tests/rgbd_model.py): the intensity map within the model's bound with the usable flag bit for bit, the halved
planes bit for bit, the step's flags bit for bit at unmarked candidates, its 31 sums within the model's rounding bound evaluated
over the kernel's own pairs, the solve and update to test_hip_icp's standard, photo_weight = 0 against dgr_icp_step's bits, the
textured fronto-parallel plane that ICP refuses, the pyramid case, aliasing, one scratch, refusals, determinism, hipGraph replay
and guard bands."""
import functools

import numpy as np
import pytest
import torch

from dgr_amd import icp, rgbd, slam

import icp_model as M
import rgbd_model as R
from test_hip_guarded_buffers import GuardedTorch
from test_hip_icp import T, bits, check_pose, intr, refused_keeps_the_input, same_bits
from test_rgbd_model import HUBERS, MAP_FRAMES, WEIGHTS, corner_frame, map_frame, right_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")


# -------------------------------------------------------------------------------------------------------------------- map
def check_map(image, mask, label):
    got = slam.intensity_map(T(image), mask_image=None if mask is None else T(mask)).cpu().numpy()
    m = R.intensity_map_model(image, mask_image=mask)
    H, W = image.shape[-2:]
    assert got.shape == (H, W, 4) and got.dtype == np.float32
    usable = got[..., 3] != 0
    err = np.abs(got[..., :3] - m["imap"][..., :3])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(usable[..., None] & (m["bound"] > 0), err / m["bound"], np.where(err == 0, 0.0, INF))
    print(f"{label}: usable {int(usable.sum())} of {H * W} (model {int(m['usable'].sum())}), largest error / bound {ratio.max():.3g}")
    assert not m["ambiguous"].any() and np.array_equal(usable, m["usable"])
    assert (ratio[usable] <= 1.0).all()
    assert np.all(got[usable][:, 3] == 1.0) and not got[~usable].any()  # u = 1.0f; unusable: four zeros (+0)
    if image.shape[0] == 1:
        assert np.array_equal(got[usable][:, 0].view(np.uint32), image[0][usable].view(np.uint32))  # the single channel's bits
    return got, m


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("W,H", MAP_FRAMES, ids=[f"{w}x{h}" for w, h in MAP_FRAMES])
def test_intensity_map_against_the_model(monkeypatch, W, H, masked):
    guarded = GuardedTorch()
    monkeypatch.setattr(rgbd, "torch", guarded)
    for seed in (0, 1):  # one and three channels
        image, mask = map_frame(W, H, masked, seed)
        got, m = check_map(image, mask, f"{W}x{H} seed {seed}")
        assert guarded.check() == 1
        if not masked:
            assert m["usable"].sum() == (H - 2) * (W - 2)
        # a non-finite pixel poisons exactly its 3 x 3 neighbourhood
        y, x = (H // 2, W // 2) if W > 3 else (1, 1)
        for value in (np.nan, np.inf, -np.inf):
            hurt = image.copy()
            hurt[-1, y, x] = value
            bad, _ = check_map(hurt, mask, f"{W}x{H} seed {seed} {value} at ({x}, {y})")
            near = np.zeros((H, W), bool)
            near[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
            assert not bad[near].any()
            assert np.array_equal(bad[~near].view(np.uint32), got[~near].view(np.uint32))
        guarded.check()


# ------------------------------------------------------------------------------------------------------------------ halve
@pytest.mark.parametrize("W,H", [(3, 3), (67, 5), (96, 80)], ids=["3x3", "67x5", "96x80"])
def test_halve_frame_against_the_model(monkeypatch, W, H):
    guarded = GuardedTorch()
    monkeypatch.setattr(rgbd, "torch", guarded)
    rng = np.random.default_rng(W)
    planes = rng.standard_normal((3, H, W)).astype(np.float32)
    planes[1, H // 2, W // 2] = np.nan
    depth = corner_frame(W, H)["model_depth"].copy() if W > 3 else np.full((3, 3), 2.0, np.float32)
    holes = rng.random((H, W))
    depth[holes < 0.1], depth[(holes > 0.1) & (holes < 0.13)] = 0.0, np.nan
    depth[(holes > 0.9)] *= 1.2  # steps beyond max_jump
    for kw in (dict(), dict(depth_range=(0.5, 2.5), max_jump=0.3)):
        got_p, got_d = slam.halve_frame(T(planes), T(depth), **kw)
        assert guarded.check() == 2
        m = R.halve_model(planes, depth, **kw)
        assert tuple(got_p.shape) == (3, H // 2, W // 2) and tuple(got_d.shape) == (H // 2, W // 2)
        gp = got_p.cpu().numpy()
        assert np.array_equal(np.isnan(gp), np.isnan(m["planes"])) and np.isnan(gp).sum() == 1
        assert np.array_equal(gp[~np.isnan(gp)].view(np.uint32), m["planes"][~np.isnan(gp)].view(np.uint32))
        free = ~m["ambiguous"]
        d = got_d.cpu().numpy()
        print(f"{W}x{H} {kw}: depths kept {int((d > 0).sum())} of {d.size}, marked {int(m['ambiguous'].sum())}")
        assert m["ambiguous"].sum() <= 0.01 * d.size and np.array_equal(d[free].view(np.uint32), m["depth"][free].view(np.uint32))
        assert W == 3 or 0 < (d > 0).sum() < d.size
    only_d = slam.halve_frame(None, T(depth))
    only_p = slam.halve_frame(T(planes[:1]))
    assert only_d[0] is None and only_p[1] is None and torch.equal(bits(only_p[0]), bits(got_p[:1]))
    assert np.array_equal(only_d[1].cpu().numpy().view(np.uint32), R.halve_model(None, depth)["depth"].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- step
def run_step(s, stride, with_obs=True, weights=(1.0, 1.0), hubers=(INF, INF), **kw):
    return rgbd.rgbd_step(T(s["depth_obs"]), T(s["vn_obs"]) if with_obs else None, T(s["vn_model"]), T(s["color_obs"]),
                          T(s["imap_model"]), T(s["model_view"]), T(s["view_in"]), *intr(s), stride=stride, geo_weight=weights[0],
                          photo_weight=weights[1], huber_delta=hubers[0], photo_huber=hubers[1], return_flags=True, **kw)


STEP_CASES = [(W, H, st, w, h) for W, H, st in ((3, 3, 1), (67, 5, 1), (67, 5, 3), (96, 80, 1), (640, 480, 4)) for w in WEIGHTS
              for h in HUBERS] + [(256, 520, 1, WEIGHTS[0], HUBERS[0])]  # (65 blocks: the finisher's second trip through its LDS)


def check_step(out, m, s, label, weights=(1.0, 1.0), **solve):
    """A hybrid step's result `out` on the frame `s` against the model's step `m` of the same arguments: the flags bit for bit at
    unmarked candidates, the 31 sums within the model's bound over the kernel's own pairs, the solve and the update to
    test_hip_icp's standard (with `solve`'s arguments).  Prints the figures first; returns (stats, want)."""
    flags, stats = out.flags.cpu().numpy(), out.stats.cpu().numpy()[0]
    amb = m["ambiguous"]
    differ = flags != m["flags"]
    geometric, photometric = (flags & 4) != 0, (flags & 8) != 0
    S31, B, mag = m["sums"](geometric, photometric)
    allowed = B + 2.0 ** -50 * mag
    sums = [k for k in range(31) if k not in (28, 30)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(allowed > 0, np.abs(stats[:31] - S31) / allowed, np.where(stats[:31] == S31, 0.0, INF))[sums]
    print(f"{label}: S {m['S']} valid {m['valid']} geometric {int(geometric.sum())} "
          f"photometric {int(photometric.sum())} (model {int(m['geometric'].sum())}, {int(m['photometric'].sum())}) marked "
          f"{int(amb.sum())} flags differ outside the marks {int((differ & ~amb).sum())} inside {int((differ & amb).sum())}; largest "
          f"|sum - model| / bound {ratio.max():.3g}; bound / sum |term| at most {(B / (mag + 1e-300)).max():.3g}")
    assert flags.shape == (m["S"],) and stats.shape == (40,) and amb.sum() <= 0.01 * m["valid"]
    assert not (differ & ~amb).any()
    assert ((flags & 1) == (m["flags"] & 1)).all() and not (flags & ~np.uint8(15)).any()
    assert not ((flags & 2) > (flags & 1) * 2).any() and not ((flags & 4) > (flags & 2) * 2).any() and not ((flags & 8) > (flags & 2) * 4).any()
    assert stats[28] == (geometric.sum() if weights[0] > 0 else 0) and stats[30] == photometric.sum() > 0
    assert (ratio <= 1.0).all() and not stats[34:].any()
    want = R.solve_update(stats[:31], s["model_view"], s["view_in"], **solve)
    icp_like = np.concatenate([R.as_icp_sums(stats[:31]), stats[31:34]])  # check_pose reads ok, |omega|, |v| at [29..31]
    check_pose(out, want, icp_like, label)
    return stats, want


@pytest.mark.parametrize("W,H,stride,weights,hubers", STEP_CASES,
                         ids=[f"{w}x{h}-stride{st}-geo{g[0]}-huber{hu[0]}" for w, h, st, g, hu in STEP_CASES])
def test_step_flags_sums_solve_and_update(W, H, stride, weights, hubers):
    s = corner_frame(W, H)
    out = run_step(s, stride, True, weights, hubers)
    check_step(out, right_step(W, H, stride, weights, hubers), s, f"{W}x{H}/{stride} weights {weights} hubers {hubers}", weights)


def test_photo_weight_zero_carries_the_bits_of_the_icp_step():
    s = corner_frame(96, 80)
    for with_obs, huber in ((True, INF), (False, 0.01)):
        ours = run_step(s, 1, with_obs, (1.0, 0.0), (huber, INF))
        theirs = icp.icp_step(T(s["depth_obs"]), T(s["vn_obs"]) if with_obs else None, T(s["vn_model"]), T(s["model_view"]),
                              T(s["view_in"]), *intr(s), huber_delta=huber, return_flags=True)
        assert same_bits((ours.viewmatrix, ours.quat, ours.trans), (theirs.viewmatrix, theirs.quat, theirs.trans))
        a, b = ours.stats[0].cpu().numpy(), theirs.stats[0].cpu().numpy()
        assert np.array_equal(a[:29].view(np.uint64), b[:29].view(np.uint64)) and a[29] == 0.0 and a[30] == 0.0
        assert np.array_equal(a[31:34].view(np.uint64), b[29:32].view(np.uint64)) and a[31] == 1.0
        assert torch.equal(ours.flags & 7, theirs.flags) and int((ours.flags & 8).ne(0).sum()) > 5000


def test_aliased_in_and_out_and_one_scratch_across_strides():
    s = corner_frame(96, 80)
    separate = run_step(s, 1)
    pose = T(s["view_in"])
    aliased = rgbd.rgbd_step(T(s["depth_obs"]), T(s["vn_obs"]), T(s["vn_model"]), T(s["color_obs"]), T(s["imap_model"]),
                             T(s["model_view"]), pose, *intr(s), viewmatrix_out=pose, return_flags=True)
    assert aliased.viewmatrix.data_ptr() == pose.data_ptr() and same_bits(separate, aliased)
    assert not np.array_equal(pose.cpu().numpy(), s["view_in"])
    scratch = torch.zeros(rgbd._capi.load().dgr_rgbd_scratch_bytes(96, 80, 1), dtype=torch.uint8, device=DEV)
    for stride in (1, 3, 1, 2, 1):
        assert same_bits(run_step(s, stride), run_step(s, stride, scratch=scratch))
    assert not scratch[:16].any()


def test_refusals_keep_the_input_s_bits():
    s = corner_frame(24, 18)
    as_icp = lambda out: type(out)(out.viewmatrix, out.quat, out.trans, torch.cat([out.stats[:, :29], out.stats[:, 31:34]], 1), out.flags)  # noqa: E731,E501
    for fill in (0.0, np.nan):
        out = run_step(dict(s, depth_obs=np.full((18, 24), fill, np.float32)), 1)
        stats = refused_keeps_the_input(as_icp(out), s["view_in"], f"all {fill}")
        assert not out.stats[0, :31].any()
    good = run_step(s, 1)
    count = int(good.stats[0, 28] + good.stats[0, 30])
    assert float(good.stats[0, 31]) == 1.0 and good.stats[0, 28] > 100 and good.stats[0, 30] > 100
    refused_keeps_the_input(as_icp(run_step(s, 1, min_points=count + 1)), s["view_in"], "both counts together below min_points")
    assert float(run_step(s, 1, min_points=count).stats[0, 31]) == 1.0
    refused_keeps_the_input(as_icp(run_step(s, 1, rcond=0.5)), s["view_in"], "rcond 0.5")
    nan_color = run_step(dict(s, color_obs=np.full((18, 24), np.nan, np.float32)), 1)  # no photometric pair: the geometric step
    assert float(nan_color.stats[0, 30]) == 0.0 and float(nan_color.stats[0, 31]) == 1.0 and not (nan_color.flags & 8).any()
    tight = run_step(s, 1, photo_max=0.0)
    assert float(tight.stats[0, 30]) == float(((tight.flags & 8) != 0).sum()) < float(good.stats[0, 30])  # only r_p = 0 is left


# ------------------------------------------------------------------------------------------------- the plane ICP refuses
def align(s, **kw):
    return slam.rgbd_align(T(s["color_obs"]), T(s["depth_obs"]), T(s["model_color"]), T(s["model_depth"]), None, T(s["model_view"]),
                           *intr(s), **kw)


@functools.lru_cache(maxsize=None)
def plane_model(iterations):
    s = R.textured_plane_scene(96, 80)
    return R.rgbd_align_model(s["color_obs"], s["depth_obs"], s["model_color"], s["model_depth"], None, s["model_view"], *intr(s),
                              iterations=iterations)


def follows_the_model(out, rows, label):
    stats = out.stats.cpu().numpy()
    print(f"{label}: counts gpu {stats[:, 28].astype(int).tolist()} {stats[:, 30].astype(int).tolist()} model "
          f"{[(r['count_g'], r['count_p'], r['marked']) for r in rows]}")
    assert stats.shape == (len(rows), 40)
    for k, r in enumerate(rows):
        assert stats[k, 31] == (1.0 if r["ok"] else 0.0), k
        assert abs(stats[k, 28] - r["count_g"]) <= r["marked"] and abs(stats[k, 30] - r["count_p"]) <= r["marked"], k


def test_the_textured_fronto_parallel_plane_is_refused_by_icp_and_aligned_by_the_hybrid_step():
    s = R.textured_plane_scene(96, 80)
    refused = slam.icp_align(T(s["depth_obs"]), T(s["model_depth"]), None, T(s["model_view"]), *intr(s), iterations=1)
    assert float(refused.stats[0, 29]) == 0.0 and float(refused.stats[0, 28]) > 5000
    assert torch.equal(bits(refused.viewmatrix), bits(T(s["model_view"])))
    imap, vn = slam.intensity_map(T(s["model_color"])), slam.depth_normals(T(s["model_depth"]), *intr(s))
    one = rgbd.rgbd_step(T(s["depth_obs"]), None, vn, T(s["color_obs"][0]), imap, T(s["model_view"]), T(s["model_view"]), *intr(s))
    assert float(one.stats[0, 31]) == 1.0
    out = align(s, iterations=3, return_flags=True)
    want = plane_model(3)
    e_start, e_gpu, e_model = (M.pose_error(v, s["true_view"]) for v in (s["model_view"], out.viewmatrix.cpu().numpy(), want["viewmatrix"]))
    print(f"textured plane: pose error (rad, m) start {e_start[0]:.3e} {e_start[1]:.3e}  gpu {e_gpu[0]:.3e} {e_gpu[1]:.3e}  model "
          f"{e_model[0]:.3e} {e_model[1]:.3e}")
    follows_the_model(out, want["rows"], "textured plane")
    assert e_gpu[0] <= max(2 * e_model[0], 1e-5) and e_gpu[1] <= max(2 * e_model[1], 1e-5)
    view, quat, trans = out.viewmatrix.cpu().numpy(), out.quat.cpu().numpy(), out.trans.cpu().numpy()
    assert np.array_equal(trans, view[3, :3]) and np.abs(M.quat_to_rotation(quat.astype(np.float64)) - view[:3, :3].T).max() <= 4 * 2.0 ** -23
    flags = out.flags.cpu().numpy()
    assert flags.shape == (96 * 80,) and int(((flags >> 3) & 1).sum()) == out.stats[-1, 30]


def test_the_pyramid_case():
    """640 x 480, a texture with a period of a few pixels: one level stays where the model stays, five levels converge as the
    model does (tests/golden/rgbd_pyramid_640x480.json: the model's figures, recorded by tests/rgbd_model.py)"""
    s, g = R.pyramid_scene(), R.golden()
    for run, kw in R.PYRAMID_RUNS.items():
        out = align(s, **kw)
        e_gpu, e_model = M.pose_error(out.viewmatrix.cpu().numpy(), s["true_view"]), g[run]["pose_error"]
        print(f"{run}: pose error (rad, m) gpu {e_gpu[0]:.3e} {e_gpu[1]:.3e}  model {e_model[0]:.3e} {e_model[1]:.3e}")
        follows_the_model(out, g[run]["rows"], run)
        assert e_gpu[0] <= max(2 * e_model[0], 1e-5) and e_gpu[1] <= max(2 * e_model[1], 1e-5)
    assert e_gpu[0] < 2e-5 and e_gpu[1] < 2e-5  # (five levels, the last run)


# ---------------------------------------------------------------------------------------- run to run, replay, guard bands
def test_two_runs_give_the_same_bits_with_a_silhouette_and_levels():
    s = R.textured_plane_scene(96, 80)
    opacity = np.ones((80, 96), np.float32)
    opacity[:, :20] = 0.5
    kw = dict(levels=3, iterations=(2, 2, 1), strides=(1, 1, 1, 2, 1), opacity_map=T(opacity), photo_huber=0.05, huber_delta=0.02,
              return_flags=True)
    a, b = align(s, **kw), align(s, **kw)
    assert same_bits(a, b) and a.stats[:, 31].tolist() == [1.0] * 5
    want = R.rgbd_align_model(s["color_obs"], s["depth_obs"], s["model_color"], s["model_depth"], None, s["model_view"], *intr(s),
                              levels=3, iterations=(2, 2, 1), strides=(1, 1, 1, 2, 1), opacity_map=opacity, photo_huber=0.05,
                              huber_delta=0.02)
    follows_the_model(a, want["rows"], "three levels, silhouette")
    e_gpu, e_model = M.pose_error(a.viewmatrix.cpu().numpy(), s["true_view"]), M.pose_error(want["viewmatrix"], s["true_view"])
    assert e_gpu[0] <= max(2 * e_model[0], 1e-5) and e_gpu[1] <= max(2 * e_model[1], 1e-5)


def test_replayed_from_a_hipgraph():
    """captured once, replayed on another frame's images written into the same buffers: that frame's eager bits"""
    old, new = R.textured_plane_scene(96, 80), R.textured_plane_scene(96, 80, twist=-0.6 * R.TEXTURED_TWIST)
    names = ("color_obs", "depth_obs", "model_color", "model_depth", "model_view")
    held = {n: T(old[n]) for n in names}

    def run(t):
        return slam.rgbd_align(t["color_obs"], t["depth_obs"], t["model_color"], t["model_depth"], None, t["model_view"], *intr(old),
                               levels=2, iterations=2, return_flags=True)

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
    for n in ("color_obs", "depth_obs"):
        held[n].copy_(T(new[n]))
    graph.replay()
    torch.cuda.synchronize()
    eager = run({n: T(new[n]) for n in names})
    assert same_bits(out, eager)
    assert float(eager.stats[-1, 31]) == 1.0
    e = M.pose_error(eager.viewmatrix.cpu().numpy(), new["true_view"])
    assert e[0] < 1e-3 and e[1] < 1e-3


def test_nothing_is_written_outside_the_buffers_of_rgbd_align(monkeypatch):
    guarded = GuardedTorch()
    monkeypatch.setattr(rgbd, "torch", guarded)
    s = R.textured_plane_scene(67, 13)
    out = align(s, levels=2, iterations=(1, 2), strides=(1, 2, 1), opacity_map=T(np.ones((13, 67), np.float32)), return_flags=True)
    assert guarded.check() == 6  # the arena of images and maps, the pose, quat + trans, the stats, the flags, the scratch
    assert out.flags.shape == (67 * 13,) and out.stats.shape == (3, 40)
