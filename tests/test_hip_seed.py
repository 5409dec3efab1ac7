"""dgr_amd.optim.seed_from_frame (csrc/seed.hip: decide, scan, apply) against the sequential restatement of its semantics in torch
on the CPU (tests/seed_model.py).  Counts, selection and order, every copied row, moments, accumulators and every constant or
colour row are compared bit for bit; the new positions and log-scales against the model's float64 ones."""
import numpy as np
import pytest
import torch

import cameras
from seed_model import seed_masks, seed_model
from dgr_amd.optim import densify_and_prune, seed_from_frame
from hip_helpers import dev
from map_step_cases import assert_rebuilt, bits_equal, leaves_of, moments_of, on_device

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
ACCS = ("xyz_gradient_accum", "denom", "max_radii2D")
FILL = {"label": 7.0, "aux4": -0.25}  # (f_rest and sh48 take the default 0)


def camera(W, H, pose=0.3):
    """an off-centre pinhole camera with fx != fy at a tilted pose"""
    R, t = cameras._synth_pose(pose)
    f = max(W, 64)  # (a pixel's footprint at depth 3 and stride 3 stays below exp(-1): see the log-scale bound)
    return cameras.Camera("seed", W, H, 0.9 * f, 0.8 * f, (W - 1) / 2 + 0.1 * W, (H - 1) / 2 - 0.15 * H, R, t)


def frame(W, H, seed, specials=True):
    """observed colour and depth (1 .. 3), a silhouette, a rendered depth around the observed one and a camera, on the CPU.
    `specials`: NaN, 0, negative and +inf pixels in depth_obs and NaN pixels in opacity_map and depth, where the frame has room."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    cam = camera(W, H)
    f = dict(cam=cam, color_obs=torch.rand((3, H, W), generator=g), depth_obs=1.0 + 2.0 * torch.rand((H, W), generator=g),
             opacity_map=torch.rand((1, H, W), generator=g), view=torch.from_numpy(cam.matrices()[0].copy()))
    f["depth"] = f["depth_obs"] + 0.2 * torch.randn((H, W), generator=g)
    if specials and W * H >= 64:
        flat = torch.randperm(W * H, generator=g)[:48]
        for i, v in enumerate((NAN, 0.0, -1.5, INF)):
            f["depth_obs"].view(-1)[flat[8 * i:8 * i + 8]] = v
        f["opacity_map"].view(-1)[flat[28:40]] = NAN   # (some on special depth_obs pixels, some not)
        f["depth"].view(-1)[flat[36:48]] = NAN
    return f


MASKS = {  # name -> the keyword arguments of the selection (images by name)
    "silhouette": dict(images=("opacity_map",), silhouette_threshold=0.35),
    "depth": dict(images=("depth",), depth_error_min=0.1),
    "both": dict(images=("opacity_map", "depth"), silhouette_threshold=0.2, depth_error_min=0.15),
    "neither": dict(images=()),
}


def selection(f, mask):
    kw = dict(mask)
    images = kw.pop("images")
    return {name: f[name] for name in images}, kw


def assert_off_threshold(f, images, kw):
    """no pixel sits on a threshold (what the wrapper and the model form: float64, rounded once)"""
    f32 = lambda x: torch.tensor(x, dtype=torch.float64).float()  # noqa: E731
    for t in kw.get("depth_range", (0.0, INF)):
        if t not in (0.0, INF):  # (0 and +inf pixels are there on purpose: 0 > 0 and inf < inf are false without any rounding)
            assert not (f["depth_obs"] == f32(t)).any()
    if "opacity_map" in images:
        assert not (images["opacity_map"] == f32(kw.get("silhouette_threshold", 0.5))).any()
    if "depth" in images:
        d = images["depth"].reshape(f["depth_obs"].shape)
        assert not (d == f["depth_obs"]).any() and not ((d - f["depth_obs"]) == f32(kw.get("depth_error_min", INF))).any()


def state_of(P, seed):
    """leaves with the extra tensors of map_step_cases.py (k = 1, 3, 4, 45, 48), moments for every leaf, the accumulators"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = leaves_of(P, g)
    M = moments_of(L, g)
    A = {"xyz_gradient_accum": torch.rand((P, 1), generator=g), "denom": torch.randint(0, 5, (P, 1), generator=g).float(),
         "max_radii2D": torch.floor(torch.rand(P, generator=g) * 60.0)}
    return L, M, A


def run_hip(f, L, M, A, images, kw, error_on_device=False):
    """the HIP step on copies of the CPU inputs; returns (leaves, moments by name, accumulators by name, counts, optimiser)"""
    d, cam = dev(), f["cam"]
    params, opt, _, before = on_device(L, M)
    kw = dict(kw)
    if error_on_device:
        kw["depth_error_min"] = torch.tensor([kw["depth_error_min"]], dtype=torch.float64).float().to(d)
    accs = {name: None if t is None else t.to(d) for name, t in A.items()}
    out, a, dn, mr, counts = seed_from_frame(params, opt, f["color_obs"].to(d), f["depth_obs"].to(d), f["view"].to(d), cam.fx, cam.fy,
                                             cam.cx, cam.cy, fill=FILL, **{n: t.to(d) for n, t in images.items()}, **accs, **kw)
    torch.cuda.synchronize()
    assert_rebuilt(before, out, opt)
    return out, {name: opt.state[out[name]] for name in M}, dict(zip(ACCS, (a, dn, mr))), counts, opt, params


def ulps(got, want64):
    """|got - fp32(want64)| in units of fp32(want64)'s spacing"""
    want = want64.float().numpy()
    return np.abs(got.numpy().astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


WORST = {"xyz": 0.0, "scaling": 0.0}


def check_against_model(f, P, mask, seed=5, error_on_device=False, stride=1, **extra):
    L, M, A = state_of(P, seed)
    images, kw = selection(f, mask)
    kw.update(extra, stride=stride)
    assert_off_threshold(f, images, kw)
    cam = f["cam"]
    ref = seed_model(L, M, A, f["color_obs"], f["depth_obs"], f["view"], cam.fx, cam.fy, cam.cx, cam.cy, fill=FILL, **images, **kw)
    out, moments, accs, counts, _, params = run_hip(f, L, M, A, images, kw, error_on_device)
    assert tuple(counts) == ref["counts"], (tuple(counts), ref["counts"])
    n = ref["counts"][1]
    if n == 0:  # the inputs come back as they are
        assert all(out[name] is params[name] for name in L)
        return ref, out
    for name, t in ref["leaves"].items():
        if name in ("xyz", "scaling"):
            assert bits_equal(out[name][:P], t), name   # the old rows
        elif name not in ("xyz_new", "scaling_new"):
            assert bits_equal(out[name], t), name
    for name, (m, v) in ref["moments"].items():
        assert bits_equal(moments[name][0], m) and bits_equal(moments[name][1], v), name
        assert not m[P:].any() and not v[P:].any()
    for name, t in ref["accumulators"].items():
        assert bits_equal(accs[name], t), name
    # positions: within 1e-5 of max(1, |p_cam| + |campos|) of float64, and each lands on its own pixel, in the model's order
    got = out["xyz"][P:].detach().cpu()
    err = (got.double() - ref["leaves"]["xyz_new"]).abs().max(dim=1).values
    scale = ref["xyz_scale"].clamp_min(1.0)
    p_cam = torch.from_numpy(cam.to_camera(got.double().numpy()))
    px = torch.stack([cam.fx * p_cam[:, 0] / p_cam[:, 2] + cam.cx, cam.fy * p_cam[:, 1] / p_cam[:, 2] + cam.cy], dim=1)
    assert torch.equal(torch.round(px).long(), ref["pixels"])
    worst_xyz = float((err / scale).max())
    # log-scales: within 4 ulp of the float64 value rounded to fp32
    got_s = out["scaling"][P:].detach().cpu()
    worst_s = float(ulps(got_s, ref["leaves"]["scaling_new"]).max())
    WORST["xyz"], WORST["scaling"] = max(WORST["xyz"], worst_xyz), max(WORST["scaling"], worst_s)
    print(f"{cam.W} x {cam.H} stride {stride}, P = {P} -> {counts.rows}: counts {ref['counts']}; new xyz error / scale: worst "
          f"{worst_xyz:.3e} (bound 1e-5); new scaling_raw: worst {worst_s:.2f} ulp (bound 4)")
    assert (err <= 1e-5 * scale).all()
    assert float(ref["leaves"]["scaling_new"].max()) < -1.0  # (|log| >= 1: an ulp of the result is no finer than the argument's rounding)
    assert worst_s <= 4.0
    return ref, out


@pytest.mark.parametrize("P", [0, 1, 1000])
@pytest.mark.parametrize("W, H, stride", [(37, 23, 1), (37, 23, 2), (37, 23, 3), (1, 1, 1), (300, 220, 1)],
                         ids=["37x23", "37x23-stride2", "37x23-stride3", "1x1", "300x220"])
def test_shapes_match_the_model(W, H, stride, P):
    """candidate-grid edges on a frame that is no multiple of anything; one pixel; 66 000 candidates = 258 blocks: the block
    totals' scan takes a second pass and block boundaries fall mid-row.  9 leaves with moments + 3 accumulators = 30 tensors:
    the apply runs as two launches of the table."""
    f = frame(W, H, 100 + W + stride)
    ref, _ = check_against_model(f, P, MASKS["both" if W * H > 1 else "neither"], stride=stride)
    rows, n, valid, unseen, infront = ref["counts"]
    cands = -(-W // stride) * -(-H // stride)
    if W * H == 1:
        assert (rows, n, valid, unseen, infront) == (P + 1, 1, 1, 0, 0)
    else:
        assert 0 < n < valid <= cands and 0 < unseen < n and 0 < infront < n and unseen + infront >= n
    if W * H > 10000:  # every kind of candidate is there: invalid, unseen only, in front only, both, neither
        assert valid < cands and unseen + infront > n and n > 256 * 64


@pytest.mark.parametrize("mask", list(MASKS))
def test_mask_cases_match_the_model(mask):
    f = frame(37, 23, 7)
    ref, _ = check_against_model(f, 1000, MASKS[mask])
    rows, n, valid, unseen, infront = ref["counts"]
    assert valid == 37 * 23 - 32  # NaN, 0 and negative pixels are not valid, and +inf is not below depth_max = +inf
    if mask == "neither":
        assert n == valid and unseen == 0 and infront == 0
    else:
        assert 0 < n < valid


def test_a_finite_depth_range_decides_valid():
    f = frame(37, 23, 8)
    ref, _ = check_against_model(f, 1, MASKS["neither"], depth_range=(1.5, 2.5))
    assert 0 < ref["counts"][1] == ref["counts"][2] < 37 * 23 // 2 + 100


def test_special_pixels_are_never_selected():
    """NaN, 0, negative and +inf in depth_obs are not valid; a NaN opacity_map is not unseen and a NaN depth not in front"""
    f = frame(37, 23, 9)
    bad = ~((f["depth_obs"] > 0) & (f["depth_obs"] < INF))
    assert int(bad.sum()) == 32 and f["depth_obs"].isnan().sum() == 8
    ref, _ = check_against_model(f, 1000, dict(images=("opacity_map", "depth"), silhouette_threshold=2.0, depth_error_min=-1.0))
    ok = ~bad.flatten()
    nan_o, nan_d = f["opacity_map"].flatten().isnan(), f["depth"].flatten().isnan()
    assert (nan_o & ok).any() and (nan_d & ok).any() and (nan_o & nan_d & ok).any()
    select = seed_masks(f["depth_obs"], f["opacity_map"], f["depth"], silhouette_threshold=2.0, depth_error_min=-1.0)[0].flatten()
    # with these thresholds every valid pixel is unseen unless its opacity is NaN, then in front if the depth is larger
    assert not select[~ok].any() and not select[nan_o & nan_d].any() and select[ok & ~nan_o].all()


def test_nothing_selected_returns_the_inputs():
    f = frame(37, 23, 10)
    ref, _ = check_against_model(f, 1000, dict(images=("opacity_map", "depth"), silhouette_threshold=-1.0, depth_error_min=50.0))
    assert ref["counts"] == (1000, 0, 37 * 23 - 32, 0, 0)
    ref, _ = check_against_model(f, 0, dict(images=("opacity_map",), silhouette_threshold=0.0))
    assert ref["counts"][:2] == (0, 0)


def test_everything_selected():
    f = frame(37, 23, 11, specials=False)
    ref, out = check_against_model(f, 1000, dict(images=("opacity_map",), silhouette_threshold=1.5))
    assert ref["counts"] == (1000 + 37 * 23, 37 * 23, 37 * 23, 37 * 23, 0)
    assert torch.equal(ref["pixels"], torch.stack(torch.meshgrid(torch.arange(37), torch.arange(23), indexing="xy"), dim=-1).reshape(-1, 2))


def test_depth_error_min_as_a_device_scalar_takes_the_same_decisions():
    f = frame(37, 23, 12)
    ref_host, out_host = check_against_model(f, 1000, MASKS["depth"])
    ref_dev, out_dev = check_against_model(f, 1000, MASKS["depth"], error_on_device=True)
    assert ref_host["counts"] == ref_dev["counts"] and ref_host["counts"][4] > 50
    for name in out_host:
        assert bits_equal(out_host[name], out_dev[name]), name


def test_without_accumulators_or_optimizer_and_with_roles():
    f, d = frame(37, 23, 13), dev()
    cam = f["cam"]
    g = torch.Generator(device="cpu").manual_seed(3)
    L = leaves_of(50, g, {"colour": (1, 3), "f_rest": (15, 3)})
    ref = seed_model({("f_dc" if n == "colour" else n): t for n, t in L.items()}, {}, {}, f["color_obs"], f["depth_obs"], f["view"],
                     cam.fx, cam.fy, cam.cx, cam.cy, stride=2, init_opacity=0.1, scale_factor=0.5)
    params = {n: t.to(d) for n, t in L.items()}
    out, a, dn, mr, counts = seed_from_frame(params, None, f["color_obs"].to(d), f["depth_obs"].to(d), f["view"].to(d), cam.fx, cam.fy,
                                             cam.cx, cam.cy, stride=2, init_opacity=0.1, scale_factor=0.5, roles={"f_dc": "colour"})
    assert (a, dn, mr) == (None, None, None) and tuple(counts) == ref["counts"]
    for name in ("rotation", "opacity", "f_rest"):
        assert bits_equal(out[name], ref["leaves"][name]), name
    assert bits_equal(out["colour"], ref["leaves"]["f_dc"])
    assert ulps(out["scaling"][50:].cpu(), ref["leaves"]["scaling_new"]).max() <= 4.0
    assert not any(p.requires_grad for p in out.values())


def test_both_resize_steps_in_sequence_keep_the_optimizer_consistent():
    """seed_from_frame, densify_and_prune on its output, seed_from_frame again, on one model (P = 300, the nine leaves with moments
    and the accumulators; 37 x 23 at stride 2): what the two steps share -- the table with the moments interleaved, the hand-over
    to the optimiser -- seen from both callers.  Nothing numerical beyond the bits of the copied rows."""
    d, P = dev(), 300
    L, M, A = state_of(P, 8)
    f = frame(37, 23, 8)
    cam = f["cam"]
    params, opt, _, _ = on_device(L, M)
    accs = [A[name].to(d) for name in ACCS]

    def seed(params, accs):
        return seed_from_frame(params, opt, f["color_obs"].to(d), f["depth_obs"].to(d), f["view"].to(d), cam.fx, cam.fy, cam.cx,
                               cam.cy, stride=2, fill=FILL, **dict(zip(ACCS, accs)))

    def consistent(out, rows):
        assert list(out) == list(L) and all(p.shape[0] == rows for p in out.values())
        assert all(len(g["params"]) == 1 and g["params"][0] is out[name] for g, name in zip(opt.param_groups, L))
        assert len(opt.state) == len(L) and opt.steps == 3
        for name, p in out.items():
            m, v = opt.state[p]
            assert m.shape == p.shape and v.shape == p.shape, name

    out, *accs, counts = seed(params, accs)
    assert counts.rows == P + counts.new and counts.new > 0
    consistent(out, counts.rows)
    for name, t in L.items():
        assert bits_equal(out[name][:P], t), name
        assert bits_equal(opt.state[out[name]][0][:P], M[name][0]) and bits_equal(opt.state[out[name]][1][:P], M[name][1]), name
    for got, name in zip(accs, ACCS):
        assert bits_equal(got[:P], A[name]) and not got[P:].any(), name

    out, *accs, counts = densify_and_prune(out, opt, *accs, grad_threshold=0.3, extent=10.0)
    assert counts.rows == counts.survivors + counts.clones + counts.children and counts.clones > 0 and counts.children > 0
    consistent(out, counts.rows)
    assert all(a.shape[0] == counts.rows and not a.any() for a in accs)

    rows = counts.rows
    out, *accs, counts = seed(out, accs)
    assert counts.rows == rows + counts.new and counts.new > 0
    consistent(out, counts.rows)
    assert all(a.shape[0] == counts.rows for a in accs)


def test_two_runs_give_the_same_bits():
    f = frame(300, 220, 14)
    L, M, A = state_of(1000, 6)
    images, kw = selection(f, MASKS["both"])
    runs = [run_hip(f, L, M, A, images, kw) for _ in range(2)]
    assert tuple(runs[0][3]) == tuple(runs[1][3]) and runs[0][3].new > 10000
    for name in L:
        assert bits_equal(runs[0][0][name], runs[1][0][name]), name
        for j in (0, 1):
            assert bits_equal(runs[0][1][name][j], runs[1][1][name][j]), name
    for name in ACCS:
        assert bits_equal(runs[0][2][name], runs[1][2][name]), name


def test_a_capturing_stream_is_refused_and_the_capture_goes_on():
    d, f = dev(), frame(16, 8, 15, specials=False)
    cam = f["cam"]
    g = torch.Generator(device="cpu").manual_seed(4)
    params = {name: t.to(d) for name, t in leaves_of(64, g, {}).items()}
    args = (params, None, f["color_obs"].to(d), f["depth_obs"].to(d), f["view"].to(d), cam.fx, cam.fy, cam.cx, cam.cy)
    x = torch.arange(8, device=d, dtype=torch.float32)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=d)
    side.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(RuntimeError, match="hipGraph"):
                seed_from_frame(*args)
            y = x * 2.0 + 1.0   # the capture is still alive: this is recorded
    torch.cuda.current_stream(d).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, x * 2.0 + 1.0)
    # and outside the capture the same call works
    out, _, _, _, counts = seed_from_frame(*args)
    assert tuple(counts) == (64 + 128, 128, 128, 0, 0) and out["xyz"].shape == (192, 3)


def test_wrong_shapes_are_refused():
    d, f = dev(), frame(16, 8, 16, specials=False)
    cam = f["cam"]
    g = torch.Generator(device="cpu").manual_seed(4)
    params = {name: t.to(d) for name, t in leaves_of(64, g, {"f_dc": (1, 3)}).items()}
    color, depth_obs, view = f["color_obs"].to(d), f["depth_obs"].to(d), f["view"].to(d)
    K = (cam.fx, cam.fy, cam.cx, cam.cy)
    with pytest.raises(RuntimeError, match="color_obs"):
        seed_from_frame(params, None, color[:, :, :15], depth_obs, view, *K)
    with pytest.raises(RuntimeError, match="opacity_map"):
        seed_from_frame(params, None, color, depth_obs, view, *K, opacity_map=torch.zeros((8, 15), device=d))
    with pytest.raises(RuntimeError, match="depth must"):
        seed_from_frame(params, None, color, depth_obs, view, *K, depth=torch.zeros((2, 8, 16), device=d))
    with pytest.raises(RuntimeError, match="viewmatrix"):
        seed_from_frame(params, None, color, depth_obs, view[:3], *K)
    with pytest.raises(RuntimeError, match="depth_obs"):
        seed_from_frame(params, None, color, depth_obs.double(), view, *K)
    with pytest.raises(RuntimeError, match="denom"):
        seed_from_frame(params, None, color, depth_obs, view, *K, denom=torch.zeros(63, device=d))
    with pytest.raises(RuntimeError, match="rotation"):
        seed_from_frame(dict(params, rotation=params["xyz"]), None, color, depth_obs, view, *K)
    with pytest.raises(ValueError, match="stride"):
        seed_from_frame(params, None, color, depth_obs, view, *K, stride=0)


# ---------------------------------------------------------------------------------------------------- the camera convention
def empty_leaves(d):
    return {"xyz": torch.zeros((0, 3), device=d), "scaling": torch.zeros((0, 3), device=d), "rotation": torch.zeros((0, 4), device=d),
            "opacity": torch.zeros((0, 1), device=d), "f_dc": torch.zeros((0, 1, 3), device=d),
            "f_rest": torch.zeros((0, 15, 3), device=d)}


def tilted_plane(cam):
    """a depth image in 1 .. 3, valid everywhere"""
    x, y = np.meshgrid(np.arange(cam.W), np.arange(cam.H))
    return torch.from_numpy((1.0 + 1.4 * x / max(cam.W - 1, 1) + 0.6 * y / max(cam.H - 1, 1)).astype(np.float32))


def seed_plane(cam, **kw):
    d = dev()
    g = torch.Generator(device="cpu").manual_seed(17)
    color = torch.rand((3, cam.H, cam.W), generator=g)
    view = torch.from_numpy(cam.matrices()[0].copy())
    out, _, _, _, counts = seed_from_frame(empty_leaves(d), None, color.to(d), tilted_plane(cam).to(d), view.to(d), cam.fx, cam.fy,
                                           cam.cx, cam.cy, **kw)
    return out, counts, color


@pytest.mark.parametrize("cid", ["skewed_pp", "far"])
def test_seeded_points_project_onto_their_pixels(cid):
    """the rasterizer's own convention, float64: p_hom = (x, y, z, 1) projmatrix, ndc2Pix(v, S) = ((v + 1) S - 1) / 2.  A
    convention slip is 0.5 px or a transpose; fp32 leaves about 1e-4 px at this width."""
    cam = cameras.CAMERAS[cid].at(64)
    out, counts, _ = seed_plane(cam)
    assert tuple(counts) == (cam.W * cam.H, cam.W * cam.H, cam.W * cam.H, 0, 0)
    _, proj, _, _ = cam.matrices()
    xyz = out["xyz"].cpu().double().numpy()
    hom = np.concatenate([xyz, np.ones((len(xyz), 1))], axis=1) @ proj.astype(np.float64)
    ndc = hom[:, :2] / hom[:, 3:4]
    px = np.stack([((ndc[:, 0] + 1.0) * cam.W - 1.0) / 2.0, ((ndc[:, 1] + 1.0) * cam.H - 1.0) / 2.0], axis=1)
    x, y = np.meshgrid(np.arange(cam.W), np.arange(cam.H))
    want = np.stack([x.reshape(-1), y.reshape(-1)], axis=1)   # row-major: y, then x
    worst = float(np.abs(px - want).max())
    print(f"{cid} at {cam.W} x {cam.H}: seeded points land within {worst:.2e} px of their pixels (bound 1e-2)")
    assert worst <= 1e-2
    depth = cam.to_camera(xyz)[:, 2]
    assert np.abs(depth - tilted_plane(cam).numpy().reshape(-1)).max() <= 1e-4


# ---------------------------------------------------------------------------------------------------- closing the loop
def seeded_scene(cam, leaves, color):
    """the seeded map as a synth Scene of `cam` (activated values, as the rasterizer takes them)"""
    from dgr_amd.synth import Scene
    view, proj, persp, campos = cam.matrices()
    n = leaves["xyz"].shape[0]
    np32 = lambda t: np.ascontiguousarray(t.detach().cpu().float().numpy())  # noqa: E731
    shs = np.zeros((n, 16, 3), np.float32)
    shs[:, 0, :] = np32(leaves["f_dc"]).reshape(n, 3)
    zero = np.zeros((cam.H, cam.W), np.float32)
    return Scene(n, cam.W, cam.H, cam.tanfovx, cam.tanfovy, view, proj, persp, campos, np32(leaves["xyz"]),
                 np.exp(np32(leaves["scaling"])), np32(leaves["rotation"]), 1.0 / (1.0 + np.exp(-np32(leaves["opacity"]))), shs,
                 tilted_plane(cam).numpy(), np.array([0.1, 0.2, 0.3], np.float32), np.zeros((3, cam.H, cam.W), np.float32), zero, zero,
                 zero)


def test_a_seeded_map_explains_its_own_frame():
    """every pixel's own Gaussian sits on its pixel centre with alpha ~ 0.7, in front of the near plane: the light forward's
    opacity_map is >= 0.69 everywhere (the CPU oracle gives 0.9746 .. 0.9999 on this scene: the neighbours' tails add to the
    pixel's own 0.7), and a second seed_from_frame from that silhouette adds nothing"""
    import hip_helpers as hh
    cam = cameras.CAMERAS["skewed_pp"].at(64)
    out, counts, color = seed_plane(cam, init_opacity=0.7)
    assert counts.new == cam.W * cam.H
    s = seeded_scene(cam, out, color)
    _, rendered = hh.hip_forward(s, 0)
    opacity_map = rendered["opacity_map"]
    print(f"opacity_map of the seeded map: min {opacity_map.min():.4f}, max {opacity_map.max():.4f}")
    assert opacity_map.min() >= 0.69
    d = dev()
    again, _, _, _, counts2 = seed_from_frame(out, None, color.to(d), tilted_plane(cam).to(d), torch.from_numpy(s.view.copy()).to(d),
                                              cam.fx, cam.fy, cam.cx, cam.cy, opacity_map=torch.from_numpy(opacity_map).to(d),
                                              silhouette_threshold=0.5)
    assert tuple(counts2) == (counts.rows, 0, cam.W * cam.H, 0, 0) and again is out


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_a_degree_zero_model_with_an_empty_f_rest(capturable):
    """3DGS's degree-0 model has f_rest [P, 0, 3]: the step runs, f_rest and its moments come back [rows, 0, 3], and everything
    else carries the bits of the same call without that leaf (tests/degree_zero.py) -- before and after a further step()."""
    import degree_zero
    d, P = dev(), 300
    L, _, A = state_of(P, 8)
    f = frame(37, 23, 8)
    cam = f["cam"]
    images, kw = selection(f, MASKS["both"])
    seen = {}
    for with_rest in (False, True):
        params = degree_zero.model(L, d, with_rest)
        opt = degree_zero.stepped_adam(params, capturable)
        out, a, dn, mr, counts = seed_from_frame(params, opt, f["color_obs"].to(d), f["depth_obs"].to(d), f["view"].to(d), cam.fx, cam.fy,
                                                 cam.cx, cam.cy, **{n: t.to(d) for n, t in images.items()},
                                                 **{n: t.to(d) for n, t in A.items()}, **kw)
        assert counts.new > 0 and counts.rows == P + counts.new
        after = degree_zero.snapshot(out, opt, xyz_gradient_accum=a, denom=dn, max_radii2D=mr, counts=tuple(counts))
        if with_rest:
            degree_zero.check_rest(out, opt, counts.rows)
        degree_zero.step_again(opt, out, capturable)
        seen[with_rest] = (after, degree_zero.snapshot(out, opt))
    for with_leaf, without in zip(seen[True], seen[False]):
        degree_zero.assert_same_bits(with_leaf, without)
