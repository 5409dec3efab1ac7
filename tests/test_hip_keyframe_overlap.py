"""slam.keyframe_overlap / slam.select_keyframes on the GPU against the float64 model (tests/overlap_model.py): flags bit for bit
at every pair the model does not mark ambiguous, counts equal to the sums of the kernel's own flags, the score the one fp32
division; closed forms; occlusion against keyframe depths; determinism, hipGraph replay, guarded buffers, argument errors.
Shapes are the smallest at which the kernel can go wrong: one candidate, a partial last row and column, a frame of one row, more
than one block of candidates per keyframe (96 x 80 at stride 1: four blocks and the second launch), the workload's 640 x 480 at
stride 16 (one block, five trips), 1, 3 and 70 keyframes."""
import numpy as np
import pytest
import torch

from dgr_amd import keyframes, slam

import cameras
import overlap_model as M
from test_hip_guarded_buffers import GuardedTorch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")


def w2ct(R, t):
    """W2C^T as float32 [4,4]"""
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m.T.astype(np.float32)


def camera(W, H):
    """An off-centre camera with fx != fy at a tilted pose."""
    R, t = cameras._synth_pose(0.3)
    return cameras.Camera("overlap", W, H, 0.8 * max(W, 24), 0.7 * max(W, 24), (W - 1) / 2 + 0.07 * W, (H - 1) / 2 - 0.05 * H, R, t)


def special_values(rng, img, share=0.04):
    """NaN, 0, a negative depth and +inf scattered over a copy of `img`"""
    img = img.copy()
    flat = img.reshape(-1)
    for value in (np.nan, 0.0, -1.5, np.inf):
        flat[rng.random(flat.size) < share / 4] = value
    return img


def random_case(W, H, stride, K, seed, edge):
    """Random depths in [1, 4] with special values, keyframes at random poses around the current one (rotations up to 0.5 rad,
    a few of them looking away, centres up to 0.4 apart)."""
    rng = np.random.default_rng(seed)
    cam = camera(W, H)
    depth = special_values(rng, rng.uniform(1.0, 4.0, (H, W)).astype(np.float32))
    views = []
    for k in range(K):
        angle = rng.uniform(0.0, 0.5) if k % 7 != 5 else rng.uniform(2.0, 3.1)
        Rk = cameras.rotation(rng.normal(size=3), angle) @ cam.R
        centre = -cam.R.T @ cam.t + rng.uniform(-0.4, 0.4, 3)
        views.append(w2ct(Rk, -Rk @ centre))
    kw = dict(stride=stride, edge=edge)
    return dict(depth_obs=depth, viewmatrix=w2ct(cam.R, cam.t), keyframe_viewmatrices=np.stack(views), fx=cam.fx, fy=cam.fy,
                cx=cam.cx, cy=cam.cy, kw=kw)


def same_bits(a, b):
    """two KeyframeOverlap results, field by field"""
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t  # noqa: E731
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def run(case, **more):
    """(KeyframeOverlap on the GPU with flags, the model's dict)"""
    kw = dict(case["kw"], **more)
    args = [torch.from_numpy(np.ascontiguousarray(case[n])).to(DEV) for n in ("depth_obs", "viewmatrix", "keyframe_viewmatrices")]
    gkw = dict(kw)
    if gkw.get("keyframe_depths") is not None:
        gkw["keyframe_depths"] = torch.from_numpy(np.ascontiguousarray(gkw["keyframe_depths"])).to(DEV)
    out = slam.keyframe_overlap(*args, case["fx"], case["fy"], case["cx"], case["cy"], return_flags=True, **gkw)
    model = M.overlap_model(case["depth_obs"], case["viewmatrix"], case["keyframe_viewmatrices"], case["fx"], case["fy"], case["cx"],
                            case["cy"], **kw)
    return out, model


def check(out, model, label=""):
    """The comparison every case shares; prints the figures first."""
    flags = out.flags.cpu().numpy()
    amb = model["ambiguous"]
    S = model["S"]
    per_kf = amb.sum(1)
    differ = (flags != model["flags"])
    print(f"{label}: K {flags.shape[0]} S {S} valid {model['valid']} inside {model['inside'].tolist()[:8]} ambiguous per keyframe "
          f"max {int(per_kf.max())} mismatches outside the band {int((differ & ~amb).sum())} inside it {int((differ & amb).sum())}")
    assert int(per_kf.max()) <= max(4, 0.005 * S), "the inputs put too many pairs on a threshold: choose another seed"
    assert flags.shape == model["flags"].shape and not (differ & ~amb).any()
    assert ((flags & 1) == (model["flags"] & 1)).all()  # valid is a raw fp32 comparison: never ambiguous
    assert not (flags & ~np.uint8(7)).any() and not ((flags & 2) > (flags & 1) * 2).any() and not ((flags & 4) > (flags & 2) * 2).any()
    inside, visible, valid = out.inside.cpu().numpy(), out.visible.cpu().numpy(), int(out.valid.cpu()[0])
    assert out.inside.dtype == out.visible.dtype == out.valid.dtype == torch.int32 and out.score.dtype == torch.float32
    assert np.array_equal(inside, ((flags >> 1) & 1).sum(1)) and np.array_equal(visible, ((flags >> 2) & 1).sum(1))
    assert valid == int((flags[0] & 1).sum()) == model["valid"]
    want = visible.astype(np.float32) / np.float32(valid) if valid else np.zeros(len(visible), np.float32)
    score = out.score.cpu().numpy()
    assert np.array_equal(score.view(np.uint32), want.view(np.uint32))
    if not amb.any():
        assert np.array_equal(inside, model["inside"]) and np.array_equal(visible, model["visible"])
        assert np.array_equal(score.view(np.uint32), model["score"].view(np.uint32))
    return flags


SHAPES = [  # W, H, stride, K, seed, edge
    (1, 1, 1, 3, 135, 0.0), (37, 23, 3, 3, 2, 2.5), (257, 1, 1, 3, 3, 0.0), (96, 80, 1, 3, 4, 5.0), (640, 480, 16, 3, 5, 20.0),
    (37, 23, 3, 1, 6, 2.5), (37, 23, 3, 70, 7, 2.5), (96, 80, 1, 70, 8, 5.0), (640, 480, 16, 70, 9, 20.0), (640, 480, 16, 1, 10, 20.0),
]


@pytest.mark.parametrize("W,H,stride,K,seed,edge", SHAPES, ids=[f"{s[0]}x{s[1]}-stride{s[2]}-K{s[3]}" for s in SHAPES])
def test_flags_counts_and_scores_against_the_model(W, H, stride, K, seed, edge):
    case = random_case(W, H, stride, K, seed, edge)
    out, model = run(case)
    flags = check(out, model, f"{W}x{H}/{stride}")
    assert flags.shape == (K, -(-W // stride) * -(-H // stride))
    if H >= 23 and K >= 3:  # the case exercises both decisions
        assert 0 < int(out.inside.sum()) < K * model["valid"]


def test_a_depth_range_and_a_near_plane():
    case = random_case(96, 80, 2, 5, 11, 3.0)
    out, model = run(case, depth_range=(1.5, 3.25), near=2.0)
    check(out, model, "range")
    plain = M.overlap_model(case["depth_obs"], case["viewmatrix"], case["keyframe_viewmatrices"], case["fx"], case["fy"], case["cx"],
                            case["cy"], **case["kw"])
    assert 0 < model["valid"] < plain["valid"] and 0 < int(model["inside"].sum()) < int(plain["inside"].sum())


def test_a_frame_without_a_valid_pixel_scores_zero():
    case = random_case(37, 23, 3, 3, 12, 2.5)
    for fill in (0.0, NAN, INF, -2.0):
        case["depth_obs"] = np.full((23, 37), fill, np.float32)
        out, model = run(case)
        check(out, model, f"all {fill}")
        assert int(out.valid[0]) == 0 and out.score.tolist() == [0.0, 0.0, 0.0] and not out.flags.any()
    case["depth_obs"] = np.full((23, 37), 2.0, np.float32)
    out, _ = run(case, depth_range=(3.0, 4.0))
    assert int(out.valid[0]) == 0 and out.score.tolist() == [0.0, 0.0, 0.0]


def plane_case(W=96, H=80, stride=3, depth=2.0, edge=2.5, shift_px=10.25):
    """A constant-depth frame seen from a tilted pose, fx = 64 != fy = 48; keyframe 0 at the current pose, 1 looking the opposite
    way from the same centre, 2 shifted along its own x axis so that every point moves by shift_px pixels exactly, 3 along y."""
    cam = camera(W, H)._replace(fx=64.0, fy=48.0, cx=40.0, cy=35.0)
    half_turn = np.diag([-1.0, 1.0, -1.0])
    views = [w2ct(cam.R, cam.t), w2ct(half_turn @ cam.R, half_turn @ cam.t),
             w2ct(cam.R, cam.t + np.array([shift_px * depth / cam.fx, 0.0, 0.0])),
             w2ct(cam.R, cam.t + np.array([0.0, shift_px * depth / cam.fy, 0.0]))]
    return dict(depth_obs=np.full((H, W), depth, np.float32), viewmatrix=views[0], keyframe_viewmatrices=np.stack(views), fx=cam.fx,
                fy=cam.fy, cx=cam.cx, cy=cam.cy, kw=dict(stride=stride, edge=edge))


def pose_of(view):
    """(R, t) of a W2C^T matrix, float64"""
    w2c = np.asarray(view, np.float64).T
    return w2c[:3, :3], w2c[:3, 3]


def grid_count(n, stride, lo, hi, shift=0.0):
    """grid points g = 0, stride, ... < n with lo < g + shift < hi"""
    return sum(1 for g in range(0, n, stride) if lo < g + shift < hi)


def test_closed_forms():
    W, H, stride, edge, shift = 96, 80, 3, 2.5, 10.25
    out, model = run(plane_case(W, H, stride, edge=edge, shift_px=shift))
    check(out, model, "plane")
    assert not model["ambiguous"].any()  # a half-integer edge: no candidate sits on a border
    nx, ny = grid_count(W, stride, edge, W - edge), grid_count(H, stride, edge, H - edge)
    want = [nx * ny, 0, grid_count(W, stride, edge, W - edge, shift) * ny, nx * grid_count(H, stride, edge, H - edge, shift)]
    assert out.inside.tolist() == want == out.visible.tolist() and len(set(want)) == 4
    S = -(-W // stride) * -(-H // stride)
    assert int(out.valid[0]) == S and out.score.tolist() == [float(np.float32(n) / np.float32(S)) for n in want]


def test_occlusion_against_keyframe_depths():
    case = plane_case()
    K, H, W = 4, 80, 96
    same = np.full((K, H, W), 2.0, np.float32)  # the keyframes look along the plane's normal: they see it at the same depth
    out, model = run(case, keyframe_depths=same)
    check(out, model, "same plane")
    assert out.visible.tolist() == out.inside.tolist() and int(out.inside[0]) > 0
    out, model = run(case, keyframe_depths=same * 0.5)  # something stands in front of the plane in every keyframe
    check(out, model, "halved")
    assert out.visible.tolist() == [0, 0, 0, 0] and out.score.tolist() == [0.0] * 4 and int(out.inside[0]) > 0
    holes = same.copy()
    holes[0], holes[2], holes[3] = 0.0, NAN, INF  # no usable depth in the keyframe: nothing is confirmed
    out, model = run(case, keyframe_depths=holes)
    check(out, model, "holes")
    assert out.visible.tolist() == [0, 0, 0, 0]
    out, model = run(case, keyframe_depths=same * 1.04, depth_tolerance=0.05)  # |2 - 2.08| = 0.08 <= 0.104
    assert out.visible.tolist() == out.inside.tolist()
    out, model = run(case, keyframe_depths=same * 1.04, depth_tolerance=0.03)
    check(out, model, "tolerance")
    assert out.visible.tolist() == [0, 0, 0, 0]


def mixed_case(seed=21, W=96, H=80, stride=1):
    """Depths drawn from {1, 2, 4} (with special values) and keyframes shifted along their own x / y so that every point moves by
    41.2 / d or 30.6 / d pixels: no landing position within 0.1 px of a pixel's edge, so that which keyframe pixel is read is
    decided -- and random keyframe depths within 15 % of {1, 2, 4} (with special values), half of which agree to the 10 %
    tolerance when they belong to the same level."""
    rng = np.random.default_rng(seed)
    case = plane_case(W, H, stride, edge=2.5)
    R, t = pose_of(case["viewmatrix"])
    case["keyframe_viewmatrices"] = np.stack([w2ct(R, t), w2ct(R, t + np.array([41.2 / 64.0, 0.0, 0.0])),
                                              w2ct(R, t + np.array([0.0, -30.6 / 48.0, 0.0]))])
    case["depth_obs"] = special_values(rng, rng.choice([1.0, 2.0, 4.0], (H, W)).astype(np.float32))
    kd = rng.choice([1.0, 2.0, 4.0], (3, H, W)) * rng.uniform(0.85, 1.15, (3, H, W))
    return case, special_values(rng, kd.astype(np.float32), share=0.08)


def test_a_mixed_occlusion_case_against_the_model():
    case, kd = mixed_case()
    out, model = run(case, keyframe_depths=kd, depth_tolerance=0.1)
    check(out, model, "mixed")
    for k in range(3):
        assert 0 < int(out.visible[k]) < int(out.inside[k]) < model["valid"]
    out, model = run(case, keyframe_depths=kd, depth_tolerance=0.1, depth_range=(1.5, 3.0), stride=3)
    check(out, model, "mixed, range")
    assert 0 < int(out.visible.sum()) < int(out.inside.sum())


def test_edge_zero_reads_no_pixel_outside_the_keyframe():
    """With edge = 0 a point may land within half a pixel of the right or lower border: its nearest pixel is outside the image,
    and it is not visible."""
    case = plane_case(edge=0.0, stride=1)
    R, t = pose_of(case["viewmatrix"])  # u = x + 10.75: x = 85 lands at 95.75, nearest pixel 96 = W; v = y + 0.25
    case["keyframe_viewmatrices"] = w2ct(R, t + np.array([10.75 * 2.0 / 64.0, 0.25 * 2.0 / 48.0, 0.0]))[None]
    out, model = run(case, keyframe_depths=np.full((1, 80, 96), 2.0, np.float32))
    flags = check(out, model, "edge 0")
    row = flags[0].reshape(80, 96)[5]
    assert row[85] == 3 and row[84] == 7 and row[86] == 1
    assert int(out.inside[0]) == 86 * 80 and int(out.visible[0]) == 85 * 80


def test_two_runs_give_the_same_bits():
    case, kd = mixed_case(seed=22)
    a, _ = run(case, keyframe_depths=kd, depth_tolerance=0.1)
    b, _ = run(case, keyframe_depths=kd, depth_tolerance=0.1)
    assert same_bits(a, b)


@pytest.mark.parametrize("W,H,stride", [(96, 80, 1), (640, 480, 16)], ids=["two-launches", "one-launch"])
def test_replayed_from_a_hipgraph(W, H, stride):
    old, new = random_case(W, H, stride, 5, 31, 5.0), random_case(W, H, stride, 5, 32, 5.0)
    names = ("depth_obs", "viewmatrix", "keyframe_viewmatrices")
    held = {n: torch.from_numpy(old[n]).to(DEV) for n in names}

    def step():
        return slam.keyframe_overlap(*(held[n] for n in names), old["fx"], old["fy"], old["cx"], old["cy"], return_flags=True,
                                     **old["kw"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for n in names:
        held[n].copy_(torch.from_numpy(new[n]))
    graph.replay()
    torch.cuda.synchronize()
    eager, model = run(new)
    check(eager, model, "eager on the new contents")
    assert same_bits(out, eager)


@pytest.mark.parametrize("W,H,stride,K", [(37, 23, 3, 3), (96, 80, 1, 5), (1, 1, 1, 1), (257, 1, 1, 70)])
def test_nothing_is_written_outside_the_outputs(monkeypatch, W, H, stride, K):
    """Every buffer the call allocates (the counts and scores, the flags, the scratch) lies between two guard regions."""
    guarded = GuardedTorch()
    monkeypatch.setattr(keyframes, "torch", guarded)
    case = random_case(W, H, stride, K, 41, 0.5)
    kd = np.random.default_rng(42).uniform(1.0, 4.0, (K, H, W)).astype(np.float32)
    out, _ = run(case, keyframe_depths=kd, depth_tolerance=0.5)
    assert guarded.check() == 3
    assert out.flags.shape == (K, -(-W // stride) * -(-H // stride)) and out.score.shape == (K,)


def test_no_keyframes_returns_empty_tensors():
    case = random_case(37, 23, 3, 1, 51, 2.5)
    args = [torch.from_numpy(case[n]).to(DEV) for n in ("depth_obs", "viewmatrix")]
    out = slam.keyframe_overlap(*args, torch.zeros((0, 4, 4), device=DEV), 30.0, 30.0, 18.0, 11.0, stride=3, return_flags=True)
    assert out.score.shape == out.inside.shape == out.visible.shape == (0,) and out.flags.shape == (0, 104)
    assert out.valid.tolist() == [0] and out.score.dtype == torch.float32 and out.flags.dtype == torch.uint8
    idx, n = slam.select_keyframes(out.score, 2)
    assert idx.tolist() == [-1, -1] and int(n) == 0


def test_wrong_dtype_device_or_shape_raises():
    case = random_case(37, 23, 3, 3, 52, 2.5)
    d, vm, kv = (torch.from_numpy(case[n]).to(DEV) for n in ("depth_obs", "viewmatrix", "keyframe_viewmatrices"))
    f = lambda *a, **kw: slam.keyframe_overlap(*a, 30.0, 30.0, 18.0, 11.0, **kw)  # noqa: E731
    f(d, vm, kv)
    with pytest.raises(ValueError, match="depth_obs must be float32"):
        f(d.double(), vm, kv)
    with pytest.raises(ValueError, match="keyframe_viewmatrices must be float32"):
        f(d, vm, kv.half())
    with pytest.raises(ValueError, match="GPU tensors"):
        f(d, vm.cpu(), kv)
    with pytest.raises(ValueError, match="GPU tensors"):
        f(d, vm, kv, keyframe_depths=torch.ones(3, 23, 37))
    with pytest.raises(ValueError, match=r"viewmatrix is \[4,4\]"):
        f(d, kv, kv)
    with pytest.raises(ValueError, match=r"keyframe_viewmatrices is \[K,4,4\]"):
        f(d, vm, vm)
    with pytest.raises(ValueError, match="keyframe_depths .* is not"):
        f(d, vm, kv, keyframe_depths=torch.ones(3, 23, 36, device=DEV))
    with pytest.raises(ValueError, match="depth_obs is"):
        f(d.reshape(-1), vm, kv)
    # a transposed view is read through a contiguous copy, not refused
    a, b = f(d, vm, kv), f(d.t().contiguous().t(), vm.t().contiguous().t(), kv)
    assert torch.equal(a.inside, b.inside) and torch.equal(a.valid, b.valid)


def test_select_keyframes_on_the_device_without_a_host_read():
    """The selection reads nothing on the host: under torch.cuda.set_sync_debug_mode("error") a synchronising call raises (shown
    first on an .item()), and keyframe_overlap followed by select_keyframes in both modes does not."""
    score = torch.tensor([0.2, 0.9, 0.0, 0.9, 0.5, 0.1], device=DEV)
    case = random_case(37, 23, 3, 6, 61, 2.5)
    args = [torch.from_numpy(case[n]).to(DEV) for n in ("depth_obs", "viewmatrix", "keyframe_viewmatrices")]
    gen = torch.Generator(device=DEV).manual_seed(5)
    slam.keyframe_overlap(*args, case["fx"], case["fy"], case["cx"], case["cy"], **case["kw"])  # (the library is loaded)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            score.sum().item()
        out = slam.keyframe_overlap(*args, case["fx"], case["fy"], case["cx"], case["cy"], **case["kw"])
        window = slam.select_keyframes(out.score, 3)
        top = slam.select_keyframes(score, 3)
        more = slam.select_keyframes(score, 8)
        few = slam.select_keyframes(score, 4, min_overlap=0.45)
        shuffled = slam.select_keyframes(score, 4, min_overlap=0.15, mode="random", generator=gen)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t[0].is_cuda and t[1].is_cuda and t[0].dtype == torch.int64 for t in (window, top, more, few, shuffled))
    assert top[0].tolist() == [1, 3, 4] and int(top[1]) == 3  # the tie goes to the lower index
    assert more[0].tolist() == [1, 3, 4, 0, 5, -1, -1, -1] and int(more[1]) == 5
    assert few[0].tolist() == [1, 3, 4, -1] and int(few[1]) == 3
    assert int(shuffled[1]) == 4 and sorted(shuffled[0].tolist()) == [0, 1, 3, 4]
    n = int(window[1])
    order = window[0].tolist()
    s = out.score.tolist()
    assert order[n:] == [-1] * (3 - n) and all(s[i] > 0 for i in order[:n])
    assert order[:n] == sorted(range(6), key=lambda i: (-s[i], i))[:n]
    seen = {tuple(slam.select_keyframes(score, 4, min_overlap=0.15, mode="random", generator=gen)[0].tolist()) for _ in range(8)}
    assert len(seen) > 1 and all(sorted(p) == [0, 1, 3, 4] for p in seen)
