"""The complete pose gradient on the GPU (option "pose_grad" = 1, include/dgr_hip.h): against the float64 formulation of
tests/fp64_model.py (complete_forward), the translation identity at size, tracking (map_off) against mapping, the default mode
untouched, deterministic sums, the batched entry points and the options snapshot of a forward."""
import numpy as np
import pytest
import torch

import hip_helpers as hh
from dgr_amd import _capi
from dgr_amd import light as L
from dgr_amd.synth import heavy_tail_scene
from fp64_model import CASES, complete_grad, oracle_run, scaled_grads
from hip_helpers import binding  # noqa: F401  (fixture)
from util import make_scene

pytestmark = pytest.mark.gpu


def _precomp(s, kind):
    if kind == "colors":
        return dict(colors_precomp=np.random.default_rng(5).uniform(0.0, 1.0, (s.P, 3)).astype(np.float32))
    if kind == "cov3D":
        return dict(cov3D_precomp=hh.hip_cov3D(s).astype(np.float32))
    return {}


def hip_view_grad(s, variant, deg, grads, map_off=False, pose_grad=None, **pre):
    """dL_dview [16] (and the full gradient dict) of one HIP forward + backward; pose_grad None: the option left alone."""
    g32 = tuple(np.asarray(x, np.float32) for x in grads)
    opts = {} if pose_grad is None else dict(pose_grad=pose_grad)
    with _capi.thread_options(**opts):
        if variant == "light":
            out, _ = hh.hip_forward(s, deg, **pre)
            g = hh.hip_backward(s, deg, out, map_off=map_off, grads=g32, **pre)
        else:
            out, _ = hh.hip_full_forward(s, deg, **pre)
            g = hh.hip_full_backward(s, deg, out, grads=g32, **pre)
    torch.cuda.synchronize()
    return np.asarray(g["dL_dview"], np.float64).reshape(-1), g


FP64_CASES = [(c, "sh") for c in CASES] + [(CASES[0], "colors"), (CASES[2], "cov3D")]


@pytest.mark.parametrize("mode", ["light", "light_map_off", "full"])
@pytest.mark.parametrize("case,pre", FP64_CASES)
def test_complete_pose_gradient_against_fp64(oracle, case, pre, mode):
    P, W, H, deg, seed = case
    variant = "full" if mode == "full" else "light"
    s = make_scene(P, W, H, seed)
    kw = _precomp(s, pre)
    grads = scaled_grads(s, variant)
    st, ref, _ = oracle_run(oracle, s, variant, deg, grads, **kw)
    want, _, _, _ = complete_grad(s, variant, deg, st, ref, grads, **kw)
    scale = np.abs(want).max()
    got, _ = hip_view_grad(s, variant, deg, grads, map_off=mode == "light_map_off", pose_grad=1, **kw)
    assert np.abs(got - want).max() <= 5e-5 * scale, f"complete: {np.abs(got - want).max() / scale:.2e} of scale"
    dflt, _ = hip_view_grad(s, variant, deg, grads, map_off=mode == "light_map_off", **kw)
    assert np.abs(dflt - want).max() >= 1e-3 * scale, "the default mode is indistinguishable from the complete gradient here"


def _identity_distance(s, g_view, g_means):
    Rc = s.view[:3, :3].T.astype(np.float64)  # Rcam[j][k] = v[4k + j]
    rhs = np.asarray(g_view, np.float64).reshape(-1)[12:15]
    lhs = Rc @ np.asarray(g_means, np.float64).sum(0)
    return float(np.abs(lhs - rhs).max() / np.abs(rhs).max())


@pytest.mark.parametrize("scene", ["uniform", "heavy_tail"])
@pytest.mark.parametrize("mode", ["light", "light_map_off", "full"])
def test_translation_identity_at_size(scene, mode):
    s = make_scene(100000, 640, 480, 0)
    if scene == "heavy_tail":
        s = heavy_tail_scene(s)
    variant = "full" if mode == "full" else "light"
    grads = (s.gC, s.gD, s.gM, s.gV) if variant == "light" else (s.gC, s.gD, s.gV)
    d = {}
    for name, pg in (("complete", 1), ("default", 0)):
        gv, g = hip_view_grad(s, variant, 3, grads, map_off=mode == "light_map_off", pose_grad=pg)
        gm = g["dL_dmeans3D"] if mode != "light_map_off" else hip_view_grad(s, variant, 3, grads, pose_grad=pg)[1]["dL_dmeans3D"]
        d[name] = _identity_distance(s, gv, gm)
    print(f"\n{scene} {mode}: |dL/dt - Rcam sum dL/dmeans3D| / |dL/dt| = {d['complete']:.2e} complete, {d['default']:.2e} default")
    assert d["complete"] <= 2e-4, d
    assert d["default"] >= 10 * 2e-4, d  # the bar separates the two modes


def test_tracking_equals_mapping_and_leaves_the_per_gaussian_outputs_alone():
    s = make_scene(20000, 320, 240, 4)
    grads = (s.gC, s.gD, s.gM, s.gV)
    v_map, _ = hip_view_grad(s, "light", 3, grads, pose_grad=1)
    v_trk, g_trk = hip_view_grad(s, "light", 3, grads, map_off=True, pose_grad=1)
    assert np.abs(v_trk - v_map).max() <= 2e-6 * np.abs(v_map).max()
    _, g_def = hip_view_grad(s, "light", 3, grads, map_off=True, pose_grad=0)
    for k, v in g_def.items():
        if k != "dL_dview":
            assert np.array_equal(np.asarray(g_trk[k]).view(np.uint32), np.asarray(v).view(np.uint32)), k


@pytest.mark.parametrize("variant", ["light", "full"])
def test_explicit_default_is_bit_identical(variant):
    s = make_scene(20000, 320, 240, 5)
    grads = (s.gC, s.gD, s.gM, s.gV) if variant == "light" else (s.gC, s.gD, s.gV)
    with _capi.thread_options(deterministic_grads=1):
        _, a = hip_view_grad(s, variant, 3, grads)
        _, b = hip_view_grad(s, variant, 3, grads, pose_grad=0)
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), k


def _render_views_pose(ss, variant, complete, batch):
    from dgr_amd import slam
    from test_hip_full_batch import Model
    s = ss[0]
    H, W = s.H, s.W
    bg, gt = hh.T(s.bg), hh.T(s.gt)
    gen = torch.Generator(device="cpu").manual_seed(9)
    w = [(torch.randn((len(ss), c, H, W), generator=gen) / (H * W) ** 0.5).to(hh.dev()) for c in (3, 1)]
    cams = [dict(viewmatrix=hh.T(x.view).requires_grad_(), fov=(x.tanfovx, x.tanfovy), HW=(H, W), gt_depth=gt) for x in ss]
    pc = Model(s, hh.dev())
    if batch:
        out = slam.render_views(cams, pc, None, bg, variant=variant, complete_pose=complete)
        ((out["render"] * w[0]).sum() + (out["depth"] * w[1]).sum()).backward()
    else:
        for k, c in enumerate(cams):
            o = slam.render(None, pc, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"], HW=c["HW"], gt_depth=gt,
                            variant=variant, complete_pose=complete)
            ((o["render"] * w[0][k]).sum() + (o["depth"] * w[1][k]).sum()).backward()
    torch.cuda.synchronize()
    return [c["viewmatrix"].grad.detach().cpu().numpy().astype(np.float64) for c in cams]


@pytest.mark.parametrize("variant", ["light", "full"])
def test_batched_views_match_the_one_view_calls(variant):
    ss = [make_scene(20000, 256, 192, 3, view_index=v) for v in range(3)]
    one = _render_views_pose(ss, variant, True, batch=False)
    bat = _render_views_pose(ss, variant, True, batch=True)
    dflt = _render_views_pose(ss, variant, False, batch=True)
    for k in range(3):
        scale = np.abs(one[k]).max()
        assert np.abs(bat[k] - one[k]).max() <= 1e-5 * scale, k
        assert np.abs(dflt[k] - one[k]).max() > 1e-3 * scale, k  # (the batch does run the complete mode)


def test_deterministic_complete_pose_repeats_bit_for_bit():
    s = make_scene(20000, 320, 240, 6)
    ss = [make_scene(20000, 256, 192, 3, view_index=v) for v in range(3)]
    with _capi.thread_options(deterministic_grads=1, pose_grad=1):
        for variant, grads in (("light", (s.gC, s.gD, s.gM, s.gV)), ("full", (s.gC, s.gD, s.gV))):
            a, _ = hip_view_grad(s, variant, 3, grads)
            b, _ = hip_view_grad(s, variant, 3, grads)
            assert np.array_equal(a, b), variant
        a = _render_views_pose(ss, "light", False, batch=True)  # (complete through the enclosing thread option)
        b = _render_views_pose(ss, "light", False, batch=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_backward_follows_its_forwards_pose_grad(binding):
    from dgr_amd.multiview import make_settings
    s = make_scene(20000, 320, 240, 7)
    rast = L.GaussianRasterizer(make_settings(s, 3, hh.dev()))

    def run(fwd_opts, bwd_opts):
        leaves = [hh.T(a).requires_grad_() for a in (s.means, s.shs, s.opac, s.scales, s.rots, s.view)]
        m2 = torch.zeros((s.P, 3), device=hh.dev(), requires_grad=True)
        with _capi.thread_options(**fwd_opts):
            o = rast(means3D=leaves[0], means2D=m2, opacities=leaves[2], shs=leaves[1], scales=leaves[3], rotations=leaves[4],
                     viewmatrix=leaves[5], gt_depth=hh.T(s.gt))
        with _capi.thread_options(**bwd_opts):
            torch.autograd.backward([o[0], o[2], o[3], o[4]],
                                    [hh.T(s.gC), hh.T(s.gD[None]), hh.T(s.gM[None]), hh.T(s.gV[None])])
        torch.cuda.synchronize()
        return leaves[5].grad.cpu().numpy().astype(np.float64)

    inside = run(dict(pose_grad=1), dict(pose_grad=1))
    after = run(dict(pose_grad=1), {})         # the block has exited: the backward follows the forward's snapshot
    crossed = run({}, dict(pose_grad=1))       # ... and a later setting does not reach an earlier forward's backward
    scale = np.abs(inside).max()
    assert np.abs(after - inside).max() <= 2e-6 * scale
    assert np.abs(crossed - inside).max() > 1e-3 * scale
