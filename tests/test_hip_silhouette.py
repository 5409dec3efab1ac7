"""The exact silhouette gradient on the GPU (option "silhouette_grad", include/dgr_hip.h: dgr_*_backward*_silhouette).

The float64 reference is tests/fp64_model.complete_forward: the silhouette A = sum alpha T = 1 - T_final, and the
forward's colour carries T_final through its background term, so a loss sum g_A A is (up to a constant) the colour loss
-sum g_A T_final of a second call with zero colours, background (1, 0, 0) and colour gradient (-g_A, 0, 0) -- same decisions,
same leaves.  Its gradients are added to those of the first call's loss.  Without the feature the HIP gradients of a silhouette
loss are zero (light) or the depth-variance quirk (full), and the parity tests fail.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hip_helpers as hh
from dgr_amd import _capi
from dgr_amd import full as F
from dgr_amd import light as L
from fp64_model import C0, absgrad_of_pairs, complete_forward, oracle_run, torch_full, torch_light
from hip_helpers import binding  # noqa: F401  (fixture)
from util import bits_equal, make_scene

pytestmark = pytest.mark.gpu

T, E = hh.T, hh.E
CASES = [(400, 64, 48, 3, 11), (300, 40, 40, 0, 12), (500, 70, 45, 2, 13)]
PER_GAUSSIAN = {"opacities": 2, "means3D": 3, "shs": 5, "scales": 6, "rotations": 7}  # leaf -> index in the backward's tuple


def sil_image(s, seed=3):
    return np.random.default_rng(seed).normal(0.0, 1.0, (s.H, s.W))


def fp64_grads(s, variant, deg, st, ref, grads, gA, added):
    """float64 dL/dleaf of sum <grads, images> + sum gA * silhouette (complete_forward; `added`: its complete pose formulation,
    else the light reference split).  Returns {leaf: array} with view [16] (3, 7, 11, 15 zeroed)."""
    dec = (ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"))
    out = {}

    def run(scene, g, **kw):
        loss, leaves, _, _ = complete_forward(scene, variant, deg, *dec, g, added=added, **kw)
        loss.backward()
        for k in list(PER_GAUSSIAN) + ["view"]:
            if leaves[k].grad is not None:
                out[k] = out.get(k, 0.0) + leaves[k].grad.numpy().astype(np.float64)

    if grads is not None:
        run(s, grads)
    if gA is not None:
        zero = np.zeros((s.H, s.W))
        gC = np.stack([-np.asarray(gA, np.float64), zero, zero])
        g2 = (gC, zero, zero, zero) if variant == "light" else (gC, zero, zero)
        run(s._replace(bg=np.array([1.0, 0.0, 0.0], np.float32)), g2, colors_precomp=np.zeros((s.P, 3), np.float32))
    out["view"] = out["view"].reshape(-1).copy()
    out["view"][[3, 7, 11, 15]] = 0.0
    return out


def _host(g):
    torch.cuda.synchronize()
    return [None if x is None else x.detach().cpu().numpy().astype(np.float64) for x in g]


def hip_light(s, deg, out, grads, gA=None, **kw):
    return _host(hh.hip_backward_raw(s, deg, out, grads=grads, silhouette=gA, **kw))


def hip_full(s, deg, out, grads, gA=None, **kw):
    return _host(hh.hip_full_backward_raw(s, deg, out, grads=grads, silhouette=gA, **kw))


def check(got, want, what, tol=5e-5):
    scale = np.abs(want).max()
    assert scale > 0, what
    err = np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max() / scale
    assert err <= tol, f"{what}: {err:.2e} of the tensor's scale"


def close(a, b, what, tol=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    assert np.abs(a - b).max() <= tol * scale, f"{what}: {np.abs(a - b).max() / scale:.2e} of scale"


f32 = np.float32  # (_host brings the gradients over as float64, each the exact image of an fp32 value: back to the computed bits)


def model_leaves(pc):
    return {"means3D": pc.get_xyz, "opacities": pc.get_opacity, "scales": pc.get_scaling, "rotations": pc.get_rotation,
            "shs": pc.get_features}


class _Cam:
    """the scene's own projection (Proj^T) for slam.render, so that its frame is the oracle's"""
    def __init__(self, s):
        self.projection_matrix = T(s.persp)


def view16(g):
    v = np.asarray(g, np.float64).reshape(-1).copy()
    v[[3, 7, 11, 15]] = 0.0
    return v


# ---- 1. parity with float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["silhouette", "all", "all_lean"])
@pytest.mark.parametrize("pose_grad", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_light_silhouette_matches_fp64(oracle, binding, case, pose_grad, loss):
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    k = (W * H) ** 0.5
    grads = [np.asarray(g, np.float64) * k for g in (s.gC, s.gD, s.gM, s.gV)]
    zero = np.zeros((H, W))
    if loss == "silhouette":
        grads = [np.zeros((3, H, W)), zero, zero, zero]
    elif loss == "all_lean":
        grads[2], grads[3] = zero, zero
    gA = sil_image(s) * k
    st, ref, _ = oracle_run(oracle, s, "light", deg, grads)
    want = fp64_grads(s, "light", deg, st, ref, None if loss == "silhouette" else grads, gA, added=pose_grad == 1)
    with _capi.thread_options(pose_grad=pose_grad):
        out, d = hh.hip_forward(s, deg)
        assert np.array_equal(d["radii"], ref["radii"])
        lean = loss != "all"
        g = hip_light(s, deg, out, [grads[0], grads[1], None if lean else grads[2], None if lean else grads[3]], gA)
    for leaf, i in PER_GAUSSIAN.items():
        if leaf == "shs" and loss == "silhouette":
            assert np.abs(g[i]).max() == 0.0
            continue
        # (the SH gradient is colour-only -- the silhouette term does not reach it -- and carries fp32 SH evaluation error)
        check(g[i], want[leaf], f"light {loss} pose_grad={pose_grad} {leaf}", tol=2e-4 if leaf == "shs" else 5e-5)
    check(view16(g[8]), want["view"], f"light {loss} pose_grad={pose_grad} view")


@pytest.mark.parametrize("loss", ["silhouette", "all"])
@pytest.mark.parametrize("case", CASES)
def test_full_silhouette_matches_fp64(oracle, binding, case, loss):
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    k = (W * H) ** 0.5
    zero = np.zeros((H, W))
    grads = [np.zeros((3, H, W)), zero, zero] if loss == "silhouette" else [np.asarray(s.gC) * k, np.asarray(s.gD) * k, zero]
    gA = sil_image(s) * k
    st, ref, _ = oracle_run(oracle, s, "full", deg, grads)
    want = fp64_grads(s, "full", deg, st, ref, None if loss == "silhouette" else grads, gA, added=True)
    with _capi.thread_options(pose_grad=1):
        out, d = hh.hip_full_forward(s, deg)
        assert np.array_equal(d["radii"], ref["radii"])
        g = hip_full(s, deg, out, [grads[0], grads[1], None], gA)
    for leaf, i in PER_GAUSSIAN.items():
        if leaf == "shs" and loss == "silhouette":
            continue
        check(g[i], want[leaf], f"full {loss} {leaf}", tol=2e-4 if leaf == "shs" else 5e-5)
    check(view16(g[8]), want["view"], f"full {loss} view (pose_grad=1)")


def test_full_reference_pose_gradient_does_not_see_the_silhouette():
    """pose_grad = 0: the full variant's dL_dview reads the colour-only and front-most-depth sums, which no background share
    reaches (include/dgr_hip.h): the same bits with and without the silhouette image."""
    s = make_scene(3000, 96, 64, 4)
    gA = sil_image(s)
    with _capi.thread_options(deterministic_grads=1, pose_grad=0):
        out, _ = hh.hip_full_forward(s, 3)
        a = hip_full(s, 3, out, [s.gC, s.gD, None], gA)
        b = hip_full(s, 3, out, [s.gC, s.gD, None])
    assert bits_equal(f32(a[8]), f32(b[8])), "dL_dview"
    assert np.abs(a[3] - b[3]).max() > 0  # (while the per-Gaussian gradients do change)


# ---- 2. background identity ---------------------------------------------------------------------------------------------------
def bg_identity(s, variant, map_off=False, deg=3):
    """g_A = <bg, g_C> per pixel with bg against bg = 0 and no silhouette image, from one forward state."""
    gA = np.einsum("c,chw->hw", np.asarray(s.bg, np.float64), np.asarray(s.gC, np.float64))
    zero_bg = np.zeros(3, np.float32)
    if variant == "light":
        out, _ = hh.hip_forward(s, deg)
        a = hip_light(s, deg, out, [s.gC, s.gD, None, None], gA, map_off=map_off)
        b = hip_light(s, deg, out, [s.gC, s.gD, None, None], bg=zero_bg, map_off=map_off)
    else:
        out, _ = hh.hip_full_forward(s, deg)
        a = hip_full(s, deg, out, [s.gC, s.gD, None], gA)
        b = hip_full(s, deg, out, [s.gC, s.gD, None], bg=zero_bg)
    return a, b


@pytest.mark.parametrize("mode", ["light", "light_map_off", "full"])
def test_background_identity(mode):
    s = make_scene(20000, 320, 240, 5)
    a, b = bg_identity(s, "full" if mode == "full" else "light", map_off=mode == "light_map_off")
    if mode == "light_map_off":
        close(view16(a[8]), view16(b[8]), "dL_dview")
        return
    for i, name in enumerate(("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations", "view")):
        close(a[i], b[i], name)


# ---- 3. linearity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["light", "full"])
def test_linearity(variant):
    s = make_scene(20000, 320, 240, 8)
    gA = sil_image(s)
    zc, zd = np.zeros_like(s.gC), np.zeros_like(s.gD)
    if variant == "light":
        out, _ = hh.hip_forward(s, 3)
        both = hip_light(s, 3, out, [s.gC, s.gD, None, None], gA)
        cd = hip_light(s, 3, out, [s.gC, s.gD, None, None])
        sil = hip_light(s, 3, out, [zc, zd, None, None], gA)
    else:
        out, _ = hh.hip_full_forward(s, 3)
        both = hip_full(s, 3, out, [s.gC, s.gD, None], gA)
        cd = hip_full(s, 3, out, [s.gC, s.gD, None])
        sil = hip_full(s, 3, out, [zc, zd, None], gA)
    for i in (0, 2, 3, 5, 6, 7, 8):
        close(both[i], cd[i] + sil[i], f"{variant} {i}", tol=2e-6)
    assert np.abs(sil[3]).max() > 0


# ---- 4. every path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lists", [0, 1, 2])
@pytest.mark.parametrize("alpha_mode", [0, 1, 2])
def test_identity_on_every_lane_list_and_alpha_mode(alpha_mode, lists):
    s = make_scene(20000, 320, 240, 9)
    _capi.set_option("lane_lists", lists)
    try:
        with _capi.thread_options(alpha_mode=alpha_mode):
            for mode in ("light", "light_map_off", "full"):
                a, b = bg_identity(s, "full" if mode == "full" else "light", map_off=mode == "light_map_off")
                close(view16(a[8]), view16(b[8]), f"{mode} view")
                if mode != "light_map_off":
                    for i in (0, 2, 3, 6, 7):
                        close(a[i], b[i], f"{mode} {i}")
    finally:
        _capi.set_option("lane_lists", 2)


@pytest.mark.parametrize("variant", ["light", "full"])
def test_deterministic_silhouette_repeats_bit_for_bit(variant):
    s = make_scene(20000, 320, 240, 10)
    gA = sil_image(s)
    with _capi.thread_options(deterministic_grads=1):
        for lean in (True, False):
            if variant == "light":
                out, _ = hh.hip_forward(s, 3)
                gr = [s.gC, s.gD, None if lean else s.gM, None if lean else s.gV]
                a, b = (hip_light(s, 3, out, gr, gA) for _ in range(2))
            else:
                out, _ = hh.hip_full_forward(s, 3)
                a, b = (hip_full(s, 3, out, [s.gC, s.gD, None if lean else s.gV], gA) for _ in range(2))
            for i, (x, y) in enumerate(zip(a, b)):
                if x is not None:
                    assert bits_equal(f32(x), f32(y)), f"{variant} lean={lean} {i}"
            # ... and the identity holds there too
            if lean:
                p, q = bg_identity(s, variant)
                close(p[3], q[3], "means3D")


@pytest.mark.parametrize("alpha_mode", [0, 1])
@pytest.mark.parametrize("variant", ["light", "full"])
def test_absgrad_with_silhouette(variant, alpha_mode):
    """absgrad's v_p(g) is every term reaching it through alpha at p: with the silhouette term, the absgrad of (colour, bg) with
    g_A = <bg, g_C> equals that of bg = 0 without it (the identity per pixel, so per |v_p| too)."""
    s = make_scene(20000, 320, 240, 12)
    gA = np.einsum("c,chw->hw", np.asarray(s.bg, np.float64), np.asarray(s.gC, np.float64))
    zero_bg = np.zeros(3, np.float32)
    with _capi.thread_options(alpha_mode=alpha_mode):
        if variant == "light":
            out, _ = hh.hip_forward(s, 3)
            a = hip_light(s, 3, out, [s.gC, s.gD, None, None], gA, absgrad=True)
            b = hip_light(s, 3, out, [s.gC, s.gD, None, None], bg=zero_bg, absgrad=True)
            c = hip_light(s, 3, out, [s.gC, s.gD, None, None], absgrad=True)
        else:
            out, _ = hh.hip_full_forward(s, 3)
            a = hip_full(s, 3, out, [s.gC, s.gD, None], gA, absgrad=True)
            b = hip_full(s, 3, out, [s.gC, s.gD, None], bg=zero_bg, absgrad=True)
            c = hip_full(s, 3, out, [s.gC, s.gD, None], absgrad=True)
    assert len(a) == 10
    close(a[9], b[9], "absgrad", tol=2e-6)
    close(a[3], b[3], "means3D")
    assert np.abs(a[9] - c[9]).max() > 1e-4 * np.abs(c[9]).max()  # (the term does reach absgrad)


@pytest.mark.parametrize("variant", ["light", "full"])
def test_batch_matches_one_view_calls(binding, variant):
    from dgr_amd import slam
    from test_hip_full_batch import Model
    ss = [make_scene(20000, 256, 192, 3, view_index=v) for v in range(3)]
    s = ss[0]
    H, W = s.H, s.W
    bg, gt = T(s.bg), T(s.gt)
    gen = torch.Generator(device="cpu").manual_seed(4)
    wc = (torch.randn((3, 3, H, W), generator=gen) / (H * W) ** 0.5).to(hh.dev())
    wa = (torch.randn((3, 1, H, W), generator=gen) / (H * W) ** 0.5).to(hh.dev())  # a different g_A per view

    def run(batch):
        pc = Model(s, hh.dev())
        cams = [dict(viewmatrix=T(x.view).requires_grad_(), fov=(x.tanfovx, x.tanfovy), HW=(H, W), gt_depth=gt) for x in ss]
        if batch:
            out = slam.render_views(cams, pc, None, bg, variant=variant, silhouette_grad=True, absgrad=True)
            ((out["render"] * wc).sum() + (out["opacity_map"] * wa).sum()).backward()
            ab = out["viewspace_points_abs"].grad
        else:
            ab = []
            for k, c in enumerate(cams):
                o = slam.render(None, pc, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"], HW=c["HW"], gt_depth=gt,
                                variant=variant, silhouette_grad=True, absgrad=True)
                ((o["render"] * wc[k]).sum() + (o["opacity_map"] * wa[k]).sum()).backward()
                ab.append(o["viewspace_points_abs"].grad)
            ab = torch.stack(ab)
        torch.cuda.synchronize()
        g = {n: t.grad.detach().cpu().numpy().astype(np.float64) for n, t in model_leaves(pc).items()}
        g.update({f"absgrad{k}": ab[k].detach().cpu().numpy().astype(np.float64) for k in range(len(cams))})
        g.update({f"view{k}": c["viewmatrix"].grad.detach().cpu().numpy().astype(np.float64) for k, c in enumerate(cams)})
        return g

    one, bat = run(False), run(True)
    for n in one:
        close(bat[n], one[n], n, tol=1e-5)


def test_tracking_step_replayed_from_a_graph_equals_eager(monkeypatch):
    monkeypatch.setenv("DGR_SYNC_MODE", "lazy")  # (a capturable forward: the status words are read lazily)
    s = make_scene(20000, 320, 240, 13)
    gA = T(sil_image(s).astype(np.float32)[None])
    gC, gD, gt = T(s.gC), T(s.gD[None]), T(s.gt)
    from dgr_amd.multiview import make_settings
    rast = L.GaussianRasterizer(make_settings(s, 3, hh.dev(), map_off=True))
    means, shs, opac, scales, rots = (T(a) for a in (s.means, s.shs, s.opac, s.scales, s.rots))
    view = T(s.view).requires_grad_()
    m2 = torch.zeros((s.P, 3), device=hh.dev())

    def step():
        view.grad = None
        with _capi.thread_options(silhouette_grad=1):
            o = rast(means3D=means, means2D=m2, opacities=opac, shs=shs, scales=scales, rotations=rots, viewmatrix=view,
                     gt_depth=gt)
        ((o[0] * gC).sum() + (o[2] * gD).sum() + (o[5] * gA).sum()).backward()
        return view.grad

    step()
    eager = step().clone()
    L.check_async_errors()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = step()
    L.check_async_errors()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        close(res.cpu().numpy(), eager.cpu().numpy(), "replayed dL_dview", tol=2e-6)
    L.check_captured_status()
    # (and the silhouette term is in it: the eager step without it differs)
    with _capi.thread_options(silhouette_grad=0):
        view.grad = None
        o = rast(means3D=means, means2D=m2, opacities=opac, shs=shs, scales=scales, rotations=rots, viewmatrix=view, gt_depth=gt)
        ((o[0] * gC).sum() + (o[2] * gD).sum() + (o[5] * gA).sum()).backward()
    torch.cuda.synchronize()
    assert (view.grad - eager).abs().max().item() > 1e-4 * eager.abs().max().item()


def fp64_absgrad(s, variant, deg, st, ref, grads, gA):
    """float64 sum_p |v_p(g)| of sum <grads, images> + sum gA * silhouette: the per-(Gaussian, pixel) leaves of the two calls of
    fp64_grads (torch_light / torch_full in pairs mode), added per pixel before the absolute value"""
    dec = (ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"))
    zero = np.zeros((s.H, s.W))
    gC = np.stack([-np.asarray(gA, np.float64), zero, zero])
    s2 = s._replace(bg=np.array([1.0, 0.0, 0.0], np.float32))
    p1, p2 = [], []
    if variant == "light":
        torch_light(s, deg, *dec, grads, pairs=p1)[0].backward()
        torch_light(s2, deg, *dec, (gC, zero, zero, zero), pairs=p2, colors_precomp=np.zeros((s.P, 3), np.float32))[0].backward()
    else:  # (no colour input: SH whose colour is 0, C0 sh_0 + 1/2 = 0)
        torch_full(s, deg, *dec, grads, pairs=p1)[0].backward()
        sh0 = np.zeros_like(np.asarray(s.shs, np.float64))
        sh0[:, 0, :] = -0.5 / C0
        torch_full(s2._replace(shs=sh0), deg, *dec, (gC, zero, zero), pairs=p2)[0].backward()
    assert len(p1) == len(p2)
    merged = []
    for (ids, a), (ids2, b) in zip(p1, p2):
        assert torch.equal(ids, ids2)
        ga = a.grad if a.grad is not None else torch.zeros_like(a)
        gb = b.grad if b.grad is not None else torch.zeros_like(b)
        merged.append((ids, SimpleNamespace(grad=ga + gb)))
    return absgrad_of_pairs(merged, np.nonzero(ref["radii"] > 0)[0], s.P, s.W, s.H)


@pytest.mark.parametrize("alpha_mode", [0, 1])
@pytest.mark.parametrize("variant", ["light", "full"])
def test_absgrad_with_silhouette_matches_fp64(oracle, binding, variant, alpha_mode):
    P, W, H, deg, seed = CASES[0]
    s = make_scene(P, W, H, seed)
    k = (W * H) ** 0.5
    zero = np.zeros((H, W))
    grads = [np.asarray(s.gC, np.float64) * k, np.asarray(s.gD, np.float64) * k, zero] + ([zero] if variant == "light" else [])
    gA = sil_image(s) * k
    st, ref, _ = oracle_run(oracle, s, variant, deg, grads)
    want = fp64_absgrad(s, variant, deg, st, ref, grads, gA)
    with _capi.thread_options(alpha_mode=alpha_mode):
        if variant == "light":
            out, _ = hh.hip_forward(s, deg)
            g = hip_light(s, deg, out, [grads[0], grads[1], None, None], gA, absgrad=True)
            g0 = hip_light(s, deg, out, [grads[0], grads[1], None, None], absgrad=True)
        else:
            out, _ = hh.hip_full_forward(s, deg)
            g = hip_full(s, deg, out, [grads[0], grads[1], None], gA, absgrad=True)
            g0 = hip_full(s, deg, out, [grads[0], grads[1], None], absgrad=True)
    check(g[9], want, f"{variant} absgrad with silhouette")
    assert np.all(g[9][:, 2] == 0)
    assert np.abs(g0[9] - want).max() > 1e-3 * np.abs(want).max()  # (without the image it is not this)


# ---- 5. default off -----------------------------------------------------------------------------------------------------------
def _node_grads(s, variant, loss_outputs, opts):
    from dgr_amd.multiview import make_settings
    mod = L if variant == "light" else F
    settings = make_settings(s, 3, hh.dev())
    if variant == "full":
        settings = F.GaussianRasterizationSettings(**{k: getattr(settings, k) for k in F.GaussianRasterizationSettings._fields})
    rast = mod.GaussianRasterizer(settings)
    leaves = [T(a).requires_grad_() for a in (s.means, s.shs, s.opac, s.scales, s.rots, s.view)]
    m2 = torch.zeros((s.P, 3), device=hh.dev(), requires_grad=True)
    with _capi.thread_options(**opts):
        o = rast(means3D=leaves[0], means2D=m2, opacities=leaves[2], shs=leaves[1], scales=leaves[3], rotations=leaves[4],
                 viewmatrix=leaves[5], gt_depth=T(s.gt))
    imgs = {"color": o[0], "depth": o[2], "sil": o[5] if variant == "light" else o[3]}
    w = {"color": T(s.gC), "depth": T(s.gD[None]), "sil": T(sil_image(s).astype(np.float32)[None])}
    sum((imgs[n] * w[n]).sum() for n in loss_outputs).backward()
    torch.cuda.synchronize()
    return [t.grad.detach().cpu().numpy() for t in leaves + [m2]]


@pytest.mark.parametrize("variant", ["light", "full"])
def test_default_off_is_bit_identical(variant):
    s = make_scene(20000, 320, 240, 14)
    det = dict(deterministic_grads=1)
    if variant == "light":  # a loss on opacity_map trains nothing, as in the reference
        a = _node_grads(s, "light", ("color", "depth", "sil"), det)
        b = _node_grads(s, "light", ("color", "depth"), det)
    else:  # the uncertainty gradient is the variance quirk: the image as dL_duncertainties
        a = _node_grads(s, "full", ("color", "depth", "sil"), det)
        with _capi.thread_options(**det):
            out, _ = hh.hip_full_forward(s, 3)
            g = hip_full(s, 3, out, [s.gC, s.gD, sil_image(s)])
        b = [g[3], g[5], g[2], g[6], g[7], view16(g[8]).reshape(4, 4), g[0]]
        a[5] = view16(a[5]).reshape(4, 4)
    for i, (x, y) in enumerate(zip(a, b)):
        assert bits_equal(f32(x), f32(y)), f"{variant} {i}"
    on = _node_grads(s, variant, ("color", "depth", "sil"), dict(det, silhouette_grad=1))
    assert np.abs(on[0] - a[0]).max() > 0  # (and the option does change them)


class _NullSilhouette:
    """The library with every namesake call routed to its _silhouette entry point and a NULL image -- or, for the batches, a NULL
    array (`entries` None) or an array of NULL entries (`entries` True)."""

    def __init__(self, lib, entries):
        self._lib, self._entries = lib, entries

    def __getattr__(self, name):
        lib, fn = self._lib, getattr(self._lib, name)
        if name in ("dgr_light_backward", "dgr_full_backward"):
            return lambda *a: getattr(lib, name + "_silhouette")(*a, None, None)
        if name in ("dgr_light_backward_absgrad", "dgr_full_backward_absgrad"):
            return lambda *a: getattr(lib, name.replace("_absgrad", "_silhouette"))(*a, None)
        if name in ("dgr_light_backward_batch", "dgr_full_backward_batch"):
            return lambda *a: getattr(lib, name + "_silhouette")(*a, None, self._array(a[1]))
        if name in ("dgr_light_backward_batch_absgrad", "dgr_full_backward_batch_absgrad"):
            return lambda *a: getattr(lib, name.replace("_absgrad", "_silhouette"))(*a, self._array(a[1]))
        return fn

    def _array(self, n_views):
        return (C.c_void_p * n_views)(*([None] * n_views)) if self._entries else None


def _ctypes_grads(s, lean):
    """one-view light and full backwards and a light and full batch through the ctypes binding, under deterministic_grads (absgrad
    has no deterministic form: its namesakes are routed as the others, but cannot be compared bit for bit)"""
    from dgr_amd import slam
    from test_hip_full_batch import Model
    res = []
    with _capi.thread_options(deterministic_grads=1):
        out, _ = hh.hip_forward(s, 3)
        res += hip_light(s, 3, out, [s.gC, s.gD, None if lean else s.gM, None if lean else s.gV])
        outf, _ = hh.hip_full_forward(s, 3)
        res += hip_full(s, 3, outf, [s.gC, s.gD, None if lean else s.gV])
    ss = [make_scene(3000, 96, 64, 3, view_index=v) for v in range(3)]
    with _capi.thread_options(deterministic_grads=1):
        for variant in ("light", "full"):
            pc = Model(ss[0], hh.dev())
            cams = [dict(viewmatrix=T(x.view).requires_grad_(), fov=(x.tanfovx, x.tanfovy), HW=(x.H, x.W), gt_depth=T(ss[0].gt))
                    for x in ss]
            o = slam.render_views(cams, pc, None, T(ss[0].bg), variant=variant)
            ((o["render"] * T(np.stack([x.gC for x in ss]))).sum() + o["depth"].sum()).backward()
            res += [t.grad for t in model_leaves(pc).values()] + [c["viewmatrix"].grad for c in cams]
    torch.cuda.synchronize()
    return [None if x is None else (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x) for x in res]


@pytest.mark.parametrize("entries", [None, True])
def test_null_image_is_bit_identical_to_the_namesakes(monkeypatch, entries):
    monkeypatch.setattr(L, "_C", L._CtypesC)
    monkeypatch.setattr(F, "_C", F._CtypesC)
    s = make_scene(20000, 320, 240, 15)
    for lean in (True, False):
        want = _ctypes_grads(s, lean)
        lib = _capi.load()
        monkeypatch.setattr(_capi, "_lib", _NullSilhouette(lib, entries))
        got = _ctypes_grads(s, lean)
        monkeypatch.setattr(_capi, "_lib", lib)
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            if b is None:
                assert a is None, i
            else:
                assert bits_equal(f32(a), f32(b)), f"lean={lean} result {i}"


# ---- 6. SLAM surface ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["light", "full"])
def test_slam_render_opacity_map_gradient_matches_fp64(oracle, binding, variant):
    from dgr_amd import slam
    from test_hip_full_batch import Model
    P, W, H, deg, seed = CASES[0]
    s = make_scene(P, W, H, seed)
    k = (W * H) ** 0.5
    gA = sil_image(s) * k
    zero = np.zeros((H, W))
    grads = [np.zeros((3, H, W)), zero, zero, zero][: 4 if variant == "light" else 3]
    st, ref, _ = oracle_run(oracle, s, variant, deg, grads)
    want = fp64_grads(s, variant, deg, st, ref, None, gA, added=True)
    assert deg == 3  # (Model renders at SH degree 3)
    pc = Model(s, hh.dev())
    view = T(s.view).requires_grad_()
    res = slam.render(_Cam(s), pc, None, T(s.bg), viewmatrix=view, fov=(s.tanfovx, s.tanfovy), HW=(H, W), gt_depth=T(s.gt),
                      variant=variant, silhouette_grad=True, complete_pose=True)
    (res["opacity_map"] * T(gA.astype(np.float32)[None])).sum().backward()
    torch.cuda.synchronize()
    g = {n: t.grad.detach().cpu().numpy().astype(np.float64) for n, t in model_leaves(pc).items()}
    for leaf in ("means3D", "opacities", "scales", "rotations"):
        check(g[leaf], want[leaf], f"{variant} slam {leaf}")
    check(view16(view.grad.cpu().numpy()), want["view"], f"{variant} slam view")
