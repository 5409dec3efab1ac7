"""absgrad -- the absolute screen-space gradient of AbsGS (include/dgr_hip.h: dgr_*_backward*_absgrad) -- on the GPU.

The reference: the float64 forwards of tests/fp64_model.py (torch_light, torch_full: written from SURVEY.md Appendix A, not from
the kernels) in pairs mode -- the screen-space mean enters each tile as a leaf per (Gaussian, pixel), the Gaussian's value
repeated over the tile's pixels.  Autograd then gives every pixel's own contribution v_p(g) to dL/dmean2D; absgrad is
sum_p |v_p(g)| per component, times the ndc scale W/2, H/2.  The integer path (visibility, lists, last contributors) is the
oracle's, as there.
"""
import numpy as np
import pytest
import torch

import hip_helpers as hh
from dgr_amd import _capi
from dgr_amd import full as F
from dgr_amd import light as L
from fp64_model import CASES, absgrad_of_pairs, torch_full, torch_light
from hip_helpers import binding, set_lane_lists as lane_lists  # noqa: F401  (fixtures)
from util import make_scene

pytestmark = pytest.mark.gpu


def _thread_option(name, value):
    assert _capi.load().dgr_set_thread_option(name.encode(), int(value)) == 0, _capi.last_error()


def light_backward_abs(s, deg, out, grads, lean, absgrad=True):
    """the light backward through the ctypes / compiled `_C` mirror; lean: no median / variance gradient image (NULL)"""
    gC, gD, gM, gV = grads
    return hh.hip_backward_raw(s, deg, out, grads=(gC, gD, None if lean else gM, None if lean else gV), absgrad=absgrad)


def full_backward_abs(s, deg, out, grads, lean, absgrad=True):
    gC, gD, gU = grads
    return hh.hip_full_backward_raw(s, deg, out, grads=(gC, gD, None if lean else gU), absgrad=absgrad)



def check_against(a, b, radii, what):
    a = np.asarray(a, np.float64)
    scale = np.abs(b).max()
    assert scale > 0, what
    err = np.abs(a - b).max() / scale
    assert err <= 5e-5, f"{what}: absgrad differs from the float64 reference by {err:.2e} of the tensor's scale"
    assert np.all(a[:, 2] == 0) and np.all(a[radii == 0] == 0), what


@pytest.mark.parametrize("lists", [0, 1])
@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_light_absgrad_matches_fp64(oracle, lane_lists, case, lean, lists):
    P, W, H, deg, seed = case
    lane_lists(lists)
    s = make_scene(P, W, H, seed)
    grads = [np.asarray(g, np.float64) * (W * H) ** 0.5 for g in (s.gC, s.gD, s.gM, s.gV)]
    if lean:
        grads[2], grads[3] = np.zeros_like(grads[2]), np.zeros_like(grads[3])
    st, ref = oracle.light_forward(s.bg, s.means, None, s.opac, s.scales, s.rots, 1.0, None, s.view, s.gt, s.proj,
                                   s.tanfovx, s.tanfovy, H, W, s.shs, deg, s.campos)
    pairs = []
    loss, leaves, img = torch_light(s, deg, ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"),
                                    grads, pairs=pairs)
    loss.backward()
    want = absgrad_of_pairs(pairs, img["_idx"], P, W, H)
    out, d = hh.hip_forward(s, deg)
    assert np.array_equal(d["radii"], ref["radii"])
    g = light_backward_abs(s, deg, out, grads, lean)
    assert len(g) == 10 and tuple(g[9].shape) == (P, 3) and g[9].dtype == torch.float32
    check_against(g[9].cpu().numpy(), want, d["radii"], f"light lean={lean} lists={lists}")


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_full_absgrad_matches_fp64(oracle, case, lean):
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    grads = [np.asarray(g, np.float64) * (W * H) ** 0.5 for g in (s.gC, s.gD, s.gV)]
    if lean:
        grads[2] = np.zeros_like(grads[2])
    st, ref = oracle.full_forward(s.bg, s.means, None, s.opac, s.scales, s.rots, 1.0, None, s.view, s.gt, s.proj,
                                  s.tanfovx, s.tanfovy, H, W, s.shs, deg, s.campos)
    pairs = []
    loss, leaves, img = torch_full(s, deg, ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"),
                                   grads, pairs=pairs)
    loss.backward()
    idx = np.nonzero(ref["radii"] > 0)[0]
    want = absgrad_of_pairs(pairs, idx, P, W, H)
    out, d = hh.hip_full_forward(s, deg)
    assert np.array_equal(d["radii"], ref["radii"])
    g = full_backward_abs(s, deg, out, grads, lean)
    assert len(g) == 10 and tuple(g[9].shape) == (P, 3)
    check_against(g[9].cpu().numpy(), want, d["radii"], f"full lean={lean}")


# BASELINE configs 1-3 (config 2: the full variant)
BIG = [("light", 10000, 256, 256, 0), ("full", 100000, 640, 480, 3), ("light", 500000, 1920, 1080, 3)]


def _big_scene(P, W, H, seed=5):
    from dgr_amd.synth import make_scene as synth_scene
    return synth_scene(P, W, H, seed)


@pytest.mark.parametrize("alpha_mode", [0, 1])
@pytest.mark.parametrize("cfg", BIG, ids=["config1", "config2-full", "config3"])
def test_absgrad_invariants_at_baseline_sizes(cfg, alpha_mode):
    variant, P, W, H, deg = cfg
    s = _big_scene(P, W, H)
    _thread_option("alpha_mode", alpha_mode)
    try:
        if variant == "light":
            grads = (s.gC, s.gD, s.gM, s.gV)
            out, d = hh.hip_forward(s, deg)
            g0 = light_backward_abs(s, deg, out, grads, False, absgrad=False)
            g1 = light_backward_abs(s, deg, out, grads, False)
            out2, d2 = hh.hip_forward(s, deg)
            img = ("color", "depth", "depth_median", "depth_var", "opacity_map")
        else:
            grads = (s.gC, s.gD, s.gV)
            out, d = hh.hip_full_forward(s, deg)
            g0 = full_backward_abs(s, deg, out, grads, False, absgrad=False)
            g1 = full_backward_abs(s, deg, out, grads, False)
            out2, d2 = hh.hip_full_forward(s, deg)
            img = ("color", "depth", "uncertainty")
        torch.cuda.synchronize()
    finally:
        _thread_option("alpha_mode", -1)
    for k in img:  # (a forward before and after an absgrad backward)
        assert np.array_equal(d[k], d2[k]), k
    assert len(g0) == 9 and len(g1) == 10
    for i in range(9):
        if g0[i] is None:
            continue
        a, b = g0[i].double(), g1[i].double()
        scale = max(b.abs().max().item(), 1e-30)
        # (the same kernels' sums but for the extra pair of values: only the order of the float atomics differs)
        assert (a - b).abs().max().item() <= 1e-6 * scale, i
    ab, m2 = g1[9].double(), g1[0].double()
    scale = m2.abs().max().item()
    assert torch.isfinite(ab).all()
    assert (ab[:, :2] >= m2[:, :2].abs() - 1e-6 * scale).all()
    assert (ab[:, 2] == 0).all()
    radii = torch.as_tensor(d["radii"], device=ab.device)
    assert (ab[radii == 0] == 0).all()
    assert (ab[radii > 0, :2].sum(1) > 0).any()


def _rasterizer(s, deg, variant, map_off=False):
    T = hh.T
    if variant == "light":
        rs = L.GaussianRasterizationSettings(image_height=s.H, image_width=s.W, tanfovx=s.tanfovx, tanfovy=s.tanfovy,
                                             bg=T(s.bg), scale_modifier=1.0, viewmatrix=T(s.view), projmatrix=T(s.proj),
                                             sh_degree=deg, campos=T(s.campos), prefiltered=False, debug=False,
                                             perspec_matrix=T(s.persp), track_off=False, map_off=map_off)
        return L.GaussianRasterizer(rs)
    rs = F.GaussianRasterizationSettings(image_height=s.H, image_width=s.W, tanfovx=s.tanfovx, tanfovy=s.tanfovy,
                                         bg=T(s.bg), scale_modifier=1.0, viewmatrix=T(s.view), projmatrix=T(s.proj),
                                         sh_degree=deg, campos=T(s.campos), prefiltered=False, perspec_matrix=T(s.persp))
    return F.GaussianRasterizer(rs)


class _Step:
    """render -> L1 loss on colour and depth -> backward, through GaussianRasterizer.forward (every tensor it needs made up
    front: a step can be captured into a hipGraph)"""

    def __init__(self, s, deg, variant):
        self.r = _rasterizer(s, deg, variant)
        self.view, self.gt = hh.T(s.view), hh.T(s.gt)
        self.obs = 0.1 * self.gt[None]

    def __call__(self, leaves, abs_leaf):
        means3D, shs, opac, scales, rots = leaves
        means2D = torch.zeros_like(means3D, requires_grad=True)
        out = self.r(means3D, means2D, opac, shs=shs, scales=scales, rotations=rots, viewmatrix=self.view, gt_depth=self.gt,
                     means2D_abs=abs_leaf)
        color, depth = out[0], out[2]
        loss = (color - self.obs).abs().mean() + 0.5 * (depth - self.gt[None]).abs().mean()
        loss.backward()
        return means2D


def _step(s, deg, variant, leaves, abs_leaf):
    return _Step(s, deg, variant)(leaves, abs_leaf)


def _leaves(s):
    T = hh.T
    return [T(a).requires_grad_(True) for a in (s.means, s.shs, s.opac, s.scales, s.rots)]


@pytest.mark.parametrize("variant", ["light", "full"])
def test_module_absgrad_matches_the_backward_and_accumulates(variant):
    s = _big_scene(20000, 320, 240)
    leaves = _leaves(s)
    ab = torch.zeros((s.P, 3), device=hh.dev(), requires_grad=True)
    m2 = _step(s, 3, variant, leaves, ab)
    torch.cuda.synchronize()
    one = ab.grad.clone()
    assert (one[:, 2] == 0).all() and (one[:, :2] >= m2.grad[:, :2].abs() - 1e-6 * m2.grad.abs().max()).all()
    assert one.abs().sum() > 0
    _step(s, 3, variant, leaves, ab)  # a second backward into the same leaf: .grad accumulates
    torch.cuda.synchronize()
    assert torch.allclose(ab.grad, 2 * one, rtol=1e-5, atol=1e-6 * one.abs().max().item())
    # the default call path: no abs leaf, the same signed gradient
    m2b = _step(s, 3, variant, _leaves(s), None)
    torch.cuda.synchronize()
    assert torch.allclose(m2b.grad, m2.grad, rtol=0, atol=1e-6 * m2.grad.abs().max().item())


@pytest.mark.parametrize("variant", ["light", "full"])
def test_absgrad_step_replayed_from_a_hipgraph(variant, monkeypatch):
    monkeypatch.setenv("DGR_SYNC_MODE", "lazy")  # (a capturable forward: the status words are read lazily)
    s = _big_scene(20000, 320, 240)
    leaves = _leaves(s)
    ab = torch.zeros((s.P, 3), device=hh.dev(), requires_grad=True)

    run = _Step(s, 3, variant)

    def step():
        ab.grad = None
        for t in leaves:
            t.grad = None
        run(leaves, ab)
        return ab.grad, leaves[0].grad

    step()
    eager = [t.clone() for t in step()]
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
        for a, b in zip(res, eager):
            assert torch.allclose(a, b, rtol=0, atol=1e-6 * b.abs().max().item())
    L.check_captured_status()


def test_bindings_agree_on_absgrad():
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    pkg = os.path.join(root, "diff-gaussian-rasterization_amd")
    code = ("import sys; sys.path[:0] = %r\n"
            "import numpy as np, torch, hip_helpers as hh\n"
            "from dgr_amd.synth import make_scene\n"
            "from test_hip_absgrad import light_backward_abs, full_backward_abs\n"
            "s = make_scene(20000, 320, 240, 3)\n"
            "a = light_backward_abs(s, 3, hh.hip_forward(s, 3)[0], (s.gC, s.gD, s.gM, s.gV), False)[9]\n"
            "b = full_backward_abs(s, 3, hh.hip_full_forward(s, 3)[0], (s.gC, s.gD, s.gV), False)[9]\n"
            "np.save(sys.argv[1], np.concatenate([a.cpu().numpy(), b.cpu().numpy()]))\n") % ([root, pkg, here],)
    import tempfile
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for binding in ("compiled", "ctypes"):
            f = os.path.join(tmp, binding + ".npy")
            env = dict(os.environ, DGR_BINDING=binding)
            subprocess.run([sys.executable, "-c", code, f], env=env, check=True, timeout=300)
            res[binding] = np.load(f)
    a, b = res["compiled"], res["ctypes"]
    assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()


def test_device_refusals():
    s = _big_scene(2000, 64, 64)
    leaves = _leaves(s)
    ab = torch.zeros((s.P, 3), device=hh.dev(), requires_grad=True)
    r = _rasterizer(s, 3, "light", map_off=True)
    with pytest.raises(ValueError):
        r(leaves[0], torch.zeros_like(leaves[0]), leaves[2], shs=leaves[1], scales=leaves[3], rotations=leaves[4],
          viewmatrix=hh.T(s.view), gt_depth=hh.T(s.gt), means2D_abs=ab)
    out, d = hh.hip_forward(s, 3)
    grads = (s.gC, s.gD, s.gM, s.gV)
    with pytest.raises(RuntimeError, match="map_off"):
        hh.hip_backward_raw(s, 3, out, map_off=True, absgrad=True)
    _thread_option("deterministic_grads", 1)
    try:
        with pytest.raises(RuntimeError, match="deterministic"):
            light_backward_abs(s, 3, out, grads, False)
        fo, _ = hh.hip_full_forward(s, 3)
        with pytest.raises(RuntimeError, match="deterministic"):
            full_backward_abs(s, 3, fo, (s.gC, s.gD, s.gV), False)
    finally:
        _thread_option("deterministic_grads", -1)
    _thread_option("alpha_mode", 2)
    try:
        with pytest.raises(RuntimeError, match="alpha_mode"):
            light_backward_abs(s, 3, out, grads, False)
    finally:
        _thread_option("alpha_mode", -1)
    torch.cuda.synchronize()


def _close(a, b, tol=1e-6):
    a, b = (x.detach().double().cpu() for x in (a, b))
    d, scale = (a - b).abs().max().item(), b.abs().max().item()
    if d > tol * scale:
        print(f"max |a - b| = {d:.3e} of scale {scale:.3e}")
    return d <= tol * scale


@pytest.mark.parametrize("variant", ["light", "full"])
def test_batched_absgrad_matches_one_view_calls(binding, variant):
    from dgr_amd import batch as B
    from dgr_amd import batch_full as BF
    T, E = hh.T, hh.E
    V, deg = 4, 3
    ss = [make_scene(20000, 320, 200, 0, view_index=v) for v in range(V)]
    s = ss[0]
    views, projs, campos, gts = (T(np.stack([getattr(x, n) for x in ss])) for n in ("view", "proj", "campos", "gt"))
    gC = T(np.stack([x.gC for x in ss]))
    gD, gM, gV = (T(np.stack([getattr(x, n)[None] for x in ss])) for n in ("gD", "gM", "gV"))
    if variant == "light":
        out = B._forward_batch(T(s.bg), T(s.means), E(), T(s.opac), T(s.scales), T(s.rots), 1.0, E(), views, gts, projs,
                               s.tanfovx, s.tanfovy, s.H, s.W, T(s.shs), deg, campos, False)
        (R, color, depth, median, var, alpha, radii, geom, binning, img, _, _) = out
        g = B._backward_batch(T(s.bg), T(s.means), radii, E(), T(s.scales), T(s.rots), 1.0, E(), views, projs, s.tanfovx,
                              s.tanfovy, gC, gD, gM, gV, gts, T(s.shs), deg, campos, geom, binning, img, alpha, T(s.persp),
                              False, False, True, True, num_rendered=R, absgrad=True)
    else:
        out = BF._forward_batch(T(s.bg), T(s.means), E(), T(s.opac), T(s.scales), T(s.rots), 1.0, E(), views, gts, projs,
                                s.tanfovx, s.tanfovy, s.H, s.W, T(s.shs), deg, campos, False)
        (R, color, depth, unc, radii, geom, binning, img, _) = out
        g = BF._backward_batch(T(s.bg), T(s.means), radii, E(), T(s.scales), T(s.rots), 1.0, E(), views, projs, s.tanfovx,
                               s.tanfovy, gC, gD, gV, gts, T(s.shs), deg, campos, geom, binning, img, T(s.persp), True, True, R,
                               absgrad=True)
    assert len(g) == 10 and tuple(g[9].shape) == (V, s.P, 3)
    for v in range(V):
        x = ss[v]
        if variant == "light":
            one = (R[v], color[v], depth[v], median[v], var[v], alpha[v], radii[v], geom[v], binning[v], img[v], None, None)
            gv = light_backward_abs(x, deg, one, (x.gC, x.gD, x.gM, x.gV), False)
        else:
            one = (R[v], 0, color[v], depth[v], unc[v], radii[v], geom[v], binning[v], img[v])
            gv = full_backward_abs(x, deg, one, (x.gC, x.gD, x.gV), False)
        assert _close(g[9][v], gv[9]), v
        assert _close(g[0][v], gv[0]), v
        assert (g[9][v][radii[v] == 0] == 0).all() and (g[9][v][:, 2] == 0).all()


def test_a_null_view_pointer_leaves_that_views_buffer_untouched():
    """dgr_light_backward_batch_absgrad with view 1's pointer NULL: views 0, 2, 3 as the one-view calls, view 1's buffer (filled
    with a sentinel before) unchanged"""
    import ctypes as C
    from dgr_amd import batch as B
    T, E = hh.T, hh.E
    V, deg = 4, 3
    ss = [make_scene(20000, 320, 200, 0, view_index=v) for v in range(V)]
    s, dev = ss[0], hh.dev()
    views, projs, campos, gts = (T(np.stack([getattr(x, n) for x in ss])) for n in ("view", "proj", "campos", "gt"))
    out = B._forward_batch(T(s.bg), T(s.means), E(), T(s.opac), T(s.scales), T(s.rots), 1.0, E(), views, gts, projs, s.tanfovx,
                           s.tanfovy, s.H, s.W, T(s.shs), deg, campos, False)
    (R, color, depth, median, var, alpha, radii, geom, binning, img, _, _) = out
    gC = T(np.stack([x.gC for x in ss]))
    gD, gM, gV = (T(np.stack([getattr(x, n)[None] for x in ss])) for n in ("gD", "gM", "gV"))
    lib, P, M = _capi.load(), s.P, T(s.shs).size(1)
    f32 = dict(dtype=torch.float32, device=dev)
    arena = {k: torch.zeros(P, n, **f32) for k, n in (("op", 1), ("col", 3), ("m3", 3), ("sc", 3), ("rot", 4))}
    dsh = torch.zeros(P, M, 3, **f32)
    d2, dview = torch.empty((V, P, 3), **f32), torch.empty((V, 4, 4), **f32)
    nscr = (lib.dgr_light_backward_scratch_bytes_r(P, s.W, s.H, max(R)) + 255) // 256 * 256
    scratch = torch.empty((V, nscr), dtype=torch.uint8, device=dev)
    dabs = torch.full((V, P, 3), 7.0, **f32)
    persp, bg, means, shs, scales, rots = T(s.persp), T(s.bg), T(s.means), T(s.shs), T(s.scales), T(s.rots)
    w = (_capi.LightViewGrad * V)()
    for v in range(V):
        r = B._row
        x = w[v]
        x.geometry_buffer, x.binning_buffer, x.image_buffer = r(geom, v), r(binning, v), r(img, v)
        x.viewmatrix, x.projmatrix, x.cam_pos, x.perspec_matrix = r(views, v), r(projs, v), r(campos, v), persp.data_ptr()
        x.alphas, x.gt_depth, x.radii = r(alpha, v), r(gts, v), r(radii, v)
        x.dL_dpix, x.dL_dpix_depth, x.dL_dpix_median_depth, x.dL_dpix_depth_var = r(gC, v), r(gD, v), r(gM, v), r(gV, v)
        x.dL_dmean2D, x.dL_dview, x.scratch, x.scratch_bytes, x.num_rendered = r(d2, v), r(dview, v), r(scratch, v), nscr, R[v]
    ptrs = (C.c_void_p * V)(*(None if v == 1 else dabs[v].data_ptr() for v in range(V)))
    p = _capi.ptr
    rc = lib.dgr_light_backward_batch_absgrad(
        _capi.stream_handle(dev.index), V, w, P, deg, M, p(bg), s.W, s.H, p(means), p(shs), None, p(scales), 1.0, p(rots), None,
        s.tanfovx, s.tanfovy, p(arena["op"]), p(arena["col"]), p(arena["m3"]), None, p(dsh), p(arena["sc"]), p(arena["rot"]),
        0, 0, ptrs)
    assert rc == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert (dabs[1] == 7.0).all()
    for v in (0, 2, 3):
        x = ss[v]
        one = (R[v], color[v], depth[v], median[v], var[v], alpha[v], radii[v], geom[v], binning[v], img[v], None, None)
        gv = light_backward_abs(x, deg, one, (x.gC, x.gD, x.gM, x.gV), False)
        assert _close(dabs[v], gv[9]), v


class _Map:
    """the accessors of 3DGS's GaussianModel that slam.render() reads, as leaves"""

    def __init__(self, s):
        self.get_xyz, self.get_features, self.get_opacity, self.get_scaling, self.get_rotation = _leaves(s)
        self.active_sh_degree = 3


@pytest.mark.parametrize("variant", ["light", "full"])
def test_slam_renders_with_absgrad(variant):
    from dgr_amd import pose, slam
    V, H, W = 3, 200, 320
    ss = [make_scene(20000, W, H, 0, view_index=v) for v in range(V)]
    s, dev = ss[0], hh.dev()
    gt, bg = hh.T(s.gt), hh.T(s.bg)
    cams = [dict(viewmatrix=hh.T(x.view), fov=(x.tanfovx, x.tanfovy), HW=(H, W), gt_depth=gt) for x in ss]
    kw = dict(track_off=True) if variant == "light" else dict(variant="full")
    targets = [0.1 * gt[None]] * V

    def loss_fn(out, k):
        return (out["render"] - targets[k]).abs().mean() + 0.5 * (out["depth"] - gt[None]).abs().mean()

    # the module-level call per view: GaussianRasterizer(...)(..., means2D_abs=leaf), with the camera tensors slam derives
    # from the viewmatrix (dgr_amd.slam.render: the same operations) and, light, its track_off
    want = []
    for k, x in enumerate(ss):
        ab = torch.zeros((s.P, 3), device=dev, requires_grad=True)
        vm = hh.T(x.view)
        perspec = pose._perspec_cached(x.tanfovx, x.tanfovy, 0.01, 100.0, dev)
        cam = dict(image_height=H, image_width=W, tanfovx=x.tanfovx, tanfovy=x.tanfovy, bg=bg, scale_modifier=1.0, viewmatrix=vm,
                   projmatrix=pose._matmul_fixed_order(vm, perspec).contiguous(), sh_degree=3, campos=pose._campos(vm),
                   prefiltered=False, perspec_matrix=perspec)
        if variant == "light":
            r = L.GaussianRasterizer(L.GaussianRasterizationSettings(**cam, debug=False, track_off=True, map_off=False))
        else:
            r = F.GaussianRasterizer(F.GaussianRasterizationSettings(**cam))
        pc = _Map(s)
        out = r(pc.get_xyz, torch.zeros_like(pc.get_xyz, requires_grad=True), pc.get_opacity, shs=pc.get_features,
                scales=pc.get_scaling, rotations=pc.get_rotation, viewmatrix=vm, gt_depth=gt, means2D_abs=ab)
        loss_fn({"render": out[0], "depth": out[2]}, k).backward()
        want.append(ab.grad)
    # slam.render, one view at a time
    for k, c in enumerate(cams):
        pc = _Map(s)
        o = slam.render(None, pc, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"], HW=c["HW"], gt_depth=gt, absgrad=True, **kw)
        loss_fn(o, k).backward()
        assert _close(o["viewspace_points_abs"].grad, want[k]), k
        o2 = slam.render(None, pc, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"], HW=c["HW"], gt_depth=gt, **kw)
        assert "viewspace_points_abs" not in o2
    # render_views / render_batch_fused: one batched call
    pc = _Map(s)
    losses, out = slam.render_batch_fused(cams, pc, None, bg, loss_fn, absgrad=True, **kw)
    assert out["viewspace_points_abs"].shape == (V, s.P, 3)
    for k in range(V):
        assert _close(out["viewspace_points_abs"].grad[k], want[k]), k
    out2 = slam.render_views(cams, _Map(s), None, bg, **kw)
    assert "viewspace_points_abs" not in out2 and "viewspace_points_abs" not in slam._ViewOf(out2, 0)
    # render_batch: every view's dict as render()'s
    seen = {}

    def keep(out, k):
        seen[k] = out["viewspace_points_abs"]
        return loss_fn(out, k)
    slam.render_batch(cams, _Map(s), None, bg, keep, absgrad=True, **kw)
    torch.cuda.synchronize()
    for k in range(V):
        assert _close(seen[k].grad, want[k]), k


@pytest.mark.parametrize("variant", ["light", "full"])
def test_batch_rasterizer_classes_with_means2D_abs(variant):
    """GaussianRasterizerBatch / GaussianRasterizerBatchFull(..., means2D_abs=[V,P,3] leaf) against one-view modules"""
    from dgr_amd import batch as B
    from dgr_amd import batch_full as BF
    T = hh.T
    V, H, W = 3, 200, 320
    ss = [make_scene(20000, W, H, 0, view_index=v) for v in range(V)]
    s = ss[0]
    views, projs, campos, gts = (T(np.stack([getattr(x, n) for x in ss])) for n in ("view", "proj", "campos", "gt"))
    rs = B.BatchRasterizationSettings(image_height=H, image_width=W, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=T(s.bg),
                                      scale_modifier=1.0, viewmatrices=views, projmatrices=projs, sh_degree=3, campos=campos,
                                      prefiltered=False, debug=False, perspec_matrix=T(s.persp), track_off=False, map_off=False)
    cls = B.GaussianRasterizerBatch if variant == "light" else BF.GaussianRasterizerBatchFull
    lv = _leaves(s)
    ab = torch.zeros((V, s.P, 3), device=hh.dev(), requires_grad=True)
    out = cls(rs)(lv[0], torch.zeros((V, s.P, 3), device=hh.dev(), requires_grad=True), lv[2], shs=lv[1], scales=lv[3],
                  rotations=lv[4], viewmatrices=views, gt_depths=gts, means2D_abs=ab)
    obs = 0.1 * gts[:, None]
    ((out[0] - obs).abs().mean(dim=(1, 2, 3)).sum() + 0.5 * (out[2] - gts[:, None]).abs().mean(dim=(1, 2, 3)).sum()).backward()
    for k, x in enumerate(ss):
        one = torch.zeros((s.P, 3), device=hh.dev(), requires_grad=True)
        lk = _leaves(s)
        o = _rasterizer(x, 3, variant)(lk[0], torch.zeros_like(lk[0], requires_grad=True), lk[2], shs=lk[1], scales=lk[3],
                                       rotations=lk[4], viewmatrix=T(x.view), gt_depth=T(x.gt), means2D_abs=one)
        ((o[0] - 0.1 * T(x.gt)[None]).abs().mean() + 0.5 * (o[2] - T(x.gt)[None]).abs().mean()).backward()
        assert _close(ab.grad[k], one.grad), k
