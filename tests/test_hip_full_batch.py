"""The full variant's batched multi-view entry points (dgr_full_forward_batch / dgr_full_backward_batch, dgr_amd.batch_full):
V cameras over one set of Gaussians per call.

What is pinned (the counterpart of tests/test_hip_batch.py for the -full variant):
  * every view's colour, depth, uncertainty, radii, num_related and forward state are BIT-IDENTICAL to a one-view
    dgr_amd.full call, and the views are checked against the oracle directly with the bars of tests/test_hip_full_parity.py;
  * the Gaussians' gradients are the sum over the views: against the sum of the oracle's per-view full backward passes, and
    against the one-view HIP backward accumulated in view order to 1e-5 of each tensor's scale; pose gradients and
    dL_dmeans2D stay per view;
  * the lean blend backward (uncertainty not in the loss) equals an all-zero uncertainty gradient bit for bit, deterministic
    gradients repeat bit for bit, a captured batch replays, bad view counts are refused and an empty scene gives zeros;
  * slam.render_views(variant="full") + one backward equals V one-view slam.render(variant="full") calls.
"""
import os

import numpy as np
import pytest
import torch

from util import assert_grad_close, make_scene
import hip_helpers as hh
from hip_helpers import binding  # noqa: F401  (fixture)
from dgr_amd import _capi
from dgr_amd import batch_full as BF
from dgr_amd import light as L

pytestmark = pytest.mark.gpu
T, E = hh.T, hh.E


@pytest.fixture(autouse=True)
def batch_binding(binding):
    """every test runs over the compiled torch extension (csrc/torch_ext.cpp: full_forward_batch / full_backward_batch) and
    over the ctypes binding of the same C ABI"""
    assert (BF._ext() is not None) == (binding == "compiled")


def close(a, b, tol=1e-5):
    """max |a - b| <= tol * max |b|: two runs of the blend backward add their float atomics in different orders"""
    a, b = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    return float(np.abs(a.astype(np.float64) - b).max()) <= tol * float(np.abs(b).max()) + 1e-30


def scenes(P, W, H, V, seed=0):
    return [make_scene(P, W, H, seed, view_index=v) for v in range(V)]


def cams_of(ss):
    return tuple(T(np.stack([getattr(x, n) for x in ss])) for n in ("view", "proj", "campos", "gt"))


def batch_forward(ss, deg, colors_precomp=None, cov3D_precomp=None):
    s = ss[0]
    use_sh, use_sr = colors_precomp is None, cov3D_precomp is None
    views, projs, campos, gts = cams = cams_of(ss)
    out = BF._forward_batch(T(s.bg), T(s.means), E() if use_sh else T(colors_precomp), T(s.opac),
                            T(s.scales) if use_sr else E(), T(s.rots) if use_sr else E(), 1.0,
                            E() if use_sr else T(cov3D_precomp), views, gts, projs, s.tanfovx, s.tanfovy, s.H, s.W,
                            T(s.shs) if use_sh else E(), deg, campos, False)
    return out, cams


def batch_backward(ss, deg, out, cams, grads, colors_precomp=None, cov3D_precomp=None, lean=False):
    s = ss[0]
    use_sh, use_sr = colors_precomp is None, cov3D_precomp is None
    (R, color, depth, unc, radii, geom, binning, img, _) = out
    views, projs, campos, gts = cams
    gC = T(np.stack([g[0] for g in grads]))
    gD = T(np.stack([g[1][None] for g in grads]))
    gU = None if lean else T(np.stack([g[2][None] for g in grads]))
    g = BF._backward_batch(T(s.bg), T(s.means), radii, E() if use_sh else T(colors_precomp), T(s.scales) if use_sr else E(),
                           T(s.rots) if use_sr else E(), 1.0, E() if use_sr else T(cov3D_precomp), views, projs, s.tanfovx,
                           s.tanfovy, gC, gD, gU, gts, T(s.shs) if use_sh else E(), deg, campos, geom, binning, img,
                           T(s.persp), True, True, R)
    names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations",
             "dL_dview"]
    return {n: (None if v is None else v.cpu().numpy()) for n, v in zip(names, g)}


def one_view(out, v):
    """the batch's outputs of view v in the shape of dgr_amd.full's `_C.rasterize_gaussians` tuple"""
    (R, color, depth, unc, radii, geom, binning, img, status) = out
    return (R[v], int(status[v, 3]), color[v], depth[v], unc[v], radii[v], geom[v], binning[v], img[v])


def grads_of(ss):
    return [tuple(x * (s.W * s.H) ** 0.5 for x in (s.gC, s.gD, s.gV)) for s in ss]


def cov3D_of(s):
    return hh.hip_cov3D(s)


FWD_CASES = [(2000, 64, 48, 0, 1, 1), (2000, 70, 45, 3, 2, 3), (10000, 256, 256, 0, 0, 8), (10000, 256, 256, 3, 0, 3),
             (100000, 640, 480, 3, 0, 4)]


@pytest.mark.parametrize("case", FWD_CASES)
def test_every_view_is_bit_identical_to_a_one_view_call_and_matches_the_oracle(oracle, case):
    P, W, H, deg, seed, V = case
    ss = scenes(P, W, H, V, seed)
    out, _ = batch_forward(ss, deg)
    for v, s in enumerate(ss):
        one, d1 = hh.hip_full_forward(s, deg)
        ov = one_view(out, v)
        assert ov[0] == one[0] and ov[1] == one[1], v
        for k, name in ((2, "color"), (3, "depth"), (4, "uncertainty"), (5, "radii")):
            assert torch.equal(ov[k], one[k]), (v, name)
        dv = {"num_rendered": ov[0], "geom": ov[6], "binning": ov[7], "img": ov[8]}
        for name in ("point_list", "n_contrib", "n_valid", "final_T"):
            assert np.array_equal(hh.hip_state(name, s, dv).view(np.uint8), hh.hip_state(name, s, d1).view(np.uint8)), (v, name)
        # against the oracle directly (tests/test_hip_full_parity.py: test_full_forward)
        st, ref, _ = hh.oracle_full(oracle, s, deg, backward=False)
        d = {"color": ov[2].cpu().numpy(), "depth": ov[3].cpu().numpy(), "uncertainty": ov[4].cpu().numpy()}
        assert np.array_equal(ov[5].cpu().numpy(), ref["radii"]) and ov[0] == ref["num_rendered"]
        assert np.array_equal(hh.hip_state("point_list", s, dv), st.get("point_list"))
        assert np.array_equal(d["uncertainty"], ref["uncertainty"])
        for k in ("color", "depth"):
            a, b = d[k].astype(np.float64), ref[k].astype(np.float64)
            assert np.all(np.abs(a - b) <= 1e-6 * np.maximum(1.0, np.abs(b))), (v, k)
        assert np.array_equal(hh.hip_state("n_contrib", s, dv), st.get("n_contrib"))
        assert np.array_equal(hh.hip_state("n_valid", s, dv), st.get("n_valid_contrib"))
        assert ov[1] == ref["num_related"]
        assert np.array_equal(hh.hip_state("final_T", s, dv).view(np.float32), st.get("final_T"))


@pytest.mark.parametrize("inputs", ["colors_precomp", "cov3D_precomp", "both"])
def test_precomputed_colours_and_covariances(inputs):
    P, W, H, deg, V = 5000, 160, 96, 3, 3
    ss = scenes(P, W, H, V, 5)
    colors = np.random.default_rng(7).uniform(0, 1, (P, 3)).astype(np.float32) if inputs != "cov3D_precomp" else None
    cov = cov3D_of(ss[0]) if inputs != "colors_precomp" else None
    out, cams = batch_forward(ss, deg, colors_precomp=colors, cov3D_precomp=cov)
    grads = grads_of(ss)
    g = batch_backward(ss, deg, out, cams, grads, colors_precomp=colors, cov3D_precomp=cov)
    acc = None
    for v, s in enumerate(ss):
        one, _ = hh.hip_full_forward(s, deg, colors_precomp=colors, cov3D_precomp=cov)
        ov = one_view(out, v)
        assert ov[0] == one[0] and ov[1] == one[1]
        for k in (2, 3, 4, 5):
            assert torch.equal(ov[k], one[k]), (v, k)
        g1 = hh.hip_full_backward(s, deg, ov, colors_precomp=colors, cov3D_precomp=cov, grads=grads[v])
        assert close(g["dL_dview"][v], g1["dL_dview"]) and close(g["dL_dmeans2D"][v], g1["dL_dmeans2D"]), v
        acc = {k: g1[k].copy() for k in g1} if acc is None else {k: acc[k] + g1[k] for k in g1}
    keys = ["dL_dmeans3D", "dL_dopacity", "dL_dcov3D"]
    keys += ["dL_dcolors"] if colors is not None else ["dL_dsh"]
    keys += ["dL_dscales", "dL_drotations"] if cov is None else []
    for k in keys:
        assert close(g[k], acc[k]), k


@pytest.mark.parametrize("case", [(2000, 70, 45, 3, 2, 3), (10000, 256, 256, 3, 0, 8), (100000, 640, 480, 3, 0, 4)])
def test_summed_gradients_against_the_oracle_and_the_one_view_backward(oracle, case):
    P, W, H, deg, seed, V = case
    ss = scenes(P, W, H, V, seed)
    grads = grads_of(ss)
    out, cams = batch_forward(ss, deg)
    g = batch_backward(ss, deg, out, cams, grads)
    acc, ref_sum = None, None
    tol = dict(rel_to_max=1e-5, elem_rtol=2e-3, elem_frac=1e-3)  # tests/test_hip_full_parity.py: test_full_backward
    for v, s in enumerate(ss):
        ov = one_view(out, v)
        # (the one-view backward on the state buffers the BATCHED forward left: they are interchangeable)
        g1 = hh.hip_full_backward(s, deg, ov, grads=grads[v])
        assert close(g["dL_dmeans2D"][v], g1["dL_dmeans2D"]), v
        assert close(g["dL_dview"][v], g1["dL_dview"]), v
        acc = {k: g1[k].copy() for k in g1} if acc is None else {k: acc[k] + g1[k] for k in g1}  # view order, float32
        st, ref, gr = hh.oracle_full(oracle, s, deg, grads=grads[v])
        dv = {"num_rendered": ov[0], "geom": ov[6], "binning": ov[7], "img": ov[8]}
        assert np.array_equal(hh.hip_state("n_contrib", s, dv), st.get("n_contrib"))
        assert_grad_close(g["dL_dmeans2D"][v], gr["dL_dmeans2D"], f"dL_dmeans2D[{v}]", **tol)
        assert_grad_close(g["dL_dview"][v], gr["dL_dview"], f"dL_dview[{v}]", rel_to_max=tol["rel_to_max"] * 5, elem_rtol=5e-3,
                          elem_frac=0.1)
        ref_sum = {k: gr[k].astype(np.float64) for k in gr} if ref_sum is None else {k: ref_sum[k] + gr[k] for k in gr}
    for k in ("dL_dmeans3D", "dL_dsh", "dL_dopacity", "dL_dcov3D", "dL_dscales", "dL_drotations"):
        assert close(g[k], acc[k]), k
    for k in ("dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"):
        assert_grad_close(g[k], ref_sum[k].reshape(g[k].shape), k, **tol)


def test_lean_backward_and_deterministic_gradients_repeat_bit_for_bit():
    """With deterministic_grads every sum has a fixed order: two runs give the same bits, and leaving the uncertainty out of the
    loss (NULL: the lean blend backward) gives the bits of an all-zero uncertainty gradient image."""
    P, W, H, deg, V = 20000, 320, 200, 3, 3
    ss = scenes(P, W, H, V, 0)
    grads = [(gc, gd, np.zeros_like(gu)) for gc, gd, gu in grads_of(ss)]
    with _capi.thread_options(deterministic_grads=1):
        out, cams = batch_forward(ss, deg)
        a = batch_backward(ss, deg, out, cams, grads)
        b = batch_backward(ss, deg, out, cams, grads)
        lean = batch_backward(ss, deg, out, cams, grads, lean=True)
        full_grads = grads_of(ss)
        c = batch_backward(ss, deg, out, cams, full_grads)
        d = batch_backward(ss, deg, out, cams, full_grads)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], lean[k]), k
        assert np.array_equal(c[k], d[k]), k
    # ... and the deterministic sums are the float-atomic ones up to their order
    g = batch_backward(ss, deg, out, cams, full_grads)
    for k in ("dL_dmeans3D", "dL_dsh", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans2D"):
        assert close(g[k], c[k]), k
    assert close(g["dL_dview"], c["dL_dview"])


def test_a_captured_batch_replays():
    P, W, H, deg, V = 20000, 320, 200, 3, 4
    ss = scenes(P, W, H, V, 0)
    s = ss[0]
    views, projs, campos, gts = cams_of(ss)
    means, shs, opac, scales, rots = (T(a) for a in (s.means, s.shs, s.opac, s.scales, s.rots))
    gr = grads_of(ss)
    gC, gD, gU = (T(np.stack([g[i] if i == 0 else g[i][None] for g in gr])) for i in range(3))
    old = os.environ.get("DGR_SYNC_MODE")
    os.environ["DGR_SYNC_MODE"] = "lazy"
    try:
        bg, persp, e0 = T(s.bg), T(s.persp), E()

        def step():
            out = BF._forward_batch(bg, means, e0, opac, scales, rots, 1.0, e0, views, gts, projs, s.tanfovx, s.tanfovy, H, W,
                                    shs, deg, campos, False)
            g = BF._backward_batch(bg, means, out[4], e0, scales, rots, 1.0, e0, views, projs, s.tanfovx, s.tanfovy, gC, gD, gU,
                                   gts, shs, deg, campos, out[5], out[6], out[7], persp, True, True, out[0])
            return out[1], out[3], g[3], g[8]
        step()  # (learns the capacity)
        L.check_async_errors()
        eager = [t.clone() for t in step()]  # (lazy: the capacity the replay will use; creates the internal streams)
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
            for t in res:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(res[0], eager[0]) and torch.equal(res[1], eager[1])
            assert close(res[2], eager[2]) and close(res[3], eager[3])
        L.check_captured_status()
    finally:
        if old is None:
            os.environ.pop("DGR_SYNC_MODE", None)
        else:
            os.environ["DGR_SYNC_MODE"] = old


def test_bad_view_counts_are_refused_and_an_empty_scene_gives_zeros():
    ss = scenes(100, 64, 48, 9, 0)
    with pytest.raises(RuntimeError, match="views per batch"):
        batch_forward(ss, 3)
    s = ss[0]
    empty = lambda *shape: torch.empty(shape, device=hh.dev())  # noqa: E731
    with pytest.raises(RuntimeError, match="views per batch"):  # V = 0
        BF._forward_batch(T(s.bg), T(s.means), E(), T(s.opac), T(s.scales), T(s.rots), 1.0, E(), empty(0, 4, 4),
                          empty(0, 48, 64), empty(0, 4, 4), s.tanfovx, s.tanfovy, 48, 64, T(s.shs), 3, empty(0, 3), False)
    ss = scenes(0, 64, 48, 2, 0)
    out, cams = batch_forward(ss, 3)
    assert out[0] == [0, 0]
    for k in (1, 2, 3):
        assert float(out[k].abs().max()) == 0.0
    grads = [(np.ones((3, 48, 64), np.float32), np.ones((48, 64), np.float32), np.ones((48, 64), np.float32))] * 2
    g = batch_backward(ss, 3, out, cams, grads)
    assert g["dL_dview"].shape == (2, 4, 4) and not g["dL_dview"].any()


class Model:
    """the accessors of 3DGS's GaussianModel that slam.render() reads, as leaves"""

    def __init__(self, s, dev):
        for name, a in (("get_xyz", s.means), ("get_opacity", s.opac), ("get_scaling", s.scales), ("get_rotation", s.rots),
                        ("get_features", s.shs)):
            setattr(self, name, T(a).clone().requires_grad_())
        self.active_sh_degree = 3


def test_render_views_full_equals_the_one_view_renders_accumulated():
    from dgr_amd import slam
    dev = hh.dev()
    P, W, H, V = 20000, 256, 192, 4
    ss = scenes(P, W, H, V, 3)
    s = ss[0]
    bg, gt = T(s.bg), T(s.gt)
    w = [torch.randn((V, c, H, W), device=dev) / (H * W) ** 0.5 for c in (3, 1, 1)]

    def cams():
        return [dict(viewmatrix=T(x.view).requires_grad_(), fov=(x.tanfovx, x.tanfovy), HW=(H, W), gt_depth=gt) for x in ss]

    a, ca = Model(s, dev), cams()
    one = []
    for k, c in enumerate(ca):
        o = slam.render(None, a, None, bg, viewmatrix=c["viewmatrix"], fov=c["fov"], HW=c["HW"], gt_depth=gt, variant="full")
        ((o["render"] * w[0][k]).sum() + (o["depth"] * w[1][k]).sum() + (o["opacity_map"] * w[2][k]).sum()).backward()
        one.append({n: o[n].detach() for n in ("render", "depth", "opacity_map", "radii")})
        one[-1]["pts"] = o["viewspace_points"].grad
    b, cb = Model(s, dev), cams()
    out = slam.render_views(cb, b, None, bg, variant="full")
    assert set(out) == {"render", "depth", "opacity_map", "viewspace_points", "visibility_filter", "radii"}
    assert out["render"].shape == (V, 3, H, W) and out["opacity_map"].shape == (V, 1, H, W) and out["radii"].shape == (V, P)
    ((out["render"] * w[0]).sum() + (out["depth"] * w[1]).sum() + (out["opacity_map"] * w[2]).sum()).backward()
    for k in range(V):
        for n in ("render", "depth", "opacity_map", "radii"):
            assert torch.equal(out[n][k], one[k][n]), (k, n)
        view = slam._ViewOf(out, k)
        assert set(view) == set(out) and torch.equal(view["render"], out["render"][k])
        assert close(out["viewspace_points"].grad[k], one[k]["pts"]), k
        assert close(cb[k]["viewmatrix"].grad, ca[k]["viewmatrix"].grad), k
    for n in ("get_xyz", "get_opacity", "get_scaling", "get_rotation", "get_features"):
        assert close(getattr(b, n).grad, getattr(a, n).grad), n
    from dgr_amd.multiview import GradientArena
    span = GradientArena([b.get_xyz, b.get_features, b.get_opacity, b.get_scaling, b.get_rotation]).fused_span()
    assert span is not None and span.numel() >= P * (3 + 3 + 48 + 1 + 3 + 4)
