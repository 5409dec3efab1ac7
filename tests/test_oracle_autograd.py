"""The oracle's backward math against the float64 formulation of tests/fp64_model.py (written from SURVEY.md Appendix A, not from
oracle/dgr_oracle.cpp, differentiated by autograd) on tiny scenes, both variants; the model's pairs mode against its ordinary
run; the rigid-camera identity."""
import numpy as np
import pytest
import torch

from cameras import CAMERA_CASES, assert_placement_edge, camera_case_id, camera_case_scene
from fp64_model import CASES, oracle_run, scaled_grads, torch_full, torch_light
from util import make_scene


@pytest.mark.parametrize("case", CASES)
def test_oracle_backward_equals_fp64_autograd(oracle, case):
    P, W, H, deg, seed = case
    check_light_against_fp64(oracle, make_scene(P, W, H, seed), deg)


@pytest.mark.parametrize("case", CAMERA_CASES, ids=camera_case_id)
def test_oracle_backward_equals_fp64_autograd_at_cameras(oracle, case):
    s, deg, info = camera_case_scene(case)
    ref = check_light_against_fp64(oracle, s, deg, img_tol=2.0)
    assert_placement_edge(oracle, case[1], s, info, ref["radii"])


def check_light_against_fp64(oracle, s, deg, img_tol=1.0):
    """`img_tol` scales the image bars (2: the camera cases, whose bands put up to ~70 more float32 terms into a pixel's sums)."""
    P, W, H = s.P, s.W, s.H
    grads = tuple(np.asarray(g, np.float64) * (W * H) ** 0.5 for g in (s.gC, s.gD, s.gM, s.gV))
    st, ref = oracle.light_forward(s.bg, s.means, None, s.opac, s.scales, s.rots, 1.0, None, s.view, s.gt, s.proj,
                                   s.tanfovx, s.tanfovy, H, W, s.shs, deg, s.campos)
    loss, leaves, img = torch_light(s, deg, ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"),
                                    grads)
    # same decisions: the float64 forward reproduces the oracle's float32 images to rounding
    for k, tol in (("color", 2e-6), ("depth", 1e-5), ("opacity_map", 2e-6)):
        d = np.abs(img[k].reshape(-1) - ref[k].astype(np.float64).reshape(-1))
        assert d.max() <= tol * img_tol, f"{k}: float64 forward differs from the oracle by {d.max():.2e}"
    loss.backward()
    g = oracle.light_backward(st, s.bg, s.means, None, s.scales, s.rots, 1.0, None, s.view, s.proj, s.tanfovx, s.tanfovy,
                              *(np.asarray(x, np.float32) for x in grads), s.gt, s.shs, deg, s.campos,
                              img["opacity_map"].astype(np.float32)[None], s.persp)
    pairs = dict(dL_dmeans3D=leaves["means3D"].grad, dL_dscales=leaves["scales"].grad, dL_drotations=leaves["rotations"].grad,
                 dL_dopacity=leaves["opacities"].grad, dL_dsh=leaves["shs"].grad,
                 dL_dview=leaves["view_ndc"].grad + leaves["view_depth"].grad)
    for k, t in pairs.items():
        a, b = np.asarray(g[k], np.float64).reshape(-1), t.numpy().reshape(-1)
        if k == "dL_dview":
            b = b.copy()
            b[[3, 7, 11, 15]] = 0.0  # never written by the reference (L/rasterize_points.cu:235)
        scale = np.abs(b).max()
        assert scale > 0, k
        err = np.abs(a - b).max() / scale
        # the oracle works in float32 (and forms T_final = 1 - alpha, a cancellation): measured 1e-6 .. 3e-5 of scale on
        # these scenes; a wrong term or sign in any component shows up at >= 1e-3
        assert err <= 5e-5, f"{k}: oracle vs float64 autograd differ by {err:.2e} of the tensor's scale"
    return ref


@pytest.mark.parametrize("case", CASES)
def test_oracle_full_backward_equals_fp64_autograd(oracle, case):
    """a12 / a16: the full variant's per-Gaussian gradients (uncertainty consumed as a variance) and its pose gradient
    (ComputePG part 1 + part 2-1, depth terms of the front-most valid Gaussian only) against the formulation above."""
    P, W, H, deg, seed = case
    check_full_against_fp64(oracle, make_scene(P, W, H, seed), deg)


@pytest.mark.parametrize("case", CAMERA_CASES, ids=camera_case_id)
def test_oracle_full_backward_equals_fp64_autograd_at_cameras(oracle, case):
    s, deg, info = camera_case_scene(case)
    check_full_against_fp64(oracle, s, deg, img_tol=2.0)


def check_full_against_fp64(oracle, s, deg, img_tol=1.0):
    P, W, H = s.P, s.W, s.H
    grads = tuple(np.asarray(g, np.float64) * (W * H) ** 0.5 for g in (s.gC, s.gD, s.gV))
    st, ref = oracle.full_forward(s.bg, s.means, None, s.opac, s.scales, s.rots, 1.0, None, s.view, s.gt, s.proj,
                                  s.tanfovx, s.tanfovy, H, W, s.shs, deg, s.campos)
    loss, leaves, img = torch_full(s, deg, ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"), grads)
    for k, tol in (("color", 2e-6), ("depth", 1e-5), ("uncertainty", 2e-6)):
        d = np.abs(img[k].reshape(-1) - ref[k].astype(np.float64).reshape(-1))
        assert d.max() <= tol * img_tol, f"{k}: float64 forward differs from the oracle by {d.max():.2e}"
    loss.backward()
    g = oracle.full_backward(st, s.bg, s.means, None, s.scales, s.rots, 1.0, None, s.view, s.gt, s.proj, s.tanfovx,
                             s.tanfovy, *(np.asarray(x, np.float32) for x in grads), s.shs, deg, s.campos, s.persp)
    pairs = dict(dL_dmeans3D=leaves["means3D"].grad, dL_dscales=leaves["scales"].grad, dL_drotations=leaves["rotations"].grad,
                 dL_dopacity=leaves["opacities"].grad, dL_dsh=leaves["shs"].grad,
                 dL_dview=sum(leaves[k].grad for k in ("view_ndc", "view_depth", "view_campos") if leaves[k].grad is not None))
    # (SH degree 0: the colour does not depend on the view direction, so nothing reaches view_campos)
    for k, t in pairs.items():
        a, b = np.asarray(g[k], np.float64).reshape(-1), t.numpy().reshape(-1)
        if k == "dL_dview":
            b = b.copy()
            b[[3, 7, 11, 15]] = 0.0  # never written by the reference (quirk F7)
        scale = np.abs(b).max()
        assert scale > 0, k
        err = np.abs(a - b).max() / scale
        assert err <= 5e-5, f"{k}: oracle vs float64 autograd differ by {err:.2e} of the tensor's scale"


def _pairs_scene(which):
    if which == "synth":
        P, W, H, deg, seed = CASES[0]
        return make_scene(P, W, H, seed), deg
    return camera_case_scene(CAMERA_CASES[1])[:2]


@pytest.mark.parametrize("variant", ["light", "full"])
@pytest.mark.parametrize("which", ["synth", camera_case_id(CAMERA_CASES[1])])
def test_pair_gradients_add_up_to_the_mean2D_gradient(oracle, which, variant):
    """Pairs mode (absgrad's reference, otherwise reached by GPU tests only): a Gaussian's per-pixel gradients v_p(g) add up to
    the ordinary run's dL/dmean2D (`_pix.grad`), within 1e-12 of that tensor's max -- a sum of at most 256 float64 terms per
    tile, 256 x 2.2e-16 = 6e-14, and a margin for the tiles a Gaussian touches."""
    s, deg = _pairs_scene(which)
    forward = torch_light if variant == "light" else torch_full
    grads = scaled_grads(s, variant)
    st, ref, _ = oracle_run(oracle, s, variant, deg, grads)
    decisions = (ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"))
    loss, _, img = forward(s, deg, *decisions, grads)
    loss.backward()
    want = img["_pix"].grad
    pairs = []
    loss_p, _, img_p = forward(s, deg, *decisions, grads, pairs=pairs)
    loss_p.backward()
    assert loss_p.item() == loss.item()
    for k in ("color", "depth"):
        assert np.array_equal(img_p[k], img[k]), k
    got = torch.zeros_like(want)
    for ids, leaf in pairs:
        if leaf.grad is not None:
            got.index_add_(0, ids, leaf.grad.sum(1))
    scale = want.abs().max().item()
    assert scale > 0
    err = (got - want).abs().max().item() / scale
    print(f"\n{which} {variant}: pair gradients vs dL/dmean2D: {err:.1e} of scale")
    assert err <= 1e-12, f"{which} {variant}: {err:.2e} of the tensor's scale"


def test_rigid_camera_identity(oracle):
    """for a rigid camera dL/dt = R sum_g dL_dmeans3D[g]; the light pose gradient omits the cov2D
    branch, so the identity holds to a few per cent in x and y (a convention check of view / proj / perspec)."""
    s = make_scene(3000, 96, 64, 7)
    N = s.W * s.H
    z = np.zeros((s.H, s.W), np.float32)
    st, ref = oracle.light_forward(s.bg, s.means, None, s.opac, s.scales, s.rots, 1.0, None, s.view, s.gt, s.proj,
                                   s.tanfovx, s.tanfovy, s.H, s.W, s.shs, 0, s.campos)
    g = oracle.light_backward(st, s.bg, s.means, None, s.scales, s.rots, 1.0, None, s.view, s.proj, s.tanfovx, s.tanfovy,
                              s.gC * N, s.gD * N, z, z, s.gt, s.shs, 0, s.campos, ref["opacity_map"], s.persp)
    Rm = s.view[:3, :3].T.astype(np.float64)  # view = W2C^T
    lhs = Rm @ g["dL_dmeans3D"].astype(np.float64).sum(0)
    rhs = g["dL_dview"].reshape(-1)[[12, 13, 14]].astype(np.float64)
    assert np.all(np.abs(lhs[:2] - rhs[:2]) <= 0.05 * np.abs(rhs[:2])), (lhs, rhs)
    assert np.sign(lhs[2]) == np.sign(rhs[2])