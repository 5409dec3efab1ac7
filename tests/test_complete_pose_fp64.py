"""The complete pose gradient (option "pose_grad" = 1, include/dgr_hip.h) in float64, on the CPU: fp64_model.complete_forward
against the oracle's images and reference pose gradient, the translation identity and central differences (every detached
quantity / decision frozen at the unperturbed view, `frozen`); and the option's host state."""
import numpy as np
import pytest
import torch

from cameras import CAMERA_CASES, assert_placement_edge, camera_case_id, camera_case_scene
from fp64_model import CASES, complete_forward, complete_grad, oracle_run, orthonormal_view, scaled_grads
from util import make_scene

WRITTEN = [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]  # the view entries a pose gradient writes (3, 7, 11, 15 stay 0)
IMG_TOL = {"color": 2e-6, "depth": 1e-5, "opacity_map": 2e-6, "uncertainty": 2e-6}


@pytest.mark.parametrize("variant", ["light", "full"])
@pytest.mark.parametrize("case", CASES)
def test_complete_formulation_images_and_reference_split(oracle, case, variant):
    """(1) the one-leaf formulation renders the oracle's images; (2) light: with the added paths detached its dL/dview is the
    oracle's reference pose gradient, so the complete gradient differs from it by exactly the added branches."""
    P, W, H, deg, seed = case
    check_formulation_and_reference_split(oracle, make_scene(P, W, H, seed), deg, variant)


@pytest.mark.parametrize("variant", ["light", "full"])
@pytest.mark.parametrize("case", CAMERA_CASES, ids=camera_case_id)
def test_complete_formulation_and_reference_split_at_cameras(oracle, case, variant):
    """As above at the cameras of tests/cameras.py: off-centre (the reference split then needs the reference's shortened ndc
    Jacobian), fx != fy, the Jacobian clamp, the near plane."""
    s, deg, info = camera_case_scene(case)
    ref = check_formulation_and_reference_split(oracle, s, deg, variant, img_tol=2.0)
    assert_placement_edge(oracle, case[1], s, info, ref["radii"])


def check_formulation_and_reference_split(oracle, s, deg, variant, img_tol=1.0):
    grads = scaled_grads(s, variant)
    st, ref, g = oracle_run(oracle, s, variant, deg, grads)
    gv, _, _, img = complete_grad(s, variant, deg, st, ref, grads)
    for k, v in img.items():
        d = np.abs(v.reshape(-1) - ref[k].astype(np.float64).reshape(-1))
        assert d.max() <= IMG_TOL[k] * img_tol, f"{k}: float64 forward differs from the oracle by {d.max():.2e}"
    assert np.abs(gv).max() > 0
    if variant == "light":
        gr, _, _, _ = complete_grad(s, variant, deg, st, ref, grads, added=False)
        want = np.asarray(g["dL_dview"], np.float64).reshape(-1)
        err = np.abs(gr - want).max() / np.abs(want).max()
        assert err <= 5e-5, f"reference split: {err:.2e} of scale"
        # (and the added branches are not negligible here: the complete gradient is a different vector)
        assert np.abs(gv - gr).max() >= 1e-3 * np.abs(gv).max()
    return ref


@pytest.mark.parametrize("variant", ["light", "full"])
@pytest.mark.parametrize("case", CASES[:2])
def test_complete_translation_identity(oracle, case, variant):
    """(3) for a rigid (orthonormal) view dL/dt = Rcam sum_g dL/dmeans3D[g]: the complete gradient is the means' counterpart."""
    P, W, H, deg, seed = case
    check_translation_identity(oracle, make_scene(P, W, H, seed), deg, variant)


@pytest.mark.parametrize("variant", ["light", "full"])
@pytest.mark.parametrize("case", CAMERA_CASES, ids=camera_case_id)
def test_complete_translation_identity_at_cameras(oracle, case, variant):
    """(3) at the cameras of tests/cameras.py: dL_dmeans3D goes through the full projection, so must the complete pose."""
    s, deg, _ = camera_case_scene(case)
    check_translation_identity(oracle, s, deg, variant)


def check_translation_identity(oracle, s, deg, variant):
    grads = scaled_grads(s, variant)
    st, ref, _ = oracle_run(oracle, s, variant, deg, grads)
    V = orthonormal_view(s.view)
    gv, gm, _, _ = complete_grad(s, variant, deg, st, ref, grads, view=V)
    Rc = V[:3, :3].t().numpy()
    lhs = Rc @ gm.sum(0)
    rhs = gv[12:15]
    assert np.abs(lhs - rhs).max() <= 1e-9 * np.abs(rhs).max(), (lhs, rhs)


@pytest.mark.parametrize("variant", ["light", "full"])
def test_complete_gradient_matches_central_differences(oracle, variant):
    """(4) central differences of the loss over the 12 written view entries, every decision and detached value frozen at the
    unperturbed view, agree with autograd's dL/dview."""
    P, W, H, deg, seed = CASES[0]
    check_central_differences(oracle, make_scene(P, W, H, seed), deg, variant)


@pytest.mark.parametrize("variant", ["light", "full"])
@pytest.mark.parametrize("case", [CAMERA_CASES[1], CAMERA_CASES[2]], ids=camera_case_id)
def test_complete_gradient_matches_central_differences_at_cameras(oracle, case, variant):
    """(4) at an off-centre camera with fx != fy, and with Gaussians beyond the Jacobian clamp."""
    s, deg, _ = camera_case_scene(case)
    check_central_differences(oracle, s, deg, variant)


def check_central_differences(oracle, s, deg, variant):
    grads = scaled_grads(s, variant)
    st, ref, _ = oracle_run(oracle, s, variant, deg, grads)
    args = (s, variant, deg, ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"), grads)
    V0 = torch.tensor(np.asarray(s.view, np.float64))
    loss, leaves, _, fr = complete_forward(*args, view=V0)
    loss.backward()
    ga = leaves["view"].grad.numpy().reshape(-1)
    h = 1e-6
    fd = np.zeros(16)
    with torch.no_grad():
        for i in WRITTEN:
            e = torch.zeros(16, dtype=torch.float64)
            e[i] = h
            lp = complete_forward(*args, view=V0 + e.reshape(4, 4), frozen=fr)[0].item()
            lm = complete_forward(*args, view=V0 - e.reshape(4, 4), frozen=fr)[0].item()
            fd[i] = (lp - lm) / (2 * h)
    scale = np.abs(ga[WRITTEN]).max()
    err = np.abs(fd[WRITTEN] - ga[WRITTEN]).max() / scale
    assert err <= 1e-6, f"finite differences vs autograd: {err:.2e} of scale"


def test_pose_grad_option_round_trip_and_refusal():
    """dgr_set_option / dgr_set_thread_option "pose_grad" and its field (bits 12-15) of the options word -- host state only."""
    from dgr_amd import _capi
    lib = _capi.load()
    assert lib.dgr_get_option(b"pose_grad") == 0 and lib.dgr_get_thread_option(b"pose_grad") == 0
    assert lib.dgr_set_option(b"pose_grad", 1) == 0 and lib.dgr_get_option(b"pose_grad") == 1
    assert lib.dgr_get_thread_option(b"pose_grad") == 1
    assert lib.dgr_set_option(b"pose_grad", 0) == 0 and lib.dgr_get_option(b"pose_grad") == 0
    assert lib.dgr_set_option(b"pose_grad", 2) == _capi.DGR_ERR_BAD_ARGUMENT and b"pose_grad" in lib.dgr_last_error()
    assert lib.dgr_get_option(b"pose_grad") == 0
    with pytest.raises(ValueError):
        _capi.set_option("pose_grad", 2)
    assert lib.dgr_set_thread_option(b"pose_grad", 2) == _capi.DGR_ERR_BAD_ARGUMENT
    assert (lib.dgr_thread_options_effective() >> 12) & 15 == 1       # effective 0 -> field 1
    with _capi.thread_options(pose_grad=1):
        assert lib.dgr_get_thread_option(b"pose_grad") == 1 and lib.dgr_get_option(b"pose_grad") == 0
        word = lib.dgr_thread_options_effective()
        assert (word >> 12) & 15 == 2 and (word & 0xfff) == (lib.dgr_thread_options_effective() & 0xfff)
    assert lib.dgr_get_thread_option(b"pose_grad") == 0
    prev = lib.dgr_thread_options_swap(word)                            # a forward's snapshot installed around a backward
    assert lib.dgr_get_thread_option(b"pose_grad") == 1
    lib.dgr_thread_options_swap(prev)
    assert lib.dgr_get_thread_option(b"pose_grad") == 0
    with pytest.raises(ValueError):
        with _capi.thread_options(pose_grad=2):
            pass
    assert lib.dgr_get_thread_option(b"pose_grad") == 0
