"""The kernels at general pinhole cameras (tests/cameras.py): off-centre principal points, fx != fy, wide and narrow fields of
view, a camera far from the world origin, Gaussians beyond the Jacobian clamp and at the near plane.  Every other GPU test sees
synth's one symmetric frustum, where a swapped focal / limit pair or a dropped off-diagonal perspec entry gives the right answer.

Outcome recorded here: the forward, the default backward, absgrad and the batched paths carried the oracle's bits / bars at every
camera and placement; the complete pose gradient (pose_grad = 1) left out the principal point (persp[8], persp[9]) of the ndc
rows and missed the float64 formulation at an off-centre camera -- fixed in bwd_view_terms (csrc/preprocess_bwd.hip)."""
import numpy as np
import pytest
import torch

import hip_helpers as hh
from cameras import (CAMERAS, CAMERA_CASES, CAMERA_IDS, PLACEMENTS, assert_clamp_edge, assert_near_edge, camera_case_id,
                     camera_case_scene, placed)
from fp64_model import absgrad_of_pairs, complete_grad, oracle_run, scaled_grads, torch_light
from test_hip_complete_pose import _identity_distance, hip_view_grad
from test_hip_light_parity import IMAGES, assert_images_carry_the_references_bits, check_backward
from test_hip_random_sweep import assert_full_images_carry_the_references_bits
from util import assert_grad_close, mask_flipped_pixels

pytestmark = pytest.mark.gpu

PAIRS = [(c, p) for c in CAMERA_IDS for p in PLACEMENTS]
SMALL_W, SMALL_P = 200, 8000


def small(cid, placement, seed=40):
    return placed(CAMERAS[cid].at(SMALL_W), SMALL_P, placement, seed)


def assert_edge(placement, s, info, ref):
    from oracle import oracle as O
    if placement == "clamp":
        assert_clamp_edge(s, info, ref["radii"])
    elif placement == "near":
        vis = O.mark_visible(s.means, s.view, s.proj)
        assert_near_edge(s, info, vis, ref["radii"])
        from dgr_amd import light as L
        got = L._C.mark_visible(hh.T(s.means), hh.T(s.view), hh.T(s.proj)).cpu().numpy().astype(bool)
        assert np.array_equal(got, vis)                                    # every Gaussian, the ulp group included
        assert np.array_equal(got[info["ulp"]], vis[info["ulp"]])


def far_pose_gradient(oracle, s, map_off, what):
    """dL_dview at the `far` camera, stage-isolated and end to end, at 2e-5 of scale for every entry.  The camera sits 36 units
    from the origin, so a rotation entry sums terms m_k ~ 30 times larger than itself: one of the 16 entries may miss
    check_backward's per-element 1e-3 relative bar by the order of the float atomics (far-clamp: -5.526 against -5.515 where
    the tensor's scale is > 500, 2e-5 of it), and is allowed to here."""
    grads = tuple(g * (s.W * s.H) ** 0.5 for g in (s.gC, s.gD, s.gM, s.gV))
    out, d = hh.hip_forward(s, 3)
    st, ref = hh.oracle_forward(oracle, s, 3)
    grads, _ = mask_flipped_pixels(grads, hh.hip_state("n_contrib", s, d), st.get("n_contrib"), s.W, s.H, what,
                                   images=[(d[k], ref[k]) for k in IMAGES],
                                   median_margin=oracle.light_median_margin(st, ref["opacity_map"]))
    gr = hh.oracle_backward(oracle, st, s, 3, ref["opacity_map"], map_off=map_off, grads=grads)
    for label, alphas in (("isolated", ref["opacity_map"]), ("end-to-end", None)):
        g = hh.hip_backward(s, 3, out, map_off=map_off, grads=grads, alphas=alphas)
        assert not g["dL_dview"].reshape(-1)[[3, 7, 11, 15]].any()
        assert_grad_close(g["dL_dview"], gr["dL_dview"], f"dL_dview [{label}]", rel_to_max=2e-5, elem_rtol=1e-3,
                          elem_frac=1 / 16)


@pytest.mark.parametrize("mode", ["default", "track_off", "map_off"])
@pytest.mark.parametrize("cid,placement", PAIRS, ids=[f"{c}-{p}" for c, p in PAIRS])
def test_light_at_camera(oracle, cid, placement, mode):
    """Integer path and threshold-carrying images bit for bit, the backward stage-isolated and end to end in all three modes, at
    test_hip_random_sweep.py's bars (2e-5 of scale: near-plane Gaussians of sigma up to 80 px put one frame's pose sum into a few
    large, cancelling terms -- measured 1.3e-5 on dL_dview at tum-near, the order of the float atomics).  At the `far` camera the
    pose gradient is compared by far_pose_gradient, every per-Gaussian gradient by check_backward as everywhere else."""
    s, info = small(cid, placement)
    far = cid == "far"
    d, st, ref = check_backward(oracle, s, 3, track_off=mode == "track_off" or far, map_off=mode == "map_off", rel_to_max=2e-5,
                                view_rel_to_max=2e-5, what=f"camera {cid} {placement} {mode}")
    if far and mode != "track_off":
        far_pose_gradient(oracle, s, mode == "map_off", f"camera {cid} {placement} {mode} pose")
    assert d["num_rendered"] == ref["num_rendered"] and np.array_equal(d["radii"], ref["radii"])
    assert np.array_equal(hh.hip_state("point_list", s, d), st.get("point_list"))
    assert np.array_equal(hh.hip_state("ranges", s, d), st.get("ranges"))
    assert_images_carry_the_references_bits(d, st, ref, s)
    if mode == "default":
        assert_edge(placement, s, info, ref)


@pytest.mark.parametrize("cid,placement", PAIRS, ids=[f"{c}-{p}" for c, p in PAIRS])
def test_full_at_camera(oracle, cid, placement):
    s, info = small(cid, placement, seed=41)
    npx = s.W * s.H
    grads = tuple(g * npx ** 0.5 for g in (s.gC, s.gD, s.gV))
    out, d = hh.hip_full_forward(s, 3)
    st, ref, _ = hh.oracle_full(oracle, s, 3, backward=False)
    assert np.array_equal(d["radii"], ref["radii"]) and d["num_rendered"] == ref["num_rendered"]
    assert np.array_equal(hh.hip_state("point_list", s, d), st.get("point_list"))
    assert_full_images_carry_the_references_bits(d, st, ref, s)
    assert_edge(placement, s, info, ref)
    grads, _ = mask_flipped_pixels(grads, hh.hip_state("n_contrib", s, d), st.get("n_contrib"), s.W, s.H,
                                   f"camera full {cid} {placement}", images=[(d[k], ref[k]) for k in ("color", "depth", "uncertainty")])
    g = hh.hip_full_backward(s, 3, out, grads=grads)
    gr = hh.oracle_full_backward(oracle, st, s, 3, grads=grads)
    for k in ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"):
        assert_grad_close(g[k], gr[k], k, rel_to_max=2e-5, elem_rtol=2e-3, elem_frac=2e-3, outlier_rows=0)
    assert_grad_close(g["dL_dview"], gr["dL_dview"], "dL_dview", rel_to_max=1e-5, elem_rtol=5e-3, elem_frac=0.1)


def test_full_size_tum_frame(oracle):
    """One TUM fr1 frame at its own size, 100 k Gaussians, with test_hip_random_sweep.py's bars."""
    s, _ = placed(CAMERAS["tum"], 100000, "plain", 42)
    d, st, ref = check_backward(oracle, s, 3, rel_to_max=2e-5, view_rel_to_max=2e-5, what="camera tum full size")
    assert d["num_rendered"] == ref["num_rendered"] and np.array_equal(d["radii"], ref["radii"])
    assert np.array_equal(hh.hip_state("point_list", s, d), st.get("point_list"))
    assert_images_carry_the_references_bits(d, st, ref, s)


# ------------------------------------------------------------------------------------------ the complete pose gradient
@pytest.mark.parametrize("mode", ["light", "light_map_off", "full"])
@pytest.mark.parametrize("case", CAMERA_CASES, ids=camera_case_id)
def test_complete_pose_at_camera_against_fp64(oracle, case, mode):
    """The complete pose gradient against the float64 complete formulation at 5e-5 of scale (skewed_pp-clamp: an off-centre
    principal point with Gaussians beyond the Jacobian clamp).  Before the fix the ndc rows read persp[0] and persp[5] only and
    missed at every off-centre camera."""
    s, deg, _ = camera_case_scene(case)
    variant = "full" if mode == "full" else "light"
    grads = scaled_grads(s, variant)
    st, ref, _ = oracle_run(oracle, s, variant, deg, grads)
    want, _, _, _ = complete_grad(s, variant, deg, st, ref, grads)
    scale = np.abs(want).max()
    got, _ = hip_view_grad(s, variant, deg, grads, map_off=mode == "light_map_off", pose_grad=1)
    err = np.abs(got - want).max() / scale
    assert err <= 5e-5, f"complete at {camera_case_id(case)}: {err:.2e} of scale"


@pytest.mark.parametrize("mode", ["light", "full"])
@pytest.mark.parametrize("cid", ["tum", "skewed_pp"])
def test_complete_translation_identity_at_size(cid, mode):
    s, _ = placed(CAMERAS[cid], 100000, "plain", 43)
    grads = (s.gC, s.gD, s.gM, s.gV) if mode == "light" else (s.gC, s.gD, s.gV)
    gv, g = hip_view_grad(s, mode, 3, grads, pose_grad=1)
    dist = _identity_distance(s, gv, g["dL_dmeans3D"])
    print(f"\n{cid} {mode}: |dL/dt - Rcam sum dL/dmeans3D| / |dL/dt| = {dist:.2e}")
    assert dist <= 2e-4, dist


def test_complete_pose_with_a_transposed_perspec_view():
    """Callers hold Proj^T as `projection.transpose(0, 1)`; the default mode reads its diagonal in place, the complete mode
    needs the off-diagonal entries where a contiguous Proj^T has them."""
    s, _ = small("skewed_pp", "plain", 44)
    grads = (s.gC, s.gD, s.gM, s.gV)
    ref_v, _ = hip_view_grad(s, "light", 3, grads, pose_grad=1)
    tp = s._replace(persp=np.ascontiguousarray(s.persp.T))  # storage = Proj; the tensor passed below is its transposed view
    from dgr_amd import _capi
    with _capi.thread_options(pose_grad=1):
        out, _ = hh.hip_forward(s, 3)
        g = hh.hip_backward_raw(s, 3, out, grads=grads, persp=hh.T(tp.persp).t())
    got = torch.sum(g[8], dim=0).cpu().numpy().astype(np.float64).reshape(-1)
    assert np.abs(got - ref_v).max() <= 2e-6 * np.abs(ref_v).max()


# ------------------------------------------------------------------------------------------ absgrad
@pytest.mark.parametrize("case", [CAMERA_CASES[1], CAMERA_CASES[2]], ids=camera_case_id)
def test_absgrad_at_camera(oracle, case):
    from test_hip_absgrad import check_against
    s, deg, _ = camera_case_scene(case)
    W, H, P = s.W, s.H, s.P
    grads = [np.asarray(g, np.float64) * (W * H) ** 0.5 for g in (s.gC, s.gD, s.gM, s.gV)]
    st, ref = oracle.light_forward(s.bg, s.means, None, s.opac, s.scales, s.rots, 1.0, None, s.view, s.gt, s.proj,
                                   s.tanfovx, s.tanfovy, H, W, s.shs, deg, s.campos)
    pairs = []
    loss, leaves, img = torch_light(s, deg, ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"),
                                    grads, pairs=pairs)
    loss.backward()
    want = absgrad_of_pairs(pairs, img["_idx"], P, W, H)
    out, d = hh.hip_forward(s, deg)
    assert np.array_equal(d["radii"], ref["radii"])
    g = hh.hip_backward_raw(s, deg, out, grads=grads, absgrad=True)
    check_against(g[9].cpu().numpy(), want, d["radii"], f"camera {camera_case_id(case)}")


# ------------------------------------------------------------------------------------------ batched entry points
def batch_views(V=4, seed=45):
    """V views of the skewed_pp sensor (one tan_fov) whose principal points and poses differ per view: every view's
    perspec_matrix is its own."""
    from cameras import rotation
    base = CAMERAS["skewed_pp"].at(SMALL_W)
    ss = []
    for v in range(V):
        cam = base.with_pp(base.cx - 9.0 * v, base.cy + 6.0 * v)._replace(R=rotation([0.3, 1.0, 0.2], 0.3 + 0.04 * v))
        ss.append(placed(cam, SMALL_P, "plain", seed)[0])
    # one set of Gaussians for the batch (the scene of view 0), each view's own camera and gradient images
    return [x._replace(means=ss[0].means, scales=ss[0].scales, rots=ss[0].rots, opac=ss[0].opac, shs=ss[0].shs) for x in ss]


@pytest.mark.parametrize("pose_grad", [0, 1])
@pytest.mark.parametrize("variant", ["light", "full"])
def test_batch_with_a_projection_per_view(variant, pose_grad):
    """Every view bit-identical to its one-view call, its pose gradient that of the one-view backward (which reads the view's
    own perspec_matrix; pose_grad = 1 reads its principal point), the Gaussians' gradients the serial sum."""
    from dgr_amd import _capi
    import test_hip_batch as TB
    import test_hip_full_batch as TF
    ss = batch_views()
    assert len({x.persp.tobytes() for x in ss}) == len(ss)
    persp = hh.T(np.stack([x.persp for x in ss]))
    with _capi.thread_options(pose_grad=pose_grad):
        if variant == "light":
            out, cams = TB.batch_forward(ss, 3)
            grads = [tuple(x * (s.W * s.H) ** 0.5 for x in (s.gC, s.gD, s.gM, s.gV)) for s in ss]
            (R, color, depth, median, var, alpha, radii, geom, binning, img, _, _) = out
            views, projs, campos, gts = cams
            gC = hh.T(np.stack([g[0] for g in grads]))
            gD, gM, gV = (hh.T(np.stack([g[i][None] for g in grads])) for i in (1, 2, 3))
            from dgr_amd import batch as B
            gb = B._backward_batch(hh.T(ss[0].bg), hh.T(ss[0].means), radii, hh.E(), hh.T(ss[0].scales), hh.T(ss[0].rots), 1.0,
                                   hh.E(), views, projs, ss[0].tanfovx, ss[0].tanfovy, gC, gD, gM, gV, gts, hh.T(ss[0].shs), 3,
                                   campos, geom, binning, img, alpha, persp, False, False, True, True, num_rendered=R)
            one_view = TB.one_view_dict
        else:
            out, cams = TF.batch_forward(ss, 3)
            grads = [tuple(x * (s.W * s.H) ** 0.5 for x in (s.gC, s.gD, s.gV)) for s in ss]
            (R, color, depth, unc, radii, geom, binning, img, _) = out
            views, projs, campos, gts = cams
            gC = hh.T(np.stack([g[0] for g in grads]))
            gD, gU = (hh.T(np.stack([g[i][None] for g in grads])) for i in (1, 2))
            from dgr_amd import batch_full as BF
            gb = BF._backward_batch(hh.T(ss[0].bg), hh.T(ss[0].means), radii, hh.E(), hh.T(ss[0].scales), hh.T(ss[0].rots), 1.0,
                                    hh.E(), views, projs, ss[0].tanfovx, ss[0].tanfovy, gC, gD, gU, gts, hh.T(ss[0].shs), 3,
                                    campos, geom, binning, img, persp, True, True, R)
            one_view = TF.one_view
        names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations",
                 "dL_dview"]
        gb = {n: (None if v is None else v.cpu().numpy()) for n, v in zip(names, gb)}
        acc = None
        for v, s in enumerate(ss):
            if variant == "light":
                one, _ = hh.hip_forward(s, 3)
                for k in (1, 2, 3, 5, 6):  # colour, depth, median, opacity map, radii
                    assert torch.equal(out[k][v], one[k]), (v, k)
                g1 = hh.hip_backward(s, 3, one_view(out, v), grads=grads[v])
            else:
                one, _ = hh.hip_full_forward(s, 3)
                for k in (1, 2, 3, 4):  # colour, depth, uncertainty, radii
                    assert torch.equal(out[k][v], one[k + 1]), (v, k)
                g1 = hh.hip_full_backward(s, 3, one_view(out, v), grads=grads[v])
            assert TB.close(gb["dL_dview"][v], g1["dL_dview"], 1e-5), v
            acc = {k: g1[k].copy() for k in g1} if acc is None else {k: acc[k] + g1[k] for k in g1}
    for k in ("dL_dmeans3D", "dL_dsh", "dL_dopacity", "dL_dscales", "dL_drotations"):
        assert TB.close(gb[k], acc[k]), k


# ------------------------------------------------------------------------------------------ slam.render
@pytest.mark.parametrize("complete", [False, True])
def test_slam_render_with_an_off_centre_projection(complete):
    """slam.render with `viewpoint_camera.projection_matrix` = an off-centre Proj^T against the direct GaussianRasterizer call
    on the camera tensors render() forms on the device from it (projmatrix = viewmatrix x perspec and campos, each one ulp
    from synth's float64 products): the same images bit for bit and the same gradients."""
    from types import SimpleNamespace
    from dgr_amd import _capi
    from dgr_amd import light as L
    from dgr_amd import pose, slam
    from dgr_amd.multiview import make_settings
    from test_hip_full_batch import Model
    s, _ = small("tum", "plain", 46)
    dev = hh.dev()
    gC, gD = hh.T(s.gC), hh.T(s.gD)
    cam = SimpleNamespace(projection_matrix=hh.T(s.persp), znear=0.01, zfar=100.0)
    vm = hh.T(s.view).requires_grad_()
    pc = Model(s, dev)
    o = slam.render(cam, pc, None, hh.T(s.bg), viewmatrix=vm, fov=(s.tanfovx, s.tanfovy), HW=(s.H, s.W), gt_depth=hh.T(s.gt),
                    complete_pose=complete)
    ((o["render"] * gC).sum() + (o["depth"].reshape(s.H, s.W) * gD).sum()).backward()
    vm2 = hh.T(s.view).requires_grad_()
    pc2 = Model(s, dev)
    with torch.no_grad():
        v0 = hh.T(s.view)
        settings = make_settings(s, 3, dev)._replace(projmatrix=pose._matmul_fixed_order(v0, hh.T(s.persp)).contiguous(),
                                                     campos=pose._campos(v0))
    with _capi.thread_options(pose_grad=int(complete)):
        r = L.GaussianRasterizer(settings)(
            means3D=pc2.get_xyz, means2D=torch.zeros_like(pc2.get_xyz), opacities=pc2.get_opacity, shs=pc2.get_features,
            scales=pc2.get_scaling, rotations=pc2.get_rotation, viewmatrix=vm2, gt_depth=hh.T(s.gt))
        ((r[0] * gC).sum() + (r[2].reshape(s.H, s.W) * gD).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(o["render"].detach(), r[0].detach()) and torch.equal(o["depth"].detach().reshape(-1), r[2].detach().reshape(-1))
    a, b = vm.grad.cpu().numpy().astype(np.float64), vm2.grad.cpu().numpy().astype(np.float64)
    assert np.abs(a - b).max() <= 2e-6 * np.abs(b).max()
    for x, y in ((pc.get_xyz, pc2.get_xyz), (pc.get_opacity, pc2.get_opacity)):
        assert np.abs(x.grad.cpu().numpy() - y.grad.cpu().numpy()).max() <= 2e-6 * np.abs(y.grad.cpu().numpy()).max()
