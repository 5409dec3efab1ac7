"""The complete pose gradient (option "pose_grad" = 1, include/dgr_hip.h) in float64, on the CPU.

`complete_forward` is the light / full forward of tests/test_oracle_autograd.py (torch_light, torch_full) rewritten so that ONE
view-matrix leaf feeds every path: the ndc position (through view x perspec), the camera-space z of the depth, variance and
median images, Rcam and t_cam of the 2D covariance (A = Ju Rcam) and campos = -Rcam^T t of the SH colour.  Its dL/dview is the
view-matrix counterpart of its dL/dmeans3D -- the contract of the complete mode.  The variants' quirks stay as the per-Gaussian
gradients have them (straight-through alpha clamp, the t.x/t.z clamp treated as independent of t.z, the light median criterion,
the full variant's uncertainty consumed as a variance).  Hard decisions come from the oracle's integer path, as in
test_oracle_autograd.py, and every detached quantity / decision can be frozen at the unperturbed view (`frozen`), which makes
the function that central differences see the one autograd differentiates."""
import numpy as np
import pytest
import torch

from test_oracle_autograd import (CAMERA_CASES, CASES, assert_placement_edge, camera_case_id, camera_case_scene,
                                  reference_ndc_pose, sh_to_rgb)
from util import make_scene

WRITTEN = [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]  # the view entries a pose gradient writes (3, 7, 11, 15 stay 0)


def complete_forward(s, variant, deg, vis, point_list, ranges, n_contrib, grads, colors_precomp=None, cov3D_precomp=None,
                     added=True, view=None, frozen=None):
    """Returns (loss, leaves, images, frozen).  `added=False` (light only) detaches the paths the reference's pose gradient
    leaves out -- cov2D, SH campos, the variance and median z -- so that dL/dview is the reference's.  `view`: a float64 [4,4]
    view matrix instead of the scene's; `frozen`: the dict of detached values / decisions of an earlier call, reused.  The ndc
    position is differentiated through the full perspec in the complete formulation and through the reference's symmetric-
    frustum Jacobian (test_oracle_autograd.reference_ndc_pose) in the reference split: the two part where persp[8] or
    persp[9] (an off-centre principal point) is not 0."""
    f = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    fr = {} if frozen is None else frozen

    def keep(name, fn):
        if name not in fr:
            fr[name] = fn().detach()
        return fr[name]

    W, H = s.W, s.H
    leaves = dict(means3D=f(s.means), scales=f(s.scales), rotations=f(s.rots), opacities=f(s.opac), shs=f(s.shs),
                  view=(f(s.view) if view is None else view.detach().clone()))
    if colors_precomp is not None:
        leaves["colors"] = f(colors_precomp)
    if cov3D_precomp is not None:
        leaves["cov3D"] = f(cov3D_precomp)
    for v in leaves.values():
        v.requires_grad_(True)
    V = leaves["view"]
    Va = V if added else V.detach()  # what the added paths see
    persp, bg, gt = f(s.persp), f(s.bg), f(s.gt)
    idx = torch.tensor(np.nonzero(vis)[0])
    m = leaves["means3D"][idx]
    mh = torch.cat([m, torch.ones(len(idx), 1, dtype=torch.float64)], 1)
    p_hom = mh @ ((V if added else V.detach()) @ persp)        # ndc path (complete: the full projection's derivative)
    p_w = 1.0 / (p_hom[:, 3] + 1e-7)
    pix = torch.stack([((p_hom[:, 0] * p_w + 1.0) * W - 1.0) * 0.5, ((p_hom[:, 1] * p_w + 1.0) * H - 1.0) * 0.5], 1)
    if not added:  # the reference's pose Jacobian of the ndc position (persp[0], persp[5] and m_hom only)
        pix = pix + reference_ndc_pose(mh, V, persp, p_hom, W, H)
    z_depth = (mh @ V)[:, 2]                                   # the depth image's z (a reference path)
    t = (mh @ Va)[:, :3]                                       # t_cam = Rcam m + t: cov2D, variance, median
    z_cam = t[:, 2]
    Rc = Va[:3, :3].t()                                        # Rcam[j][k] = v[4k + j]
    if cov3D_precomp is not None:
        c6 = leaves["cov3D"][idx]
        Sigma = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(-1, 3, 3)
    else:
        q = leaves["rotations"][idx]
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
        sc = leaves["scales"][idx]
        Sigma = R @ torch.diag_embed(sc * sc) @ R.transpose(1, 2)
    fx, fy = W / (2.0 * s.tanfovx), H / (2.0 * s.tanfovy)
    limx, limy = 1.3 * s.tanfovx, 1.3 * s.tanfovy
    rx, ry = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    tx = torch.where(keep("clx", lambda: rx.abs() > limx), keep("tx", lambda: torch.clamp(rx, -limx, limx) * t[:, 2]), t[:, 0])
    ty = torch.where(keep("cly", lambda: ry.abs() > limy), keep("ty", lambda: torch.clamp(ry, -limy, limy) * t[:, 2]), t[:, 1])
    tz = t[:, 2]
    zero = torch.zeros_like(tz)
    Ju = torch.stack([fx / tz, zero, -fx * tx / (tz * tz), zero, fy / tz, -fy * ty / (tz * tz)], 1).reshape(-1, 2, 3)
    A = Ju @ Rc
    cov = A @ Sigma @ A.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c - b * b
    con_a, con_b, con_c = c / det, -b / det, a / det
    # campos = -Rcam^T t (the library differentiates it so; the scene's campos is that of its view matrix)
    campos = -(Va[:3, :3] @ Va[3, :3]) if added else f(s.campos)
    dirs = m - campos
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    rgb = sh_to_rgb(deg, leaves["shs"][idx], dirs) if colors_precomp is None else leaves["colors"][idx]
    opac = leaves["opacities"][idx, 0]
    slot = np.full(s.P, -1, np.int64)
    slot[np.nonzero(vis)[0]] = np.arange(len(idx))

    color = torch.zeros(3, H, W, dtype=torch.float64)
    depth = torch.zeros(H, W, dtype=torch.float64)
    alpha_img = torch.zeros(H, W, dtype=torch.float64)
    var = torch.zeros(H, W, dtype=torch.float64)
    median = torch.zeros(H, W, dtype=torch.float64)
    gx = (W + 15) // 16
    nc = torch.tensor(np.asarray(n_contrib, np.int64).reshape(H, W))
    for tile, (lo, hi) in enumerate(np.asarray(ranges).reshape(-1, 2)):
        if hi <= lo:
            continue
        x0, y0 = (tile % gx) * 16, (tile // gx) * 16
        x1, y1 = min(x0 + 16, W), min(y0 + 16, H)
        ids = torch.tensor(slot[np.asarray(point_list[lo:hi], np.int64)])
        ys, xs = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        pxs, pys = xs.reshape(-1).double(), ys.reshape(-1).double()
        dx = pix[ids, 0:1] - pxs[None]
        dy = pix[ids, 1:2] - pys[None]
        power = -0.5 * (con_a[ids, None] * dx * dx + con_c[ids, None] * dy * dy) - con_b[ids, None] * dx * dy
        oG = opac[ids, None] * torch.exp(power)
        alpha = oG + keep(f"st{tile}", lambda: torch.clamp(oG, max=0.99) - oG)   # straight-through clamp
        pos = torch.arange(hi - lo)[:, None]
        ncp = nc[y0:y1, x0:x1].reshape(-1)[None]
        valid = keep(f"valid{tile}", lambda: (power <= 0) & (alpha >= 15.0 / 255.0) & (pos < ncp))
        av = torch.where(valid, alpha, torch.zeros_like(alpha))
        Tincl = torch.cumprod(1.0 - av, 0)
        Texcl = torch.cat([torch.ones(1, av.shape[1], dtype=torch.float64), Tincl[:-1]], 0)
        w = av * Texcl
        T_final = Tincl[-1]
        sel = (slice(None), slice(y0, y1), slice(x0, x1))
        color[sel] = ((w[:, :, None] * rgb[ids][:, None, :]).sum(0) + T_final[:, None] * bg[None]).t().reshape(3, y1 - y0, x1 - x0)
        depth[sel[1:]] = (w * (z_depth if variant == "light" else z_cam)[ids, None]).sum(0).reshape(y1 - y0, x1 - x0)
        alpha_img[sel[1:]] = w.sum(0).reshape(y1 - y0, x1 - x0)
        e = z_cam[ids, None] - gt[y0:y1, x0:x1].reshape(-1)[None]
        var[sel[1:]] = (w * e * e).sum(0).reshape(y1 - y0, x1 - x0)
        if variant == "light":  # deepest valid Gaussian whose transmittance before it exceeds 0.5 (the backward's criterion)
            last = keep(f"last{tile}", lambda: (valid & (Texcl > 0.5)) * (pos + 1)).max(0).values - 1
            has = last >= 0
            zm = z_cam[ids][last.clamp(min=0)]
            median[sel[1:]] = torch.where(has, zm, torch.zeros_like(zm)).reshape(y1 - y0, x1 - x0)
    if variant == "light":
        gC, gD, gM, gV = (f(g) for g in grads)
        loss = (gC * color).sum() + (gD * depth).sum() + (gM * median).sum() + (gV * var).sum()
        imgs = dict(color=color.detach().numpy(), depth=depth.detach().numpy(), opacity_map=alpha_img.detach().numpy())
    else:  # the uncertainty image is sum alpha T; its gradient is consumed as that of the variance sum (F2)
        gC, gD, gU = (f(g) for g in grads)
        loss = (gC * color).sum() + (gD * depth).sum() + (gU * var).sum()
        imgs = dict(color=color.detach().numpy(), depth=depth.detach().numpy(), uncertainty=alpha_img.detach().numpy())
    return loss, leaves, imgs, fr


def scaled_grads(s, variant):
    g = (s.gC, s.gD, s.gM, s.gV) if variant == "light" else (s.gC, s.gD, s.gV)
    return tuple(np.asarray(x, np.float64) * (s.W * s.H) ** 0.5 for x in g)


def oracle_run(O, s, variant, deg, grads, colors_precomp=None, cov3D_precomp=None):
    """The oracle's forward (decisions, images) and backward (the reference's pose gradient)."""
    use_sh, use_sr = colors_precomp is None, cov3D_precomp is None
    fw = O.light_forward if variant == "light" else O.full_forward
    st, ref = fw(s.bg, s.means, colors_precomp, s.opac, s.scales if use_sr else None, s.rots if use_sr else None, 1.0,
                 cov3D_precomp, s.view, s.gt, s.proj, s.tanfovx, s.tanfovy, s.H, s.W, s.shs if use_sh else None, deg, s.campos)
    g32 = [np.asarray(x, np.float32) for x in grads]
    if variant == "light":
        g = O.light_backward(st, s.bg, s.means, colors_precomp, s.scales if use_sr else None, s.rots if use_sr else None, 1.0,
                             cov3D_precomp, s.view, s.proj, s.tanfovx, s.tanfovy, *g32, s.gt, s.shs if use_sh else None, deg,
                             s.campos, ref["opacity_map"], s.persp)
    else:
        g = O.full_backward(st, s.bg, s.means, colors_precomp, s.scales if use_sr else None, s.rots if use_sr else None, 1.0,
                            cov3D_precomp, s.view, s.gt, s.proj, s.tanfovx, s.tanfovy, *g32, s.shs if use_sh else None, deg,
                            s.campos, s.persp)
    return st, ref, g


def complete_grad(s, variant, deg, st, ref, grads, colors_precomp=None, cov3D_precomp=None, added=True, view=None):
    """(dL/dview [16] with 3, 7, 11, 15 zeroed, dL/dmeans3D, leaves, images) of the float64 formulation."""
    loss, leaves, img, _ = complete_forward(s, variant, deg, ref["radii"] > 0, st.get("point_list"), st.get("ranges"),
                                            st.get("n_contrib"), grads, colors_precomp, cov3D_precomp, added=added, view=view)
    loss.backward()
    gv = leaves["view"].grad.numpy().reshape(-1).copy()
    gv[[3, 7, 11, 15]] = 0.0
    return gv, leaves["means3D"].grad.numpy(), leaves, img


def orthonormal_view(view):
    """The scene's view matrix with its rotation block made orthonormal in float64 (the float32 one is so to 1e-7 only)."""
    v = torch.tensor(np.asarray(view, np.float64)).clone()
    u, _, vt = torch.linalg.svd(v[:3, :3])
    v[:3, :3] = u @ vt
    return v


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
