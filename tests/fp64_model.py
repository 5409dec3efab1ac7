"""The float64 PyTorch formulation the tests measure against: an INDEPENDENT check of the backward math,
written from SURVEY.md Appendix A's formulas (not from oracle/dgr_oracle.cpp) and differentiated by autograd.  A transcription
error in one component of, say, dL_drotations that the oracle and the kernels share would pass every oracle-vs-kernel test; it
cannot pass a comparison with this model.

Three formulations stand on one set of building blocks (projection, covariance, conic, SH colour, the walk over the tiles, alpha,
blend weights, the light median):
  torch_light       the light variant as the reference differentiates it;
  torch_full        the -full variant, with ComputePG's shaping of the pose gradient (its own blend step);
  complete_forward  either variant with ONE view-matrix leaf feeding every path (option "pose_grad" = 1, include/dgr_hip.h).
`pairs` (torch_light, torch_full) hands the screen-space mean to each tile as a tensor per (Gaussian, pixel), for absgrad.

Hard decisions (visibility, the per-pair alpha / power tests, the last contributor) are evaluated in float64 from the
same formulas on the oracle's integer path (`vis`, `point_list`, `ranges`, `n_contrib`, pinned separately by SURVEY Appendix C);
the tests first assert that the resulting images equal the oracle's, i.e. that the decisions agree.
Where the reference's analytic backward is deliberately NOT the derivative of its forward, the forward is
shaped so that autograd produces the reference's quantity (each is a documented quirk):
  * alpha = min(0.99, o G) but the backward never masks the clamp (L/cr/backward.cu:627): straight-through clamp;
  * depth_var is 0 in the forward yet its gradient is consumed as d/d sum (d - gt)^2 alpha T (:600-608): the loss
    contains that sum;
  * the median-depth gradient goes to the deepest valid Gaussian with T > 0.5 after the division (:656-663);
  * the pose gradient covers only mean2D and the depth sum (:633-651): the view matrix enters torch_light as three
    tensors (ndc path, depth path, everything else) and only the first two are differentiated;
  * its ndc Jacobian is the symmetric frustum's (:725-739, F/cr/backward.cu:516-534): x column m_w persp[0], y column
    m_w persp[5], z column -m_hom m_w^2 with m_hom from the full projection -- persp[8] and persp[9] (the principal point)
    and every other entry are left out (`reference_ndc_pose`); dL_dmeans3D uses the full projection;
  * the clamp of t.x / t.z treats the clamped coordinate as independent of t.z (:175-176,262-264).
"""
from types import SimpleNamespace

import numpy as np
import torch

# (P, W, H, SH degree, seed) of util.make_scene
CASES = [(400, 64, 48, 3, 11), (300, 40, 40, 0, 12), (500, 70, 45, 2, 13), (300, 40, 40, 1, 15)]

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435]


def f64(a):
    return torch.tensor(np.asarray(a, np.float64))


# ------------------------------------------------------------------------------------------ per Gaussian
def sh_to_rgb(deg, sh, d, clamp=True):
    """SURVEY A-P 9 / A-G: basis order and signs of */cr/forward.cu:30-59; sh [V,16,3], d [V,3] unit directions.  `clamp=False`
    leaves out the final max(., 0): what dgc_dCampos differentiates (F/cuda_rasterizer/backward.cu:159-166)."""
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    r = C0 * sh[:, 0]
    if deg > 0:
        r = r - C1 * y * sh[:, 1] + C1 * z * sh[:, 2] - C1 * x * sh[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        r = (r + C2[0] * xy * sh[:, 4] + C2[1] * yz * sh[:, 5] + C2[2] * (2 * zz - xx - yy) * sh[:, 6]
             + C2[3] * xz * sh[:, 7] + C2[4] * (xx - yy) * sh[:, 8])
        if deg > 2:
            r = (r + C3[0] * y * (3 * xx - yy) * sh[:, 9] + C3[1] * xy * z * sh[:, 10]
                 + C3[2] * y * (4 * zz - xx - yy) * sh[:, 11] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12]
                 + C3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + C3[5] * z * (xx - yy) * sh[:, 14]
                 + C3[6] * x * (xx - 3 * yy) * sh[:, 15])
    return torch.clamp(r + 0.5, min=0.0) if clamp else r + 0.5


def reference_ndc_pose(mh, view, persp, p_hom, W, H):
    """A zero-valued [n, 2] pixel offset whose gradient w.r.t. `view` is the reference's pose Jacobian of the ndc position
    (L/cuda_rasterizer/backward.cu:725-739, F/cuda_rasterizer/backward.cu:516-534): d ndc_x / d t_cam = (m_w persp[0], 0,
    -m_hom.x m_w^2), d ndc_y / d t_cam = (0, m_w persp[5], -m_hom.y m_w^2), m_hom = the full projection of the mean (detached,
    as are `mh` and `persp`).  For a symmetric frustum (persp[8] = persp[9] = 0, persp[11] = 1) it is the exact derivative."""
    tc = mh.detach() @ view                                   # t_cam (homogeneous), gradient -> view only
    pf = persp.detach().reshape(-1)
    ph = p_hom.detach()
    mw = 1.0 / (ph[:, 3] + 1e-7)
    nx = mw * pf[0] * tc[:, 0] - ph[:, 0] * mw * mw * tc[:, 2]
    ny = mw * pf[5] * tc[:, 1] - ph[:, 1] * mw * mw * tc[:, 2]
    return torch.stack([(nx - nx.detach()) * (0.5 * W), (ny - ny.detach()) * (0.5 * H)], 1)


def make_leaves(s, colors_precomp=None, cov3D_precomp=None, **views):
    """The inputs as float64 leaves; `views`: the view-matrix leaves of the formulation.  `colors_precomp` [P, 3] / `cov3D_precomp`
    [P, 6] (xx, xy, xz, yy, yz, zz) replace the SH evaluation / R diag(s^2) R^T as in the reference
    (L/cuda_rasterizer/forward.cu:208-218, 242-247); their gradients are then leaves `colors` / `cov3D`."""
    leaves = dict(means3D=f64(s.means), scales=f64(s.scales), rotations=f64(s.rots), opacities=f64(s.opac), shs=f64(s.shs), **views)
    if colors_precomp is not None:
        leaves["colors"] = f64(colors_precomp)
    if cov3D_precomp is not None:
        leaves["cov3D"] = f64(cov3D_precomp)
    for v in leaves.values():
        v.requires_grad_(True)
    return leaves


def homogeneous(m):
    return torch.cat([m, torch.ones(len(m), 1, dtype=torch.float64)], 1)


def pixels(p_hom, W, H):
    """A-P 2, 7: p_hom = proj m, p_w = 1 / (w + 1e-7), pixel = ((ndc + 1) S - 1) / 2"""
    p_w = 1.0 / (p_hom[:, 3] + 1e-7)
    return torch.stack([((p_hom[:, 0] * p_w + 1.0) * W - 1.0) * 0.5, ((p_hom[:, 1] * p_w + 1.0) * H - 1.0) * 0.5], 1)


def covariance(leaves, idx):
    """A-P 3 / A-G: Sigma = R diag(s^2) R^T with the UNNORMALISED quaternion (r, x, y, z), or the precomputed one (an off-diagonal
    value stands at two places of Sigma: its gradient is their sum, backward.cu:281-283)."""
    if "cov3D" in leaves:
        c6 = leaves["cov3D"][idx]
        return torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(-1, 3, 3)
    q = leaves["rotations"][idx]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    sc = leaves["scales"][idx]
    return R @ torch.diag_embed(sc * sc) @ R.transpose(1, 2)


def detached(name, fn):
    """The `keep` hook with nothing to freeze: the value, detached."""
    return fn().detach()


def conic(s, t, Sigma, Rcam, keep=detached):
    """A-P 4 / A-G: cov2D = A Sigma A^T + 0.3 I, A = Ju Rcam, t.x/t.z clamped to +-1.3 tanfov (the clamped coordinate detached);
    returns the conic (a, b, c)."""
    fx, fy = s.W / (2.0 * s.tanfovx), s.H / (2.0 * s.tanfovy)
    limx, limy = 1.3 * s.tanfovx, 1.3 * s.tanfovy
    rx, ry = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    tx = torch.where(keep("clx", lambda: rx.abs() > limx), keep("tx", lambda: torch.clamp(rx, -limx, limx) * t[:, 2]), t[:, 0])
    ty = torch.where(keep("cly", lambda: ry.abs() > limy), keep("ty", lambda: torch.clamp(ry, -limy, limy) * t[:, 2]), t[:, 1])
    tz = t[:, 2]
    zero = torch.zeros_like(tz)
    Ju = torch.stack([fx / tz, zero, -fx * tx / (tz * tz), zero, fy / tz, -fy * ty / (tz * tz)], 1).reshape(-1, 2, 3)
    A = Ju @ Rcam
    cov = A @ Sigma @ A.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c - b * b
    return c / det, -b / det, a / det


# ------------------------------------------------------------------------------------------ per tile
def tiles(s, vis, point_list, ranges, n_contrib):
    """The non-empty tiles of `ranges`: `ids` (rows of the visible Gaussians, front to back), the pixels' coordinates `pxs`, `pys`
    [npix], the list positions `pos` [n, 1], the pixels' last contributors `ncp` [1, npix] and the tile's window `sel` / `hw`."""
    W, H = s.W, s.H
    slot = np.full(s.P, -1, np.int64)
    slot[np.nonzero(vis)[0]] = np.arange(int(np.count_nonzero(vis)))
    gx = (W + 15) // 16
    nc = torch.tensor(np.asarray(n_contrib, np.int64).reshape(H, W))
    for tile, (lo, hi) in enumerate(np.asarray(ranges).reshape(-1, 2)):
        if hi <= lo:
            continue
        x0, y0 = (tile % gx) * 16, (tile // gx) * 16
        x1, y1 = min(x0 + 16, W), min(y0 + 16, H)
        ys, xs = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        yield SimpleNamespace(tile=tile, ids=torch.tensor(slot[np.asarray(point_list[lo:hi], np.int64)]),
                              pxs=xs.reshape(-1).double(), pys=ys.reshape(-1).double(), pos=torch.arange(hi - lo)[:, None],
                              ncp=nc[y0:y1, x0:x1].reshape(-1)[None], sel=(slice(y0, y1), slice(x0, x1)), hw=(y1 - y0, x1 - x0))


def tile_xy(pix, tl, pairs=None):
    """The screen-space means of a tile's Gaussians, (x, y) as [n, 1] -- or, absgrad (`pairs` a list): repeated over the tile's
    pixels as a leaf [n, npix, 2] of its own, whose gradient is every pixel's own contribution v_p(g) to dL/dmean2D; (ids, leaf)
    goes to `pairs`."""
    if pairs is None:
        return pix[tl.ids, 0:1], pix[tl.ids, 1:2]
    lf = pix[tl.ids].detach()[:, None, :].expand(-1, len(tl.pxs), -1).clone().requires_grad_(True)
    pairs.append((tl.ids, lf))
    return lf[:, :, 0], lf[:, :, 1]


def absgrad_of_pairs(pairs, idx, P, W, H):
    """sum over the pixels of |v_p(g)|, scattered back to the Gaussians' rows, in ndc units (x W/2, y H/2); z = 0."""
    acc = torch.zeros(len(idx), 2, dtype=torch.float64)
    for ids, lf in pairs:
        if lf.grad is not None:
            acc.index_add_(0, ids, lf.grad.abs().sum(1))
    out = np.zeros((P, 3))
    out[np.asarray(idx), :2] = (acc * torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float64)).numpy()
    return out


def alpha_of(tl, xy, con, opac, keep=detached):
    """A-R: d = xy - pixel, power, alpha = min(0.99, o G) with the straight-through clamp (backward.cu:627)"""
    dx = xy[0] - tl.pxs[None]
    dy = xy[1] - tl.pys[None]
    ids = tl.ids
    power = -0.5 * (con[0][ids, None] * dx * dx + con[2][ids, None] * dy * dy) - con[1][ids, None] * dx * dy
    oG = opac[ids, None] * torch.exp(power)
    return power, oG + keep(f"st{tl.tile}", lambda: torch.clamp(oG, max=0.99) - oG)


def valid_pairs(tl, power, alpha):
    return (power <= 0) & (alpha >= 15.0 / 255.0) & (tl.pos < tl.ncp)


def blend_weights(av):
    """(alpha T, T before each Gaussian, T_final) down a tile's list"""
    Tincl = torch.cumprod(1.0 - av, 0)
    Texcl = torch.cat([torch.ones(1, av.shape[1], dtype=torch.float64), Tincl[:-1]], 0)
    return av * Texcl, Texcl, Tincl[-1]


def put_color(color, tl, w, rgb, T_final, bg):
    color[(slice(None),) + tl.sel] = ((w[:, :, None] * rgb[tl.ids][:, None, :]).sum(0) + T_final[:, None] * bg[None]).t().reshape(3, *tl.hw)


def put(img, tl, pixel_values):
    img[tl.sel] = pixel_values.reshape(tl.hw)


def blend(s, decisions, pix, con, opac, rgb, z_depth, z_cam, median=True, keep=detached, pairs=None):
    """The images of torch_light and of complete_forward: colour, depth (of `z_depth`), sum alpha T, the variance sum
    sum (z_cam - gt)^2 alpha T and, `median`, the light median depth."""
    bg, gt = f64(s.bg), f64(s.gt)
    color = torch.zeros(3, s.H, s.W, dtype=torch.float64)
    depth, alpha_img, var, med = (torch.zeros(s.H, s.W, dtype=torch.float64) for _ in range(4))
    for tl in tiles(s, *decisions):
        power, alpha = alpha_of(tl, tile_xy(pix, tl, pairs), con, opac, keep)
        valid = keep(f"valid{tl.tile}", lambda: valid_pairs(tl, power, alpha))
        w, Texcl, T_final = blend_weights(torch.where(valid, alpha, torch.zeros_like(alpha)))
        put_color(color, tl, w, rgb, T_final, bg)
        put(depth, tl, (w * z_depth[tl.ids, None]).sum(0))
        put(alpha_img, tl, w.sum(0))
        e = z_cam[tl.ids, None] - gt[tl.sel].reshape(-1)[None]
        put(var, tl, (w * e * e).sum(0))
        if median:  # deepest valid Gaussian whose transmittance before it exceeds 0.5 (the backward's criterion, :656-663)
            last = keep(f"last{tl.tile}", lambda: (valid & (Texcl > 0.5)) * (tl.pos + 1)).max(0).values - 1
            zm = z_cam[tl.ids][last.clamp(min=0)]
            put(med, tl, torch.where(last >= 0, zm, torch.zeros_like(zm)))
    return color, depth, alpha_img, var, med


def weighted(grads, images):
    return sum((f64(g) * img).sum() for g, img in zip(grads, images))


# ------------------------------------------------------------------------------------------ the three formulations
def torch_light(s, deg, vis, point_list, ranges, n_contrib, grads, colors_precomp=None, cov3D_precomp=None, pairs=None):
    """Returns (loss, leaves dict, images dict); `_pix` / `_idx` of the images: the screen-space means (their .grad is dL_dmeans2D
    in pixels) and their rows.  `pairs`: see tile_xy."""
    W, H = s.W, s.H
    leaves = make_leaves(s, colors_precomp, cov3D_precomp, view_ndc=f64(s.view), view_depth=f64(s.view))
    view_o, persp = f64(s.view), f64(s.persp)
    idx = torch.tensor(np.nonzero(vis)[0])
    m = leaves["means3D"][idx]
    mh = homogeneous(m)
    p_hom = mh @ (view_o @ persp)
    pix = pixels(p_hom, W, H) + reference_ndc_pose(mh, leaves["view_ndc"], persp, p_hom, W, H)   # (pose path 1: the reference's Jacobian)
    pix.retain_grad()
    z_depth = (mh @ leaves["view_depth"])[:, 2]                                                  # (pose path 2)
    t = (mh @ view_o)[:, :3]                                                                      # (no pose gradient)
    z_cam = t[:, 2]
    con = conic(s, t, covariance(leaves, idx), view_o[:3, :3].t())
    dirs = m - f64(s.campos)                                                                      # A-P 9
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    rgb = sh_to_rgb(deg, leaves["shs"][idx], dirs) if colors_precomp is None else leaves["colors"][idx]
    opac = leaves["opacities"][idx, 0]
    color, depth, alpha_img, var, median = blend(s, (vis, point_list, ranges, n_contrib), pix, con, opac, rgb, z_depth, z_cam,
                                                 pairs=pairs)
    loss = weighted(grads, (color, depth, median, var))
    return loss, leaves, dict(color=color.detach().numpy(), depth=depth.detach().numpy(),
                              opacity_map=alpha_img.detach().numpy(), _pix=pix, _idx=idx.numpy())


def torch_full(s, deg, vis, point_list, ranges, n_contrib, grads, pairs=None):
    """The -full variant, written from SURVEY.md Appendix A (A-R, A-F) and the structure of ComputePG
    (F/cuda_rasterizer/backward.cu:990-1072, 1246-1289, 1316-1338) -- not from oracle/dgr_oracle.cpp.  Differences to the
    light formulation above, each shaped so that autograd yields the reference's quantity:
      * the terminating Gaussian IS blended (n_contrib includes it); no median; the third image is U = sum alpha T in the
        forward but its gradient is consumed as d/d sum (d - gt)^2 alpha T (quirk F2): the loss contains that sum;
      * the pose gradient is part 1 + part 2-1 of ComputePG only (part 2-2 is computed and never summed, F3):
          part 1   colour -> campos -> view, with campos = -(v0 v12 + v1 v13 + v2 v14, v4 v12 + .., v8 v12 + ..) and the colour's
                   derivative NOT masked by the 0-clamp (dgc_dCampos, F:159-166): an unclamped copy of the colour carries it;
          part 2-1 alpha -> ndc -> view for the COLOUR channels of every valid pair, without the background's share;
          depth    dL_depth * dd_dv is ASSIGNED per pair, not accumulated (F4): only the pixel's front-most valid Gaussian
                   contributes, through its own depth (v2, v6, v10, v14) and through its alpha's ndc path;
          the uncertainty channel does not enter the pose gradient (F7).
        Hence three copies of alpha per pair -- for the colour, the depth and the uncertainty channel -- equal in value and
        different in what they let a gradient reach.
    `pairs` (see tile_xy) replaces the means' screen-space position, not the pose path's."""
    W, H = s.W, s.H
    leaves = make_leaves(s, view_ndc=f64(s.view), view_depth=f64(s.view), view_campos=f64(s.view))
    view_o, persp, campos, bg, gt = f64(s.view), f64(s.persp), f64(s.campos), f64(s.bg), f64(s.gt)
    idx = torch.tensor(np.nonzero(vis)[0])
    m = leaves["means3D"][idx]
    mh, mh_c = homogeneous(m), homogeneous(m.detach())
    pix = pixels(mh @ (view_o @ persp), W, H)            # gradient -> means
    pix.retain_grad()
    # gradient -> view (ndc path, the reference's Jacobian), nothing else
    pix_pose = pix.detach() + reference_ndc_pose(mh_c, leaves["view_ndc"], persp, mh_c @ (view_o @ persp), W, H)
    t = (mh @ view_o)[:, :3]
    z = t[:, 2]                                          # gradient -> means
    z_pose = (mh_c @ leaves["view_depth"])[:, 2]         # gradient -> view (depth path)
    con = conic(s, t, covariance(leaves, idx), view_o[:3, :3].t())
    dirs = m - campos
    rgb = sh_to_rgb(deg, leaves["shs"][idx], dirs / dirs.norm(dim=1, keepdim=True))
    # part 1: campos as the reference differentiates it, reached through an UNCLAMPED copy of the colour
    vc = leaves["view_campos"].reshape(-1)
    cam_v = -torch.stack([vc[0] * vc[12] + vc[1] * vc[13] + vc[2] * vc[14], vc[4] * vc[12] + vc[5] * vc[13] + vc[6] * vc[14],
                          vc[8] * vc[12] + vc[9] * vc[13] + vc[10] * vc[14]])
    assert float((cam_v.detach() - campos).abs().max()) < 1e-5  # (the scene's campos is that of its view matrix)
    dirs_c = m.detach() - cam_v
    rgb_c = sh_to_rgb(deg, leaves["shs"][idx].detach(), dirs_c / dirs_c.norm(dim=1, keepdim=True), clamp=False)
    rgb = rgb + (rgb_c - rgb_c.detach())
    opac = leaves["opacities"][idx, 0]
    con_d, opac_d = tuple(c.detach() for c in con), opac.detach()

    color = torch.zeros(3, H, W, dtype=torch.float64)
    depth, unc, var = (torch.zeros(H, W, dtype=torch.float64) for _ in range(3))
    first_contrib, n_valid = (torch.zeros(H, W, dtype=torch.int64) for _ in range(2))
    for tl in tiles(s, vis, point_list, ranges, n_contrib):
        power, alpha = alpha_of(tl, tile_xy(pix, tl, pairs), con, opac)
        _, alpha_p = alpha_of(tl, tile_xy(pix_pose, tl), con_d, opac_d)
        valid = valid_pairs(tl, power, alpha)
        first = valid & (torch.cumsum(valid.long(), 0) == 1)   # the pixel's front-most valid Gaussian
        put(first_contrib, tl, (first * (tl.pos + 1)).sum(0))   # (1-based list position, 0: no valid Gaussian)
        put(n_valid, tl, valid.sum(0))
        zeros = torch.zeros_like(alpha)
        pose_term = alpha_p - alpha_p.detach()                  # value 0, gradient -> view (ndc path)
        w_col = blend_weights(torch.where(valid, alpha + pose_term, zeros))[0]
        w_dep = blend_weights(torch.where(valid, alpha + torch.where(first, pose_term, zeros), zeros))[0]
        # (dpixel_dalpha = T (c - accum_rec), F/cuda_rasterizer/backward.cu:692: the background's share of dL/dalpha (:733)
        #  is NOT in the pose gradient -- the background is weighted with the transmittance that carries no pose term)
        w_unc, _, T_final = blend_weights(torch.where(valid, alpha, zeros))
        zd = z[tl.ids, None] + torch.where(first, (z_pose - z_pose.detach())[tl.ids, None], zeros)
        put_color(color, tl, w_col, rgb, T_final, bg)
        put(depth, tl, (w_dep * zd).sum(0))
        put(unc, tl, w_unc.sum(0))
        e = z[tl.ids, None] - gt[tl.sel].reshape(-1)[None]
        put(var, tl, (w_unc * e * e).sum(0))
    loss = weighted(grads, (color, depth, var))
    return loss, leaves, dict(color=color.detach().numpy(), depth=depth.detach().numpy(), uncertainty=unc.detach().numpy(),
                              first_contrib=first_contrib.numpy(), n_valid=n_valid.numpy(), _pix=pix, _idx=idx.numpy())


def complete_forward(s, variant, deg, vis, point_list, ranges, n_contrib, grads, colors_precomp=None, cov3D_precomp=None,
                     added=True, view=None, frozen=None):
    """The complete pose gradient (option "pose_grad" = 1, include/dgr_hip.h): the light / full forward with ONE view-matrix leaf
    feeding every path -- the ndc position (through view x perspec), the camera-space z of the depth, variance and median images,
    Rcam and t_cam of the 2D covariance (A = Ju Rcam) and campos = -Rcam^T t of the SH colour.  Its dL/dview is the view-matrix
    counterpart of its dL/dmeans3D.  The variants' quirks stay as the per-Gaussian gradients have them (straight-through alpha
    clamp, the t.x/t.z clamp treated as independent of t.z, the light median criterion, the full variant's uncertainty consumed
    as a variance); the full variant's blend is the plain one, not torch_full's ComputePG shaping.

    Returns (loss, leaves, images, frozen).  `added=False` (light only) detaches the paths the reference's pose gradient
    leaves out -- cov2D, SH campos, the variance and median z -- so that dL/dview is the reference's.  `view`: a float64 [4,4]
    view matrix instead of the scene's; `frozen`: the dict of detached values / decisions of an earlier call, reused, which makes
    the function that central differences see the one autograd differentiates.  The ndc position is differentiated through the
    full perspec in the complete formulation and through the reference's symmetric-frustum Jacobian (reference_ndc_pose) in the
    reference split: the two part where persp[8] or persp[9] (an off-centre principal point) is not 0."""
    fr = {} if frozen is None else frozen

    def keep(name, fn):
        if name not in fr:
            fr[name] = fn().detach()
        return fr[name]

    W, H = s.W, s.H
    leaves = make_leaves(s, colors_precomp, cov3D_precomp, view=(f64(s.view) if view is None else view.detach().clone()))
    V = leaves["view"]
    Va = V if added else V.detach()  # what the added paths see
    persp = f64(s.persp)
    idx = torch.tensor(np.nonzero(vis)[0])
    m = leaves["means3D"][idx]
    mh = homogeneous(m)
    p_hom = mh @ (Va @ persp)                                  # ndc path (complete: the full projection's derivative)
    pix = pixels(p_hom, W, H)
    if not added:  # the reference's pose Jacobian of the ndc position (persp[0], persp[5] and m_hom only)
        pix = pix + reference_ndc_pose(mh, V, persp, p_hom, W, H)
    z_depth = (mh @ V)[:, 2]                                   # the depth image's z (a reference path)
    t = (mh @ Va)[:, :3]                                       # t_cam = Rcam m + t: cov2D, variance, median
    z_cam = t[:, 2]
    Rc = Va[:3, :3].t()                                        # Rcam[j][k] = v[4k + j]
    con = conic(s, t, covariance(leaves, idx), Rc, keep)
    # campos = -Rcam^T t (the library differentiates it so; the scene's campos is that of its view matrix)
    campos = -(Va[:3, :3] @ Va[3, :3]) if added else f64(s.campos)
    dirs = m - campos
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    rgb = sh_to_rgb(deg, leaves["shs"][idx], dirs) if colors_precomp is None else leaves["colors"][idx]
    opac = leaves["opacities"][idx, 0]
    light = variant == "light"
    color, depth, alpha_img, var, median = blend(s, (vis, point_list, ranges, n_contrib), pix, con, opac, rgb,
                                                 z_depth if light else z_cam, z_cam, median=light, keep=keep)
    # (full: the uncertainty image is sum alpha T; its gradient is consumed as that of the variance sum, F2)
    loss = weighted(grads, (color, depth, median, var) if light else (color, depth, var))
    imgs = dict(color=color.detach().numpy(), depth=depth.detach().numpy())
    imgs["opacity_map" if light else "uncertainty"] = alpha_img.detach().numpy()
    return loss, leaves, imgs, fr


# ------------------------------------------------------------------------------------------ drivers
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
