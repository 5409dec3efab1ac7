"""Three parties, one arbiter: what the tests against the reference rasterizer's own source share (tests/test_hip_reference_*.py
on the GPU, tests/test_oracle_reference_pinned.py and tests/test_ref_parity_helper.py on the CPU).

A *party* is a dict of numpy arrays -- one implementation's results on one case: the reference library (oracle/reference.py),
the HIP kernels through the C ABI, the oracle in its float build and in its DGRO_C_MATH build, or the reference's recorded
outputs under tests/golden/reference/.  Integer state is compared with the reference's exactly, outside COUNTED flips whose
caps are conditions; real-valued results are measured against the float64 formulation of tests/fp64_model.py, evaluated on the
REFERENCE's decisions (its point_list, ranges and n_contrib): with e_ref = |reference - fp64| and e_x = |x - fp64|, both at
pixels and Gaussians no counted flip touches, a party passes when e_x <= max(2 e_ref, bar).  `bar` is the project's bar for
that quantity against the oracle (1e-6 max(1, |ref|) for colour and depth, 1e-5 of scale for gradients); the factor 2 over
the reference's OWN error is there because both sides sum with float atomics in an order that changes from run to run.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

import fp64_model as M
from dgr_amd.synth import cluster_scene, heavy_tail_scene, make_scene
from util import mask_flipped_pixels

# ------------------------------------------------------------------------------------------ cases
# name, P, W, H, SH degree, seed, what.  The seeds are committed: on each the float oracle against the C-math oracle (the CPU
# proxy for "same source, other libm / contraction") stays at or below HALF of every cap below (test_ref_parity_helper.py).
LIGHT_CASES = [
    ("deg0", 3000, 96, 64, 0, 7, {}),
    ("deg1", 3000, 96, 64, 1, 7, {}),
    ("deg2", 3000, 96, 64, 2, 7, {}),
    ("deg3", 3000, 96, 64, 3, 7, {}),
    ("ragged", 2000, 70, 45, 3, 2, {}),                                 # neither side a multiple of 16, background != 0
    ("one_tile", 1500, 16, 16, 3, 3, dict(scale_modifier=6.0)),        # one tile, a list of ~1500
    ("large", 20000, 320, 200, 3, 0, {}),
    ("heavy_tail", 20000, 256, 256, 3, 0, dict(scene="heavy_tail")),
    ("clustered", 10000, 256, 256, 3, 0, dict(scene="clustered")),
    ("precomp", 3000, 96, 64, 3, 7, dict(precomp=True)),               # colors_precomp and cov3D_precomp
]
FULL_CASES = LIGHT_CASES[:4]
MODES = [("mapping+pose", False, False), ("mapping", True, False), ("tracking", False, True)]  # name, track_off, map_off
GOLDEN_CASES = [("golden_deg3", 1500, 64, 48, 3, 21, {}), ("golden_deg0", 1500, 64, 48, 0, 22, {})]        # tests/golden/reference/

CAP_RADII = 1e-3      # of the Gaussians, each by at most 1
CAP_SWAPS = 1e-3      # of num_rendered
# (n_contrib / image flips: mask_flipped_pixels' own asserted bound, 3e-4 of the pixels)
BAR_IMAGE, BAR_GRAD, BAR_UNCERTAINTY = 1e-6, 1e-5, 1e-5

IMAGES_LIGHT = ("color", "depth", "depth_median", "opacity_map")
IMAGES_FULL = ("color", "depth", "uncertainty")
GRADS = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dview")


def case_id(case):
    return case[0]


def build_case(case):
    """-> namespace(name, s, deg, kw): kw = colors_precomp / cov3D_precomp / scale_modifier as the drivers of hip_helpers take them"""
    name, P, W, H, deg, seed, what = case
    s = make_scene(P, W, H, seed)
    if what.get("scene") == "heavy_tail":
        s = heavy_tail_scene(s)
    elif what.get("scene") == "clustered":
        s = cluster_scene(s)
    kw = {}
    if "scale_modifier" in what:
        kw["scale_modifier"] = what["scale_modifier"]
    if what.get("precomp"):
        rng = np.random.default_rng(seed + 1000)
        kw["colors_precomp"] = rng.uniform(0.0, 1.0, (P, 3)).astype(np.float32)
        with torch.no_grad():
            S = M.covariance(dict(rotations=M.f64(s.rots), scales=M.f64(s.scales)), torch.arange(P)).numpy()
        kw["cov3D_precomp"] = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)
    return SimpleNamespace(name=name, s=s, deg=deg, kw=kw)


def pixel_grads(s, variant="light"):
    """all four (light) / three (full) pixel-gradient images non-zero, scaled as fp64_model.scaled_grads does"""
    return tuple(np.asarray(g, np.float32) for g in M.scaled_grads(s, variant))


# ------------------------------------------------------------------------------------------ parties
def reference_library(variant):
    """oracle/reference.py with the variant's library loaded; a missing library FAILS the calling test and names the build step"""
    import pytest
    from oracle import reference as R
    try:
        R.lib(variant)
    except FileNotFoundError as e:
        pytest.fail(str(e))
    return R


STATE = ("point_list", "ranges", "n_contrib", "depths", "means2D", "conic_opacity", "rgb")


def module_forward(O, c, variant="light"):
    """A party from a module shaped like oracle/oracle.py (the oracle, or oracle/reference.py).  Returns (state, party)."""
    import hip_helpers as hh
    s = c.s
    if variant == "light":
        st, out = hh.oracle_forward(O, s, c.deg, **c.kw)
    else:
        assert not c.kw
        st, out, _ = hh.oracle_full(O, s, c.deg, backward=False)
    p = dict(out)
    for k in STATE:
        p[k] = st.get(k)
    if variant == "full":
        p["n_valid"] = st.get("n_valid_contrib")
    return st, p


def module_backward(O, st, c, alphas, grads, track_off, map_off):
    import hip_helpers as hh
    g = hh.oracle_backward(O, st, c.s, c.deg, alphas, track_off=track_off, map_off=map_off, grads=grads, **c.kw)
    return {k: np.asarray(g[k]) for k in GRADS}


def hip_forward(c, variant="light"):
    import hip_helpers as hh
    s = c.s
    if variant == "light":
        out, d = hh.hip_forward(s, c.deg, **c.kw)
    else:
        out, d = hh.hip_full_forward(s, c.deg)
    p = {k: v for k, v in d.items() if k not in ("geom", "binning", "img")}
    for k in STATE:
        p[k] = hh.hip_state(k, s, d)
    if variant == "full":
        p["n_valid"] = hh.hip_state("n_valid", s, d)
    return out, p


def hip_backward(out, c, alphas, grads, track_off, map_off):
    import hip_helpers as hh
    g = hh.hip_backward(c.s, c.deg, out, track_off=track_off, map_off=map_off, grads=grads, alphas=alphas, **c.kw)
    return {k: np.asarray(g[k]) for k in GRADS}


# ------------------------------------------------------------------------------------------ integer state
def ulps(a, b):
    """distance in float32 steps between same-sign finite values (depths are > 0.2)"""
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def compare_integer_state(ref, x, W, H, what, share=1.0):
    """radii, num_rendered, ranges and point_list of party `x` against the reference's.  A Gaussian whose radius differs is
    removed from both sides' lists; per tile the lists must then agree as sets, and as sequences except for swaps between
    entries whose REFERENCE depths are within 1 ulp of each other.  Caps (conditions, `share` of each: 0.5 for the seeds' CPU
    pre-check): radii differ on <= 1e-3 of the Gaussians and by <= 1; swapped positions <= 1e-3 of num_rendered.
    Returns namespace(radii_flips, swaps, flip [P] bool, tiles [T] bool: tiles some flip touches)."""
    P = len(ref["radii"])
    ra, rb = np.asarray(ref["radii"], np.int64), np.asarray(x["radii"], np.int64)
    assert ra.shape == rb.shape, f"{what}: radii shape"
    flip = ra != rb
    nflip = int(flip.sum())
    assert nflip <= share * CAP_RADII * P, f"{what}: radii differ on {nflip} of {P} Gaussians (cap {share * CAP_RADII * P:.1f})"
    assert nflip == 0 or np.abs(ra - rb)[flip].max() <= 1, f"{what}: a radius differs by {np.abs(ra - rb).max()}"
    R = int(ref["num_rendered"])
    ranges_a, ranges_b = np.asarray(ref["ranges"]).reshape(-1, 2), np.asarray(x["ranges"]).reshape(-1, 2)
    assert ranges_a.shape == ranges_b.shape, f"{what}: ranges shape"
    pla, plb = np.asarray(ref["point_list"], np.int64), np.asarray(x["point_list"], np.int64)
    if nflip == 0:
        assert int(x["num_rendered"]) == R, f"{what}: num_rendered {int(x['num_rendered'])} != {R}"
        assert np.array_equal(ranges_a, ranges_b), f"{what}: ranges differ"
    assert len(pla) == R and len(plb) == int(x["num_rendered"]), f"{what}: point_list length"
    depth = np.asarray(ref["depths"], np.float32)
    tiles = np.zeros(len(ranges_a), bool)
    swaps = 0
    if nflip == 0 and np.array_equal(pla, plb):
        return SimpleNamespace(radii_flips=0, swaps=0, flip=flip, tiles=tiles)
    for t, ((lo_a, hi_a), (lo_b, hi_b)) in enumerate(zip(ranges_a, ranges_b)):
        la, lb = pla[lo_a:hi_a], plb[lo_b:hi_b]
        if nflip:
            fa, fb = flip[la], flip[lb]
            if fa.any() or fb.any():
                tiles[t] = True
                la, lb = la[~fa], lb[~fb]
        if np.array_equal(la, lb):
            continue
        assert len(la) == len(lb) and np.array_equal(np.sort(la), np.sort(lb)), f"{what}: tile {t}: the lists differ as sets"
        bad = la != lb
        assert ulps(depth[la[bad]], depth[lb[bad]]).max() <= 1, \
            f"{what}: tile {t}: list order differs between entries whose reference depths are more than 1 ulp apart"
        swaps += int(bad.sum())
        tiles[t] = True
    assert swaps <= share * CAP_SWAPS * max(R, 1), f"{what}: {swaps} swapped list positions of {R} (cap {share * CAP_SWAPS * R:.1f})"
    return SimpleNamespace(radii_flips=nflip, swaps=swaps, flip=flip, tiles=tiles)


def tile_pixels(tiles, W, H):
    """[H, W] bool: the pixels of the marked tiles"""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    return np.kron(np.asarray(tiles, bool).reshape(gy, gx), np.ones((16, 16), bool))[:H, :W]


def flipped_pixels(ref, x, W, H, what, median_margin=None):
    """[H, W] bool through util.mask_flipped_pixels and its asserted bound: n_contrib differs (a flipped termination), or
    `median_margin` < 1e-5.  A flipped alpha test in the middle of a list is found by margin instead (forward64's `_ambiguous`,
    arbiter_flips): two float32 implementations of these scenes' longest lists part by 2e-5 of a pixel's depth through rounding
    alone, which an image criterion at 1e-5 would count as flips; one that stays unmasked fails the images' own rule."""
    ones = (np.ones((H, W), np.float32),)
    got, _ = mask_flipped_pixels(ones, ref["n_contrib"], x["n_contrib"], W, H, what, median_margin=median_margin)
    return np.asarray(got[0]) == 0


def arbiter_flips(ref, f64, images, W, H, what):
    """[H, W] bool: pixels on which the float64 formulation may decide a threshold otherwise than a float32 implementation.
    First by margin (forward64's `_ambiguous`), held to the 1e-3 of the pixels that the parties' own flips are granted.
    Then, as a net under it, by the images: a pixel off by more than float32 summation explains -- a float32 sum of n products
    of three factors is within (n + 3) 2^-24 of the exact one relative to the sum of magnitudes; twice that, and never less than
    1e-4 (the factors themselves, alpha above all, are measured up to ~1e-5 off) relative to max(1, |reference|) -- under
    mask_flipped_pixels' bound for image flips."""
    amb = np.asarray(f64["_ambiguous"], bool).reshape(H, W)
    assert int(amb.sum()) <= max(4, int(1e-3 * W * H)), f"{what}: {int(amb.sum())} of {W * H} pixels within the decision windows"
    nc = np.asarray(ref["n_contrib"], np.float64).reshape(H, W)
    tol = np.maximum(1e-4, 2.0 * (nc + 3.0) * 2.0 ** -24)
    bad = np.zeros((H, W), bool)
    for k in images:
        a, b = np.asarray(f64[k], np.float64).reshape(-1, H, W), np.asarray(ref[k], np.float64).reshape(-1, H, W)
        bad |= (np.abs(a - b) > tol * np.maximum(1.0, np.abs(b))).any(0)
    bad &= ~amb
    n = int(bad.sum())
    assert n <= max(2, int(3e-4 * W * H)), f"{what}: {n} of {W * H} pixels decided differently in float64, outside the windows"
    _log(f"{what:<48} masked by the arbiter: within the decision windows {int(amb.sum())}, off in an image {n}, of {W * H}")
    return bad | amb


def tainted_gaussians(f64, mask, P):
    """[P] bool: the Gaussians that can be the median Gaussian of a masked pixel on some side (forward64's `_band`).  The
    per-Gaussian forward sums -- gau_uncertainty, gau_related_pixels -- receive a pixel's term at its median Gaussian only, and
    cannot be compared on these: the sides include the masked pixels, possibly at different Gaussians."""
    out = np.zeros(P, bool)
    pix, gid = f64["_band"]
    out[gid[np.asarray(mask, bool).reshape(-1)[pix]]] = True
    return out


def compare_counts(ref, x, keep, what, name="gau_related_pixels"):
    a, b = np.asarray(ref[name]).reshape(-1)[keep], np.asarray(x[name]).reshape(-1)[keep]
    assert np.array_equal(a, b), f"{what}: {name} differs on {int((a != b).sum())} untouched entries"


# ------------------------------------------------------------------------------------------ the float64 arbiter
def scene64(c):
    """the scene as the float64 formulation takes it: scale_modifier folded into the scales (in float64)"""
    sm = c.kw.get("scale_modifier", 1.0)
    return c.s if sm == 1.0 else c.s._replace(scales=np.asarray(c.s.scales, np.float64) * sm)


ALPHA_WINDOW = 2e-5   # relative: a float32 alpha is measured up to ~1e-5 from the exact one (cancelling terms of the exponent)
T_WINDOW = 1e-5       # absolute, around 0.5 (mask_flipped_pixels' median margin)


def forward64(c, ref, variant="light"):
    """The forward in float64 on the reference's decisions, from fp64_model's building blocks: the images (full: colour, depth
    of the camera-space z, uncertainty = sum alpha T), the per-Gaussian preprocess outputs (rows of the visible Gaussians) and,
    for the light variant, the median depth by the FORWARD's criterion (T > 0.5 before, < 0.5 after, forward.cu:381) with
    gau_uncertainty and gau_related_pixels summed over those pixels.  `_ambiguous` [H, W]: pixels with a pair whose exact alpha
    is within ALPHA_WINDOW of 15/255, or (light) a transmittance within T_WINDOW of 0.5 -- there float64 and a float32
    implementation may decide differently, and neither is wrong."""
    s, deg = scene64(c), c.deg
    vis = np.asarray(ref["radii"]) > 0
    dec = (vis, ref["point_list"], ref["ranges"], ref["n_contrib"])
    cp, cv = c.kw.get("colors_precomp"), c.kw.get("cov3D_precomp")
    light = variant == "light"
    with torch.no_grad():
        leaves = M.make_leaves(s, cp, cv)
        view, persp, gt = M.f64(s.view), M.f64(s.persp), M.f64(s.gt)
        idx = torch.tensor(np.nonzero(vis)[0])
        m = leaves["means3D"][idx]
        mh = M.homogeneous(m)
        pix = M.pixels(mh @ (view @ persp), s.W, s.H)
        t = (mh @ view)[:, :3]
        z = t[:, 2]
        con = M.conic(s, t, M.covariance(leaves, idx), view[:3, :3].t())
        dirs = m - M.f64(s.campos)
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        rgb = M.sh_to_rgb(deg, leaves["shs"][idx], dirs) if cp is None else leaves["colors"][idx]
        opac = leaves["opacities"][idx, 0]
        color, depth, alpha, _, _ = M.blend(s, dec, pix, con, opac, rgb, z, z, median=False)
        med, amb = torch.zeros(s.H, s.W, dtype=torch.float64), torch.zeros(s.H, s.W, dtype=torch.bool)
        unc = torch.zeros(len(idx), dtype=torch.float64)
        cnt = torch.zeros(len(idx), dtype=torch.float64)
        thr = 15.0 / 255.0
        band_pix, band_gid = [], []
        for tl in M.tiles(s, *dec):
            power, a = M.alpha_of(tl, M.tile_xy(pix, tl), con, opac)
            offered = (power <= 0) & (tl.pos < tl.ncp)
            close = (offered & ((a - thr).abs() < ALPHA_WINDOW * thr)).any(0)
            if light:
                valid = M.valid_pairs(tl, power, a)
                w, Texcl, _ = M.blend_weights(torch.where(valid, a, torch.zeros_like(a)))
                Tincl = Texcl * (1.0 - a)
                close |= (valid & (((Texcl - 0.5).abs() < T_WINDOW) | ((Tincl - 0.5).abs() < T_WINDOW))).any(0)
                hit = valid & (Texcl > 0.5) & (Tincl < 0.5)       # at most one per pixel
                zt = z[tl.ids, None]
                M.put(med, tl, (hit * zt).sum(0))
                e = zt - gt[tl.sel].reshape(-1)[None]
                unc.index_add_(0, tl.ids, (hit * e * e * w).sum(1))
                cnt.index_add_(0, tl.ids, hit.sum(1).double())
            M.put(amb, tl, close)
            if light:   # who can be a pixel's median Gaussian on any side: its step from T before to T after reaches into 0.5 +- 0.1
                # (one flipped alpha at the threshold moves every later T by 6 %, 0.03 at the crossing)
                gi, pi = torch.nonzero(offered & (Texcl >= 0.4) & (Tincl <= 0.6), as_tuple=True)
                ys = torch.arange(tl.sel[0].start, tl.sel[0].stop).repeat_interleave(tl.hw[1])
                xs = torch.arange(tl.sel[1].start, tl.sel[1].stop).repeat(tl.hw[0])
                band_pix.append((ys[pi] * s.W + xs[pi]).numpy())
                band_gid.append(idx[tl.ids[gi]].numpy())
    P = s.P
    full = lambda v, w=1: _scatter(v.numpy().reshape(len(idx), w), idx.numpy(), P)  # noqa: E731
    out = dict(color=color.numpy(), depth=depth.numpy(), means2D=full(pix, 2), conic=full(torch.stack(con, 1), 3), depths=full(z),
               rgb=full(rgb, 3), _vis=vis, _ambiguous=amb.numpy())
    if light:
        out.update(opacity_map=alpha.numpy(), depth_median=med.numpy(), gau_uncertainty=full(unc), gau_related_pixels=full(cnt),
                   _band=(np.concatenate(band_pix) if band_pix else np.zeros(0, np.int64),
                          np.concatenate(band_gid) if band_gid else np.zeros(0, np.int64)))
    else:
        out.update(uncertainty=alpha.numpy())
    return out


def _scatter(rows, idx, P):
    out = np.zeros((P, rows.shape[1]))
    out[idx] = rows
    return out


def grads64(c, ref, grads, alphas=None, f64=None):
    """The gradients of the float64 formulation on the reference's decisions, keyed as GRADS (absent where the formulation has no
    such leaf); dL_dmeans2D in the reference's units (ndc: x W/2, y H/2, z = 0), dL_dview with entries 3, 7, 11, 15 zeroed
    (never written by the reference).  `alphas`: the alpha image the sides' backward is handed."""
    s, deg = scene64(c), c.deg
    vis = np.asarray(ref["radii"]) > 0
    cp, cv = c.kw.get("colors_precomp"), c.kw.get("cov3D_precomp")
    gC, gD, gM, gV = (np.asarray(g, np.float64) for g in grads)
    if alphas is not None:
        # The backward starts its transmittance chain from T_final = 1 - alpha IMAGE in float32 (backward.cu:477), and every term
        # of a pixel but the median's is linear in that chain (:570-623): handed an alpha image a relative d away from the exact
        # 1 - T_final, the reference computes the pixel's colour, depth and variance terms (1 + d) times the exact ones -- up to
        # 3e-4 on a nearly opaque pixel, from the image's rounding to float32 alone.  That is the interface's error, not a
        # side's: the float64 formulation takes it in through the pixel gradients.
        k = alpha_interface_factor(f64 if f64 is not None else forward64(c, ref), alphas)
        gC, gD, gV = gC * k, gD * k, gV * k
    loss, leaves, img = M.torch_light(s, deg, vis, ref["point_list"], ref["ranges"], ref["n_contrib"], (gC, gD, gM, gV), cp, cv)
    loss.backward()
    gv = (leaves["view_ndc"].grad + leaves["view_depth"].grad).numpy().copy().reshape(-1)
    gv[[3, 7, 11, 15]] = 0.0
    m2 = np.zeros((s.P, 3))
    m2[img["_idx"], :2] = img["_pix"].grad.numpy() * np.array([0.5 * s.W, 0.5 * s.H])
    g = dict(dL_dmeans2D=m2, dL_dopacity=leaves["opacities"].grad.numpy(), dL_dmeans3D=leaves["means3D"].grad.numpy(),
             dL_dview=gv.reshape(4, 4))
    if cp is None:
        g["dL_dsh"] = leaves["shs"].grad.numpy()
    else:
        g["dL_dcolors"] = leaves["colors"].grad.numpy()
    if cv is None:
        # the reference's dL_dscale is the derivative by the MODIFIED scale mod * s: computeCov3D's backward leaves the factor mod
        # out (L/cuda_rasterizer/backward.cu:297,324-327) -- which is what the gradient of the folded scales is
        g["dL_dscales"] = leaves["scales"].grad.numpy()
        g["dL_drotations"] = leaves["rotations"].grad.numpy()
    else:
        g["dL_dcov3D"] = leaves["cov3D"].grad.numpy()
    return g, img


# ------------------------------------------------------------------------------------------ distances
def image_distance(a, f64, keep=None):
    """max |a - f64| / max(1, |f64|) over the kept pixels ([.., H, W] arrays, keep [H, W])"""
    a, b = np.asarray(a, np.float64), np.asarray(f64, np.float64)
    d = np.abs(a.reshape(b.shape) - b) / np.maximum(1.0, np.abs(b))
    if keep is not None:
        d = d[..., keep]
    return float(d.max()) if d.size else 0.0


def rows_distance(a, f64, keep, plus_one=False):
    """per-Gaussian values: max |a - f64| / max(1, |f64|) (or 1 + |f64|) over the kept rows"""
    b = np.asarray(f64, np.float64)
    a = np.asarray(a, np.float64).reshape(b.shape)
    d = np.abs(a - b) / ((1.0 + np.abs(b)) if plus_one else np.maximum(1.0, np.abs(b)))
    d = d[keep]
    return float(d.max()) if d.size else 0.0


def scale_distance(a, f64):
    """max |a - f64| / max |f64|: the gradient tests' measure"""
    b = np.asarray(f64, np.float64)
    a = np.asarray(a, np.float64).reshape(b.shape)
    scale = np.abs(b).max()
    assert scale > 0
    return float(np.abs(a - b).max() / scale)


SANITY = 1e-3  # a wrong term, sign or slot in a gradient shows at >= 1e-3 of scale (tests/test_oracle_autograd.py)
MEASURED = []  # (case, tensor, e_ref, {party: e})


def judge(case, tensor, bar, e_ref, e_parties):
    """e_x <= max(2 e_ref, bar) for every party; the reference itself must stand within SANITY of the float64 formulation
    (else the formulation, not a party, is what the comparison would be measuring)."""
    MEASURED.append((case, tensor, e_ref, dict(e_parties)))
    line = f"{case:<22} {tensor:<22} e_ref {e_ref:9.2e}  " + "  ".join(f"e_{k} {v:9.2e}" for k, v in e_parties.items())
    _log(line)
    assert e_ref <= SANITY, f"{case} {tensor}: the reference is {e_ref:.2e} away from the float64 formulation"
    for k, e in e_parties.items():
        assert e <= max(2.0 * e_ref, bar), f"{case} {tensor}: {k} is {e:.2e} from float64; the reference {e_ref:.2e}, bar {bar:.0e}"


def _log(line):
    print(line)
    log = os.environ.get("DGR_REF_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


def log_flips(case, party, fl, n_contrib_flips, n_margin, npix_masked, npix):
    _log(f"{case:<22} flips vs reference  {party:<12} radii {fl.radii_flips}  swapped positions {fl.swaps}  n_contrib {n_contrib_flips}  "
         f"median margin {n_margin}  masked pixels {npix_masked} of {npix}")


# ------------------------------------------------------------------------------------------ the comparisons
def alpha_interface_factor(f64, alphas):
    """[H, W] float64: (1 - alphas in float32) / (the exact final transmittance) -- what the light backward's transmittance
    chain is scaled by when it is handed `alphas` (see grads64)."""
    a32 = np.asarray(alphas, np.float32).reshape(f64["opacity_map"].shape)
    return (np.float32(1.0) - a32).astype(np.float64) / (1.0 - f64["opacity_map"])


def compare_forward(c, ref, parties, variant="light", margin_fn=None, share=1.0):
    """Integer state of every party against the reference, then the real-valued forward results against float64.
    `parties`: {name: party}; `margin_fn(alphas)` -> [H, W] min_k |T_k - 0.5| of the backward's re-derived transmittances
    (oracle.light_median_margin on a float oracle state).  Returns (mask [H, W]: pixels some counted flip touches, for the
    backward; f64 dict)."""
    s = c.s
    W, H, P = s.W, s.H, s.P
    images = IMAGES_LIGHT if variant == "light" else IMAGES_FULL
    mask = np.zeros((H, W), bool)
    gflip = np.zeros(P, bool)
    f64 = forward64(c, ref, variant)
    median_margin = None
    if margin_fn is not None:
        # the sides re-derive T from the alpha image they are handed, the float64 formulation has the exact one: the two part by
        # the interface factor, so a T_k that close to 0.5 can pick another median Gaussian (on top of mask_flipped_pixels' 1e-5)
        alphas = arbiter_alphas(f64)
        median_margin = np.asarray(margin_fn(alphas), np.float64).reshape(H, W) - np.abs(alpha_interface_factor(f64, alphas) - 1.0)
    for name, x in parties.items():
        what = f"{variant} {c.name}: {name} vs reference"
        fl = compare_integer_state(ref, x, W, H, what, share)
        m = tile_pixels(fl.tiles, W, H) | flipped_pixels(ref, x, W, H, what, median_margin)
        n_nc = int((np.asarray(ref["n_contrib"]).reshape(-1) != np.asarray(x["n_contrib"]).reshape(-1)).sum())
        log_flips(f"{variant} {c.name}", name, fl, n_nc, 0 if median_margin is None else int((median_margin < 1e-5).sum()), int(m.sum()), W * H)
        mask |= m
        gflip |= fl.flip
    # the arbiter's own flips: float64 decides alpha >= 15/255 (and the median's T against 0.5) on exact values, the reference
    # on float32 ones -- such a pixel is off by a whole term in the float64 image; counted under the same bound
    mask |= arbiter_flips(ref, f64, images, W, H, f"{variant} {c.name}: float64 vs reference")
    keep = ~mask
    case = f"{variant} {c.name}"
    for k in images:
        judge(case, k, BAR_IMAGE, image_distance(ref[k], f64[k], keep), {n: image_distance(x[k], f64[k], keep) for n, x in parties.items()})
    for name, x in parties.items():
        what = f"{case}: {name}"
        assert np.array_equal(np.asarray(ref["n_contrib"]).reshape(H, W)[keep], np.asarray(x["n_contrib"]).reshape(H, W)[keep]), what
        if variant == "full":
            assert np.array_equal(np.asarray(ref["n_valid"]).reshape(H, W)[keep], np.asarray(x["n_valid"]).reshape(H, W)[keep]), what
            assert int(x["num_related"]) == int(np.asarray(x["n_valid"], np.int64).sum()), what
            if not mask.any():
                assert int(x["num_related"]) == int(ref["num_related"]), what
    if variant == "full":
        assert int(ref["num_related"]) == int(np.asarray(ref["n_valid"], np.int64).sum())
        return mask, f64
    assert not np.asarray(ref["depth_var"]).any() and all(not np.asarray(x["depth_var"]).any() for x in parties.values())
    rows = f64["_vis"] & ~gflip
    for k, mine, w in (("means2D", "means2D", 2), ("conic", "conic_opacity", 4), ("depths", "depths", 1), ("rgb", "rgb", 3)):
        if k == "rgb" and "colors_precomp" in c.kw:
            continue  # (the rgb field is not written)
        pick = lambda p: np.asarray(p[mine]).reshape(P, w)[:, :3 if k == "conic" else w]  # noqa: E731
        judge(case, k, BAR_IMAGE, rows_distance(pick(ref), f64[k], rows), {n: rows_distance(pick(x), f64[k], rows) for n, x in parties.items()})
    clean = rows & ~tainted_gaussians(f64, mask, P)
    _log(f"{case:<22} per-Gaussian forward sums compared on {int(clean.sum())} of {int(rows.sum())} visible Gaussians")
    assert clean.sum() >= 0.75 * rows.sum(), f"{case}: only {int(clean.sum())} of {int(rows.sum())} Gaussians left to compare"
    for name, x in parties.items():
        compare_counts(ref, x, clean, f"{case}: {name}")
    assert np.array_equal(np.asarray(ref["gau_related_pixels"]).reshape(-1)[clean], f64["gau_related_pixels"].reshape(-1)[clean].astype(np.int64)), \
        f"{case}: float64 median pixels differ from the reference's on untouched Gaussians"
    judge(case, "gau_uncertainty", BAR_UNCERTAINTY, rows_distance(ref["gau_uncertainty"], f64["gau_uncertainty"], clean, True),
          {n: rows_distance(x["gau_uncertainty"], f64["gau_uncertainty"], clean, True) for n, x in parties.items()})
    return mask, f64


def arbiter_alphas(f64):
    """The alpha image every side's backward is handed: the float64 one, rounded once.  The light backward recovers the final
    transmittance as T_final = 1 - alpha (L/cuda_rasterizer/backward.cu:477), which turns the few ulp of a float32 forward's
    alpha sum into up to 1e-3 of every gradient of a nearly opaque pixel (T_final ~ 1e-4) -- an error of the forward that the
    float64 gradients do not have and that would drown what the backward comparison is after.  Stage isolation, as in
    tests/test_oracle_autograd.py; the forwards' own alpha images are judged by compare_forward."""
    return np.asarray(f64["opacity_map"], np.float32)[None]


def masked(grads, mask):
    out = []
    for g in grads:
        g = np.array(g, dtype=np.float32, copy=True)
        g[..., mask] = 0.0
        out.append(g)
    return tuple(out)


def compare_backward(c, mode, g64, g_ref, g_parties):
    """One track_off / map_off mode: `g64` the float64 gradients (of the full backward; a mode only switches outputs off),
    `g_ref` / `g_parties` the reference's and the parties' GRADS dicts of that mode."""
    name, track_off, map_off = mode
    case = f"light {c.name} {name}"
    for k in GRADS:
        off = track_off if k == "dL_dview" else map_off
        if off:  # switched off: exactly zero, for everyone (L/cuda_rasterizer/backward.cu:593,609,633,654,666,683)
            assert not np.asarray(g_ref[k]).any(), f"{case}: the reference's {k} is not zero"
            for n, g in g_parties.items():
                assert not np.asarray(g[k]).any(), f"{case}: {n}'s {k} is not zero"
            continue
        if k == "dL_dview":
            for g in (g_ref, *g_parties.values()):
                assert not np.asarray(g[k]).reshape(-1)[[3, 7, 11, 15]].any(), case
        if k not in g64:
            # no leaf of the float64 formulation: with precomputed colours / covariances dL_dsh / dL_dscales and dL_drotations are
            # never written -- exactly zero on every side; otherwise dL_dcolors / dL_dcov3D are intermediates whose every
            # consumer (dL_dsh, dL_dscales, dL_drotations, dL_dmeans3D) is judged
            if not np.asarray(g_ref[k]).any():
                for n, g in g_parties.items():
                    assert not np.asarray(g[k]).any(), f"{case}: {n}'s {k} is not zero where the reference's is"
            continue
        judge(case, k, BAR_GRAD, scale_distance(g_ref[k], g64[k]), {n: scale_distance(g[k], g64[k]) for n, g in g_parties.items()})


CAP_END_TO_END = 2e-2   # of the pixels, see end_to_end_mask


def end_to_end_mask(c, f64, mask, margin_fn, alpha_images):
    """`mask` widened for the END-TO-END backward, in which every side starts from its OWN forward's alpha image: a float32
    alpha sum is a few ulp (~2e-7) off, which T_final = 1 - alpha turns into a relative d of up to 2e-3 on a nearly opaque pixel
    (T_final >= 1e-4), and every T_k the backward re-derives is off by that d.  A pixel with some T_k within 0.5 d of 0.5 may
    pick another median Gaussian than float64 does.  Blended alphas are >= 15/255, so the T_k near 0.5 are >= 0.03 apart: at
    most 2 x 1e-3 / 0.03 = 7 % of the nearly opaque pixels qualify, and a far smaller share of the others; 2 % of all pixels is
    the cap (the isolated comparison's own caps stay as they are)."""
    s = c.s
    m = np.array(mask, dtype=bool, copy=True)
    for a in alpha_images:
        close = np.asarray(margin_fn(a), np.float64).reshape(s.H, s.W) - np.abs(alpha_interface_factor(f64, a) - 1.0) < 1e-5
        m |= close
    extra = int((m & ~mask).sum())
    _log(f"light {c.name:<16} end to end: {extra} more pixels masked for the median's margin under the sides' own alpha images, of {s.W * s.H}")
    assert extra <= max(4, int(CAP_END_TO_END * s.W * s.H)), f"light {c.name}: {extra} pixels within the end-to-end median margin"
    return m


def compare_end_to_end(c, ref, f64, grads, g_ref, parties):
    """The mapping+pose backward with every side on its OWN forward's alpha image: `g_ref` the reference's gradients,
    `parties` {name: (gradients, alpha image)}.  Each side is measured against the float64 gradients that carry ITS alpha
    image's interface factor (grads64), and judged by the same rule as the isolated modes."""
    case = f"light {c.name} end-to-end"
    cache = {}

    def arbiter(alphas):
        key = np.asarray(alphas, np.float32).tobytes()
        if key not in cache:
            cache[key] = grads64(c, ref, grads, alphas, f64)[0]
        return cache[key]

    g64_ref = arbiter(ref["opacity_map"])
    for k in GRADS:
        if k in g64_ref:
            judge(case, k, BAR_GRAD, scale_distance(g_ref[k], g64_ref[k]),
                  {n: scale_distance(g[k], arbiter(a)[k]) for n, (g, a) in parties.items()})


# ------------------------------------------------------------------------------------------ recorded outputs of the reference
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
RECORDED_LIGHT = ("radii", "num_rendered", "ranges", "point_list", "n_contrib", "depths", "means2D", "conic_opacity", "rgb",
                  "color", "depth", "depth_median", "depth_var", "opacity_map", "gau_uncertainty", "gau_related_pixels")
RECORDED_FULL = ("radii", "num_rendered", "num_related", "ranges", "point_list", "n_contrib", "n_valid", "depths", "color", "depth",
                 "uncertainty")


def scene_hash(s):
    """identifies the inputs a recorded file belongs to (regenerated from the committed seed through dgr_amd.synth)"""
    import hashlib
    h = hashlib.sha256()
    for a in (s.view, s.proj, s.persp, s.campos, s.means, s.scales, s.rots, s.opac, s.shs, s.gt, s.bg, s.gC, s.gD, s.gM, s.gV):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def golden_path(variant, case, what):
    return os.path.join(GOLDEN_DIR, f"{variant}_{what}_{case[0].replace('golden_', '')}.npz" if variant == "full"
                        else f"{variant}_{case[0].replace('golden_', '')}_{what}.npz")


def recorded(variant, case, what, c):
    """one recorded file of the reference as a party dict, checked to belong to the inputs the committed seed gives"""
    z = np.load(golden_path(variant, case, what))
    assert str(z["scene_hash"]) == scene_hash(c.s), "the recorded outputs belong to other inputs than the committed seed gives"
    d = {k: z[k] for k in z.files}
    for k in ("num_rendered", "num_related"):
        if k in d:
            d[k] = int(d[k])
    return d


def oracle_parties(oracle, c, variant):
    """(float state, C-math state, {"oracle": .., "oracle_cmath": ..})"""
    oracle.use_cmath(True)
    try:
        st_c, oc = module_forward(oracle, c, variant)
    finally:
        oracle.use_cmath(False)
    st_f, of = module_forward(oracle, c, variant)
    return st_f, st_c, {"oracle": of, "oracle_cmath": oc}
