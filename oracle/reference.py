"""ctypes front-end of the reference rasterizer's own source, compiled for gfx950 by oracle/build_ref.py into
oracle/_ref/libdgr_ref_{light,full}.so (through the C wrapper oracle/ref_capi.hip).  Needs a GPU.

TEST INFRASTRUCTURE ONLY.  Shaped like oracle/oracle.py -- light_forward / light_backward / full_forward with the same argument
lists, a state object with .get(name) -- so that tests/hip_helpers.oracle_forward / oracle_backward take this module in place of
the oracle.  Same statements as the reference, not the same compiler or libm as an NVIDIA build.

Never given to the reference (the wrapper refuses the first two, the callers see to the rest): prefiltered = True (in_frustum
would trap), P = 0 (forward reads point_offsets[P - 1]), a frame with no rendered instance, anything NaN.  The full variant's
backward is not built into an entry point: ComputePG returns ahead of block-wide barriers.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBS = {}
BUILD_STEP = "python oracle/build_ref.py  (needs the reference checkout: $DGR_REFERENCE_DIR, default ../reference)"


def library_path(variant):
    return os.path.join(_HERE, "_ref", f"libdgr_ref_{variant}.so")


def available(variant=None):
    return all(os.path.exists(library_path(v)) for v in ([variant] if variant else ["light", "full"]))


def lib(variant):
    """Both variants define CudaRasterizer::*: each library is loaded RTLD_LOCAL."""
    if variant not in _LIBS:
        path = library_path(variant)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing: build it with  {BUILD_STEP}")
        import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch has mapped, as dgr_amd._capi does)
        l = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
        l.dgr_ref_variant.restype = C.c_char_p
        assert l.dgr_ref_variant() == variant.encode()
        l.dgr_ref_state_new.restype = C.c_void_p
        l.dgr_ref_state_free.argtypes = [C.c_void_p]
        l.dgr_ref_state_num_rendered.argtypes = [C.c_void_p]
        l.dgr_ref_state_get.restype = C.c_long
        l.dgr_ref_state_get.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_long]
        _LIBS[variant] = l
    return _LIBS[variant]


_DTYPES = {  # name -> (dtype, elements as a function of (P, R, tiles, N))
    "radii": (np.int32, lambda P, R, T, N: P), "depths": (np.float32, lambda P, R, T, N: P),
    "means2D": (np.float32, lambda P, R, T, N: 2 * P), "conic_opacity": (np.float32, lambda P, R, T, N: 4 * P),
    "rgb": (np.float32, lambda P, R, T, N: 3 * P), "clamped": (np.uint8, lambda P, R, T, N: 3 * P),
    "cov3D": (np.float32, lambda P, R, T, N: 6 * P), "tiles_touched": (np.uint32, lambda P, R, T, N: P),
    "point_offsets": (np.uint32, lambda P, R, T, N: P), "point_list": (np.uint32, lambda P, R, T, N: R),
    "keys": (np.uint64, lambda P, R, T, N: R), "point_list_keys": (np.uint64, lambda P, R, T, N: R),
    "ranges": (np.uint32, lambda P, R, T, N: 2 * T), "n_contrib": (np.uint32, lambda P, R, T, N: N),
    "accum_alpha": (np.float32, lambda P, R, T, N: N), "n_valid_contrib": (np.uint32, lambda P, R, T, N: N),
}


def _check(rc, what):
    if rc != 0:
        refused = {-1: "prefiltered = True is never given to the reference", -2: "P = 0 is never given to the reference",
                   -3: "the reference threw", -4: "backward without a matching forward, or of a frame with no instance"}
        raise RuntimeError(f"reference {what}: " + refused.get(rc, f"HIP error {rc}"))


class ReferenceState:
    """The Geometry / Binning / Image buffers of one forward call of the reference, on the device; .get copies a field out."""

    def __init__(self, variant, P, W, H):
        self.variant = variant
        self._l = lib(variant)
        self._h = C.c_void_p(self._l.dgr_ref_state_new())
        self._P, self._W, self._H = P, W, H
        self.radii = None

    def __del__(self):
        if getattr(self, "_h", None):
            self._l.dgr_ref_state_free(self._h)
            self._h = None

    @property
    def num_rendered(self):
        return self._l.dgr_ref_state_num_rendered(self._h)

    def get(self, name):
        if name not in _DTYPES:
            raise KeyError(name)
        dt, count = _DTYPES[name]
        tiles = ((self._W + 15) // 16) * ((self._H + 15) // 16)
        n = count(self._P, max(self.num_rendered, 0), tiles, self._W * self._H)
        out = np.zeros(max(n, 1), dt)
        got = self._l.dgr_ref_state_get(self._h, name.encode(), C.c_void_p(out.ctypes.data), out.nbytes)
        if got == -1:
            raise KeyError(name)
        if got != n:
            raise RuntimeError(f"reference state '{name}': expected {n} elements, got {got}")
        return out[:n]


def _f(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    if a is None or a.size == 0:
        return C.c_void_p(None)
    assert a.flags["C_CONTIGUOUS"]
    return C.c_void_p(a.ctypes.data)


def _finite(*arrays):
    for a in arrays:
        if a is not None and not np.all(np.isfinite(a)):
            raise ValueError("the reference is never given anything NaN / infinite")


def _inputs(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos):
    a = [_f(x) for x in (means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos)]
    _finite(*a)
    P = a[0].shape[0]
    M = a[1].shape[1] if a[1] is not None and a[1].size else 0
    return (P, M, *a)


def _forward(variant, bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
             gt_depth, projmatrix, tanfovx, tanfovy, H, W, shs, sh_degree, campos, prefiltered):
    (P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix,
     campos) = _inputs(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos)
    bg, gt_depth = _f(bg), _f(gt_depth)
    _finite(bg, gt_depth)
    assert gt_depth.size == W * H and opacities.size == P
    st = ReferenceState(variant, P, W, H)
    R, NG = C.c_int(0), C.c_int(0)
    head = (st._h, P, sh_degree, M, _p(bg), W, H, _p(means3D), _p(shs), _p(colors_precomp), _p(opacities), _p(scales),
            C.c_float(scale_modifier), _p(rotations), _p(cov3D_precomp), _p(viewmatrix), _p(projmatrix), _p(campos),
            C.c_float(tanfovx), C.c_float(tanfovy), int(bool(prefiltered)))
    if variant == "light":
        out = dict(color=np.zeros((3, H, W), np.float32), depth=np.zeros((1, H, W), np.float32),
                   depth_median=np.zeros((1, H, W), np.float32), depth_var=np.zeros((1, H, W), np.float32),
                   opacity_map=np.zeros((1, H, W), np.float32), radii=np.zeros(P, np.int32),
                   gau_uncertainty=np.zeros((P, 1), np.float32), gau_related_pixels=np.zeros((P, 1), np.int32))
        rc = st._l.dgr_ref_forward(*head, _p(out["color"]), _p(out["depth"]), _p(out["depth_median"]), _p(out["opacity_map"]),
                                   _p(gt_depth), _p(out["depth_var"]), _p(out["gau_uncertainty"]), _p(out["gau_related_pixels"]),
                                   _p(out["radii"]), C.byref(R))
    else:
        out = dict(color=np.zeros((3, H, W), np.float32), depth=np.zeros((1, H, W), np.float32),
                   uncertainty=np.zeros((1, H, W), np.float32), radii=np.zeros(P, np.int32))
        rc = st._l.dgr_ref_forward(*head, _p(out["color"]), _p(out["depth"]), _p(gt_depth), _p(out["uncertainty"]),
                                   _p(out["radii"]), C.byref(R), C.byref(NG))
        out["num_related"] = NG.value
    _check(rc, f"{variant} forward")
    out["num_rendered"] = R.value
    st.radii = out["radii"].copy()
    return st, out


def light_forward(bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, gt_depth,
                  projmatrix, tanfovx, tanfovy, H, W, shs, sh_degree, campos, prefiltered=False):
    """Argument order of oracle.light_forward.  Returns (state, dict)."""
    return _forward("light", bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                    gt_depth, projmatrix, tanfovx, tanfovy, H, W, shs, sh_degree, campos, prefiltered)


def full_forward(bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, gt_depth,
                 projmatrix, tanfovx, tanfovy, H, W, shs, sh_degree, campos, prefiltered=False):
    """Argument order of oracle.full_forward.  Returns (state, dict)."""
    return _forward("full", bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                    gt_depth, projmatrix, tanfovx, tanfovy, H, W, shs, sh_degree, campos, prefiltered)


def light_backward(st, bg, means3D, colors_precomp, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                   tanfovx, tanfovy, dL_dcolor, dL_ddepth, dL_dmedian, dL_dvar, gt_depth, shs, sh_degree, campos, alphas,
                   perspec_matrix, track_off=False, map_off=False, per_pixel_pose=False):
    """Argument order of oracle.light_backward.  dL_dview is the per-pixel [H W, 4, 4] array summed over the pixels here (in
    float64, rounded once), as the reference's __init__.py sums it."""
    assert st.variant == "light"
    (P, M, means3D, shs, colors_precomp, _, scales, rotations, cov3D_precomp, viewmatrix, projmatrix,
     campos) = _inputs(means3D, shs, colors_precomp, None, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos)
    W, H = st._W, st._H
    imgs = [_f(x) for x in (dL_dcolor, dL_ddepth, dL_dmedian, dL_dvar, gt_depth, alphas)]
    bg, persp = _f(bg), _f(perspec_matrix)
    _finite(bg, persp, *imgs)
    assert imgs[0].size == 3 * W * H and all(x.size == W * H for x in imgs[1:]) and persp.size == 16 and P == st._P
    g = dict(dL_dmeans2D=np.zeros((P, 3), np.float32), dL_dcolors=np.zeros((P, 3), np.float32),
             dL_ddepths=np.zeros((P, 1), np.float32), dL_dconic=np.zeros((P, 2, 2), np.float32),
             dL_dopacity=np.zeros((P, 1), np.float32), dL_dmeans3D=np.zeros((P, 3), np.float32),
             dL_dcov3D=np.zeros((P, 6), np.float32), dL_dsh=np.zeros((P, M, 3), np.float32),
             dL_dscales=np.zeros((P, 3), np.float32), dL_drotations=np.zeros((P, 4), np.float32))
    pix = np.zeros((H * W, 4, 4), np.float32)
    rc = st._l.dgr_ref_backward(
        st._h, P, sh_degree, M, st.num_rendered, _p(bg), W, H, _p(means3D), _p(shs), _p(colors_precomp), _p(imgs[5]), _p(scales),
        C.c_float(scale_modifier), _p(rotations), _p(cov3D_precomp), _p(viewmatrix), _p(projmatrix), _p(campos),
        C.c_float(tanfovx), C.c_float(tanfovy), _p(st.radii), _p(imgs[0]), _p(imgs[1]), _p(imgs[2]), _p(imgs[3]),
        _p(g["dL_dmeans2D"]), _p(g["dL_dconic"]), _p(g["dL_dopacity"]), _p(g["dL_dcolors"]), _p(g["dL_ddepths"]),
        _p(g["dL_dmeans3D"]), _p(g["dL_dcov3D"]), _p(g["dL_dsh"]), _p(g["dL_dscales"]), _p(g["dL_drotations"]), _p(persp), _p(pix),
        _p(imgs[4]), int(bool(track_off)), int(bool(map_off)))
    _check(rc, "light backward")
    g["dL_dview"] = pix.sum(axis=0, dtype=np.float64).astype(np.float32)
    if per_pixel_pose:
        g["dL_dview_pix"] = pix
    return g
