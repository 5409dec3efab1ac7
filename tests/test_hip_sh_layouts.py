"""Every storage layout of the SH tensor, on every kernel family that reads or writes it.

`make_scene` hands out `shs` as a fresh, 256-byte aligned [P, 16, 3] array, so the other GPU tests run the `M == 16`, aligned
branches of csrc/gaussian_math.h (load_sh), csrc/preprocess_fwd.hip and csrc/preprocess_bwd.hip only.  Here the row width M, the
degree D, the alignment of `shs` and of `dL_dsh`, and the contiguity of the autograd leaf vary: a degree-0 SLAM model is
[P, 1, 3], a model trained at max_sh_degree 1 or 2 is [P, 4, 3] or [P, 9, 3].  include/dgr_hip.h states the contract: any M >= 1,
coefficients beyond M count as zero (so D may exceed the degree M holds: the "clipped" layouts), coefficients beyond 16 get zero
gradient.

Three references per layout:
  * the oracle run at the layout itself, with the bars of tests/test_hip_light_parity.py (not for the clipped layouts: the oracle,
    as the reference, reads (D + 1)^2 coefficients per row, past the end of a narrower one);
  * the float64 model of tests/fp64_model.py on the rows zero-padded to 16, with the bars tests/test_hip_silhouette.py and
    tests/test_hip_complete_pose.py hold the same leaves to (2e-4 of scale for the SH gradient, 5e-5 for the others);
  * the HIP run of the zero-padded, aligned [P, 16, 3] scene: the per-Gaussian arithmetic is the same on every path, only the
    loads and stores differ, so every output and -- under deterministic_grads -- every gradient carries the same bits.

P = 255, 256, 300: the tail block only, exactly one whole 256-row block, a whole block and a tail.  The DC coefficients are
multiplied by 4 so that 16 .. 20 % of the (Gaussian, channel) colours fall below zero and the backward's clamp mask takes part
(as drawn, under 0.5 % do, none at M = 1); every case asserts its share on the host before anything runs on the GPU."""
import functools

import numpy as np
import pytest
import torch

import fp64_model as M64
import hip_helpers as hh
import test_hip_batch as TB
import test_hip_full_batch as TFB
from dgr_amd import _capi, slam
from dgr_amd import light as L
from dgr_amd.multiview import GradientArena, make_settings
from hip_helpers import binding  # noqa: F401  (fixture)
from test_hip_light_parity import IMAGES, assert_images_carry_the_references_bits, check_backward
from util import assert_grad_close, make_scene, mask_flipped_pixels

pytestmark = pytest.mark.gpu

W, H, SEED = 64, 48, 31
FILL = 7.0  # what rows 16 .. M - 1 of a wide layout hold: nothing may read them
LAYOUTS = [(1, 0), (4, 0), (4, 1), (9, 1), (9, 2), (16, 3), (25, 3), (1, 3), (4, 3), (9, 3)]  # (M, D)
CLIPPED = {(1, 3), (4, 3), (9, 3)}  # D asks for more coefficients than a row holds
EVERY_SIZE = [(1, 0), (9, 2), (16, 3)]
LIGHT_CASES = [(300, M, D) for M, D in LAYOUTS] + [(P, M, D) for P in (255, 256) for M, D in EVERY_SIZE]
FAMILY_LAYOUTS = [(1, 0), (9, 2), "misaligned"]  # the other kernel families: two narrow layouts and 4-byte aligned 16-wide rows
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731


def case_id(case):
    return case if isinstance(case, str) else "-".join(str(x) for x in case)


# ------------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def base_scene(P, view_index=0, behind=False):
    """make_scene with the DC coefficients times 4; `behind`: every tenth Gaussian mirrored through the camera centre, which puts
    it behind the camera (rows no view maps)"""
    s = make_scene(P, W, H, SEED, view_index=view_index)
    shs = s.shs.copy()
    shs[:, 0, :] *= 4
    means = s.means
    if behind:
        means = means.copy()
        rows = unmapped_rows(P)
        means[rows] = (2.0 * s.campos[None] - means[rows]).astype(np.float32)
    return s._replace(shs=shs, means=means)


def unmapped_rows(P):
    return np.arange(P) % 10 == 3


def as_layout(s, M):
    """the scene with its SH rows stored M wide, contiguous; rows 16 .. M - 1 hold FILL"""
    w = min(M, 16)
    shs = np.full((s.P, M, 3), FILL, np.float32)
    shs[:, :w] = s.shs[:, :w]
    return s._replace(shs=shs)


def as_padded(s, M):
    """the canonical form of the same scene: [P, 16, 3], zeros from coefficient M on"""
    w = min(M, 16)
    shs = np.zeros((s.P, 16, 3), np.float32)
    shs[:, :w] = s.shs[:, :w]
    return s._replace(shs=shs)


def clamped_share(padded, D):
    """the share of (Gaussian, channel) colours that the forward clamps at zero, in float64"""
    dirs = padded.means.astype(np.float64) - padded.campos.astype(np.float64)[None]
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return float((M64.sh_to_rgb(D, M64.f64(padded.shs), M64.f64(dirs), clamp=False) < 0).double().mean())


def scenes_of(P, M, D, **kw):
    """(layout scene, padded scene) of a case, once the clamp is known to take part in it"""
    base = base_scene(P, **kw)
    sl, sp = as_layout(base, M), as_padded(base, M)
    share = clamped_share(sp, D)
    print(f"\n[P={P} M={M} D={D}] clamped share of the colours: {share:.3f}")
    assert 0.05 <= share <= 0.5, (P, M, D, share)
    assert sl.shs.shape == (P, M, 3) and sl.shs.flags["C_CONTIGUOUS"]
    return sl, sp


def off_by_one_float(a):
    """a contiguous device tensor of `a`'s values that starts one float into a larger buffer: 4-byte aligned only"""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=hh.dev())
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def family_scenes(layout, view_index=0):
    """(the scene for the oracle, the scene for the HIP side, M, D) of one of FAMILY_LAYOUTS"""
    if layout == "misaligned":
        s = base_scene(300, view_index)
        return s, s._replace(shs=off_by_one_float(s.shs)), 16, 3
    M, D = layout
    s = scenes_of(300, M, D, view_index=view_index)[0]
    return s, s, M, D


def pixel_grads(s):
    return tuple(g * (s.W * s.H) ** 0.5 for g in (s.gC, s.gD, s.gM, s.gV))  # as check_backward scales them: pixel sums of O(1)


# ------------------------------------------------------------------------------------------ the three references
def against_the_oracle(oracle, sl, D, M, hip_scene=None, **mode):
    d, st, ref = check_backward(oracle, sl, D, hip_scene=hip_scene, what=f"light M={M} D={D} P={sl.P}", **mode)
    assert_images_carry_the_references_bits(d, st, ref, sl)
    assert np.array_equal(d["radii"], ref["radii"]) and d["num_rendered"] == ref["num_rendered"]
    assert np.array_equal(hh.hip_state("point_list", sl, d), st.get("point_list"))


@pytest.fixture(scope="module")
def fp64_reference(oracle):
    """(P, M, D) -> the float64 gradients of the zero-padded scene, computed once: dL_dsh, dL_dmeans3D and dL_dopacity of
    torch_light, the complete dL_dview of complete_forward (option "pose_grad" = 1), on the oracle's decisions"""
    known = {}

    def reference(P, M, D):
        if (P, M, D) not in known:
            sp = as_padded(base_scene(P), M)
            g64 = [np.asarray(g, np.float64) for g in pixel_grads(sp)]
            st, ref = hh.oracle_forward(oracle, sp, D)
            decisions = (ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"))
            loss, leaves, img = M64.torch_light(sp, D, *decisions, g64)
            loss.backward()
            for k in ("color", "depth", "opacity_map"):  # (the decisions are the oracle's: so are the images)
                assert np.abs(img[k] - ref[k].reshape(img[k].shape)).max() <= 2e-5, k
            view = M64.complete_grad(sp, "light", D, st, ref, g64)[0]
            known[P, M, D] = dict(radii=ref["radii"], dL_dsh=leaves["shs"].grad.numpy(), dL_dmeans3D=leaves["means3D"].grad.numpy(),
                                  dL_dopacity=leaves["opacities"].grad.numpy(), dL_dview=view)
        return known[P, M, D]
    return reference


def within(got, want, what, tol):  # tests/test_hip_silhouette.py: check
    scale = np.abs(want).max()
    assert scale > 0, what
    err = np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max() / scale
    print(f"[{what}] {err:.2e} of the tensor's scale (bar {tol:.0e})")
    assert err <= tol, f"{what}: {err:.2e} of the tensor's scale"


def against_fp64(want, sl, D, M, hip_scene=None):
    what = f"fp64 M={M} D={D} P={sl.P}"
    s = sl if hip_scene is None else hip_scene
    grads = pixel_grads(sl)
    out, d = hh.hip_forward(s, D)
    assert np.array_equal(d["radii"], want["radii"])
    g = hh.hip_backward(s, D, out, grads=grads)
    w = min(M, 16)
    assert g["dL_dsh"].shape == (sl.P, M, 3)
    within(g["dL_dsh"][:, :w], want["dL_dsh"][:, :w], f"{what} dL_dsh", 2e-4)
    within(g["dL_dmeans3D"], want["dL_dmeans3D"], f"{what} dL_dmeans3D", 5e-5)
    within(g["dL_dopacity"], want["dL_dopacity"], f"{what} dL_dopacity", 5e-5)
    with _capi.thread_options(pose_grad=1):
        out, _ = hh.hip_forward(s, D)
        g = hh.hip_backward(s, D, out, grads=grads)
    view = np.asarray(g["dL_dview"], np.float64).reshape(-1).copy()
    view[[3, 7, 11, 15]] = 0.0
    within(view, want["dL_dview"], f"{what} dL_dview (pose_grad = 1)", 5e-5)


FORWARD_OUTPUTS = ("color", "depth", "depth_median", "opacity_map", "radii")
FORWARD_STATE = ("n_contrib", "point_list")


def deterministic_run(s, D, grads):
    with _capi.thread_options(deterministic_grads=1):
        out, d = hh.hip_forward(s, D)
        g = hh.hip_backward(s, D, out, grads=grads)
    for name in FORWARD_STATE:
        d[name] = hh.hip_state(name, s, d)
    return d, g


def same_bits_as_the_canonical_layout(sl, sp, D, M, hip_scene=None, run=deterministic_run):
    what = f"M={M} D={D} P={sl.P}"
    grads = pixel_grads(sl)
    d, g = run(sl if hip_scene is None else hip_scene, D, grads)
    dc, gc = run(sp, D, grads)
    assert d["num_rendered"] == dc["num_rendered"], what
    for name in FORWARD_OUTPUTS + FORWARD_STATE:
        assert np.array_equal(d[name].view(np.uint8), dc[name].view(np.uint8)), (what, name)
    w = min(M, 16)
    assert g["dL_dsh"].shape == (sl.P, M, 3) and gc["dL_dsh"].shape == (sl.P, 16, 3)
    assert np.abs(g["dL_dsh"][:, :w]).max() > 0
    for name in hh.GRAD_NAMES:
        a, b = (g[name][:, :w], gc[name][:, :w]) if name == "dL_dsh" else (g[name], gc[name])
        assert np.array_equal(bits(a), bits(b)), (what, name, float(np.abs(a.astype(np.float64) - b).max()))
    assert not g["dL_dsh"][:, 16:].any(), what  # coefficients the SH basis does not have: zero gradient, mapped rows included
    return g


# ------------------------------------------------------------------------------------------ light, one view
@pytest.mark.parametrize("case", [c for c in LIGHT_CASES if c[1:] not in CLIPPED], ids=case_id)
def test_light_layout_against_the_oracle(oracle, case):
    """The oracle at the same (M, D, shs): what tests/test_hip_light_parity.py holds for [P, 16, 3], bar for bar.  The clipped
    layouts are left out here and only here: the oracle (as the reference) would read past the end of their rows."""
    P, M, D = case
    sl, _ = scenes_of(P, M, D)
    against_the_oracle(oracle, sl, D, M)


@pytest.mark.parametrize("case", LIGHT_CASES, ids=case_id)
def test_light_layout_against_fp64(fp64_reference, case):
    P, M, D = case
    sl, _ = scenes_of(P, M, D)
    against_fp64(fp64_reference(P, M, D), sl, D, M)


@pytest.mark.parametrize("case", LIGHT_CASES, ids=case_id)
def test_light_layout_carries_the_canonical_layouts_bits(case):
    P, M, D = case
    sl, sp = scenes_of(P, M, D)
    same_bits_as_the_canonical_layout(sl, sp, D, M)


def test_light_sh_rows_four_byte_aligned(oracle, fp64_reference):
    """`shs` [300, 16, 3] one float into a larger buffer: no 16-byte loads in the forward, no LDS or 16-byte stores of dL_dsh"""
    s = base_scene(300)
    share = clamped_share(s, 3)
    print(f"\n[misaligned shs] clamped share of the colours: {share:.3f}")
    assert 0.05 <= share <= 0.5
    hip_scene = s._replace(shs=off_by_one_float(s.shs))
    against_the_oracle(oracle, s, 3, 16, hip_scene=hip_scene)
    against_fp64(fp64_reference(300, 16, 3), s, 3, 16, hip_scene=hip_scene)
    same_bits_as_the_canonical_layout(s, s, 3, 16, hip_scene=hip_scene)


def test_light_dL_dsh_four_byte_aligned(oracle, monkeypatch):
    """`dL_dsh` one float off while `shs` is aligned: the forward takes its 16-byte loads, the backward may not take its 16-byte
    stores.  Through the ctypes binding only, whose gradient arena Python lays out (the `sh` segment is moved one float into a
    buffer of its own, filled with NaN); the compiled binding carves its arena in C++ and offers no way to place it."""
    placed = []
    real_arena = L._grad_arena

    def arena(P, M, f32):
        seg = real_arena(P, M, f32)
        buf = torch.full((3 * P * M + 1,), float("nan"), **f32)
        seg["sh"] = buf[1:].view(P, M, 3)
        placed.append(seg["sh"].data_ptr() % 16)
        return seg

    monkeypatch.setattr(L, "_C", L._CtypesC)
    monkeypatch.setattr(L, "_grad_arena", arena)
    s = base_scene(300)
    against_the_oracle(oracle, s, 3, 16)
    n = len(placed)
    assert n >= 2 and set(placed) == {4}

    def run(scene, D, grads):  # the canonical run: with the arena as the library lays it out
        if scene is s:
            return deterministic_run(scene, D, grads)
        with monkeypatch.context() as m:
            m.setattr(L, "_grad_arena", real_arena)
            return deterministic_run(scene, D, grads)

    canonical = as_padded(s, 16)
    assert canonical is not s
    same_bits_as_the_canonical_layout(s, canonical, 3, 16, run=run)
    assert len(placed) == n + 1


@pytest.mark.parametrize("layout", LAYOUTS + ["misaligned"], ids=case_id)
def test_rows_no_view_maps_get_zero_sh_gradient(binding, monkeypatch, layout):
    """A tenth of the Gaussians stands behind the camera: their dL_dsh rows are exactly zero -- each store of the mapped rows has a
    zero-row twin -- and nothing of the arena's SH segment stays unwritten (NaN beforehand where Python owns the arena: ctypes)."""
    P = 300
    base = base_scene(P, behind=True)
    if layout == "misaligned":
        M, D = 16, 3
        s = base._replace(shs=off_by_one_float(base.shs))
    else:
        M, D = layout
        s = as_layout(base, M)
    filled = []
    if binding == "ctypes":
        real_arena = L._grad_arena

        def arena(P, M, f32):
            seg = real_arena(P, M, f32)
            seg["sh"]._base.fill_(float("nan"))
            filled.append(M)
            return seg
        monkeypatch.setattr(L, "_grad_arena", arena)
    out, d = hh.hip_forward(s, D)
    g = hh.hip_backward(s, D, out, grads=pixel_grads(base))
    assert filled == ([M] if binding == "ctypes" else [])
    unmapped = d["radii"] == 0
    assert unmapped[unmapped_rows(P)].all() and 0.1 * P <= unmapped.sum() < 0.5 * P
    assert g["dL_dsh"].shape == (P, M, 3)
    for name in ("dL_dsh", "dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dcov3D"):
        assert np.isfinite(g[name]).all(), name
        assert not g[name][unmapped].any(), name
    assert np.abs(g["dL_dsh"][~unmapped][:, :min(M, 16)]).max() > 0
    assert not g["dL_dsh"][:, 16:].any()


@pytest.mark.parametrize("mode", ["map_off", "track_off"])
@pytest.mark.parametrize("layout", FAMILY_LAYOUTS, ids=case_id)
def test_light_modes(oracle, layout, mode):
    s, hip_scene, M, D = family_scenes(layout)
    against_the_oracle(oracle, s, D, M, hip_scene=hip_scene, **{mode: True})


# ------------------------------------------------------------------------------------------ the other kernel families
FULL_TOL = dict(rel_to_max=1e-5, elem_rtol=2e-3, elem_frac=1e-3)  # tests/test_hip_full_parity.py: test_full_backward


def full_forward_matches(d, st, ref, s, what):  # tests/test_hip_full_parity.py: test_full_forward
    assert np.array_equal(d["radii"], ref["radii"]) and d["num_rendered"] == ref["num_rendered"], what
    assert np.array_equal(hh.hip_state("point_list", s, d), st.get("point_list")), what
    assert np.array_equal(d["uncertainty"], ref["uncertainty"]), what
    for k in ("color", "depth"):
        a, b = d[k].astype(np.float64), ref[k].astype(np.float64)
        assert np.all(np.abs(a - b) <= 1e-6 * np.maximum(1.0, np.abs(b))), (what, k, float(np.abs(a - b).max()))
    assert np.array_equal(hh.hip_state("n_contrib", s, d), st.get("n_contrib")), what
    assert np.array_equal(hh.hip_state("n_valid", s, d), st.get("n_valid_contrib")), what
    assert d["num_related"] == ref["num_related"], what
    assert np.array_equal(hh.hip_state("final_T", s, d).view(np.float32), st.get("final_T")), what


@pytest.mark.parametrize("layout", FAMILY_LAYOUTS, ids=case_id)
def test_full_variant(oracle, layout):
    """The full variant, one view, with the bars of tests/test_hip_full_parity.py: its dgc_dCampos term reads the SH direction
    derivatives the forward kept, formed from the row as load_sh delivered it."""
    s, hip_scene, M, D = family_scenes(layout)
    grads = tuple(g * (W * H) ** 0.5 for g in (s.gC, s.gD, s.gV))
    out, d = hh.hip_full_forward(hip_scene, D)
    g = hh.hip_full_backward(hip_scene, D, out, grads=grads)
    st, ref, gr = hh.oracle_full(oracle, s, D, grads=grads)
    full_forward_matches(d, st, ref, s, f"full {layout}")
    assert g["dL_dsh"].shape == (s.P, M, 3)
    for k in ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"):
        assert g[k].shape == gr[k].shape, k
        assert_grad_close(g[k], gr[k], k, **FULL_TOL)
    assert g["dL_dview"].shape == (4, 4) and not g["dL_dview"].reshape(-1)[[3, 7, 11, 15]].any()
    assert_grad_close(g["dL_dview"], gr["dL_dview"], "dL_dview", rel_to_max=FULL_TOL["rel_to_max"] * 5, elem_rtol=5e-3, elem_frac=0.1)


@pytest.mark.parametrize("layout", FAMILY_LAYOUTS, ids=case_id)
def test_light_batch(oracle, binding, layout):
    """Three views in one call (the batch kernel's `e < 3 M` store of the summed dL_dsh): every view bit-identical to its one-view
    call, the summed gradients against the sum of the oracle's per-view passes and against the one-view backward accumulated in
    view order, with the bars of tests/test_hip_batch.py."""
    V = 3
    pairs = [family_scenes(layout, v)[:2] for v in range(V)]
    M, D = family_scenes(layout)[2:]
    if layout == "misaligned":  # one SH tensor for the batch and its one-view calls
        pairs = [(s, hs._replace(shs=pairs[0][1].shs)) for s, hs in pairs]
    ss, hs = [p[0] for p in pairs], [p[1] for p in pairs]
    out, cams = TB.batch_forward(hs, D)
    grads, alphas, ref_sum, ref_view, ref_m2d = [], [], None, [], []
    for v, s in enumerate(ss):
        one, d1 = hh.hip_forward(hs[v], D)
        ov = TB.one_view_dict(out, v)
        assert ov[0] == one[0]
        for k in (1, 2, 3, 4, 5, 6, 11):  # colour, depth, median, variance, alpha, radii, related pixels
            assert torch.equal(ov[k], one[k]), (v, k)
        dv = {"num_rendered": ov[0], "geom": ov[7], "binning": ov[8], "img": ov[9]}
        for name in ("ranges", "point_list", "n_contrib"):
            assert np.array_equal(hh.hip_state(name, s, dv), hh.hip_state(name, s, d1)), (v, name)
        for name, w in (("rgb", 3), ("clamped", 3)):
            a, b = (hh.hip_state(name, s, x).reshape(s.P, w)[d1["radii"] > 0] for x in (dv, d1))
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), (v, name)
        st, ref = hh.oracle_forward(oracle, s, D)
        assert ov[0] == ref["num_rendered"] and np.array_equal(d1["radii"], ref["radii"])
        assert np.array_equal(d1["opacity_map"], ref["opacity_map"]) and np.array_equal(d1["depth_median"], ref["depth_median"])
        g = mask_flipped_pixels(pixel_grads(s), hh.hip_state("n_contrib", s, dv), st.get("n_contrib"), W, H, f"batch view {v}",
                                images=[(d1[k], ref[k]) for k in IMAGES],
                                median_margin=oracle.light_median_margin(st, ref["opacity_map"]))[0]
        gr = hh.oracle_backward(oracle, st, s, D, ref["opacity_map"], grads=g)
        grads.append(g)
        alphas.append(ref["opacity_map"])
        ref_view.append(gr["dL_dview"])
        ref_m2d.append(gr["dL_dmeans2D"])
        ref_sum = {k: gr[k].astype(np.float64) for k in gr} if ref_sum is None else {k: ref_sum[k] + gr[k] for k in gr}
    g = TB.batch_backward(hs, D, out, cams, grads, alphas=alphas)
    assert g["dL_dsh"].shape == (ss[0].P, M, 3)
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"):
        assert_grad_close(g[k], ref_sum[k].reshape(g[k].shape), k, rel_to_max=1e-5, elem_rtol=1e-3, elem_frac=1e-4)
    acc = None
    for v in range(V):
        assert_grad_close(g["dL_dmeans2D"][v], ref_m2d[v], f"dL_dmeans2D[{v}]", rel_to_max=1e-5, elem_rtol=1e-3, elem_frac=1e-4)
        assert_grad_close(g["dL_dview"][v], ref_view[v], f"dL_dview[{v}]", rel_to_max=1e-4, elem_rtol=1e-2, elem_frac=0.25)
        g1 = hh.hip_backward(hs[v], D, TB.one_view_dict(out, v), grads=grads[v], alphas=alphas[v])
        acc = {k: g1[k].copy() for k in g1} if acc is None else {k: acc[k] + g1[k] for k in g1}
    for k in ("dL_dmeans3D", "dL_dsh", "dL_dopacity", "dL_dscales", "dL_drotations"):
        assert TB.close(g[k], acc[k]), k


@pytest.mark.parametrize("layout", FAMILY_LAYOUTS, ids=case_id)
def test_full_batch(oracle, binding, layout):
    """Two views of the full variant in one call, with the bars of tests/test_hip_full_batch.py."""
    V = 2
    pairs = [family_scenes(layout, v)[:2] for v in range(V)]
    M, D = family_scenes(layout)[2:]
    if layout == "misaligned":
        pairs = [(s, hs._replace(shs=pairs[0][1].shs)) for s, hs in pairs]
    ss, hs = [p[0] for p in pairs], [p[1] for p in pairs]
    grads = TFB.grads_of(ss)
    out, cams = TFB.batch_forward(hs, D)
    g = TFB.batch_backward(hs, D, out, cams, grads)
    assert g["dL_dsh"].shape == (ss[0].P, M, 3)
    acc, ref_sum = None, None
    for v, s in enumerate(ss):
        one, d1 = hh.hip_full_forward(hs[v], D)
        ov = TFB.one_view(out, v)
        assert ov[0] == one[0] and ov[1] == one[1], v
        for k in (2, 3, 4, 5):  # colour, depth, uncertainty, radii
            assert torch.equal(ov[k], one[k]), (v, k)
        dv = {"num_rendered": ov[0], "num_related": ov[1], "geom": ov[6], "binning": ov[7], "img": ov[8]}
        dv.update({k: ov[i].cpu().numpy() for i, k in ((2, "color"), (3, "depth"), (4, "uncertainty"), (5, "radii"))})
        g1 = hh.hip_full_backward(hs[v], D, ov, grads=grads[v])
        assert TFB.close(g["dL_dmeans2D"][v], g1["dL_dmeans2D"]) and TFB.close(g["dL_dview"][v], g1["dL_dview"]), v
        acc = {k: g1[k].copy() for k in g1} if acc is None else {k: acc[k] + g1[k] for k in g1}
        st, ref, gr = hh.oracle_full(oracle, s, D, grads=grads[v])
        full_forward_matches(dv, st, ref, s, f"full batch {layout} view {v}")
        assert_grad_close(g["dL_dmeans2D"][v], gr["dL_dmeans2D"], f"dL_dmeans2D[{v}]", **FULL_TOL)
        assert_grad_close(g["dL_dview"][v], gr["dL_dview"], f"dL_dview[{v}]", rel_to_max=FULL_TOL["rel_to_max"] * 5, elem_rtol=5e-3,
                          elem_frac=0.1)
        ref_sum = {k: gr[k].astype(np.float64) for k in gr} if ref_sum is None else {k: ref_sum[k] + gr[k] for k in gr}
    for k in ("dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"):
        assert TFB.close(g[k], acc[k]), k
        assert_grad_close(g[k], ref_sum[k].reshape(g[k].shape), k, **FULL_TOL)


# ------------------------------------------------------------------------------------------ the autograd surface
def rasterize(s, D, shs, leaves):
    """forward and backward through dgr_amd.light.GaussianRasterizer under deterministic_grads; returns the images"""
    rast = L.GaussianRasterizer(make_settings(s, D, hh.dev()))
    with _capi.thread_options(deterministic_grads=1):
        o = rast(means3D=leaves["means3D"], means2D=leaves["means2D"], opacities=leaves["opacity"], shs=shs, scales=leaves["scales"],
                 rotations=leaves["rotations"], viewmatrix=leaves["view"], gt_depth=hh.T(s.gt))
        gC, gD, gM, gV = pixel_grads(s)
        torch.autograd.backward([o[0], o[2], o[3], o[4]], [hh.T(gC), hh.T(gD[None]), hh.T(gM[None]), hh.T(gV[None])])
    torch.cuda.synchronize()
    return o


def scene_leaves(s):
    leaves = {name: hh.T(a).requires_grad_() for name, a in (("means3D", s.means), ("opacity", s.opac), ("scales", s.scales),
                                                              ("rotations", s.rots), ("view", s.view))}
    leaves["means2D"] = torch.zeros((s.P, 3), device=hh.dev(), requires_grad=True)
    return leaves


def test_a_strided_slice_of_a_wider_leaf(binding):
    """`shs = full[:, :4]` of a [P, 16, 3] leaf, sh_degree 1 (a model that grows its degree renders so): nothing raises, the
    gradient reaching full[:, :4] and every other leaf carry the bits of the canonical run (the zero-padded [P, 16, 3] leaf),
    full.grad[:, 4:] is exactly zero."""
    P, M, D = 300, 4, 1
    base = base_scene(P)
    full = hh.T(base.shs).requires_grad_()
    view = full[:, :M]
    assert not view.is_contiguous() and view.shape == (P, M, 3)
    a = scene_leaves(base)
    oa = rasterize(base, D, view, a)
    canon = hh.T(as_padded(base, M).shs).requires_grad_()
    b = scene_leaves(base)
    ob = rasterize(base, D, canon, b)
    for k in (0, 1, 2, 3, 5, 7):  # colour, radii, depth, median, alpha, related pixels (6: a sum of float atomics in either run)
        assert torch.equal(oa[k], ob[k]), k
    assert full.grad.shape == (P, 16, 3) and float(full.grad[:, :M].abs().max()) > 0
    assert torch.equal(full.grad[:, :M], canon.grad[:, :M])
    assert not bool(full.grad[:, M:].any())
    for name in a:
        assert torch.equal(a[name].grad, b[name].grad), name


class DegreeZeroModel:
    """The accessors slam.render uses, of a degree-0 model: get_features is f_dc alone, [P, 1, 3]"""
    active_sh_degree = 0

    def __init__(self, s):
        leaf = lambda a: hh.T(a).requires_grad_()  # noqa: E731
        self.get_xyz, self.get_opacity, self.get_scaling = leaf(s.means), leaf(s.opac), leaf(s.scales)
        self.get_rotation, self.get_features = leaf(s.rots), leaf(s.shs)


def test_slam_render_of_a_degree_zero_model(binding):
    """slam.render with get_features [P, 1, 3] and active_sh_degree 0: the images and the gradients of the leaves are the direct
    binding's, bit for bit under deterministic_grads, and the gradients still lie in one arena whose leading segments
    (dgr_amd.light.SPAN_SEGMENTS) form one contiguous range."""
    P, M, D = 300, 1, 0
    s, _ = scenes_of(P, M, D)
    grads = pixel_grads(s)
    d, g = deterministic_run(s, D, grads)
    pc = DegreeZeroModel(s)
    assert pc.get_features.shape == (P, 1, 3)
    view = hh.T(s.view).requires_grad_()
    with _capi.thread_options(deterministic_grads=1):
        out = slam.render(None, pc, None, hh.T(s.bg), viewmatrix=view, fov=(s.tanfovx, s.tanfovy), HW=(H, W), gt_depth=hh.T(s.gt),
                          pose_tensors=(hh.T(s.view), hh.T(s.proj), hh.T(s.persp), hh.T(s.campos)))
        gC, gD, gM, gV = grads
        torch.autograd.backward([out["render"], out["depth"], out["depth_median"], out["depth_var"]],
                                [hh.T(gC), hh.T(gD[None]), hh.T(gM[None]), hh.T(gV[None])])
    torch.cuda.synchronize()
    for name, key in (("color", "render"), ("depth", "depth"), ("depth_median", "depth_median"), ("opacity_map", "opacity_map"),
                      ("radii", "radii")):
        assert np.array_equal(out[key].detach().cpu().numpy().view(np.uint8), d[name].view(np.uint8)), name
    leaves = {"dL_dmeans3D": pc.get_xyz, "dL_dsh": pc.get_features, "dL_dopacity": pc.get_opacity, "dL_dscales": pc.get_scaling,
              "dL_drotations": pc.get_rotation, "dL_dmeans2D": out["viewspace_points"], "dL_dview": view}
    for name, leaf in leaves.items():
        assert leaf.grad is not None and tuple(leaf.grad.shape) == g[name].shape, name
        assert np.array_equal(bits(leaf.grad.cpu().numpy()), bits(g[name])), name
    assert pc.get_features.grad.shape == (P, 1, 3) and float(pc.get_features.grad.abs().max()) > 0
    span = GradientArena([pc.get_xyz, out["viewspace_points"], pc.get_features, pc.get_opacity, pc.get_scaling,
                          pc.get_rotation]).fused_span()
    assert span is not None
    # means3D, means2D, sh, opacity, scales, rotations, each segment a multiple of 64 floats, the last one as long as it is
    pad = lambda n: (n + 63) // 64 * 64  # noqa: E731
    assert span.numel() == pad(3 * P) * 2 + pad(3 * M * P) + pad(P) + pad(3 * P) + 4 * P
    assert span.data_ptr() == pc.get_xyz.grad.data_ptr()


# ------------------------------------------------------------------------------------------ the SH degree
@pytest.mark.parametrize("degree", [-1, 4])
def test_both_bindings_refuse_a_degree_outside_0_to_3(binding, degree):
    """include/dgr_hip.h: D = 0 .. 3.  A larger one used to be read as 3 by the colour and as itself by the row loads."""
    s = base_scene(300)
    for forward in (hh.hip_forward, hh.hip_full_forward):
        with pytest.raises(RuntimeError, match="SH degree must be 0 .. 3"):
            forward(s, degree)
    out, _ = hh.hip_forward(s, 3)
    with pytest.raises(RuntimeError, match="SH degree must be 0 .. 3"):
        hh.hip_backward(s, degree, out)
    out, _ = hh.hip_full_forward(s, 3)
    with pytest.raises(RuntimeError, match="SH degree must be 0 .. 3"):
        hh.hip_full_backward(s, degree, out)
