"""The light blend backward (csrc/render_light.hip: render_bwd_light_body) at the edges of its live-entry batches.

The backward walks a tile's LIVE entries -- what the forward compacted as {Gaussian id, list position << 8 | tag} -- from the back,
128 at a time (64 under deterministic_grads), in batches of equal size where its lists are paired (129 = 65 + 64, 257 = 86 + 86 +
85: the mapping instances on half-wave lists).  T, S and the median's once-per-pixel threshold are carried from batch to batch; a
pixel's cut `position < last_contributor` is taken on the list position the live record carries, not on the index the loop counts;
a tile's live list starts at its range's start, whatever its parity.

The scenes (tests/light_blend_scenes.py; tests/test_light_blend_scenes.py checks on the CPU that they are what they claim): one
tile with exactly 64 / 65 / 128 / 129 / 256 / 257 / 385 live entries, three whose 65 / 129 / 257 live entries lie among dead ones,
a frame of two tiles with 129 and 257, and two opaque tiles of 129 / 257 live entries whose pixels finish early -- the only ones
on which the cut at the last contributor keeps out a pair that passes the alpha test.  Each on both lane mappings.

Forward: the integer state is the oracle's, the live counts are the scenes' numbers exactly, the live list is the tagged entries
at the oracle-derived positions, every tag byte is written.
Backward: judged as tests/test_hip_full_blend_edges.py judges -- e_hip <= max(2 e_oracle, 1e-5) per tensor, distances to the float64
model (ref_parity.grads64) relative to the tensor's largest value, no pixel, row or element left out; dL_dview also element by
element -- in the three modes, lean, with one image missing, deterministic, with absgrad, with a silhouette image and in the
other two alpha modes.  Every side's backward is handed the model's alpha image, rounded once.
The measured table and the mutants of the kernel this file was run against: profiles/light_blend_edges/measured.txt.
"""
import numpy as np
import pytest
import torch

import fp64_model as M
import hip_helpers as hh
import light_blend_scenes as S
import ref_parity as rp
from hip_helpers import forced_lane_lists as lane_lists  # noqa: F401  (fixtures)
from dgr_amd import _capi
from ref_parity import GRADS, MODES, scale_distance
from test_hip_absgrad import check_against
from test_hip_full_blend_edges import ATOMICS_BAR, LISTS, bits, judge
from test_hip_fwd_blend_edges import assert_every_tag_byte_is_written
from test_hip_live_lists import assert_live_list_is_the_tagged_entries

pytestmark = pytest.mark.gpu

ALL = list(S.SCENES)
ONE_MISSING = ["live129", "sparse257of512"]
DETERMINISTIC = ["live64", "live65", "live128", "live129", "sparse65of200", "sparse129of400", "two_tiles", "opaque129of320"]
ABSGRAD = ["live129", "live257", "sparse129of400", "two_tiles", "opaque257of400"]
SILHOUETTE = ["live129", "sparse257of512"]
ALPHA_MODES = ["live257", "sparse129of400", "opaque257of400"]
MODE_IDS = [m[0] for m in MODES]
PER_GAUSSIAN = [k for k in hh.GRAD_NAMES if k != "dL_dview"]


# ------------------------------------------------------------------------------------------ forward
def forward_on_the_oracles_decisions(oracle, name, cmath=False):
    s = S.scene(name)
    st, ref = S.oracle_forward(oracle, name, cmath)
    out, d = hh.hip_forward(s, S.DEG)
    assert np.array_equal(d["radii"], ref["radii"]) and d["num_rendered"] == ref["num_rendered"]
    for k in ("point_list", "ranges", "n_contrib"):
        assert np.array_equal(hh.hip_state(k, s, d), ref[k]), k
    return s, out, d


@pytest.mark.parametrize("name", ALL)
def test_forward(oracle, lane_lists, name):
    s, out, d = forward_on_the_oracles_decisions(oracle, name)
    live, _ = S.live_positions(oracle, name)
    tags, counts, ranges = assert_live_list_is_the_tagged_entries(s, d)
    assert_every_tag_byte_is_written(s, d, tags, ranges)
    got = {t: int(n) for t, n in enumerate(counts) if n}
    print(f"{name + LISTS[lane_lists]:<20} forward live counts {got}")
    assert got == S.SCENES[name][1]
    for tile, (lo, hi) in enumerate(ranges):
        assert np.array_equal(np.nonzero(tags[lo:hi])[0], live[tile]), tile


# ------------------------------------------------------------------------------------------ backward
def hip_grads(s, out, grads, alphas, mode=MODES[0], without=(), **kw):
    """the nine gradients (and `absgrad`) of one call; `without`: the indices of the pixel-gradient images that are not passed"""
    _, track_off, map_off = mode
    g = hh.hip_backward_raw(s, S.DEG, out, grads=tuple(None if i in without else x for i, x in enumerate(grads)), alphas=alphas,
                            track_off=track_off, map_off=map_off, **kw)
    torch.cuda.synchronize()
    assert tuple(g[8].shape) == (1, 4, 4)
    d = {n: v.cpu().numpy() for n, v in zip(hh.GRAD_NAMES, list(g[:8]) + [g[8][0]])}
    assert not d["dL_dview"].reshape(-1)[[3, 7, 11, 15]].any()
    if len(g) > 9:
        d["absgrad"] = g[9].cpu().numpy()
    return d


def atomics_equal(case, a, b):
    """two calls that compute the same sums: every tensor within ATOMICS_BAR of its largest value (the full test's rule; one
    printed line per case, the worst tensor's)"""
    worst = (0.0, "-")
    for k in hh.GRAD_NAMES:
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        scale = float(np.abs(y).max())
        if scale == 0.0:
            assert not x.any(), f"{case} {k}"
            continue
        err = float(np.abs(x - y).max()) / scale
        worst = max(worst, (err, k))
        assert err <= ATOMICS_BAR, f"{case} {k}: {err:.2e}"
    print(f"{case:<40} worst tensor   max |a - b| / max |b| {worst[0]:9.2e}  ({worst[1]})")


def judge_mode(case, mode, g_hip, g_or, g64, **kw):
    """`judge` on the tensors the mode computes; the ones it switches off are exactly zero"""
    _, track_off, map_off = mode
    off = (["dL_dview"] if track_off else []) + (PER_GAUSSIAN if map_off else [])
    for k in off:
        assert not np.asarray(g_hip[k]).any(), f"{case} {k}: not zero where the mode switches it off"
        assert g_or is None or not np.asarray(g_or[k]).any(), f"{case} {k}: the oracle's"
    judge(case, g_hip, g_or, g64, only=[k for k in GRADS if k not in off], **kw)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ALL)
def test_backward_default(oracle, lane_lists, name, mode):
    s, out, _ = forward_on_the_oracles_decisions(oracle, name)
    grads, alphas, g_or, g64 = S.references(oracle, name, mode)
    assert all(np.any(g) for g in grads)
    judge_mode(f"{name} {mode[0]}{LISTS[lane_lists]}", mode, hip_grads(s, out, grads, alphas, mode), g_or, g64)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ALL)
def test_backward_lean(oracle, lane_lists, name, mode):
    s, out, _ = forward_on_the_oracles_decisions(oracle, name)
    grads, alphas, g_or, g64 = S.references(oracle, name, mode, "lean")
    assert not grads[2].any() and not grads[3].any()
    lean = hip_grads(s, out, grads, alphas, mode, without=(2, 3))
    zero = hip_grads(s, out, grads, alphas, mode)   # (explicit all-zero median and variance gradients)
    atomics_equal(f"{name} {mode[0]} lean vs zero images{LISTS[lane_lists]}", lean, zero)
    judge_mode(f"{name} {mode[0]} lean{LISTS[lane_lists]}", mode, lean, g_or, g64)


@pytest.mark.parametrize("missing", ["no_median", "no_var"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ONE_MISSING)
def test_backward_with_one_image_missing(oracle, lane_lists, name, mode, missing):
    """the non-lean kernel reads a NULL median or variance image as zero"""
    s, out, _ = forward_on_the_oracles_decisions(oracle, name)
    grads, alphas, g_or, g64 = S.references(oracle, name, mode, missing)
    i = 2 if missing == "no_median" else 3
    assert not grads[i].any() and grads[5 - i].any()
    got = hip_grads(s, out, grads, alphas, mode, without=(i,))
    judge_mode(f"{name} {mode[0]} {missing}{LISTS[lane_lists]}", mode, got, g_or, g64)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", DETERMINISTIC)
def test_backward_deterministic(oracle, lane_lists, name, mode):
    grads, alphas, g_or, g64 = S.references(oracle, name, mode)
    with _capi.thread_options(deterministic_grads=1):
        s, out, _ = forward_on_the_oracles_decisions(oracle, name)
        a = hip_grads(s, out, grads, alphas, mode)
        b = hip_grads(s, out, grads, alphas, mode)
    for k in hh.GRAD_NAMES:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    judge_mode(f"{name} {mode[0]} deterministic{LISTS[lane_lists]}", mode, a, g_or, g64)


def absgrad64(oracle, name, form):
    """float64 sum_p |v_p(g)| (fp64_model.absgrad_of_pairs) under the alpha image the sides are handed"""
    k = S.key(name, "absgrad64", form)
    if k not in S._cache:
        s = S.scene(name)
        st, ref = S.oracle_forward(oracle, name)
        f64, alphas = S.forward64(oracle, name)
        gC, gD, gM, gV = (np.asarray(g, np.float64) for g in S.pixel_grads(name, form))
        f = rp.alpha_interface_factor(f64, alphas)   # (ref_parity.grads64)
        pairs = []
        loss, _, img = M.torch_light(s, S.DEG, ref["radii"] > 0, ref["point_list"], ref["ranges"], ref["n_contrib"],
                                     (gC * f, gD * f, gM, gV * f), pairs=pairs)
        loss.backward()
        S._cache[k] = M.absgrad_of_pairs(pairs, img["_idx"], s.P, s.W, s.H)
    return S._cache[k]


@pytest.mark.parametrize("lean", [False, True], ids=["all images", "lean"])
@pytest.mark.parametrize("mode", MODES[:2], ids=MODE_IDS[:2])
@pytest.mark.parametrize("name", ABSGRAD)
def test_absgrad(oracle, lane_lists, name, mode, lean):
    s, out, d = forward_on_the_oracles_decisions(oracle, name)
    form = "lean" if lean else "default"
    grads, alphas, _, _ = S.references(oracle, name, mode, form)
    without = (2, 3) if lean else ()
    plain = hip_grads(s, out, grads, alphas, mode, without=without)
    ab = hip_grads(s, out, grads, alphas, mode, without=without, absgrad=True)
    what = f"{name} {mode[0]} {form} absgrad"
    atomics_equal(f"{what} vs plain{LISTS[lane_lists]}", ab, plain)
    assert ab["absgrad"].shape == (s.P, 3)
    want = absgrad64(oracle, name, form)
    print(f"{what + LISTS[lane_lists]:<40} {'absgrad':<14} max |hip - fp64| / max |fp64| {scale_distance(ab['absgrad'], want):9.2e}")
    check_against(ab["absgrad"], want, d["radii"], what)


def silhouette_grads64(oracle, name, gA):
    """float64 gradients of sum gA * (1 - T_final), the exact silhouette term: the colour loss of a second call with colour 0
    everywhere (SH degree 0: C0 sh_0 + 1/2 = 0), background (1, 0, 0) and colour gradient (-gA, 0, 0) -- same decisions, same
    leaves, the same alpha image handed over (tests/test_hip_full_blend_edges.py).  No SH gradient (the fake colours'); the light
    pose gradient is built from dL/dmean2D, which the term does reach."""
    c = S.case(name)
    st, ref = S.oracle_forward(oracle, name)
    f64, alphas = S.forward64(oracle, name)
    zero = np.zeros((c.s.H, c.s.W))
    sh0 = np.zeros_like(np.asarray(c.s.shs, np.float64))
    sh0[:, 0, :] = -0.5 / M.C0
    c.s = c.s._replace(bg=np.array([1.0, 0.0, 0.0], np.float32), shs=sh0)
    g, _ = rp.grads64(c, ref, (np.stack([-np.asarray(gA, np.float64), zero, zero]), zero, zero, zero), alphas, f64)
    g["dL_dsh"] = np.zeros_like(g["dL_dsh"])
    return g


@pytest.mark.parametrize("mode", [MODES[0], MODES[2]], ids=[MODE_IDS[0], MODE_IDS[2]])
@pytest.mark.parametrize("name", SILHOUETTE)
def test_silhouette(oracle, lane_lists, name, mode):
    """A silhouette image on top of the default form, in the default and the tracking instance.  The oracle has no silhouette
    term: the image enters the kernel through one per-pixel constant (bg_term), every sum is the default form's, so the oracle's
    ABSOLUTE error on the default form stands in for e_oracle."""
    s, out, _ = forward_on_the_oracles_decisions(oracle, name)
    grads, alphas, g_or, g64 = S.references(oracle, name, mode)
    gA = (np.random.default_rng(3).normal(0.0, 1.0, (s.H, s.W)) / (s.W * s.H) ** 0.5).astype(np.float32)
    extra = silhouette_grads64(oracle, name, gA)
    both = {k: g64[k] + extra[k] for k in g64}
    err_or = {k: float(np.abs(np.asarray(g_or[k], np.float64).reshape(g64[k].shape) - g64[k]).max()) for k in g64}
    got = hip_grads(s, out, grads, alphas, mode, silhouette=gA)
    seen = "dL_dview" if mode[2] else "dL_dmeans3D"
    assert scale_distance(got[seen], g64[seen]) > 1e-3   # (the image does reach the gradients)
    judge_mode(f"{name} {mode[0]} + silhouette{LISTS[lane_lists]}", mode, got, None, both, extra_abs=err_or)


@pytest.mark.parametrize("alpha_mode", [1, 2])
@pytest.mark.parametrize("name", ALPHA_MODES)
def test_lean_call_equals_the_zero_image_call_in_the_other_alpha_modes(oracle, lane_lists, name, alpha_mode):
    """launch_bwd_light_mode has no lean instance for alpha_mode 1 and 2: a NULL image reads as zero there.  Mode 2 (glibc's expf
    restated; quadrant lists, batches of 128 whatever the lane mapping) is also judged, against the C-math oracle and the float64
    model on its decisions."""
    cmath = alpha_mode == 2
    for mode in MODES:
        grads, alphas, g_or, g64 = S.references(oracle, name, mode, "lean", cmath=cmath)
        with _capi.thread_options(alpha_mode=alpha_mode):
            if cmath:
                s, out, _ = forward_on_the_oracles_decisions(oracle, name, cmath=True)
            else:
                s = S.scene(name)
                out, _ = hh.hip_forward(s, S.DEG)
            lean = hip_grads(s, out, grads, alphas, mode, without=(2, 3))
            zero = hip_grads(s, out, grads, alphas, mode)
        atomics_equal(f"{name} {mode[0]} alpha_mode {alpha_mode} lean vs zero{LISTS[lane_lists]}", lean, zero)
        if cmath:
            judge_mode(f"{name} {mode[0]} alpha_mode 2 lean{LISTS[lane_lists]}", mode, lean, g_or, g64)
