"""The forward fetches the SH rows of the Gaussians whose colour it evaluates, and no others; the nine SH direction derivatives
it leaves for the backward are stored packed (csrc/gaussian_math.h: sh_rows_to_lanes, csrc/preprocess_fwd.hip: fetch_sh,
csrc/dgr_common.h: shd_a / shd_b / shd_c).

A wave of 64 Gaussians moves its rows through LDS in two slabs of 32 rows with cooperative 16-byte loads; each load is
predicated on the need bit of the row its piece belongs to.  The scenes here decide per Gaussian whether it is visible -- a
culled one is mirrored through the camera centre, behind the near plane -- in patterns per 256-Gaussian block:

  none         no Gaussian visible (the block-level skip)
  lane0 .. 63  exactly one visible Gaussian per block, at lane 0, 31, 32 or 63 of one wave (the slab boundaries)
  alternating  every other Gaussian
  all          every Gaussian

at P = 256 (one whole block), 512 (two) and 512 + 37 (a ragged block behind them, which takes the per-lane loads), SH degree 0
and 3; once with an SH tensor that is 4-byte aligned only (no 16-byte loads at all).  Every case is held to the oracle with the
bars of tests/test_hip_light_parity.py (check_backward: every leaf's gradient, stage-isolated and end to end; images, radii and
lists as there).  The direction derivatives enter dL_dmeans3D only, so that bar carries the packed layout; one degree-3 scene
has no clamped colour at all, so that the term is nowhere masked to zero.

Then the same frames with the SH row of every culled Gaussian overwritten by NaN: nothing may read them, so every output carries
the same bits and stays finite (gradients under deterministic_grads, where their sums have one order)."""
import functools

import numpy as np
import pytest

import hip_helpers as hh
from dgr_amd import _capi
from test_hip_light_parity import assert_images_carry_the_references_bits, check_backward
from util import make_scene

pytestmark = pytest.mark.gpu

W = H = 64
SEED = 17
SIZES = (256, 512, 512 + 37)
DEGREES = (0, 3)
PATTERNS = ("none", "lane0", "lane31", "lane32", "lane63", "alternating", "all")
CASES = [(P, D, pat) for P in SIZES for D in DEGREES for pat in PATTERNS]
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731


def case_id(case):
    return "-".join(str(x) for x in case)


def visible_rows(P, pattern):
    """the Gaussians a pattern leaves in front of the camera"""
    i = np.arange(P)
    if pattern == "none":
        return np.zeros(P, bool)
    if pattern == "all":
        return np.ones(P, bool)
    if pattern == "alternating":
        return (i & 1) == 0
    lane, wave, block = i & 63, (i >> 6) & 3, i >> 8
    return (lane == int(pattern[4:])) & (wave == (block + 1) % 4)  # one Gaussian per block, in a wave that changes with the block


@functools.lru_cache(maxsize=None)
def scene(P, pattern, unclamped=False):
    """make_scene with every Gaussian pulled well inside the frame (camera-space x, y times 0.6: all of them visible), then the
    pattern's culled ones mirrored through the camera centre.  `unclamped`: 2 added to the DC coefficients -- no colour below zero."""
    s = make_scene(P, W, H, SEED)
    Rm, t = s.view[:3, :3].T.astype(np.float64), s.view[3, :3].astype(np.float64)
    cam = s.means.astype(np.float64) @ Rm.T + t
    cam[:, :2] *= 0.6
    means = ((cam - t) @ Rm).astype(np.float32)
    hidden = ~visible_rows(P, pattern)
    means[hidden] = (2.0 * s.campos[None] - means[hidden]).astype(np.float32)
    shs = s.shs.copy()
    if unclamped:
        shs[:, 0, :] += 2.0
    return s._replace(means=means, shs=shs)


def against_the_oracle(oracle, s, D, pattern, hip_scene=None):
    d, st, ref = check_backward(oracle, s, D, hip_scene=hip_scene, what=f"culled rows P={s.P} D={D} {pattern}")
    assert np.array_equal(ref["radii"] > 0, visible_rows(s.P, pattern))  # (the scene is what the pattern says)
    assert np.array_equal(d["radii"], ref["radii"]) and d["num_rendered"] == ref["num_rendered"]
    assert_images_carry_the_references_bits(d, st, ref, s)
    assert np.array_equal(hh.hip_state("point_list", s if hip_scene is None else hip_scene, d), st.get("point_list"))
    return d, st, ref


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_culled_rows_against_the_oracle(oracle, case):
    P, D, pattern = case
    against_the_oracle(oracle, scene(P, pattern), D, pattern)


def test_culled_rows_four_byte_aligned_sh(oracle):
    """`shs` one float into a larger buffer: the per-lane loads of every block, under `need` alone"""
    from test_hip_sh_layouts import off_by_one_float
    s = scene(512 + 37, "alternating")
    against_the_oracle(oracle, s, 3, "alternating", hip_scene=s._replace(shs=off_by_one_float(s.shs)))


@pytest.mark.parametrize("P", SIZES)
def test_direction_derivatives_of_unclamped_colours(oracle, P):
    """Degree 3, no colour clamped: d(colour)/d(direction) reaches dL_dmeans3D for every visible Gaussian and channel"""
    s = scene(P, "all", unclamped=True)
    d, st, ref = against_the_oracle(oracle, s, 3, "all")
    assert not st.get("clamped").any()
    assert not hh.hip_state("clamped", s, d).any()


def run(s, D, grads):
    out, d = hh.hip_forward(s, D)
    # (deterministic_grads sizes a row buffer by num_rendered and refuses an empty frame, whose backward has no sum to order)
    with _capi.thread_options(deterministic_grads=1 if d["num_rendered"] else 0):
        g = hh.hip_backward(s, D, out, grads=grads)
    d["n_contrib"] = hh.hip_state("n_contrib", s, d)
    return d, g


@pytest.mark.parametrize("case", [c for c in CASES if c[2] != "all"], ids=case_id)
def test_nothing_reads_the_sh_row_of_a_culled_gaussian(case):
    P, D, pattern = case
    s = scene(P, pattern)
    shs = s.shs.copy()
    shs[~visible_rows(P, pattern)] = np.nan
    grads = tuple(g * (W * H) ** 0.5 for g in (s.gC, s.gD, s.gM, s.gV))
    d0, g0 = run(s, D, grads)
    d1, g1 = run(s._replace(shs=shs), D, grads)
    assert d0["num_rendered"] == d1["num_rendered"]
    for k in ("color", "depth", "depth_median", "opacity_map", "radii", "n_contrib", "gau_related_pixels"):
        assert np.isfinite(d1[k]).all(), k
        assert np.array_equal(d0[k].view(np.uint8), d1[k].view(np.uint8)), k
    for k in hh.GRAD_NAMES:
        assert np.isfinite(g1[k]).all(), k
        assert np.array_equal(bits(g0[k]), bits(g1[k])), k
