"""CPU side of the tests against the reference's own source (tests/ref_parity.py): the committed seeds' pre-check, and the
comparison helper's own unit tests -- it must reject what a subtly wrong kernel would produce.

The C-math oracle stands in for the reference here and the float oracle is the party: the same source under another libm
binding, the CPU proxy for "same statements, different compiler"."""
import numpy as np
import pytest

import ref_parity as rp


def both_builds(oracle, c, variant="light"):
    oracle.use_cmath(True)
    try:
        st_c, oc = rp.module_forward(oracle, c, variant)
    finally:
        oracle.use_cmath(False)
    st_f, of = rp.module_forward(oracle, c, variant)
    return st_c, oc, st_f, of


@pytest.mark.parametrize("case", rp.LIGHT_CASES + rp.GOLDEN_CASES, ids=rp.case_id)
def test_seeds_keep_the_oracle_builds_within_half_of_each_cap(oracle, case):
    """float oracle against C-math oracle on every committed case: radii flips and swapped list positions at or below HALF their
    caps (the pixel flips' asserted bound, 3e-4 of the pixels, is already below half of 1e-3), and the real-valued rules hold."""
    c = rp.build_case(case)
    st_c, oc, st_f, of = both_builds(oracle, c)
    rp.compare_forward(c, oc, {"oracle": of}, margin_fn=lambda a: oracle.light_median_margin(st_f, a), share=0.5)


@pytest.mark.parametrize("case", rp.FULL_CASES + rp.GOLDEN_CASES[:1], ids=rp.case_id)
def test_seeds_keep_the_full_oracle_builds_within_half_of_each_cap(oracle, case):
    c = rp.build_case(case)
    _, oc, _, of = both_builds(oracle, c, "full")
    rp.compare_forward(c, oc, {"oracle": of}, "full", share=0.5)


@pytest.fixture(scope="module")
def small(oracle):
    """the ragged case, forward and the mapping+pose backward of both builds, shared and left unchanged"""
    c = rp.build_case(rp.LIGHT_CASES[4])
    st_c, oc, st_f, of = both_builds(oracle, c)
    mask, f64 = rp.compare_forward(c, oc, {"oracle": of}, margin_fn=lambda a: oracle.light_median_margin(st_f, a))
    grads = rp.masked(rp.pixel_grads(c.s), mask)
    alphas = rp.arbiter_alphas(f64)
    g64, _ = rp.grads64(c, oc, grads, alphas, f64)
    g_ref = rp.module_backward(oracle, st_c, c, alphas, grads, False, False)
    g_of = rp.module_backward(oracle, st_f, c, alphas, grads, False, False)
    return c, oc, of, g64, g_ref, g_of


def test_the_helper_accepts_the_oracle(small):
    c, oc, of, g64, g_ref, g_of = small
    rp.compare_backward(c, rp.MODES[0], g64, g_ref, {"oracle": g_of})


def test_the_helper_rejects_one_pose_slot_scaled_by_1_001(small):
    """what a wrong factor in one slot of the pose gradient looks like: every slot but 3, 7, 11, 15 in turn"""
    c, oc, of, g64, g_ref, g_of = small
    for slot in (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14):
        wrong = {k: np.array(v, copy=True) for k, v in g_of.items()}
        wrong["dL_dview"].reshape(-1)[slot] *= np.float32(1.001)
        share = abs(float(g_of["dL_dview"].reshape(-1)[slot])) / np.abs(g64["dL_dview"]).max()
        if share < 0.05:
            continue  # (a slot that small against the tensor's scale is below the 1e-5 bar by construction)
        with pytest.raises(AssertionError, match="dL_dview"):
            rp.compare_backward(c, rp.MODES[0], g64, g_ref, {"oracle": wrong})
    wrong = {k: np.array(v, copy=True) for k, v in g_of.items()}
    wrong["dL_dview"].reshape(-1)[int(np.abs(g_of["dL_dview"]).argmax())] *= np.float32(1.001)
    with pytest.raises(AssertionError, match="dL_dview"):
        rp.compare_backward(c, rp.MODES[0], g64, g_ref, {"oracle": wrong})


def test_the_helper_rejects_one_tiles_list_reversed(small):
    c, oc, of, *_ = small
    ranges = np.asarray(oc["ranges"]).reshape(-1, 2)
    t = int(np.argmax(ranges[:, 1].astype(np.int64) - ranges[:, 0]))
    lo, hi = ranges[t]
    assert hi - lo > 8
    wrong = dict(of)
    wrong["point_list"] = np.array(of["point_list"], copy=True)
    wrong["point_list"][lo:hi] = wrong["point_list"][lo:hi][::-1]
    with pytest.raises(AssertionError, match="more than 1 ulp apart"):
        rp.compare_integer_state(oc, wrong, c.s.W, c.s.H, "reversed")
    rp.compare_integer_state(oc, of, c.s.W, c.s.H, "untouched")


def test_the_helper_counts_radius_flips_and_refuses_a_step_of_two(small):
    c, oc, of, *_ = small
    wrong = dict(of)
    wrong["radii"] = np.array(of["radii"], copy=True)
    g = int(np.nonzero(of["radii"] > 0)[0][0])
    wrong["radii"][g] += 1
    fl = rp.compare_integer_state(oc, wrong, c.s.W, c.s.H, "one radius off by one")   # 1 of 2000: within 1e-3
    assert fl.radii_flips == 1 and fl.tiles.any()
    with pytest.raises(AssertionError, match="radii differ"):
        rp.compare_integer_state(oc, wrong, c.s.W, c.s.H, "half cap", share=0.4)
    wrong["radii"][g] += 1
    with pytest.raises(AssertionError, match="differs by 2"):
        rp.compare_integer_state(oc, wrong, c.s.W, c.s.H, "one radius off by two")
