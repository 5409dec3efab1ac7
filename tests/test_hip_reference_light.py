"""The light variant against the reference rasterizer's OWN source, compiled for gfx950 (oracle/build_ref.py -> oracle/_ref/,
driven through oracle/reference.py): three parties -- the reference library, the HIP kernels through the C ABI, the oracle in
its float and its C-math build -- and one arbiter, the float64 formulation evaluated on the reference's decisions.  The rules
are those of tests/ref_parity.py.  A missing library is a failure that names the build step, not a skip."""
import pytest

import ref_parity as rp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", rp.LIGHT_CASES, ids=rp.case_id)
def test_light_forward_and_backward_against_the_reference(oracle, case):
    """Integer state exactly outside counted flips; the images, gau_uncertainty and the per-Gaussian preprocess outputs, then
    every gradient tensor of the three track_off / map_off modes (every side handed the float64 alpha image rounded once), then
    the mapping+pose backward end to end (every side on its own forward's alpha image), at e_x <= max(2 e_ref, bar) against float64."""
    reference = rp.reference_library("light")
    c = rp.build_case(case)
    oracle.use_cmath(False)
    st_f, of = rp.module_forward(oracle, c)
    oracle.use_cmath(True)
    try:
        st_c, oc = rp.module_forward(oracle, c)
    finally:
        oracle.use_cmath(False)
    assert of["num_rendered"] > 0  # (a frame with no instance is never given to the reference)
    st_r, ref = rp.module_forward(reference, c)
    out, hip = rp.hip_forward(c)
    mask, f64 = rp.compare_forward(c, ref, {"hip": hip, "oracle": of, "oracle_cmath": oc},
                                   margin_fn=lambda a: oracle.light_median_margin(st_f, a))
    grads = rp.masked(rp.pixel_grads(c.s), mask)
    alphas = rp.arbiter_alphas(f64)
    g64, _ = rp.grads64(c, ref, grads, alphas, f64)
    for mode in rp.MODES:
        _, track_off, map_off = mode
        rp.compare_backward(c, mode, g64, rp.module_backward(reference, st_r, c, alphas, grads, track_off, map_off),
                            {"hip": rp.hip_backward(out, c, alphas, grads, track_off, map_off),
                             "oracle": rp.module_backward(oracle, st_f, c, alphas, grads, track_off, map_off),
                             "oracle_cmath": rp.module_backward(oracle, st_c, c, alphas, grads, track_off, map_off)})
    # end to end, mapping+pose: every side's backward on its OWN forward's alpha image
    fn = lambda a: oracle.light_median_margin(st_f, a)  # noqa: E731
    own = rp.masked(rp.pixel_grads(c.s), rp.end_to_end_mask(c, f64, mask, fn, [ref["opacity_map"], hip["opacity_map"], of["opacity_map"],
                                                                                 oc["opacity_map"]]))
    rp.compare_end_to_end(c, ref, f64, own, rp.module_backward(reference, st_r, c, ref["opacity_map"], own, False, False),
                          {"hip": (rp.hip_backward(out, c, None, own, False, False), hip["opacity_map"]),
                           "oracle": (rp.module_backward(oracle, st_f, c, of["opacity_map"], own, False, False), of["opacity_map"]),
                           "oracle_cmath": (rp.module_backward(oracle, st_c, c, oc["opacity_map"], own, False, False), oc["opacity_map"])})
