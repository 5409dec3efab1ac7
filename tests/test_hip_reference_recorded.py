"""The HIP kernels (and, beside them, both oracle builds) against RECORDED outputs of the reference rasterizer's own source
(tests/golden/reference/, written on an MI355X by tests/golden/make_reference_golden.py): the comparison of
tests/test_hip_reference_light.py / _full.py on the two recorded scenes, which needs no reference library.  It stands beside the live comparison, not in place of it.  Rules of tests/ref_parity.py; the float64 arbiter is recomputed here."""
import numpy as np
import pytest

import ref_parity as rp
from ref_parity import oracle_parties, recorded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", rp.GOLDEN_CASES, ids=rp.case_id)
def test_light_kernels_against_the_recorded_reference(oracle, case):
    c = rp.build_case(case)
    ref = recorded("light", case, "fwd", c)
    st_f, st_c, parties = oracle_parties(oracle, c, "light")
    out, parties["hip"] = rp.hip_forward(c)
    mask, f64 = rp.compare_forward(c, ref, parties, margin_fn=lambda a: oracle.light_median_margin(st_f, a))
    was = np.asarray(ref["mask"], bool)
    assert not (mask & ~was).any(), f"{int((mask & ~was).sum())} pixels flip that did not when the reference's gradients were recorded"
    grads, alphas = rp.masked(rp.pixel_grads(c.s), was), rp.arbiter_alphas(f64)
    g64, _ = rp.grads64(c, ref, grads, alphas, f64)
    for mode in rp.MODES:
        name, track_off, map_off = mode
        g_ref = recorded("light", case, name.replace("+", "_"), c)
        rp.compare_backward(c, mode, g64, g_ref, {"hip": rp.hip_backward(out, c, alphas, grads, track_off, map_off),
                                                  "oracle": rp.module_backward(oracle, st_f, c, alphas, grads, track_off, map_off)})


def test_full_kernels_forward_against_the_recorded_reference(oracle):
    case = rp.GOLDEN_CASES[0]
    c = rp.build_case(case)
    ref = recorded("full", case, "fwd", c)
    _, _, parties = oracle_parties(oracle, c, "full")
    _, parties["hip"] = rp.hip_forward(c, "full")
    rp.compare_forward(c, ref, parties, "full")
