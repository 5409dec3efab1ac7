"""Both oracle builds against RECORDED outputs of the reference rasterizer's own source (tests/golden/reference/, written on an
MI355X by tests/golden/make_reference_golden.py from the reference compiled for gfx950): the CPU suite's hold on the oracle
where the reference cannot run.  Rules of tests/ref_parity.py; the float64 arbiter is recomputed here.  An edit that moves the
oracle away from the reference -- a term, a threshold, a slot of the pose gradient -- fails these tests without a GPU."""
import numpy as np
import pytest

import ref_parity as rp


recorded, oracle_parties = rp.recorded, rp.oracle_parties


@pytest.mark.parametrize("case", rp.GOLDEN_CASES, ids=rp.case_id)
def test_light_oracle_against_the_recorded_reference(oracle, case):
    c = rp.build_case(case)
    ref = recorded("light", case, "fwd", c)
    st_f, st_c, parties = oracle_parties(oracle, c, "light")
    mask, f64 = rp.compare_forward(c, ref, parties, margin_fn=lambda a: oracle.light_median_margin(st_f, a))
    was = np.asarray(ref["mask"], bool)
    assert not (mask & ~was).any(), (f"{int((mask & ~was).sum())} pixels flip now that did not when the reference's gradients were "
                                     "recorded: the oracle has moved")
    grads, alphas = rp.masked(rp.pixel_grads(c.s), was), rp.arbiter_alphas(f64)
    g64, _ = rp.grads64(c, ref, grads, alphas, f64)
    for mode in rp.MODES:
        name, track_off, map_off = mode
        g_ref = recorded("light", case, name.replace("+", "_"), c)
        assert bool(g_ref["track_off"]) == track_off and bool(g_ref["map_off"]) == map_off
        rp.compare_backward(c, mode, g64, g_ref, {"oracle": rp.module_backward(oracle, st_f, c, alphas, grads, track_off, map_off),
                                                  "oracle_cmath": rp.module_backward(oracle, st_c, c, alphas, grads, track_off, map_off)})


def test_full_oracle_forward_against_the_recorded_reference(oracle):
    case = rp.GOLDEN_CASES[0]
    c = rp.build_case(case)
    ref = recorded("full", case, "fwd", c)
    _, _, parties = oracle_parties(oracle, c, "full")
    rp.compare_forward(c, ref, parties, "full")
