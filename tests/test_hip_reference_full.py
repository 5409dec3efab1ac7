"""The full variant's FORWARD against the reference rasterizer's own source compiled for gfx950 (see
tests/test_hip_reference_light.py): colour, depth, the uncertainty image, radii, n_contrib and num_related of the HIP kernels
and of both oracle builds.  The reference's full backward is never run: ComputePG returns ahead of block-wide barriers
(DESIGN.md row a16), and the library has no entry point for it."""
import pytest

import ref_parity as rp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", rp.FULL_CASES, ids=rp.case_id)
def test_full_forward_against_the_reference(oracle, case):
    reference = rp.reference_library("full")
    c = rp.build_case(case)
    oracle.use_cmath(False)
    _, of = rp.module_forward(oracle, c, "full")
    oracle.use_cmath(True)
    try:
        _, oc = rp.module_forward(oracle, c, "full")
    finally:
        oracle.use_cmath(False)
    assert of["num_rendered"] > 0
    _, ref = rp.module_forward(reference, c, "full")
    _, hip = rp.hip_forward(c, "full")
    rp.compare_forward(c, ref, {"hip": hip, "oracle": of, "oracle_cmath": oc}, "full")
