#!/usr/bin/env python3
"""Records outputs of the reference rasterizer's own source (compiled for gfx950 by oracle/build_ref.py) on two tiny scenes, so
that the CPU suite can hold the oracle to the reference where the reference is not available
(tests/test_oracle_reference_pinned.py).  Needs a GPU and oracle/_ref/*.so; run once:

    python tests/golden/make_reference_golden.py       # writes tests/golden/reference/*.npz

Inputs are NOT stored: they are regenerated from the committed seed (tests/ref_parity.GOLDEN_CASES) through dgr_amd.synth and
identified by `scene_hash`.  Stored are the reference's outputs only -- light_<scene>_fwd.npz (integer state, images,
per-Gaussian forward outputs), light_<scene>_<mode>.npz (the nine gradients of one track_off / map_off mode) and
full_fwd_<scene>.npz -- plus `mask`, the pixels whose incoming gradients were zeroed for the backward: those some counted flip
touches between the reference, the two oracle builds and the float64 arbiter (tests/ref_parity.compare_forward).  The backward
is handed the float64 alpha image rounded once (ref_parity.arbiter_alphas), as in the GPU tests."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")]
import ref_parity as rp  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import reference as R  # noqa: E402

LIMIT = max(os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), f))
            for f in os.listdir(os.path.dirname(os.path.abspath(__file__))) if f.endswith(".npz"))


def save(path, **d):
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    print(os.path.relpath(path, ROOT), size // 1024, "KiB")
    assert size <= LIMIT, f"{path}: {size} bytes, larger than the largest existing file under tests/golden/ ({LIMIT})"


def oracles(c, variant):
    O.use_cmath(True)
    try:
        st_c, oc = rp.module_forward(O, c, variant)
    finally:
        O.use_cmath(False)
    st_f, of = rp.module_forward(O, c, variant)
    return st_f, {"oracle": of, "oracle_cmath": oc}


def main():
    O.build()
    os.makedirs(rp.GOLDEN_DIR, exist_ok=True)
    for case in rp.GOLDEN_CASES:
        c = rp.build_case(case)
        head = dict(scene_hash=rp.scene_hash(c.s), P=c.s.P, W=c.s.W, H=c.s.H, seed=case[5], deg=c.deg)
        st_f, parties = oracles(c, "light")
        assert parties["oracle"]["num_rendered"] > 0
        st_r, ref = rp.module_forward(R, c)
        mask, f64 = rp.compare_forward(c, ref, parties, margin_fn=lambda a: O.light_median_margin(st_f, a))
        save(rp.golden_path("light", case, "fwd"), mask=mask, **head, **{k: np.asarray(ref[k]) for k in rp.RECORDED_LIGHT})
        grads, alphas = rp.masked(rp.pixel_grads(c.s), mask), rp.arbiter_alphas(f64)
        for name, track_off, map_off in rp.MODES:
            g = rp.module_backward(R, st_r, c, alphas, grads, track_off, map_off)
            save(rp.golden_path("light", case, name.replace("+", "_")), track_off=track_off, map_off=map_off, **head, **g)
    case = rp.GOLDEN_CASES[0]
    c = rp.build_case(case)
    _, parties = oracles(c, "full")
    _, ref = rp.module_forward(R, c, "full")
    mask, _ = rp.compare_forward(c, ref, parties, "full")
    save(rp.golden_path("full", case, "fwd"), mask=mask, scene_hash=rp.scene_hash(c.s), P=c.s.P, W=c.s.W, H=c.s.H, seed=case[5],
         deg=c.deg, **{k: np.asarray(ref[k]) for k in rp.RECORDED_FULL})


if __name__ == "__main__":
    main()
