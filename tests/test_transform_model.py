"""The float64 model of the map correction (tests/transform_model.py) without a GPU: its own properties (the colour a rotated
Gaussian shows from a rotated direction, orthogonality, composition, the covariance), the constant table of csrc/transform.hip
against it, the fp32 replica of the kernels' operation order inside the derived bars, and the mutants outside them."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import fp64_model
import transform_model as tm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diff-gaussian-rasterization_amd", "csrc")
KINDS = [("xyz", 3, 0, (tm.VALUE, tm.MOMENT1, tm.MOMENT2)), ("quat", 4, 0, (tm.VALUE, tm.MOMENT1, tm.MOMENT2)),
         ("log_scale", 3, 0, (tm.VALUE,)), ("sh", 9, 0, (tm.VALUE, tm.MOMENT1, tm.MOMENT2)),
         ("sh", 24, 0, (tm.VALUE, tm.MOMENT1, tm.MOMENT2)), ("sh", 45, 0, (tm.VALUE, tm.MOMENT1, tm.MOMENT2)),
         ("sh", 48, 3, (tm.VALUE, tm.MOMENT1, tm.MOMENT2)), ("sh", 12, 3, (tm.VALUE,)), ("sh", 27, 3, (tm.VALUE,))]


def generator():
    sys.path.insert(0, CSRC)
    try:
        import gen_sh_rotation_table
    finally:
        sys.path.remove(CSRC)
    return gen_sh_rotation_table


def rotate_sh(sh, R, C):
    """[V, 16, 3] coefficients under R: every band by its matrix, the DC row as it is"""
    out = sh.copy()
    for l in (1, 2, 3):
        out[:, l * l:(l + 1) ** 2] = np.einsum("ij,vjc->vic", tm.band_matrix(l, R, C), sh[:, l * l:(l + 1) ** 2])
    return out


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_a_rotated_gaussian_shows_the_same_colour_from_the_rotated_direction(deg):
    rng = np.random.RandomState(deg)
    for _ in range(5):
        R = tm.random_rotation(rng)
        sh = rng.standard_normal((40, 16, 3))
        d = rng.standard_normal((40, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        before = fp64_model.sh_to_rgb(deg, torch.tensor(sh), torch.tensor(d), clamp=False)
        after = fp64_model.sh_to_rgb(deg, torch.tensor(rotate_sh(sh, R, tm.C64)), torch.tensor(d @ R.T), clamp=False)
        assert float((before - after).abs().max()) < 1e-12
        # the kernels' fp32 constants give matrices within two fp32 roundings of these
        assert max(np.abs(tm.band_matrix(l, R, tm.C32) - tm.band_matrix(l, R, tm.C64)).max() for l in (1, 2, 3)) < 2.0 ** -23


def test_band_matrices_are_orthogonal_and_compose():
    rng = np.random.RandomState(11)
    for _ in range(5):
        R1, R2 = tm.random_rotation(rng), tm.random_rotation(rng)
        for l in (1, 2, 3):
            M1, M2, M12 = tm.band_matrix(l, R1, tm.C64), tm.band_matrix(l, R2, tm.C64), tm.band_matrix(l, R1 @ R2, tm.C64)
            # (orthogonal where the band's constants make the basis orthonormal up to one factor: they do, up to rounding)
            assert np.abs(M1 @ np.linalg.inv(M1) - np.eye(2 * l + 1)).max() < 1e-13
            assert np.abs(M1 @ M1.T - np.eye(2 * l + 1)).max() < 1e-7, l
            assert np.abs(M12 - M1 @ M2).max() < 1e-13, l
    assert np.abs(tm.band_matrix(3, np.eye(3)) - np.eye(7)).max() < 1e-14


def test_the_new_quaternion_and_scale_give_the_transformed_covariance():
    rng = np.random.RandomState(12)
    for s in (1.0, 0.5, 3.0):
        plan = tm.plan_model(tm.random_sim3(rng, s))
        assert abs(plan["s"] - s) < 1e-6 * s and np.abs(plan["R"] * plan["s"] - plan["A"]).max() < 1e-6 * s
        q, log_scale = rng.standard_normal(4), rng.standard_normal(3)
        Rq = tm.rotation_of(q / np.linalg.norm(q))
        cov = Rq @ np.diag(np.exp(2 * log_scale)) @ Rq.T
        q_new = tm.quat_left(plan["q"]) @ q
        assert abs(np.linalg.norm(q_new) - np.linalg.norm(q)) < 1e-14  # the norm is kept
        Rn = tm.rotation_of(q_new / np.linalg.norm(q_new))
        cov_new = Rn @ np.diag(np.exp(2 * (log_scale + plan["log_s"]))) @ Rn.T
        want = plan["s"] ** 2 * plan["R"] @ cov @ plan["R"].T
        assert np.abs(cov_new - want).max() < 1e-12 * np.abs(want).max()


def test_invalid_transforms_and_the_branches_of_the_quaternion():
    rng = np.random.RandomState(13)
    T = tm.random_sim3(rng, 2.0)
    bad = [T.copy() for _ in range(4)]
    bad[0][1, 2] = np.nan
    bad[1][:3, 0] *= -1  # a reflection
    bad[2][0, 0] *= 1.01  # a shear beyond the tolerance
    bad[3][3, 0] = np.inf  # (the bottom row is only tested for being finite)
    assert all(tm.plan_model(b) is None for b in bad) and tm.plan_model(T) is not None
    # half turns about each axis and one generic rotation: all four branches, R(q) = N each time
    for N in (np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1]), tm.random_rotation(rng)):
        assert np.abs(tm.rotation_of(tm.shepperd(N)) - N).max() < 1e-14


def test_the_constant_table_is_the_generators_and_well_conditioned():
    gen = generator()
    out = io.StringIO()
    with redirect_stdout(out):
        gen.main()
    assert out.getvalue() == open(os.path.join(CSRC, "sh_rotation_table.h")).read(), "sh_rotation_table.h is not the generator's output"
    dirs = gen.search()
    rng = np.random.RandomState(14)
    for l in (1, 2, 3):
        Y = gen.sample_matrix(l, dirs)
        assert np.linalg.cond(Y) < 5.0, (l, np.linalg.cond(Y))
        # the kernels' way, M_l = Y_l(R d) Y_l^-1, against the model's least squares; the generator's basis against the model's
        R = tm.random_rotation(rng)
        Yr = np.stack([gen.band(l, R @ d) for d in dirs[:2 * l + 1]], axis=1)
        assert np.abs(Yr @ np.linalg.inv(Y) - tm.band_matrix(l, R, tm.C32)).max() < 1e-13
        assert np.array_equal(Y, tm.band(l, dirs[:2 * l + 1], tm.C32))


def make_case(P, K, seed, scales=(1.0, 0.5, 3.0)):
    rng = np.random.RandomState(seed)
    transforms = np.stack([tm.random_sim3(rng, scales[k % len(scales)]) for k in range(K)])
    anchor = rng.randint(0, K, P).astype(np.float32)
    return rng, transforms, anchor


def test_classify_counts_every_kind_of_row():
    rng, transforms, _ = make_case(8, 3, 20)
    transforms[1, 0, 0] = np.nan
    plans = [tm.plan_model(T) for T in transforms]
    anchor = np.array([0, 1, 2, -1, 3, 2.5, np.nan, -0.0], np.float32)
    idx, counts = tm.classify(anchor, plans, 8)
    assert idx.tolist() == [0, -1, 2, -1, -1, -1, -1, 0] and counts == (3, 4, 1, 1)
    idx, counts = tm.classify(None, plans, 5)
    assert idx.tolist() == [0] * 5 and counts == (5, 0, 1, 0)


@pytest.mark.parametrize("kind, k, skip, orders", KINDS, ids=[f"{c[0]}{c[1]}" for c in KINDS])
def test_the_fp32_replica_lies_inside_the_bars_and_the_mutants_outside(kind, k, skip, orders):
    P, K = 300, 4
    rng, transforms, anchor = make_case(P, K, 30 + k)
    transforms[3, :3, 1] *= -1  # transform 3: a reflection, its rows stay
    anchor[::17] = -1
    plans = [tm.plan_model(T) for T in transforms]
    idx, counts = tm.classify(anchor, plans, P)
    assert counts[0] > 150 and counts[3] > 20 and counts[2] == 1
    for order in orders:
        t = rng.standard_normal((P, k)).astype(np.float32)
        if order == tm.MOMENT2:
            t = np.abs(t)
        want, bar = tm.transform_model(t, kind, order, idx, plans, skip)
        got = tm.replica(t, kind, order, idx, plans, skip)
        with np.errstate(invalid="ignore"):  # (0 / 0 at the DC row of a combined leaf)
            ratio = np.abs(got.astype(np.float64) - want)[idx >= 0] / bar[idx >= 0]
        print(f"{kind} k = {k} order {order}: worst error / bar = {np.nanmax(ratio):.3f}")
        assert tm.within(got, want, bar)
        assert np.array_equal(got[idx < 0].view(np.int32), t[idx < 0].view(np.int32))
        if order == tm.MOMENT2:
            assert (want >= 0).all() and (got >= 0).all()
        relevant = {"xyz": ["anchor_off_by_one"] + (["moment1_times_s"] if order == tm.MOMENT1 else []),
                    # (L o L of the right product is that of the left one: the second moment cannot tell them apart)
                    "quat": ["anchor_off_by_one"] + (["quat_right"] if order != tm.MOMENT2 else []), "log_scale": ["no_log_s", "anchor_off_by_one"],
                    "sh": ["sh_unrotated", "sh_transposed", "anchor_off_by_one"] + (["dc_rotated"] if skip else [])}[kind]
        for mutant in relevant:
            assert not tm.within(tm.replica(t, kind, order, idx, plans, skip, mutant=mutant), want, bar), (mutant, order)


def test_every_mutant_is_exercised():
    assert set(tm.MUTANTS) == {"sh_unrotated", "sh_transposed", "quat_right", "moment1_times_s", "no_log_s", "anchor_off_by_one",
                               "dc_rotated"}
    assert tm.WORST_ROUNDINGS == max(max(tm.ROUNDINGS["sh"](3)), *tm.ROUNDINGS["xyz"], *tm.ROUNDINGS["quat"]) + 1
