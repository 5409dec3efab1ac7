"""The float64 model of the contribution statistics (tests/contrib_model.py) on cases small enough to work out by hand: narrow
Gaussians that reach one pixel of a one-tile frame, with the n_contrib a forward would have left stated by hand for either variant's
ending rule."""
from types import SimpleNamespace

import numpy as np
import torch

import contrib_model as cm

FRAME = SimpleNamespace(P=0, W=16, H=16)
PIXEL = (5, 9)  # (x, y): the one pixel the narrow Gaussians reach
OFF = 1e-3      # their centres lie this far right of it (power = 0 exactly would be an ambiguous decision), so at PIXEL
G = float(np.exp(-0.5 * 50.0 * OFF * OFF))  # ... alpha = o G


def run(opacities, n_contrib_at_pixel, centres=None):
    """Gaussians of the given opacities, in list order, conic 50 I (one pixel away: alpha <= e^-25), all centred on PIXEL unless
    `centres` says otherwise; n_contrib is zero except at PIXEL"""
    n = len(opacities)
    s = SimpleNamespace(P=n, W=FRAME.W, H=FRAME.H)
    pix = torch.tensor([PIXEL] * n if centres is None else centres, dtype=torch.float64) + torch.tensor([OFF, 0.0], dtype=torch.float64)
    con = (torch.full((n,), 50.0, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.full((n,), 50.0, dtype=torch.float64))
    n_contrib = np.zeros((s.H, s.W), np.uint32)
    n_contrib[PIXEL[1], PIXEL[0]] = n_contrib_at_pixel
    return cm.stats(s, (pix, con, torch.tensor(opacities, dtype=torch.float64)), np.arange(n, dtype=np.uint32),
                    np.array([[0, n]], np.uint32), n_contrib)


def test_one_opaque_gaussian_over_one_pixel():
    m = run([1.0], 1)  # alpha = min(0.99, 1)
    assert m.count.tolist() == [1] and m.n_pairs == 1
    assert m.max[0] == 0.99 and m.sum[0] == 0.99
    assert abs(float(m.max32[0]) - 0.99) < 1e-7 and abs(m.sum32[0] - 0.99) < 1e-7
    assert m.ambiguous.tolist() == [0] and m.tainted.tolist() == [False]


def test_two_stacked_gaussians_with_known_alpha():
    m = run([0.5, 0.8], 2)
    assert m.count.tolist() == [1, 1]
    np.testing.assert_allclose(m.max, [0.5 * G, 0.8 * G * (1 - 0.5 * G)], rtol=0, atol=1e-15)
    np.testing.assert_allclose(m.sum, m.max, rtol=0, atol=0)
    np.testing.assert_allclose(m.max32, m.max, rtol=0, atol=1e-7)
    tol_max, tol_sum = cm.tolerances(m)
    assert (tol_max == 1e-6).all() and (tol_sum == 1e-6).all()  # (the floors: the replay is closer than that)


def test_a_gaussian_off_the_pixel_is_not_touched_and_a_neighbour_pixel_counts_on_its_own():
    # the second Gaussian sits one pixel to the right: PIXEL's list holds both, only the first reaches it
    m = run([0.5, 0.8], 2, centres=[PIXEL, (PIXEL[0] + 1, PIXEL[1])])
    assert m.count.tolist() == [1, 0]
    np.testing.assert_allclose(m.max, [0.5 * G, 0.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(m.sum, [0.5 * G, 0.0], rtol=0, atol=1e-15)


def test_the_light_ending_rule():
    """alpha 0.99, 0.9, 0.95, 0.5: T = 1, 1e-2, 1e-3; the third would leave T = 5e-5 < 1e-4, so the light forward ends the pixel
    WITHOUT blending it: n_contrib = 2, and the entry that ended the pixel lies behind it"""
    m = run([1.0, 0.9, 0.95, 0.5], 2)
    assert m.count.tolist() == [1, 1, 0, 0] and m.n_pairs == 2
    np.testing.assert_allclose(m.sum, [0.99, 0.9 * G * 0.01, 0.0, 0.0], rtol=0, atol=1e-15)


def test_the_full_ending_rule():
    """the same list in the full forward: the third entry is blended first and ends the pixel then: it IS n_contrib = 3"""
    m = run([1.0, 0.9, 0.95, 0.5], 3)
    assert m.count.tolist() == [1, 1, 1, 0] and m.n_pairs == 3
    T3 = 0.01 * (1 - 0.9 * G)
    assert T3 * (1 - 0.95 * G) < 1e-4 < T3
    np.testing.assert_allclose(m.sum, [0.99, 0.9 * G * 0.01, 0.95 * G * T3, 0.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(m.max, m.sum, rtol=0, atol=0)


def test_a_gaussian_below_the_alpha_threshold_is_skipped_not_blended():
    m = run([0.5, 0.05, 0.8], 3)  # 0.05 < 15/255
    assert m.count.tolist() == [1, 0, 1]
    np.testing.assert_allclose(m.sum, [0.5 * G, 0.0, 0.8 * G * (1 - 0.5 * G)], rtol=0, atol=1e-15)
    assert m.ambiguous.tolist() == [0, 0, 0]


def test_ambiguous_pairs_and_what_lies_behind_them():
    m = run([0.5, (15.0 / 255.0 + 5e-7) / G, 0.8, 0.3], 3)
    assert m.ambiguous.tolist() == [0, 1, 0, 0]          # (the fourth lies behind n_contrib: no pair of it is inside)
    assert m.tainted.tolist() == [False, True, True, False]
    assert cm.conditions(m) == (1 / 3, 2 / 3)
    # an ambiguous pair outside n_contrib is nobody's
    assert run([0.5, 15.0 / 255.0 / G, 0.8], 1).ambiguous.tolist() == [0, 0, 0]


def test_a_forward_state_counts_what_the_oracle_forward_blended(oracle):
    """on the CPU oracle's forward state (its records and its decisions): the weights add up to the alpha image, the records are
    taken over exactly, and the conditions the GPU tests assert hold (tests/test_hip_contrib.py)"""
    import hip_helpers as hh
    from dgr_amd.synth import make_scene
    s = make_scene(400, 64, 48, 11)
    st, ref = hh.oracle_forward(oracle, s, 3)
    means2D, conic_opacity = st.get("means2D"), st.get("conic_opacity")
    geom = cm.records(means2D, conic_opacity)
    assert geom[0].dtype == torch.float64 and np.array_equal(geom[0].numpy().astype(np.float32), means2D.reshape(-1, 2))
    assert np.array_equal(geom[2].numpy().astype(np.float32), conic_opacity.reshape(-1, 4)[:, 3])
    m = cm.stats(s, geom, st.get("point_list"), st.get("ranges"), st.get("n_contrib"))
    assert m.n_pairs == m.count.sum() > 0
    # (the image is an fp32 sum of fp32 weights: one rounding per add on a partial sum of at most 1, and the weights' own)
    assert abs(m.sum.sum() - ref["opacity_map"].astype(np.float64).sum()) <= m.n_pairs * 2.0 ** -23
    ambiguous, left_out = cm.conditions(m)
    assert ambiguous <= 0.02 and left_out <= 0.10
    assert np.array_equal(m.count > 0, m.max > 0) and (m.max <= m.sum + 1e-15).all() and (m.max <= 0.99).all()
    assert ((m.count > 0) <= (ref["radii"] > 0)).all()
    # the float32 replay of the same records stays far inside the floors the GPU tests use
    tol_max, tol_sum = cm.tolerances(m)
    assert np.abs(m.max32 - m.max).max() < 2.5e-7 and (tol_max == 1e-6).all()
