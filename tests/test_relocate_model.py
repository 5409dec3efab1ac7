"""The relocation model's own identities (tests/relocate_model.py), without a GPU: what the GPU tests trust it for."""
import math

import numpy as np
import pytest

from relocate_model import MAX_COPIES, logit_threshold, new_raw_values, new_values, relocate_model, sample_sources, weight

OPACITIES = (0.006, 0.05, 0.3, 0.5, 0.9, 0.999, 0.999999)


@pytest.mark.parametrize("o", OPACITIES)
def test_one_copy_is_the_identity(o):
    o1, coeff = new_values(o, 1)
    slack = 4 * 2.0 ** -52 / min(o, 1 - o)  # 1 - (1 - o) rounds twice at magnitude 1; the ratio and the logit see it relative to o, 1 - o
    assert abs(o1 - o) <= 2 * 2.0 ** -52 and abs(coeff - 1.0) <= slack
    raw = math.log(o / (1 - o))
    new_raw, log_coeff = new_raw_values(np.float32(raw), 1, 0.005)
    assert abs(new_raw - float(np.float32(raw))) <= 8 * slack and abs(log_coeff) <= 2 * slack


@pytest.mark.parametrize("o", OPACITIES)
@pytest.mark.parametrize("N", [2, 3, 7, 20, MAX_COPIES])
def test_the_copies_together_are_as_opaque_as_the_one(o, N):
    o1, _ = new_values(o, N)
    assert abs((1.0 - (1.0 - o1) ** N) - o) <= 1e-12


@pytest.mark.parametrize("o", OPACITIES)
def test_the_scale_factor_decreases_with_the_number_of_copies(o):
    coeffs = [new_values(o, N)[1] for N in range(1, MAX_COPIES + 1)]
    assert coeffs[0] == pytest.approx(1.0, abs=1e-15)
    assert all(b < a for a, b in zip(coeffs, coeffs[1:]))
    assert all(0.0 < c <= 1.0 + 1e-15 for c in coeffs)


def test_float32_would_not_do():
    """the cancellation in 1 - (1 - o)^(1/N) that makes float64 part of the contract"""
    o, N = np.float32(0.006), 51
    o32 = np.float32(1) - np.power(np.float32(1) - o, np.float32(1.0 / N))
    o64 = 1.0 - (1.0 - float(o)) ** (1.0 / N)
    assert abs(float(o32) - o64) / o64 > 1e-5


def raws():
    # rows: 0 dead, 1 live, 2 NaN, 3 dead, 4 live, 5 +inf, 6 live, 7 -inf, 8 dead
    return np.array([-9.0, 0.25, np.nan, -7.5, 2.0, np.inf, -1.0, -np.inf, -6.0], dtype=np.float32)


def test_the_extreme_draws_give_the_first_and_the_last_live_row():
    raw = raws()
    for d, want in ((0, 1), (2 ** 32 - 1, 6)):
        dead, live, source, hits, S = sample_sources(raw, np.full(9, d), 0.005)
        assert list(np.flatnonzero(dead)) == [0, 3, 8] and list(np.flatnonzero(live)) == [1, 4, 6]
        assert S == weight(raw[1]) + weight(raw[4]) + weight(raw[6])
        assert list(source) == [want, -1, -1, want, -1, -1, -1, -1, want] and hits[want] == 3 and hits.sum() == 3


def test_a_draw_lands_in_proportion_to_the_weights():
    raw = raws()
    w = [weight(raw[i]) for i in (1, 4, 6)]
    S = sum(w)
    for d in range(0, 2 ** 32, 2 ** 32 // 997):
        _, _, source, _, _ = sample_sources(raw, np.full(9, d), 0.005)
        t = (d * S) >> 32
        assert source[0] == (1 if t < w[0] else 4 if t < w[0] + w[1] else 6)


def test_nothing_live_relocates_nothing():
    raw = np.array([-9.0, np.nan, -8.0], dtype=np.float32)
    dead, live, source, hits, S = sample_sources(raw, np.zeros(3, dtype=np.int64), 0.005)
    assert S == 0 and dead.sum() == 2 and live.sum() == 0 and (source == -1).all() and hits.sum() == 0


def test_the_inputs_are_refused_on_a_threshold():
    with pytest.raises(AssertionError):
        sample_sources(np.array([float(logit_threshold(0.005)), 1.0], dtype=np.float32), np.zeros(2, dtype=np.int64), 0.005)


def test_the_whole_step_writes_what_the_semantics_say():
    P = 9
    rng = np.random.default_rng(0)
    leaves = {"xyz": rng.standard_normal((P, 3)), "scaling": rng.standard_normal((P, 3)) - 2, "rotation": rng.standard_normal((P, 4)),
              "opacity": raws().reshape(P, 1), "f": rng.standard_normal((P, 2, 2))}
    leaves = {k: v.astype(np.float32) for k, v in leaves.items()}
    moments = {k: (np.ones_like(v), np.ones_like(v)) for k, v in leaves.items()}
    accs = {"denom": np.ones((P, 1), dtype=np.float32), "max_radii2D": None}
    draws = np.array([0, 0, 0, 2 ** 32 - 1, 0, 0, 0, 0, 1], dtype=np.int64)
    out = relocate_model(leaves, moments, accs, draws)
    assert out["counts"] == (3, 3, 3, 2, 2) and list(out["source"]) == [1, -1, -1, 6, -1, -1, -1, -1, 1]
    touched = np.array([1, 1, 0, 1, 0, 0, 1, 0, 1], dtype=bool)
    for name, t in out["leaves"].items():
        same = t.view(np.int32) == leaves[name].view(np.int32)
        assert same[~touched].all(), name
        if name not in ("opacity", "scaling"):
            assert same[1].all() and same[6].all(), name
            assert (t[0].view(np.int32) == leaves[name][1].view(np.int32)).all() and (t[3].view(np.int32) == leaves[name][6].view(np.int32)).all()
    op = out["leaves"]["opacity"].reshape(P)
    assert op[0] == op[1] == op[8] and op[3] == op[6] and op[1] < leaves["opacity"][1, 0] and op[6] < leaves["opacity"][6, 0]
    sc = out["leaves"]["scaling"]
    assert (sc[0] == sc[1]).all() and (sc[1] < leaves["scaling"][1]).all()
    # three copies of row 1 are together as opaque as it was
    o_new, o_old = 1 / (1 + math.exp(-float(op[1]))), 1 / (1 + math.exp(-0.25))
    assert abs(1 - (1 - o_new) ** 3 - o_old) < 1e-6
    for m in out["moments"]["f"]:
        assert (m[touched] == 0).all() and (m[~touched] == 1).all()
    assert list(out["accs"]["denom"].reshape(P)) == [0, 1, 1, 0, 1, 1, 1, 1, 0] and out["accs"]["max_radii2D"] is None
