"""The tests of tests/step_model.py tested on the CPU: every float32 replica of a step kernel is inside the bars its GPU test
(tests/test_hip_step_kernels.py) uses, every listed wrong variant of a model is outside them, and the Python wrappers refuse bad
arguments on the host before the library is loaded.  This is what shows, without a GPU, that the chosen inputs can tell a subtly
wrong kernel from a right one."""
import math

import numpy as np
import pytest
import torch

import step_model as sm

ROWS, ROW_SHAPE = sm.ADAM_SHAPES[-1]  # 1000 x 45
K = math.prod(ROW_SHAPE)


def _as32(*arrays):
    return tuple(np.asarray(a).astype(np.float32) for a in arrays)


# ---- Adam ----
@pytest.mark.parametrize("step", sm.ADAM_STEPS)
@pytest.mark.parametrize("eps", sm.ADAM_EPS)
def test_adam_replica_meets_the_bars(eps, step):
    hyper, inp, visible = sm.adam_hyper(eps), sm.adam_inputs(ROWS * K), sm.adam_visible("mixed", ROWS)
    rep = sm.adam_check(inp, K, visible, hyper, step, *sm.adam_replica32(inp, K, visible, hyper, step))
    print(rep)
    rep.check(f"host form, eps {eps}, step {step}")
    # and the float64 model itself, rounded once
    sm.adam_check(inp, K, visible, hyper, step, *_as32(*sm.adam_model(inp, K, visible, hyper, step))).check("model")


@pytest.mark.parametrize("step", sm.ADAM_CAPTURABLE_STEPS)
@pytest.mark.parametrize("eps", sm.ADAM_EPS)
def test_capturable_adam_replica_meets_the_bars(eps, step):
    hyper, inp = sm.adam_hyper(eps), sm.adam_inputs(ROWS * K)
    rep = sm.adam_check(inp, K, None, hyper, step, *sm.adam_replica32(inp, K, None, hyper, step, capturable=True), capturable=True)
    print(rep)
    rep.check(f"capturable form, eps {eps}, step {step}")


@pytest.mark.parametrize("step", sm.ADAM_STEPS)
@pytest.mark.parametrize("eps", sm.ADAM_EPS)
@pytest.mark.parametrize("mutant", sm.ADAM_MUTANTS_FORMULA)
def test_adam_formula_mutants_are_refused(mutant, eps, step):
    """Against the LOOSER of the two parameter bars (the capturable form's), at least 5 % of the elements must miss at every
    (eps, step) where the mutant is another function; where it is the same function (a bias that is 1.0 at this step) it passes.

    Measured on these inputs (betas 0.9, 0.999): 6.8 % (`eps_before_bias` at eps = 1e-15, step 1, where the looser bar is 2048 U |u|
    and the misplaced eps shows only for sqrt(v) < 8e-12) to 98 % of the elements miss."""
    hyper, inp = sm.adam_hyper(eps), sm.adam_inputs(ROWS * K)
    out = _as32(*sm.adam_model(inp, K, None, hyper, step, mutant))
    rep = sm.adam_check(inp, K, None, hyper, step, *out, capturable=True)
    print(mutant, eps, step, rep)
    worst, outside = rep["p"]
    if sm.adam_mutant_differs(mutant, hyper, step):
        assert outside >= 0.05, f"{mutant} at eps {eps}, step {step}: only {100 * outside:.2f} % of the elements miss the bar"
    else:
        rep.check(f"{mutant} is the correct formula at step {step}")


def test_no_bias1_differs_at_steps_1_and_2_only():
    hyper = sm.adam_hyper(1e-8)
    assert [s for s in sm.ADAM_STEPS if sm.adam_mutant_differs("no_bias1", hyper, s)] == [1, 2]
    assert [s for s in sm.ADAM_STEPS if sm.adam_mutant_differs("no_bias2", hyper, s)] == [1, 2, 1000]


@pytest.mark.parametrize("mutant,shape,pattern", [("row_mod_rows", sm.ADAM_SHAPES[3], "mixed"), ("row_mod_rows", sm.ADAM_LARGE, "mod7"),
                                                  ("visible_lt_0", sm.ADAM_SHAPES[1], "mixed"), ("first_pass_only", sm.ADAM_LARGE, "mod7"),
                                                  ("first_pass_only", sm.ADAM_LARGE, "none")])
def test_adam_index_mutants_are_refused(mutant, shape, pattern):
    rows, row_shape = shape
    k = math.prod(row_shape)
    hyper, inp, visible = sm.adam_hyper(1e-15), sm.adam_inputs(rows * k), sm.adam_visible(pattern, rows)
    good = sm.adam_check(inp, k, visible, hyper, 2, *_as32(*sm.adam_model(inp, k, visible, hyper, 2)))
    good.check("the model")
    bad = sm.adam_check(inp, k, visible, hyper, 2, *_as32(*sm.adam_model(inp, k, visible, hyper, 2, mutant)))
    print(mutant, bad)
    assert not bad.ok


def test_the_large_adam_case_is_just_past_one_grid_pass():
    rows, row_shape = sm.ADAM_LARGE
    n = rows * math.prod(row_shape)
    assert sm.ADAM_GRID_PASS < n < sm.ADAM_GRID_PASS + 512 and all(r * math.prod(s) < sm.ADAM_GRID_PASS for r, s in sm.ADAM_SHAPES)
    second = sm.adam_selected(n, 48, sm.adam_visible("mod7", rows))[sm.ADAM_GRID_PASS:]
    assert second.any() and not second.all()  # the second pass meets visible and invisible rows


# ---- densification statistics ----
@pytest.mark.parametrize("rows", sm.STATS_ROWS)
def test_stats_replica_meets_the_bars(rows):
    inp = sm.stats_inputs(rows)
    rep = sm.stats_check(inp, *sm.stats_model(inp, dtype=np.float32))
    print(rep)
    rep.check(f"{rows} rows")
    if rows > 1:  # what a kernel that looked at the rows it must skip would do: the NaN gradients come through
        seen_all = dict(inp, radii=np.abs(inp["radii"]) + 1)
        assert not sm.stats_check(inp, *sm.stats_model(seen_all, dtype=np.float32)).ok


# ---- pose ----
def test_pose_replica_meets_the_bars():
    rep = sm.pose_check(sm.pose_outputs(np.float32))
    print(rep)
    rep.check("float32 replica")
    sm.pose_check(sm.pose_outputs(np.float64)).check("the closed form in float64")
    labels = sm.pose_cases()["label"]
    assert len(labels) == 2 * 3 * (sm.POSE_RANDOM + 7)


@pytest.mark.parametrize("mutant", sm.POSE_MUTANTS)
def test_pose_mutants_are_refused(mutant):
    rep = sm.pose_check(sm.pose_outputs(np.float64, mutant))
    print(mutant, rep)
    assert rep["dq"][0] > 1.0  # (every one of them is a wrong dq)
    if mutant == "no_projection":
        assert rep["q . dq"][0] > 1.0


# ---- L1 ----
@pytest.mark.parametrize("shapes", sm.L1_SHAPES, ids=lambda s: "x".join(map(str, s[0])) + "+" + "x".join(map(str, s[1])))
@pytest.mark.parametrize("family", sm.L1_FAMILIES)
def test_l1_replica_meets_the_bars_and_the_mutants_do_not(family, shapes):
    inp = sm.l1_inputs(family, shapes)
    loss64, dc, dd = sm.l1_model(inp)
    rep = sm.l1_check(inp, family, sm.l1_replica32(inp), dc, dd)
    print(rep)
    rep.check(f"{family} {shapes}")
    n_c, n_d = inp["color"].size, inp["depth"].size
    reached = {"forward_first_term_only": max(n_c, n_d) > sm.L1_FORWARD_THREADS,
               "backward_first_pass_only": max(n_c, n_d) > sm.L1_BACKWARD_PASS, "n_from_color": n_d > n_c}
    for mutant in sm.L1_MUTANTS:
        loss_m, dc_m, dd_m = sm.l1_model(inp, mutant)
        assert sm.l1_check(inp, family, np.float32(loss_m), dc_m, dd_m).ok == (not reached[mutant]), mutant


def test_l1_shapes_reach_every_pass():
    sizes = [(math.prod(c), math.prod(d)) for c, d in sm.L1_SHAPES]
    assert max(sizes[1]) < sm.L1_FORWARD_THREADS < sizes[2][0] < sm.L1_BACKWARD_PASS < sizes[3][0]
    assert sizes[4][1] > sm.L1_BACKWARD_PASS and sizes[4][1] > sizes[4][0]


# ---- the wrappers refuse on the host, before the library is loaded ----
@pytest.fixture
def no_library(monkeypatch):
    from dgr_amd import _capi
    monkeypatch.setattr(_capi, "load", lambda: pytest.fail("the library was loaded before the arguments were refused"))


def test_l1_loss_refuses_on_the_host(no_library):
    from dgr_amd import slam
    c, d = torch.zeros((3, 4, 5)), torch.zeros((1, 4, 5))
    with pytest.raises(ValueError, match="float32"):
        slam.l1_loss(c.double(), d, c.double(), d)
    with pytest.raises(ValueError, match="float32"):
        slam.l1_loss(c, d, c, d.to(torch.int32))
    with pytest.raises(ValueError, match="differ in shape"):
        slam.l1_loss(c, d, torch.zeros((3, 5, 4)), d)
    with pytest.raises(ValueError, match="differ in shape"):
        slam.l1_loss(c, d, c, torch.zeros((4, 5)))
    with pytest.raises(ValueError, match="must be a tensor"):
        slam.l1_loss(c, d, c.numpy(), d)
    with pytest.raises(ValueError, match="GPU tensors"):
        slam.l1_loss(c, d, c, d)  # a CPU image


def test_pose_to_camera_refuses_on_the_host(no_library):
    from dgr_amd import slam
    q, t = torch.tensor([1.0, 0, 0, 0]), torch.zeros(3)
    for bad_q, bad_t in ((q.double(), t), (q, t.double()), (q[:3], t), (q, torch.zeros(4)), (q, t)):  # dtype, length, a CPU pose
        with pytest.raises(ValueError, match="pose_to_camera"):
            slam.pose_to_camera(bad_q, bad_t, *sm.TANFOV)


def test_sparse_adam_refuses_on_the_host_and_keeps_its_state(no_library):
    from dgr_amd.optim import SparseAdam
    p = torch.zeros((6, 3), requires_grad=True)
    p.grad = torch.ones((6, 3))
    for capturable in (False, True):
        opt = SparseAdam([p], capturable=capturable)
        for visible, match in ((torch.ones(6), "bool or integer"), (torch.ones(6, dtype=torch.float64), "bool or integer"),
                               ([1] * 6, "bool or integer"), (torch.ones(5, dtype=torch.int32), "one entry per row"),
                               (torch.ones((6, 3), dtype=torch.bool), "one entry per row"),
                               (torch.ones(6, dtype=torch.int32), "on the GPU"), (None, "on the GPU")):  # (a CPU parameter)
            with pytest.raises(RuntimeError, match=match):
                opt.step(visible=visible)
            assert opt.steps == 0 and opt._step_dev is None and opt.state == {}


def test_densification_stats_refuse_on_the_host(no_library):
    from dgr_amd.optim import add_densification_stats
    P = 5
    d, r, a = torch.zeros((P, 3)), torch.zeros(P, dtype=torch.int32), torch.zeros(P)
    for args in ((d, r, a, a, a), (d, r.long(), None, None, None), (d[:, :2], r, None, None, None), (d.double(), r, None, None, None),
                 (d, r, torch.zeros(P + 1), None, None), (d, r, None, a.double(), None)):
        with pytest.raises(RuntimeError, match="add_densification_stats"):
            add_densification_stats(*args)
