"""dgr_amd.optim.densify_and_prune (csrc/optim.hip: decide, scan, apply) against the sequential restatement of its semantics in
torch on the CPU (tests/densify_model.py).  Everything copied is compared bit for bit; the children's positions against the
model's float64 ones."""
import math

import numpy as np
import pytest
import torch

from densify_model import densify_model
from dgr_amd.optim import SparseAdam, densify_and_prune
from hip_helpers import dev
from map_step_cases import EXTRAS, assert_rebuilt, bits_equal, leaves_of, moments_of, on_device

pytestmark = pytest.mark.gpu

ROLES = ("xyz", "scaling", "rotation", "opacity")


def between(values, q):
    """a float64 value strictly between two neighbouring data values near the q-quantile, with fp32 room on both sides"""
    v = torch.unique(values.double().flatten())
    i = min(max(int(q * (v.numel() - 1)), 0), v.numel() - 2)
    while not (v[i + 1] - v[i] > 1e-5 * max(abs(float(v[i])), abs(float(v[i + 1])))):  # (a gap of a hundred fp32 steps)
        i += 1
    return float((v[i] + v[i + 1]) / 2)


def mixed_case(P, seed):
    """inputs on the CPU + the public arguments, every threshold strictly between two data values"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = leaves_of(P, g)
    M = moments_of(L, g)
    denom = torch.randint(0, 5, (P, 1), generator=g).float()
    accum = torch.rand((P, 1), generator=g) * denom * 4e-4
    maxr = torch.floor(torch.rand(P, generator=g) * 60.0)
    noise = torch.randn((P, 2, 3), generator=g)
    m = L["scaling"].max(dim=1).values
    seen = denom.flatten() > 0
    extent = math.exp(between(m, 0.90)) / 0.1                      # log(0.1 extent): ~10 % of the rows are too large
    kw = dict(grad_threshold=between((accum.flatten() / denom.flatten())[seen], 0.5), extent=extent,
              percent_dense=math.exp(between(m, 0.5)) / extent,
              min_opacity=1.0 / (1.0 + math.exp(-between(L["opacity"], 0.10))),
              max_screen_size=between(maxr, 0.88))
    # no row sits on a threshold (what the wrapper and the model form: float64, rounded once)
    f32 = lambda x: torch.tensor(x, dtype=torch.float64).float()  # noqa: E731
    assert not (accum == f32(kw["grad_threshold"]) * denom)[denom > 0].any()
    for data, t in ((m, math.log(kw["percent_dense"] * extent)), (m, math.log(0.1 * extent)), (m - f32(math.log(1.6)), math.log(0.1 * extent)),
                    (L["opacity"], math.log(kw["min_opacity"] / (1 - kw["min_opacity"]))), (maxr, kw["max_screen_size"])):
        assert not (data == f32(t)).any()
    return L, M, accum, denom, maxr, noise, kw


def run_hip(L, M, accum, denom, maxr, noise, kw, seed=0):
    """the HIP step on copies of the CPU inputs; returns (leaves, moments by name, accumulators, counts, optimiser)"""
    params, opt, _, before = on_device(L, M)
    up = lambda t: None if t is None else t.to(dev())  # noqa: E731
    out, a, dn, mr, counts = densify_and_prune(params, opt, up(accum), up(denom), up(maxr), noise=up(noise), seed=seed, **kw)
    torch.cuda.synchronize()
    assert_rebuilt(before, out, opt)
    return out, {name: opt.state[out[name]] for name in M}, (a, dn, mr), counts, opt


def check_against_model(L, M, accum, denom, maxr, noise, kw):
    ref = densify_model(L, M, accum, denom, maxr, noise, **kw)
    out, moments, accs, counts, _ = run_hip(L, M, accum, denom, maxr, noise, kw)
    assert tuple(counts) == ref["counts"], (tuple(counts), ref["counts"])
    P_new = ref["counts"][0]
    for name, t in ref["leaves"].items():
        if name == "xyz":
            continue
        assert bits_equal(out[name], t), name
    for name, (m, v) in ref["moments"].items():
        assert bits_equal(moments[name][0], m) and bits_equal(moments[name][1], v), name
    for got, like in zip(accs, (accum, denom, maxr)):
        want = torch.zeros((P_new,) + tuple(like.shape[1:] if like is not None else ()))
        assert bits_equal(got, want)
    # positions: survivors and clones bit for bit, children within 1e-5 (|xyz_c| + sum_k exp(scaling_raw_k) |n_k|)
    got, want, slack = out["xyz"].detach().cpu(), ref["leaves"]["xyz"], ref["xyz_slack"]
    assert got.shape == want.shape and got.dtype == torch.float32
    old = ~ref["fresh"] | (slack == 0).all(dim=1)
    assert torch.equal(got[old].double(), want[old])
    err = (got.double() - want).abs()
    worst = float((err / slack.clamp_min(1e-300))[~old].max()) if (~old).any() else 0.0
    print(f"P = {L['xyz'].shape[0]} -> {P_new}: counts {ref['counts']}; child xyz error / magnitude: worst {worst:.3e} (bound 1e-5)")
    assert (err <= 1e-5 * slack).all()
    return ref, out


@pytest.mark.parametrize("P", [549, 66003])
def test_mixed_case_matches_the_sequence(P):
    """two full blocks + 37 rows, and more than 256 blocks (the block-total scan loops); 9 leaves with moments + 3
    accumulators = 30 tensors, so the apply runs as two launches of the table"""
    L, M, accum, denom, maxr, noise, kw = mixed_case(P, 11 + P)
    # every kind of row is there: >= 5 % each of keep, clone, split, pruned by opacity / by screen size / by world size
    f32 = lambda x: torch.tensor(x, dtype=torch.float64).float()  # noqa: E731
    a, d, m, op = accum.flatten(), denom.flatten(), L["scaling"].max(dim=1).values, L["opacity"].flatten()
    hot = (d > 0) & (a >= f32(kw["grad_threshold"]) * d)
    split = hot & (m > f32(math.log(kw["percent_dense"] * kw["extent"])))
    by_op, by_screen = op < f32(math.log(kw["min_opacity"] / (1 - kw["min_opacity"]))), maxr > f32(kw["max_screen_size"])
    by_world = m > f32(math.log(0.1 * kw["extent"]))
    kinds = {"keep": ~hot & ~by_op & ~by_screen & ~by_world, "clone": hot & ~split, "split": split, "opacity": by_op,
             "screen": by_screen, "world": by_world, "two at once": (by_op.int() + by_screen.int() + by_world.int() + hot.int()) >= 2}
    for name, mask in kinds.items():
        assert float(mask.float().mean()) >= 0.05, (name, float(mask.float().mean()))
    ref, _ = check_against_model(L, M, accum, denom, maxr, noise, kw)
    n, s, c, k, sp = ref["counts"]
    assert n == s + c + k and 0 < k < 2 * sp and k % 2 == 0  # (some child pairs are pruned, some are not)


def quiet_case(P, seed, extras=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = leaves_of(P, g, EXTRAS if extras is None else extras)
    M = moments_of(L, g, ROLES)
    L["opacity"] = L["opacity"].clamp(-3.0, 3.0)
    L["scaling"] = L["scaling"].clamp(-4.0, -1.0)
    denom = torch.ones((P, 1))
    accum = torch.full((P, 1), 1e-5)
    maxr = torch.full((P,), 5.0)
    noise = torch.randn((P, 2, 3), generator=g)
    # extent 10: split above log(0.1) = -2.3, pruned above log(1) = 0; opacity pruned below logit(0.005) = -5.3
    kw = dict(grad_threshold=2e-4, extent=10.0, percent_dense=0.01, min_opacity=0.005, max_screen_size=20.0)
    return L, M, accum, denom, maxr, noise, kw


def test_nothing_to_do_returns_the_input_bits():
    L, M, accum, denom, maxr, noise, kw = quiet_case(549, 1)
    ref, out = check_against_model(L, M, accum, denom, maxr, noise, kw)
    assert ref["counts"] == (549, 549, 0, 0, 0)
    for name, t in L.items():
        assert bits_equal(out[name], t), name


def test_everything_pruned_leaves_empty_tensors():
    L, M, accum, denom, maxr, noise, kw = quiet_case(549, 2)
    L["opacity"] = L["opacity"] - 20.0
    accum = torch.full_like(accum, 1.0)  # hot as well: clones and children are pruned with their originals
    ref, out = check_against_model(L, M, accum, denom, maxr, noise, kw)
    assert ref["counts"][:4] == (0, 0, 0, 0) and ref["counts"][4] > 0
    for name, t in L.items():
        assert tuple(out[name].shape) == (0,) + tuple(t.shape[1:]), name


def test_everything_split_doubles_the_rows():
    L, M, accum, denom, maxr, noise, kw = quiet_case(549, 3)
    L["scaling"] = L["scaling"].clamp(-1.8, -1.0)   # above log(0.1)
    accum = torch.full_like(accum, 1.0)
    ref, _ = check_against_model(L, M, accum, denom, maxr, noise, kw)
    assert ref["counts"] == (2 * 549, 0, 0, 2 * 549, 549)


def test_everything_cloned_doubles_the_rows():
    L, M, accum, denom, maxr, noise, kw = quiet_case(549, 4)
    L["scaling"] = L["scaling"].clamp(-4.0, -2.5)   # below log(0.1)
    accum = torch.full_like(accum, 1.0)
    ref, _ = check_against_model(L, M, accum, denom, maxr, noise, kw)
    assert ref["counts"] == (2 * 549, 549, 549, 0, 0)


@pytest.mark.parametrize("hot", [False, True])
def test_one_row(hot):
    L, M, accum, denom, maxr, noise, kw = quiet_case(1, 5)
    L["scaling"] = L["scaling"].clamp(-1.8, -1.0)
    if hot:
        accum = torch.full_like(accum, 1.0)
    ref, _ = check_against_model(L, M, accum, denom, maxr, noise, kw)
    assert ref["counts"] == ((2, 0, 0, 2, 1) if hot else (1, 1, 0, 0, 0))


def test_no_rows():
    L, M, accum, denom, maxr, noise, kw = quiet_case(0, 6)
    ref, out = check_against_model(L, M, accum, denom, maxr, noise, kw)
    assert ref["counts"] == (0, 0, 0, 0, 0)
    assert tuple(out["sh48"].shape) == (0, 16, 3)


def test_without_max_screen_size_neither_size_rule_prunes():
    L, M, accum, denom, maxr, noise, kw = mixed_case(549, 21)
    big = (maxr > kw["max_screen_size"]) | (L["scaling"].max(dim=1).values > math.log(0.1 * kw["extent"]))
    assert big.sum() > 50
    kw["max_screen_size"] = None
    ref, _ = check_against_model(L, M, accum, denom, maxr, noise, kw)
    with_rule = densify_model(L, M, accum, denom, maxr, noise, **dict(kw, max_screen_size=30.0))
    assert ref["counts"][0] > with_rule["counts"][0]


def test_without_max_radii2D():
    L, M, accum, denom, maxr, noise, kw = mixed_case(549, 22)
    ref, _ = check_against_model(L, M, accum, denom, None, noise, kw)
    assert ref["counts"][0] > densify_model(L, M, accum, denom, maxr, noise, **kw)["counts"][0]


def test_nan_and_zero_denominator_rows_are_neither_hot_nor_pruned():
    P = 549
    L, M, accum, denom, maxr, noise, kw = quiet_case(P, 7)
    nan = float("nan")
    accum[10:40] = 1.0
    denom[10:40] = 0.0          # never seen: 3DGS's 0 / 0 -> 0
    accum[100:130] = nan        # a NaN accumulator compares false
    accum[300:310] = nan
    denom[300:310] = 0.0
    L["opacity"][200:230] = nan  # a NaN opacity is not below the threshold
    L["opacity"][305:308] = nan
    ref, out = check_against_model(L, M, accum, denom, maxr, noise, kw)
    assert ref["counts"] == (P, P, 0, 0, 0)
    for name, t in L.items():
        assert bits_equal(out[name], t), name


def test_on_a_side_stream_with_inputs_produced_there():
    L, M, accum, denom, maxr, noise, kw = mixed_case(549, 23)
    ref = densify_model(L, M, accum, denom, maxr, noise, **kw)
    d = dev()
    base = {name: t.to(d) for name, t in L.items()}
    up = [t.to(d) for t in (accum, denom, maxr, noise)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=d)
    with torch.cuda.stream(side):
        spin = torch.randn((2048, 2048), device=d)
        for _ in range(4):  # keep the stream busy, so that the inputs below are still being produced when the call is made
            spin = spin @ spin * 1e-3
        params = {name: (t * 2.0) * 0.5 for name, t in base.items()}  # (exact) copies produced on this stream
        a, dn, mr, nz = [(t * 2.0) * 0.5 for t in up]
        out, a2, dn2, mr2, counts = densify_and_prune(params, None, a, dn, mr, noise=nz, **kw)
    side.synchronize()
    assert tuple(counts) == ref["counts"]
    for name, t in ref["leaves"].items():
        if name != "xyz":
            assert bits_equal(out[name], t), name
    assert ((out["xyz"].cpu().double() - ref["leaves"]["xyz"]).abs() <= 1e-5 * ref["xyz_slack"]).all()
    assert not a2.any() and not dn2.any() and not mr2.any() and a2.shape == (counts.rows, 1)


def test_internal_generator_is_seeded_and_standard_normal():
    P = 20000
    g = torch.Generator(device="cpu").manual_seed(9)
    d = dev()
    params = {"xyz": torch.randn((P, 3), generator=g).to(d), "scaling": (0.3 * torch.randn((P, 3), generator=g) - 1.0).to(d),
              "rotation": torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(P, 1).to(d), "opacity": torch.zeros((P, 1), device=d)}
    accum, denom = torch.ones((P, 1), device=d), torch.ones((P, 1), device=d)
    kw = dict(grad_threshold=2e-4, extent=1.0, percent_dense=0.01)  # log(0.01) = -4.6: every row splits
    runs = [densify_and_prune(params, None, accum, denom, None, seed=s, **kw) for s in (1234, 1234, 99)]
    for out, _, _, _, counts in runs:
        assert tuple(counts) == (2 * P, 0, 0, 2 * P, P)
    x = [r[0]["xyz"] for r in runs]
    assert bits_equal(x[0], x[1]) and bits_equal(runs[0][0]["scaling"], runs[1][0]["scaling"])
    assert not bits_equal(x[0], x[2])
    spread = torch.exp(params["scaling"].double())
    z = torch.stack([(x[0][s * P:(s + 1) * P].double() - params["xyz"].double()) / spread for s in (0, 1)])  # [2, P, 3]
    assert (z[0] != z[1]).any(dim=1).all()   # the two children of a row are different draws
    n = z.numel()
    assert n == 120000
    mean, var = float(z.mean()), float(z.var())
    print(f"internal generator: mean {mean:+.5f} (bound {4 / math.sqrt(n):.5f}), variance {var:.5f} (1 +- {4 * math.sqrt(2 / n):.5f})")
    assert abs(mean) <= 4 / math.sqrt(n)
    assert abs(var - 1.0) <= 4 * math.sqrt(2.0 / n)
    assert float((z[0] * z[1]).mean()) ** 2 <= 16.0 / (n / 2)  # and uncorrelated


def test_optimizer_continues_survivors_and_starts_new_rows_from_zero():
    """three steps, densify, two more steps -- against torch.optim.Adam on the model's rows: survivors with their moments,
    new rows with zero moments, all at step count 3 -> 4, 5.  noise = 0: a child starts exactly at its parent, so the two
    chains differ by the optimisers' rounding only."""
    d, P = dev(), 549
    g = torch.Generator(device="cpu").manual_seed(31)
    L = leaves_of(P, g, {"sh48": (16, 3)})
    # margins of 0.25 and more around every threshold: a step moves a parameter by about its learning rate
    L["scaling"] = torch.where(torch.rand((P, 1), generator=g) < 0.5, -3.0 - torch.rand((P, 3), generator=g),
                               -1.0 - torch.rand((P, 3), generator=g))
    L["opacity"] = torch.where(torch.rand((P, 1), generator=g) < 0.15, torch.full((P, 1), -8.0), 2.0 * torch.rand((P, 1), generator=g))
    lrs = {"xyz": 1.6e-4, "scaling": 5e-3, "rotation": 1e-3, "opacity": 5e-2, "sh48": 2.5e-3}
    ours = {name: t.clone().to(d).requires_grad_() for name, t in L.items()}
    theirs = {name: t.clone().to(d).requires_grad_() for name, t in L.items()}
    opt = SparseAdam([{"params": [ours[n]], "lr": lrs[n]} for n in L], eps=1e-15)
    ref = torch.optim.Adam([{"params": [theirs[n]], "lr": lrs[n]} for n in L], eps=1e-15)
    for it in range(3):
        for n in L:
            grad = torch.randn(L[n].shape, generator=g).to(d)
            ours[n].grad, theirs[n].grad = grad.clone(), grad.clone()
        opt.step()
        ref.step()
    denom = torch.randint(0, 3, (P, 1), generator=g).float()
    accum = torch.where(torch.rand((P, 1), generator=g) < 0.5, 1e-3 * denom, 1e-5 * denom)
    maxr = torch.where(torch.rand(P, generator=g) < 0.1, torch.full((P,), 50.0), torch.full((P,), 3.0))
    kw = dict(grad_threshold=2e-4, extent=10.0, percent_dense=0.01, min_opacity=0.005, max_screen_size=20.0)
    for t, cut in ((L["scaling"], math.log(0.1)), (L["scaling"], 0.0), (L["opacity"], math.log(0.005 / 0.995))):
        assert float((t - cut).abs().min()) > 0.25
    noise = torch.zeros((P, 2, 3))
    cpu = lambda t: t.detach().cpu()  # noqa: E731
    model = densify_model({n: cpu(t) for n, t in theirs.items()}, {n: (cpu(ref.state[t]["exp_avg"]), cpu(ref.state[t]["exp_avg_sq"]))
                                                                   for n, t in theirs.items()}, accum, denom, maxr, noise, **kw)
    out, a, dn, mr, counts = densify_and_prune(ours, opt, accum.to(d), denom.to(d), maxr.to(d), noise=noise.to(d), **kw)
    assert tuple(counts) == model["counts"] and counts.clones > 20 and counts.children > 20 and counts.survivors < P - 40
    assert opt.steps == 3
    theirs2 = {n: model["leaves"][n].float().to(d).requires_grad_() for n in L}
    ref2 = torch.optim.Adam([{"params": [theirs2[n]], "lr": lrs[n]} for n in L], eps=1e-15)
    for n in L:
        m, v = model["moments"][n]
        assert not m[model["fresh"]].any() and not v[model["fresh"]].any()
        ref2.state[theirs2[n]] = {"step": torch.tensor(3.0), "exp_avg": m.to(d).clone(), "exp_avg_sq": v.to(d).clone()}
    for it in range(2):
        for n in L:
            grad = torch.randn(theirs2[n].shape, generator=g).to(d)
            out[n].grad, theirs2[n].grad = grad.clone(), grad.clone()
        opt.step()   # visible=None: every row, the new ones included
        ref2.step()
        for n in L:
            np.testing.assert_allclose(cpu(out[n]).numpy(), cpu(theirs2[n]).numpy(), rtol=2e-6, atol=1e-7, err_msg=n)
    assert opt.steps == 5


def test_a_capturing_stream_is_refused_and_the_capture_goes_on():
    d = dev()
    L, M, accum, denom, maxr, noise, kw = quiet_case(64, 8, extras={})
    params = {name: t.to(d) for name, t in L.items()}
    accum, denom = accum.to(d), denom.to(d)
    x = torch.arange(8, device=d, dtype=torch.float32)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=d)
    side.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(RuntimeError, match="hipGraph"):
                densify_and_prune(params, None, accum, denom, None, **kw)
            y = x * 2.0 + 1.0   # the capture is still alive: this is recorded
    torch.cuda.current_stream(d).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, x * 2.0 + 1.0)
    # and outside the capture the same call works
    out, _, _, _, counts = densify_and_prune(params, None, accum, denom, None, **kw)
    assert tuple(counts) == (64, 64, 0, 0, 0) and bits_equal(out["xyz"], L["xyz"])


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_a_degree_zero_model_with_an_empty_f_rest(capturable):
    """3DGS's degree-0 model has f_rest [P, 0, 3]: the step runs, f_rest and its moments come back [rows, 0, 3], and everything
    else carries the bits of the same call without that leaf (tests/degree_zero.py) -- before and after a further step()."""
    import degree_zero
    d, P = dev(), 549
    L, _, accum, denom, maxr, noise, kw = mixed_case(P, 11 + P)
    seen = {}
    for with_rest in (False, True):
        params = degree_zero.model(L, d, with_rest)
        opt = degree_zero.stepped_adam(params, capturable)
        out, a, dn, mr, counts = densify_and_prune(params, opt, accum.to(d), denom.to(d), maxr.to(d), noise=noise.to(d), **kw)
        assert counts.rows not in (0, P) and counts.clones > 0 and counts.children > 0 and counts.survivors < P
        after = degree_zero.snapshot(out, opt, xyz_gradient_accum=a, denom=dn, max_radii2D=mr, counts=tuple(counts))
        if with_rest:
            degree_zero.check_rest(out, opt, counts.rows)
        degree_zero.step_again(opt, out, capturable)
        assert opt.steps == 2 + (1 if capturable else 0)  # (the replays advance the device's count only)
        seen[with_rest] = (after, degree_zero.snapshot(out, opt))
    for with_leaf, without in zip(seen[True], seen[False]):
        degree_zero.assert_same_bits(with_leaf, without)
