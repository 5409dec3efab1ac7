"""The pose-graph optimiser on the GPU (slam.pose_graph_optimize; include/dgr_hip.h: dgr_pgo_plan, dgr_pgo_solve) against the
float64 model of tests/pgo_model.py, which shares no path with the kernel: the reference ring graphs (stationarity by an
independent autograd gradient, the poses, the reported cost), every edge shape the kernel has a path for, the three kinds of
information, Huber, a rejected step, the Log at large angles, the same bits on every run and under a hipGraph replay.

The figures behind the three measured bounds are in profiles/pgo/measured.txt; every test prints its own before it asserts."""
import functools
import math

import pytest
import torch

import pgo_model as M
from dgr_amd import slam

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F64 = torch.float64
# g_kernel <= STATIONARITY_MARGIN * g_round: twice the worst ratio measured on the MI355X, which is 1.0000 at K = 12 and at K = 40
# (the kernel's result IS the model's optimum rounded to fp32 there); the issue's cap is 8
STATIONARITY_MARGIN = 2.0
# |pose - model's|, element-wise: twice the worst difference measured on the MI355X over every comparison of this file, 2.384e-7 (the
# K = 1025 chain: one fp32 ulp of a translation entry in [2, 4); every other case is below 3e-8); the issue's cap is 2e-4
POSE_TOL = 4.8e-7
# chi2 against the model's at iterations = 0, relative: twice the worst measured on the MI355X, 2.99e-8 (round-to-nearest storage
# of chi2 as fp32 costs at most 2^-24 = 5.96e-8 on any input, so the bound leaves room for that alone); the issue's cap is 1e-3
LOG_RTOL = 6.0e-8


def dev(g):
    """the model's graph as the device tensors the solver takes (poses and measurements rounded to fp32 once) and, from those same
    fp32 bits, the float64 problem the model solves"""
    vm, Z = M.to_viewmatrices(g["T0"]).to(DEV), M.to_viewmatrices(g["Z"]).to(DEV)
    out = dict(vm=vm, Z=Z, edges=g["edges"].to(torch.int32).to(DEV), info=g["Omega"].to(torch.float32).to(DEV),
               fixed=g["fixed"].to(DEV), T0=M.from_viewmatrices(vm.cpu()), Zm=M.from_viewmatrices(Z.cpu()), long=g["edges"],
               Omega=g["Omega"].to(torch.float32).to(F64), fixed_cpu=g["fixed"])
    return out


def run(d, **kw):
    kw.setdefault("information", d["info"])
    kw.setdefault("fixed", d["fixed"])
    return slam.pose_graph_optimize(d["vm"], d["edges"], d["Z"], **kw)


def model(d, keep=None, **kw):
    keep = slice(None) if keep is None else keep
    return M.solve(d["T0"], d["long"][keep], d["Zm"][keep], d["Omega"][keep], d["fixed_cpu"], **kw)


def pose_diff(res, ref_T):
    return float((res.viewmatrices.cpu().reshape(-1, 4, 4) - M.to_viewmatrices(ref_T)).abs().max())


def stats(res):
    names = ("initial", "final", "ok", "run", "accepted", "rejected", "cg", "lam", "w", "v", "g", "used", "skipped", "loose",
             "converged", "zero")
    return dict(zip(names, res.stats.tolist()))


@functools.lru_cache(maxsize=None)
def ring(K, loops):
    d = dev(M.ring_graph(K, loops))
    return d, model(d, iterations=10)


# ---------------------------------------------------------------------------------------------------------- reference graphs
@pytest.mark.parametrize("K, loops", [(12, 1), (40, 2)])
def test_the_ring_ends_at_the_stationary_point_of_the_stated_cost(K, loops):
    d, ref = ring(K, loops)
    res = run(d, return_chi2=True)
    s = stats(res)
    args = (d["long"], d["Zm"], d["Omega"], d["fixed_cpu"])
    g_start = M.gradient_norm(d["T0"], *args)
    g_kernel = M.gradient_norm(M.from_viewmatrices(res.viewmatrices.cpu()), *args)
    g_round = M.gradient_norm(M.from_viewmatrices(M.to_viewmatrices(ref["T"])), *args)
    diff = pose_diff(res, ref["T"])
    moved = float((res.viewmatrices.cpu() - d["vm"].cpu()).abs().max())
    cost64 = float(M.cost(M.from_viewmatrices(res.viewmatrices.cpu()), d["long"], d["Zm"], d["Omega"]))
    print(f"pgo-figure ring K={K}: cost {s['initial']:.6g} -> {s['final']:.6g} (model {ref['costs'][-1]:.6g}), gradient {g_start:.4g} -> "
          f"g_kernel {g_kernel:.4e}, g_round {g_round:.4e}, ratio {g_kernel / g_round:.4f}, pose diff {diff:.3e}, moved {moved:.3e}, "
          f"trials {s['run']:.0f}, cg {s['cg']:.0f}, cost rel {abs(s['final'] - cost64) / cost64:.2e}")
    assert s["ok"] == 1 and s["used"] == d["edges"].shape[0] and s["skipped"] == 0 and s["loose"] == 0 and not res.flags.item() & 7
    assert g_round < 1e-4 * g_start  # (the yardstick itself is near the optimum)
    assert g_kernel <= STATIONARITY_MARGIN * g_round
    assert moved >= 0.05 and diff <= POSE_TOL
    assert abs(s["final"] - cost64) <= 1e-6 * cost64
    assert abs(s["initial"] - ref["costs"][0]) <= 1e-9 * ref["costs"][0]
    chi2 = M.chi2(M.from_viewmatrices(res.viewmatrices.cpu()), d["long"], d["Zm"], d["Omega"])
    assert float(((res.chi2.cpu().to(F64) - chi2).abs() / chi2).max()) <= 1e-5
    assert torch.equal(res.viewmatrices[0], d["vm"][0])  # the fixed pose's bits


# ---------------------------------------------------------------------------------------------------------------- edge shapes
def test_nothing_to_solve_changes_no_bit():
    vm = M.to_viewmatrices(M.look_at_circle(5)).to(DEV)
    none = torch.zeros((0, 2), dtype=torch.int32, device=DEV)
    res = slam.pose_graph_optimize(vm[:1], none, torch.zeros((0, 4, 4), device=DEV), return_chi2=True)
    s = stats(res)
    assert torch.equal(res.viewmatrices, vm[:1]) and s["ok"] == 1 and s["run"] == 0 and s["final"] == 0 and res.chi2.shape == (0,)
    d, _ = ring(12, 1)
    res = run(d, fixed=torch.ones(12, dtype=torch.bool, device=DEV))
    s = stats(res)
    assert torch.equal(res.viewmatrices, d["vm"]) and s["ok"] == 1 and s["run"] == 0 and s["accepted"] == 0
    assert abs(s["final"] - s["initial"]) <= 1e-12 * s["initial"] and s["initial"] > 1.0


def test_two_poses_and_one_edge_have_the_closed_form():
    g = M.ring_graph(2, 0, seed=5)
    g["T0"][1] = M.exp_se3(torch.tensor([0.3, -0.2, 0.4, 0.2, 0.1, -0.3], dtype=F64)) @ g["T0"][1]
    d = dev(g)
    res = run(d, iterations=30)
    closed = M.inverse(d["Zm"][0]) @ d["T0"][0] if d["long"][0, 0] == 0 else d["Zm"][0] @ d["T0"][0]
    diff = pose_diff(res, torch.stack([d["T0"][0], closed]))
    print(f"pgo-figure closed form: pose diff {diff:.3e}, final cost {stats(res)['final']:.3e}")
    assert diff <= POSE_TOL and stats(res)["final"] < 1e-10 and torch.equal(res.viewmatrices[0], d["vm"][0])


def test_a_free_pose_without_edges_is_loose_and_keeps_its_bits():
    d, ref = ring(12, 1)
    extra = M.to_viewmatrices(M.exp_se3(torch.tensor([[0.1, 0.2, 0.3, 1.0, 2.0, 3.0]], dtype=F64))).to(DEV)
    vm = torch.cat([d["vm"][:5], extra, d["vm"][5:]])  # in the middle: pose k >= 5 becomes k + 1
    edges = d["edges"] + (d["edges"] >= 5).to(torch.int32)
    res = slam.pose_graph_optimize(vm, edges, d["Z"], information=d["info"])
    s = stats(res)
    assert s["loose"] == 1 and res.flags.item() == 4 and torch.equal(res.viewmatrices[5], extra[0])
    rest = torch.cat([res.viewmatrices[:5], res.viewmatrices[6:]])
    diff = float((rest.cpu() - M.to_viewmatrices(ref["T"])).abs().max())
    print(f"pgo-figure loose pose: pose diff {diff:.3e}")
    assert diff <= POSE_TOL


def test_every_kind_of_skipped_edge_is_counted_and_left_out():
    d, ref = ring(12, 1)
    E = d["edges"].shape[0]
    bad_edges = torch.tensor([[-1, 3], [3, 12], [4, 4], [2, 7], [2, 8], [2, 9], [1 << 30, 0]], dtype=torch.int32, device=DEV)
    Zb = d["Z"][:1].repeat(7, 1, 1).clone()
    Zb[3, :3, :3] *= 1.1            # not rigid
    Zb[4, 3, 0] = float("nan")      # not finite
    info_b = d["info"][:1].repeat(7, 1, 1).clone()
    info_b[5, 2, 4] = float("inf")  # Omega not finite
    order = torch.tensor([0, 12, 1, 2, 13, 3, 4, 14, 15, 5, 6, 16, 7, 8, 9, 17, 10, 11, 18])  # interleaved
    edges = torch.cat([d["edges"], bad_edges])[order.to(DEV)]
    Z, info = torch.cat([d["Z"], Zb])[order.to(DEV)], torch.cat([d["info"], info_b])[order.to(DEV)]
    res = slam.pose_graph_optimize(d["vm"], edges, Z, information=info, return_chi2=True)
    s = stats(res)
    skipped = order >= E
    assert s["skipped"] == 7 and s["used"] == E and res.flags.item() == 2 and s["ok"] == 1
    assert bool(torch.isnan(res.chi2.cpu()[skipped]).all()) and bool(torch.isfinite(res.chi2.cpu()[~skipped]).all())
    diff = pose_diff(res, ref["T"])
    print(f"pgo-figure skipped edges: pose diff {diff:.3e}")
    assert diff <= POSE_TOL


def test_a_weight_pair_that_is_not_finite_skips_its_edge():
    """information_kind 2: the [E,2] form's own finiteness test, one edge with an infinite rotation weight, one with a NaN
    translation weight"""
    d, ref = ring(12, 1)
    E = d["edges"].shape[0]
    edges = torch.cat([d["edges"][:4], torch.tensor([[2, 7]], dtype=torch.int32, device=DEV), d["edges"][4:],
                       torch.tensor([[3, 9]], dtype=torch.int32, device=DEV)])
    Z = torch.cat([d["Z"][:4], d["Z"][:1], d["Z"][4:], d["Z"][:1]])
    pair = torch.tensor([[100.0, 25.0]], device=DEV).repeat(E + 2, 1)
    pair[4, 0], pair[E + 1, 1] = float("inf"), float("nan")
    res = slam.pose_graph_optimize(d["vm"], edges, Z, information=pair, return_chi2=True)
    s = stats(res)
    bad = torch.zeros(E + 2, dtype=torch.bool)
    bad[[4, E + 1]] = True
    assert s["skipped"] == 2 and s["used"] == E and res.flags.item() == 2 and s["ok"] == 1
    assert bool(torch.isnan(res.chi2.cpu()[bad]).all()) and bool(torch.isfinite(res.chi2.cpu()[~bad]).all())
    diff = pose_diff(res, ref["T"])
    print(f"pgo-figure skipped weight pairs: pose diff {diff:.3e}")
    assert diff <= POSE_TOL


def _compare(g, what, **kw):
    d = dev(g)
    ref = model(d, iterations=10, **kw)
    res = run(d, **kw)
    s = stats(res)
    diff = pose_diff(res, ref["T"])
    print(f"pgo-figure {what}: pose diff {diff:.3e}, cost {s['initial']:.5g} -> {s['final']:.5g} (model {ref['costs'][-1]:.5g}), "
          f"trials {s['run']:.0f} (model {len(ref['trials'])}), cg {s['cg']:.0f}")
    assert s["ok"] == 1 and s["used"] == d["edges"].shape[0] and ref["rejected"] == 0
    assert diff <= POSE_TOL
    return d, ref, res


def test_duplicate_edges():
    g = M.ring_graph(12, 1)
    for n in ("edges", "Z", "Omega"):
        g[n] = torch.cat([g[n], g[n][-1:], g[n][3:4], g[n][-1:]])
    g["Z"][-1] = M.exp_se3(torch.tensor([0.01, 0.0, -0.01, 0.0, 0.02, 0.0], dtype=F64)) @ g["Z"][-1]
    _compare(g, "duplicate edges")


def test_a_star_whose_hub_has_degree_E():
    K = 300  # the hub's list is longer than one chunk of the plan
    g = M.ring_graph(K, 0, seed=7)
    noise = torch.randn((K - 1, 6), generator=torch.Generator().manual_seed(8), dtype=F64) * 0.02
    g["edges"] = torch.tensor([(0, k) if k % 2 else (k, 0) for k in range(1, K)], dtype=torch.long)
    g["Z"] = M.exp_se3(noise) @ g["truth"][g["edges"][:, 0]] @ M.inverse(g["truth"][g["edges"][:, 1]])
    g["Omega"] = g["Omega"][:1].expand(K - 1, 6, 6).clone()
    g["T0"] = M.exp_se3(torch.randn((K, 6), generator=torch.Generator().manual_seed(9), dtype=F64) * 0.1) @ g["truth"]
    g["fixed"][:] = False
    g["fixed"][5] = True  # the hub itself is free
    _compare(g, "star")


@pytest.mark.parametrize("E", [1023, 1024, 1025])
def test_the_edge_pass_at_its_loop_and_chunk_edges(E):
    _compare(_dense_graph(64, E, 11), f"E={E}")


def test_a_chain_across_the_node_rounds_takes_the_dense_solve_s_step():
    """K = 1025: five rounds of 256 nodes, the last with one.  One trial from a perturbed start; the damped system is solved
    tightly (cg_tolerance 1e-10), so the poses after the step are the model's after its dense solve."""
    K = 1025
    g = M.ring_graph(K, 0, seed=13)
    g["T0"] = M.exp_se3(torch.randn((K, 6), generator=torch.Generator().manual_seed(14), dtype=F64) * 0.02) @ g["truth"]
    d = dev(g)
    on = lambda t: t.to(DEV)  # noqa: E731  (the model's dense 6144 x 6144 solve in float64 on the device)
    ref = M.solve(on(d["T0"]), on(d["long"]), on(d["Zm"]), on(d["Omega"]), on(d["fixed_cpu"]), iterations=1)
    res = run(d, iterations=1, cg_tolerance=1e-10)
    s = stats(res)
    diff = pose_diff(res, ref["T"].cpu())
    step = float(ref["steps"][0].abs().max())
    print(f"pgo-figure chain K=1025: pose diff {diff:.3e}, largest step component {step:.3e}, cg {s['cg']:.0f}, "
          f"cost {s['initial']:.5g} -> {s['final']:.5g} (model {ref['costs'][-1]:.5g})")
    assert s["ok"] == 1 and s["accepted"] == 1 == ref["accepted"] and s["run"] == 1 and res.flags.item() == 0
    assert step > 0.01 and diff <= POSE_TOL


def test_the_output_may_be_the_input():
    d, _ = ring(12, 1)
    plain = run(d, return_chi2=True)
    held = d["vm"].clone()
    res = slam.pose_graph_optimize(held, d["edges"], d["Z"], information=d["info"], viewmatrices_out=held, return_chi2=True)
    assert res.viewmatrices is held
    assert all(torch.equal(a, b) for a, b in zip(plain, res))


def test_several_fixed_poses():
    g = M.ring_graph(12, 1)
    g["fixed"][[4, 9]] = True
    d, _, res = _compare(g, "several fixed")
    assert torch.equal(res.viewmatrices[[0, 4, 9]], d["vm"][[0, 4, 9]])


# ------------------------------------------------------------------------------------------------------------ other behaviour
def test_the_three_kinds_of_information_agree():
    d, _ = ring(12, 1)
    E = d["edges"].shape[0]
    full = run(d)
    pair = run(d, information=torch.tensor([[100.0, 25.0]], device=DEV).repeat(E, 1))
    lopsided = d["info"].clone()  # the same symmetric part
    lopsided[:, 1, 4] += 3.0
    lopsided[:, 4, 1] -= 3.0
    skew = run(d, information=lopsided)
    assert all(torch.equal(a, b) for a, b in zip(full[:3], pair[:3])) and all(torch.equal(a, b) for a, b in zip(full[:3], skew[:3]))
    none = run(d, information=None)
    ones = run(d, information=torch.ones((E, 2), device=DEV))
    eye = run(d, information=torch.eye(6, device=DEV).repeat(E, 1, 1))
    assert all(torch.equal(a, b) for a, b in zip(none[:3], ones[:3])) and all(torch.equal(a, b) for a, b in zip(none[:3], eye[:3]))
    assert not torch.equal(none.viewmatrices, full.viewmatrices)


def _dense_graph(K, E, seed):
    """a chain of K poses and E - (K - 1) loop edges between random pairs, noise and weights as the ring's"""
    g = M.ring_graph(K, 0, seed=seed)
    gen = torch.Generator().manual_seed(seed + E)
    extra = torch.randint(0, K, (E - (K - 1), 2), generator=gen)
    extra[:, 1] = torch.where(extra[:, 0] == extra[:, 1], (extra[:, 1] + 1) % K, extra[:, 1])
    edges = torch.cat([g["edges"], extra])
    noise = torch.randn((E, 6), generator=gen, dtype=F64) * torch.tensor([0.02] * 3 + [0.03] * 3, dtype=F64)
    g.update(edges=edges, Z=M.exp_se3(noise) @ g["truth"][edges[:, 0]] @ M.inverse(g["truth"][edges[:, 1]]),
             Omega=g["Omega"][:1].expand(E, 6, 6).clone())
    return g


def test_huber_holds_a_corrupted_loop_edge_down():
    """One loop edge off by 0.5 rad (s = 5 at Omega = 100) under huber_delta = 1, in a graph with enough loop edges to out-vote it
    (K = 64, E = 256).  On the bare ring nothing contradicts a loop edge: there the optimum of the stated cost spreads 0.5 rad over
    the chain, with or without Huber, and no edge stands out."""
    g = _dense_graph(64, 256, 17)
    g["Z"][-1] = M.exp_se3(torch.tensor([0.0, 0.5, 0.0, 0.0, 0.0, 0.0], dtype=F64)) @ g["Z"][-1]
    d = dev(g)
    kw = dict(iterations=15, huber_delta=1.0)
    ref = model(d, **kw)
    res = run(d, return_chi2=True, **kw)
    s = stats(res)
    diff = pose_diff(res, ref["T"])
    chi2 = res.chi2.cpu()
    print(f"pgo-figure huber: pose diff {diff:.3e}, chi2 of the corrupted edge {chi2[-1]:.4g}, largest other {chi2[:-1].max():.4g}, "
          f"cost {s['initial']:.5g} -> {s['final']:.5g} (model {ref['costs'][-1]:.5g}), trials {s['run']:.0f}")
    assert ref["rejected"] == 0 and diff <= POSE_TOL
    assert float(chi2[-1]) > 10.0 * float(chi2[:-1].max()) and float(chi2[-1]) > 1.0
    plain = run(d, iterations=15)  # least squares lets the corrupted edge pull its two poses further
    assert float((plain.viewmatrices - res.viewmatrices).abs().max()) > 1e-3


def test_a_rejected_step_is_taken_back():
    g = M.ring_graph(12, 1)
    g["T0"] = M.exp_se3(torch.randn((12, 6), generator=torch.Generator().manual_seed(0), dtype=F64) * 2.0) @ g["T0"]
    g["T0"][0] = g["truth"][0]
    d = dev(g)
    kw = dict(iterations=12, damping=1e-12)
    ref = model(d, **kw)
    margins = [abs(c1 - c0) / c0 for _, c0, c1 in ref["trials"]]
    res = run(d, **kw)
    s = stats(res)
    print(f"pgo-figure rejected step: model accepted {ref['accepted']} rejected {ref['rejected']}, smallest margin {min(margins):.3e}; "
          f"kernel accepted {s['accepted']:.0f} rejected {s['rejected']:.0f}, pose diff {pose_diff(res, ref['T']):.3e}")
    assert ref["rejected"] >= 1 and ref["accepted"] >= 1 and min(margins) > 1e-3  # (the inputs' own condition)
    assert s["accepted"] == ref["accepted"] and s["rejected"] == ref["rejected"] and s["run"] == len(ref["trials"])
    assert abs(s["final"] - ref["costs"][-1]) <= 1e-5 * ref["costs"][-1]


def test_the_log_at_large_angles():
    angles = [0.0, 1e-5, 1.0, 3.0, math.pi - 1e-4]
    K = len(angles) + 1
    T = M.exp_se3(torch.randn((K, 6), generator=torch.Generator().manual_seed(31), dtype=F64) * 0.5)
    axis = torch.tensor([0.6, -0.64, 0.48], dtype=F64)
    xi = torch.stack([torch.cat([axis * a, torch.tensor([0.3, -0.2, 0.5], dtype=F64)]) for a in angles])
    edges = torch.tensor([[0, k + 1] if k % 2 else [k + 1, 0] for k in range(K - 1)], dtype=torch.long)
    Z = T[edges[:, 0]] @ M.inverse(T[edges[:, 1]]) @ M.inverse(M.exp_se3(xi))  # Z^-1 T_i T_j^-1 = Exp(xi)
    g = dict(T0=T, Z=Z, edges=edges, Omega=M.omega_of(None, K - 1) * 2.0, fixed=torch.zeros(K, dtype=torch.bool))
    d = dev(g)
    res = run(d, iterations=0, return_chi2=True)
    ref = M.chi2(d["T0"], d["long"], d["Zm"], d["Omega"])
    got = res.chi2.cpu().to(F64)
    rel = ((got - ref).abs() / ref).tolist()
    seen = M.residuals(d["T0"], d["long"], d["Zm"])[:, :3].norm(dim=-1).tolist()
    print("pgo-figure log: " + ", ".join(f"angle {a:.6g} (seen {b:.6g}) rel {r:.2e}" for a, b, r in zip(angles, seen, rel)))
    assert all(abs(a - b) < 1e-6 for a, b in zip(angles, seen))  # fp32 inputs still hold the angles asked for
    assert max(rel) <= LOG_RTOL
    s = stats(res)
    assert s["run"] == 0 and torch.equal(res.viewmatrices, d["vm"]) and abs(s["final"] - float(ref.sum())) <= 1e-9 * float(ref.sum())


def test_two_runs_give_the_same_bits():
    d, _ = ring(40, 2)
    a, b = run(d, return_chi2=True, huber_delta=0.5), run(d, return_chi2=True, huber_delta=0.5)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def test_a_recorded_solve_replays_and_follows_its_inputs():
    d, _ = ring(12, 1)
    other = dev(M.ring_graph(12, 1, seed=3))
    vm, Z = d["vm"].clone(), d["Z"].clone()
    plan = slam.pose_graph_plan(d["edges"], 12)
    solve = lambda: slam.pose_graph_optimize(vm, d["edges"], Z, information=d["info"], plan=plan, return_chi2=True)  # noqa: E731
    eager = [t.clone() for t in solve()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        solve()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = solve()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(out, eager))
    vm.copy_(other["vm"])
    graph.replay()
    torch.cuda.synchronize()
    mixed = [t.clone() for t in out]
    Z.copy_(other["Z"])
    graph.replay()
    torch.cuda.synchronize()
    fresh = slam.pose_graph_optimize(other["vm"], d["edges"], other["Z"], information=d["info"], return_chi2=True)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(out, fresh))
    assert not torch.equal(mixed[0], out[0]) and not torch.equal(mixed[0], eager[0])


def test_a_pose_that_is_not_rigid_refuses_the_solve():
    d, _ = ring(12, 1)
    for spoil in (lambda v: v[7, :3, :3].mul_(1.01), lambda v: v[3, 3, 1].fill_(float("nan")), lambda v: v[5, 0, :3].neg_()):
        vm = d["vm"].clone()
        spoil(vm)
        res = slam.pose_graph_optimize(vm, d["edges"], d["Z"], information=d["info"], return_chi2=True)
        assert stats(res)["ok"] == 0 and res.flags.item() & 1 and bool(torch.isnan(res.chi2).all())
        assert torch.equal(res.viewmatrices.view(torch.int32), vm.view(torch.int32))
