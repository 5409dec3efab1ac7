"""The float64 pose-graph model (tests/pgo_model.py) against what can be known without it: its Exp and Log invert each other, a
one-edge graph has a closed form, a consistent graph has cost zero, the reference ring converges monotonically, and the Huber
weights are the definition's.  No GPU."""
import math

import pytest
import torch

import pgo_model as M

F64 = torch.float64


def _twists(n, max_angle, seed):
    g = torch.Generator().manual_seed(seed)
    axis = torch.randn((n, 3), generator=g, dtype=F64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    angle = torch.rand((n, 1), generator=g, dtype=F64) * max_angle
    return torch.cat([axis * angle, torch.randn((n, 3), generator=g, dtype=F64)], -1)


def test_log_inverts_exp_up_to_large_angles():
    xi = torch.cat([_twists(200, 3.1, 1), _twists(50, 1e-3, 2), _twists(50, 1e-7, 3), torch.zeros((1, 6), dtype=F64)])
    xi[0, :3] = torch.tensor([3.1, 0.0, 0.0], dtype=F64)
    back = M.log_se3(M.exp_se3(xi))
    assert float((back - xi).abs().max()) < 1e-9
    T = M.exp_se3(xi)
    assert float((M.exp_se3(back) - T).abs().max()) < 1e-12
    assert float((T @ M.inverse(T) - torch.eye(4, dtype=F64)).abs().max()) < 1e-13


def test_exp_is_a_rotation_and_matches_the_matrix_exponential():
    xi = _twists(20, 3.0, 4)
    T = M.exp_se3(xi)
    R = T[:, :3, :3]
    assert float((R @ R.transpose(-1, -2) - torch.eye(3, dtype=F64)).abs().max()) < 1e-13
    G = torch.zeros((20, 4, 4), dtype=F64)
    G[:, :3, :3], G[:, :3, 3] = M.hat(xi[:, :3]), xi[:, 3:]
    assert float((torch.linalg.matrix_exp(G) - T).abs().max()) < 1e-12


def test_one_edge_with_one_fixed_node_has_the_closed_form():
    T = M.exp_se3(_twists(2, 1.0, 5))
    Z = M.exp_se3(_twists(1, 2.0, 6))
    edges = torch.tensor([[0, 1]])
    fixed = torch.tensor([True, False])
    out = M.solve(T, edges, Z, M.omega_of(None, 1), fixed, iterations=30, damping=1e-6)
    assert float((out["T"][1] - M.inverse(Z[0]) @ T[0]).abs().max()) < 1e-12
    assert torch.equal(out["T"][0], T[0])


def test_a_consistent_graph_reaches_zero_cost():
    g = M.ring_graph(10, 2, seed=3, rot_noise=0.0, trans_noise=0.0)
    start = M.exp_se3(_twists(10, 0.2, 7) * 0.3) @ g["truth"]
    start[0] = g["truth"][0]
    out = M.solve(start, g["edges"], g["Z"], g["Omega"], g["fixed"], iterations=30)
    assert out["costs"][0] > 1.0 and out["costs"][-1] < 1e-20
    assert float((out["T"] - g["truth"]).abs().max()) < 1e-10


@pytest.mark.parametrize("K, loops", [(12, 1), (40, 2)])
def test_the_ring_converges_monotonically(K, loops):
    g = M.ring_graph(K, loops)
    out = M.solve(g["T0"], g["edges"], g["Z"], g["Omega"], g["fixed"], iterations=8)
    assert out["rejected"] == 0 and len(out["trials"]) <= 8
    assert all(b < a for a, b in zip(out["costs"], out["costs"][1:]))
    g0 = M.gradient_norm(g["T0"], g["edges"], g["Z"], g["Omega"], g["fixed"])
    g1 = M.gradient_norm(out["T"], g["edges"], g["Z"], g["Omega"], g["fixed"])
    assert g0 > 1.0 and g1 < 1e-9 * g0
    # the dense normal equations' g is half the autograd gradient of the cost
    _, gv = M.normal_equations(g["T0"], g["edges"], g["Z"], g["Omega"])
    auto = M.gradient(g["T0"], g["edges"], g["Z"], g["Omega"]).reshape(-1)
    assert float((2.0 * gv - auto).abs().max()) < 1e-9 * float(auto.abs().max())


def test_huber_weights_are_the_definition():
    s = torch.tensor([0.0, 0.5, 1.0, 1.5, 4.0], dtype=F64)
    rho, w = M.huber(s * s, 1.0)
    assert torch.allclose(rho, torch.tensor([0.0, 0.25, 1.0, 2.0, 7.0], dtype=F64), rtol=0, atol=1e-15)
    assert torch.allclose(w, torch.tensor([1.0, 1.0, 1.0, 1.0 / 1.5, 0.25], dtype=F64), rtol=0, atol=1e-15)
    rho, w = M.huber(s * s, M.INF)
    assert torch.equal(rho, s * s) and torch.equal(w, torch.ones_like(s))
    # and the weighted normal equations are those of rho: g = 1/2 d cost / d d under the weights
    g = M.ring_graph(8, 1, seed=2)
    g["Z"][-1] = M.exp_se3(torch.tensor([0.5, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=F64)) @ g["Z"][-1]
    _, gv = M.normal_equations(g["T0"], g["edges"], g["Z"], g["Omega"], 1.0)
    auto = M.gradient(g["T0"], g["edges"], g["Z"], g["Omega"], 1.0).reshape(-1)
    assert float(M.chi2(g["T0"], g["edges"], g["Z"], g["Omega"]).max()) > 1.0  # the corrupted edge is an outlier
    assert float((2.0 * gv - auto).abs().max()) < 1e-9 * float(auto.abs().max())


def test_rotation_of_reads_an_fp32_matrix_through_its_quaternion():
    T = M.exp_se3(_twists(8, 3.1, 9))
    R = M.rotation_of(T[:, :3, :3].to(torch.float32))
    assert float((R @ R.transpose(-1, -2) - torch.eye(3, dtype=F64)).abs().max()) < 1e-14
    assert float((R - T[:, :3, :3]).abs().max()) < 3e-7
    assert math.isclose(float(torch.linalg.det(R).min()), 1.0, abs_tol=1e-13)
