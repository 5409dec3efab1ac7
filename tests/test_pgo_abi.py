"""The pose-graph entry points (include/dgr_hip.h: dgr_pgo_scratch_bytes, dgr_pgo_plan, dgr_pgo_solve) and their Python surface
without a GPU: declared, exported and bound; the params struct's layout against the header text; the caps and the scratch size;
every argument error refused with a message before any device call; the keyword-only arguments and the ValueErrors of the Python
side."""
import ctypes as C
import re

import pytest
import torch

from dgr_amd import _capi, posegraph, slam

from abi_checks import FAKE, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_pgo_scratch_bytes", "dgr_pgo_plan", "dgr_pgo_solve")
NAN, INF = float("nan"), float("inf")
FIELDS = [("iterations", "int"), ("cg_iterations", "int"), ("cg_tolerance", "float"), ("huber_delta", "float"), ("damping", "float"),
          ("rcond", "float"), ("step_tolerance", "float"), ("cost_tolerance", "float")]


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_pgo_scratch_bytes": 2, "dgr_pgo_plan": 5, "dgr_pgo_solve": 15})
    assert _capi._SIGS["dgr_pgo_scratch_bytes"][0] is C.c_size_t


def test_params_struct_matches_the_header_text():
    body = header_text().split("} dgr_pgo_params;")[0].rsplit("typedef struct dgr_pgo_params {", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == FIELDS
    P = _capi.PgoParams
    assert [(n, {C.c_float: "float", C.c_int: "int"}[t]) for n, t in P._fields_] == fields
    assert C.sizeof(P) == 32 and [getattr(P, n).offset for n, _ in fields] == list(range(0, 32, 4))  # eight four-byte fields


def test_caps_and_scratch_size():
    f = _capi.load().dgr_pgo_scratch_bytes
    for bad in ((0, 0), (-1, 4), (65537, 4), (4, -1), (4, (1 << 18) + 1)):
        assert f(*bad) == 0, bad
    assert f(1, 0) > 0 and f(65536, 1 << 18) > 0
    last = 0
    for K, E in ((1, 0), (2, 1), (12, 12), (12, 13), (13, 13), (200, 203), (1000, 1050), (65536, 1 << 18)):
        n = f(K, E)
        # the lists (K + 1 offsets, 2 E entries) and, in double, at least a pose, a gradient and a 6 x 6 block per node and the
        # three 6 x 6 blocks per edge; a loose upper bound against a runaway layout
        assert n % 16 == 0 and 4 * (K + 1 + 2 * E) + 8 * (49 * K + 108 * E) <= n <= 4096 + 2048 * (K + E), (K, E)
        assert n > last
        last = n


def _plan(K=12, E=13, edges=FAKE, scratch=FAKE):
    return _capi.load().dgr_pgo_plan(None, K, E, edges, scratch)


@pytest.mark.parametrize("case, text", [
    (dict(K=0), "n_poses"), (dict(K=-3), "n_poses"), (dict(K=65537), "n_poses"),
    (dict(E=-1), "n_edges"), (dict(E=(1 << 18) + 1), "n_edges"),
    (dict(edges=None), "edges is NULL"), (dict(edges=FAKE + 2), "edges is not 4-byte aligned"),
    (dict(scratch=None), "scratch is NULL"), (dict(scratch=FAKE + 8), "16-byte aligned"),
])
def test_pgo_plan_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_plan(**case), "dgr_pgo_plan", text)


def _solve(K=12, E=13, poses_in=FAKE, edges=FAKE, meas=FAKE, info=None, kind=0, fixed=None, params=True, scratch=FAKE,
           poses_out=FAKE, chi2=None, stats=FAKE, flags=FAKE, iterations=10, cg_iterations=144, cg_tol=1e-6, huber=INF, damping=1e-4,
           rcond=1e-12, step_tol=1e-9, cost_tol=1e-12):
    p = _capi.PgoParams(iterations, cg_iterations, cg_tol, huber, damping, rcond, step_tol, cost_tol) if params else None
    return _capi.load().dgr_pgo_solve(None, K, E, poses_in, edges, meas, info, kind, fixed, p, scratch, poses_out, chi2, stats, flags)


@pytest.mark.parametrize("case, text", [
    (dict(params=False), "params is NULL"),
    (dict(K=0), "n_poses"), (dict(K=-1), "n_poses"), (dict(K=65537), "n_poses"),
    (dict(E=-1), "n_edges"), (dict(E=(1 << 18) + 1), "n_edges"),
    (dict(poses_in=None), "poses_in is NULL"),
    (dict(edges=None), "edges is NULL"), (dict(meas=None), "measurements is NULL"),
    (dict(kind=1), "information_kind"), (dict(kind=6), "information_kind"), (dict(kind=-36), "information_kind"),
    (dict(kind=2), "information is NULL"), (dict(kind=36), "information is NULL"),
    (dict(scratch=None), "scratch is NULL"), (dict(scratch=FAKE + 4), "16-byte aligned"),
    (dict(poses_out=None), "poses_out is NULL"),
    (dict(stats=None), "stats is NULL"), (dict(stats=FAKE + 4), "8-byte aligned"),
    (dict(flags=None), "flags is NULL"),
    (dict(iterations=-1), "iterations"), (dict(iterations=1001), "iterations"),
    (dict(cg_iterations=0), "cg_iterations"), (dict(cg_iterations=-5), "cg_iterations"), (dict(cg_iterations=(1 << 20) + 1), "cg_iterations"),
    (dict(poses_in=FAKE + 2), "4-byte aligned"), (dict(edges=FAKE + 1), "4-byte aligned"), (dict(meas=FAKE + 3), "4-byte aligned"),
    (dict(info=FAKE + 2, kind=2), "4-byte aligned"), (dict(poses_out=FAKE + 2), "4-byte aligned"), (dict(chi2=FAKE + 2), "4-byte aligned"),
    (dict(flags=FAKE + 2), "4-byte aligned"),
    (dict(cg_tol=NAN), "cg_tolerance is NaN or negative"), (dict(cg_tol=-1e-6), "cg_tolerance is NaN or negative"),
    (dict(huber=NAN), "huber_delta is NaN or negative"), (dict(huber=-1.0), "huber_delta is NaN or negative"),
    (dict(damping=NAN), "damping is NaN or negative"), (dict(damping=-1e-4), "damping is NaN or negative"),
    (dict(rcond=NAN), "rcond is NaN or negative"), (dict(rcond=-1e-12), "rcond is NaN or negative"),
    (dict(step_tol=NAN), "step_tolerance is NaN or negative"), (dict(step_tol=-1e-9), "step_tolerance is NaN or negative"),
    (dict(cost_tol=NAN), "cost_tolerance is NaN or negative"), (dict(cost_tol=-1.0), "cost_tolerance is NaN or negative"),
    (dict(cost_tol=NAN, info=FAKE, kind=36, fixed=FAKE, chi2=FAKE), "cost_tolerance is NaN or negative"),
])
def test_pgo_solve_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_solve(**case), "dgr_pgo_solve", text)


def test_an_empty_graph_needs_no_edge_pointers():
    """E = 0: edges, measurements and information may be NULL; the next refusal is the one asked for"""
    refused(_solve(E=0, edges=None, meas=None, kind=2, info=None, flags=None), "dgr_pgo_solve", "flags is NULL")


def test_python_surface():
    keyword_only(slam.pose_graph_optimize, ["viewmatrices", "edges", "measurements"],
                 dict(information=None, fixed=None, iterations=10, cg_iterations=None, cg_tolerance=1e-6, huber_delta=INF, damping=1e-4,
                      rcond=1e-12, step_tolerance=1e-9, cost_tolerance=1e-12, plan=None, viewmatrices_out=None, return_chi2=False))
    assert slam.PgoResult._fields == ("viewmatrices", "stats", "flags", "chi2")
    assert slam.pose_graph_optimize is posegraph.pose_graph_optimize and slam.pose_graph_plan is posegraph.pose_graph_plan
    assert slam.relative_pose is posegraph.relative_pose and slam.PgoResult is posegraph.PgoResult
    assert "12 K" in posegraph.pose_graph_optimize.__doc__ and "402" in posegraph.pose_graph_optimize.__doc__


def test_relative_pose_is_the_measurement_of_its_edge():
    g = torch.Generator().manual_seed(0)
    q = torch.randn((2, 5, 4), generator=g, dtype=torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    r, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(2, 5, 3, 3)
    T = torch.zeros((2, 5, 4, 4), dtype=torch.float64)
    T[..., :3, :3], T[..., :3, 3], T[..., 3, 3] = R, torch.randn((2, 5, 3), generator=g, dtype=torch.float64), 1.0
    vm = T.transpose(-1, -2).to(torch.float32)
    Z = slam.relative_pose(vm[0], vm[1])
    assert Z.shape == (5, 4, 4) and Z.dtype == torch.float32
    assert float((Z.transpose(-1, -2).double() @ T[1] - T[0]).abs().max()) < 1e-6  # Z T_j = T_i
    assert slam.relative_pose(vm[0, 2], vm[1, 2]).shape == (4, 4)
    assert float((slam.relative_pose(vm[0], vm[0]) - torch.eye(4)).abs().max()) < 1e-6


def test_python_surface_refuses_what_it_cannot_read():
    """Every check runs on the host, the device check last: CPU tensors reach each of them and never the library."""
    K, E = 4, 3
    vm, edges, Z = torch.eye(4).repeat(K, 1, 1), torch.tensor([[1, 0], [2, 1], [3, 2]], dtype=torch.int32), torch.eye(4).repeat(E, 1, 1)
    f = slam.pose_graph_optimize
    with pytest.raises(ValueError, match="GPU tensors"):
        f(vm, edges, Z)
    with pytest.raises(ValueError, match="GPU tensors"):
        f(vm.reshape(K, 16), edges, Z.reshape(E, 16), information=torch.ones(E, 2), fixed=torch.zeros(K, dtype=torch.bool),
          return_chi2=True)
    with pytest.raises(ValueError, match="GPU tensor"):
        slam.pose_graph_plan(edges, K)
    with pytest.raises(ValueError, match="viewmatrices must be a float32"):
        f(vm.double(), edges, Z)
    for bad in (torch.eye(4), torch.zeros(0, 4, 4), torch.zeros(K, 3, 4), torch.zeros(K, 12)):
        with pytest.raises(ValueError, match="viewmatrices is"):
            f(bad, edges, Z)
    with pytest.raises(ValueError, match="edges must be an int32"):
        f(vm, edges.long(), Z)
    with pytest.raises(ValueError, match=r"edges is \[E,2\]"):
        f(vm, edges.reshape(-1), Z)
    with pytest.raises(ValueError, match="edges must be an int32"):
        slam.pose_graph_plan(edges.long(), K)
    with pytest.raises(ValueError, match="measurements must be a float32"):
        f(vm, edges, Z.double())
    with pytest.raises(ValueError, match="measurements is"):
        f(vm, edges, Z[:2])
    with pytest.raises(ValueError, match="information must be a float32"):
        f(vm, edges, Z, information=torch.ones(E, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="information is"):
        f(vm, edges, Z, information=torch.ones(E, 3))
    with pytest.raises(ValueError, match="fixed must be"):
        f(vm, edges, Z, fixed=torch.zeros(K))
    with pytest.raises(ValueError, match="fixed must be"):
        f(vm, edges, Z, fixed=torch.zeros(K + 1, dtype=torch.bool))
    for bad in (-1, 1001):
        with pytest.raises(ValueError, match="iterations must be 0 .. 1000"):
            f(vm, edges, Z, iterations=bad)
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match="cg_iterations must be 1 .. 2\\^20"):
            f(vm, edges, Z, cg_iterations=bad)
    for name in ("cg_tolerance", "huber_delta", "damping", "rcond", "step_tolerance", "cost_tolerance"):
        with pytest.raises(ValueError, match=f"{name} must not be NaN"):
            f(vm, edges, Z, **{name: NAN})
        with pytest.raises(ValueError, match=f"{name} must not be negative"):
            f(vm, edges, Z, **{name: -1.0})
    with pytest.raises(ValueError, match="cannot take"):
        f(torch.eye(4).repeat(65537, 1, 1), edges, Z)
    with pytest.raises(ValueError, match="cannot take"):
        slam.pose_graph_plan(edges, 0)
    with pytest.raises(ValueError, match="plan must come from"):
        f(vm, edges, Z, plan=posegraph.PgoPlan(torch.zeros(16, dtype=torch.uint8), K + 1, E))
    with pytest.raises(ValueError, match="viewmatrices_out must be"):
        f(vm, edges, Z, viewmatrices_out=torch.zeros(K, 16))
