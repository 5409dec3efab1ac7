"""Pose-graph optimisation on the device (C ABI: dgr_pgo_plan, dgr_pgo_solve): the solver between the aligners that measure
relative poses (`icp_align`, `rgbd_align`) and the map correction that consumes the updated ones (`pose_corrections`,
`transform_map`).  One launch of one workgroup runs the whole Levenberg-Marquardt solve; nothing is read on the host."""
from typing import NamedTuple as _NamedTuple

import torch

from . import _capi

INF = float("inf")


class PgoResult(_NamedTuple):
    """What `pose_graph_optimize` leaves on the device: `viewmatrices` float32 [K,4,4] (W2C^T); `stats` float64 [16]: initial
    cost, final cost, ok, trials run, accepted, rejected, CG iterations in total, final lambda, the last accepted step's max
    |omega| and max |v|, max |g| at the result, edges used, edges skipped, loose poses, converged, 0; `flags` int32 [1] (bit 0
    refused, 1 an edge skipped, 2 a loose pose, 3 lambda at its maximum, 4 CG ran into cg_iterations, 5 no plan); `chi2` float32
    [E] = s_e^2 at the result (NaN for a skipped edge) or None."""
    viewmatrices: torch.Tensor
    stats: torch.Tensor
    flags: torch.Tensor
    chi2: torch.Tensor


class PgoPlan(_NamedTuple):
    """`pose_graph_plan`'s result: the scratch that holds the incidence lists, for K poses and the E edges it was made from."""
    scratch: torch.Tensor
    K: int
    E: int


def _edges(what, edges):
    if not isinstance(edges, torch.Tensor) or edges.dtype != torch.int32:
        raise ValueError(f"{what}: edges must be an int32 tensor [E,2]")
    if edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError(f"{what}: edges is [E,2], not {tuple(edges.shape)}")
    return edges


def _scratch_bytes(what, K, E):
    n = _capi.load().dgr_pgo_scratch_bytes(K, E)
    if not n:
        raise ValueError(f"{what}: cannot take {K} poses and {E} edges (1 .. 65536 poses, 0 .. 2^18 edges)")
    return n


def pose_graph_plan(edges, K):
    """The reusable part of a solve: every pose's incidence list for `edges` (int32 [E,2] on the GPU, rows (i, j)) among `K` poses,
    one launch.  Pass it as `plan=` when the same topology is solved again, or when the solve is recorded into a hipGraph and the
    plan is not to be part of the recording.  The `edges` tensor's contents must not change while the plan is in use."""
    what = "pose_graph_plan"
    edges = _edges(what, edges)
    K, E = int(K), int(edges.shape[0])
    n = _scratch_bytes(what, K, E)
    if not edges.is_cuda:
        raise ValueError(f"{what}: edges must be a GPU tensor (there is no CPU fallback)")
    edges = edges.contiguous()
    scratch = torch.empty((n,), dtype=torch.uint8, device=edges.device)
    _capi.call("dgr_pgo_plan", edges.device, K, E, _capi.ptr(edges), scratch.data_ptr())
    return PgoPlan(scratch, K, E)


def relative_pose(viewmatrix_i, viewmatrix_j):
    """The measurement of an edge (i, j) from two viewmatrices (W2C^T, [..,4,4]): Z = T_i T_j^-1, camera j's coordinates to camera
    i's, returned in the measurement's layout (Z^T, float32 [..,4,4]).  Float64 torch ops on the device, no host read;
    `relative_pose(rgbd_align(.., model_viewmatrix=V_j).viewmatrix, V_j)` turns an alignment against keyframe j into a loop edge."""
    Ti, Tj = (m.detach().transpose(-1, -2).to(torch.float64) for m in (viewmatrix_i, viewmatrix_j))
    R, t = Tj[..., :3, :3], Tj[..., :3, 3:]
    inv = torch.zeros_like(Tj)
    inv[..., :3, :3], inv[..., :3, 3:], inv[..., 3, 3] = R.transpose(-1, -2), -(R.transpose(-1, -2) @ t), 1.0
    return (Ti @ inv).transpose(-1, -2).to(torch.float32).contiguous()


def pose_graph_optimize(viewmatrices, edges, measurements, *, information=None, fixed=None, iterations=10, cg_iterations=None,
                        cg_tolerance=1e-6, huber_delta=INF, damping=1e-4, rcond=1e-12, step_tolerance=1e-9, cost_tolerance=1e-12,
                        plan=None, viewmatrices_out=None, return_chi2=False):
    """Pose-graph optimisation (include/dgr_hip.h: dgr_pgo_solve states the semantics): `viewmatrices` float32 [K,4,4] (or
    [K,16]) holds the keyframes' W2C^T, `edges` int32 [E,2] rows (i, j), `measurements` float32 [E,4,4] (or [E,16]) the
    transposes of Z_e ~ T_i T_j^-1 (`relative_pose`'s layout).  Minimised over the free poses is sum_e rho(sqrt(r_e^T Omega_e
    r_e)), r_e = Log(Z_e^-1 T_i T_j^-1) ordered (omega, v), with Huber's rho (`huber_delta`; inf: least squares), by
    Levenberg-Marquardt (`iterations` trials at most, initial lambda `damping`) whose damped normal equations are solved by
    conjugate gradients with a block-Jacobi preconditioner.  `information`: None (identity), float32 [E,2] (rotation and
    translation weight) or [E,6,6] (its symmetric part).  `fixed`: a bool or uint8 [K] tensor; None fixes pose 0.

    `cg_iterations` defaults to 12 K, twice the unknowns per free pose.  Block-Jacobi CG needs on the order of 2 K iterations
    on a chain, because information travels one edge per iteration: measured at a relative residual of 1e-6, K = 12 needs 54,
    K = 40 needs 141, K = 200 needs 402; and stopping early is no shortcut -- at a tolerance of 1e-1 the direction is 90 % wrong
    for K = 200.  Keep `cg_tolerance` tight.  The solve is one launch that nothing interrupts, of at most `iterations *
    cg_iterations` CG iterations (12 us each at K = 200, 64 us at K = 1000 on an MI355X, growing with K): at thousands of poses
    the defaults allow minutes, at the caps hours -- lower `cg_iterations` or `iterations` to the time the device can be held;
    `flags` bit 4 says when a CG solve was cut off.

    One launch for the plan (none with `plan=` from `pose_graph_plan`) and one for the whole solve; no host read, the same bits on
    every run, recordable into a hipGraph (a replay follows rewritten `viewmatrices`, `measurements` and `information`).
    `viewmatrices_out`: a contiguous float32 GPU tensor of `viewmatrices`' size to receive the result; it may be `viewmatrices`
    itself.  Fixed poses, loose ones (no usable edge, or a singular block) and every pose of a refused solve (a pose that is not
    rigid: stats[2] = 0) keep their bits.  Returns PgoResult(viewmatrices, stats, flags, chi2); `chi2` is None unless
    `return_chi2`.  Feed the result to `pose_corrections(viewmatrices, result.viewmatrices)` and `transform_map`."""
    what = "pose_graph_optimize"
    vm = viewmatrices
    if not isinstance(vm, torch.Tensor) or vm.dtype != torch.float32:
        raise ValueError(f"{what}: viewmatrices must be a float32 tensor [K,4,4]")
    if not ((vm.dim() == 3 and tuple(vm.shape[1:]) == (4, 4)) or (vm.dim() == 2 and vm.shape[1] == 16)) or vm.shape[0] < 1:
        raise ValueError(f"{what}: viewmatrices is [K,4,4] or [K,16] with K >= 1, not {tuple(vm.shape)}")
    K = int(vm.shape[0])
    edges = _edges(what, edges)
    E = int(edges.shape[0])
    z = measurements
    if not isinstance(z, torch.Tensor) or z.dtype != torch.float32:
        raise ValueError(f"{what}: measurements must be a float32 tensor [E,4,4]")
    if z.shape[0] != E or z.numel() != E * 16 or z.dim() not in (2, 3):
        raise ValueError(f"{what}: measurements is [E,4,4] or [E,16] with E = {E}, not {tuple(z.shape)}")
    tensors = [vm, edges, z]
    kind = 0
    if information is not None:
        if not isinstance(information, torch.Tensor) or information.dtype != torch.float32:
            raise ValueError(f"{what}: information must be a float32 tensor [E,2] or [E,6,6]")
        if tuple(information.shape) == (E, 2):
            kind = 2
        elif tuple(information.shape) in ((E, 6, 6), (E, 36)):
            kind = 36
        else:
            raise ValueError(f"{what}: information is [E,2] or [E,6,6] with E = {E}, not {tuple(information.shape)}")
        tensors.append(information)
    if fixed is not None:
        if not isinstance(fixed, torch.Tensor) or fixed.dtype not in (torch.bool, torch.uint8) or tuple(fixed.shape) != (K,):
            raise ValueError(f"{what}: fixed must be a bool or uint8 tensor [K] = [{K}]")
        tensors.append(fixed)
    iterations = int(iterations)
    if not 0 <= iterations <= 1000:
        raise ValueError(f"{what}: iterations must be 0 .. 1000, not {iterations}")
    cg_iterations = 12 * K if cg_iterations is None else int(cg_iterations)
    if not 1 <= cg_iterations <= 1 << 20:
        raise ValueError(f"{what}: cg_iterations must be 1 .. 2^20, not {cg_iterations}")
    scalars = dict(cg_tolerance=float(cg_tolerance), huber_delta=float(huber_delta), damping=float(damping), rcond=float(rcond),
                   step_tolerance=float(step_tolerance), cost_tolerance=float(cost_tolerance))
    for n, v in scalars.items():
        if v != v:
            raise ValueError(f"{what}: {n} must not be NaN")
        if v < 0.0:
            raise ValueError(f"{what}: {n} must not be negative, not {v}")
    n_bytes = _scratch_bytes(what, K, E)
    if plan is not None and (not isinstance(plan, PgoPlan) or plan.K != K or plan.E != E):
        raise ValueError(f"{what}: plan must come from pose_graph_plan(edges, {K}) with {E} edges")
    out = viewmatrices_out
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.shape == vm.shape
                                and out.is_contiguous()):
        raise ValueError(f"{what}: viewmatrices_out must be a contiguous float32 tensor {tuple(vm.shape)}")
    if any(not t.is_cuda for t in tensors) or (out is not None and not out.is_cuda):
        raise ValueError(f"{what}: the tensors must be GPU tensors (there is no CPU fallback)")
    dev = vm.device
    if any(t.device != dev for t in tensors) or (plan is not None and plan.scratch.device != dev):
        raise ValueError(f"{what}: the tensors are on different devices")
    vm_in = vm.detach().contiguous()
    edges, z = edges.contiguous(), z.detach().contiguous()
    if information is not None:
        information = information.detach().contiguous()
    if fixed is not None:
        fixed = fixed.contiguous().view(torch.uint8) if fixed.dtype == torch.bool else fixed.contiguous()
    if out is None:
        out = torch.empty_like(vm_in)
    stats = torch.empty((16,), dtype=torch.float64, device=dev)
    flags = torch.empty((1,), dtype=torch.int32, device=dev)
    chi2 = torch.empty((E,), dtype=torch.float32, device=dev) if return_chi2 else None
    params = _capi.PgoParams(iterations, cg_iterations, *scalars.values())
    with _capi.StepCalls(dev) as abi:
        if plan is None:
            scratch = torch.empty((n_bytes,), dtype=torch.uint8, device=dev)
            abi.call("dgr_pgo_plan", K, E, _capi.ptr(edges), scratch.data_ptr())
        else:
            scratch = plan.scratch
        abi.call("dgr_pgo_solve", K, E, vm_in.data_ptr(), _capi.ptr(edges), _capi.ptr(z), _capi.ptr(information), kind,
                 _capi.ptr(fixed), params, scratch.data_ptr(), out.data_ptr(), _capi.ptr(chi2), stats.data_ptr(), flags.data_ptr())
    return PgoResult(out, stats, flags, chi2)
