"""A float64 model of the pose-graph optimiser (include/dgr_hip.h: dgr_pgo_solve) that shares no path with the kernel: the same
cost, but Exp and Log through rotation MATRICES (the kernel: quaternions), Jacobians from torch.autograd.functional.jacobian of
those (the kernel: closed forms), a dense torch.linalg.solve of the damped system (the kernel: block-Jacobi conjugate
gradients), and the same accept / reject rule.  Poses are W2C matrices T [K,4,4] (not transposed); an edge (i, j, Z, Omega)
measures Z ~ T_i T_j^-1; r = Log(Z^-1 T_i T_j^-1) ordered (omega, v); the update is T_k <- Exp(d_k) T_k.  Works on any device."""
import math

import torch

F64 = torch.float64
INF = float("inf")


def hat(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def _abc(th2):
    """sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3; four-term series below th^2 = 1e-4 (next term below 1e-17)"""
    small = th2 < 1e-4
    t2 = torch.where(small, torch.ones_like(th2), th2)
    th = t2.sqrt()
    A = torch.where(small, 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0 * (1.0 - th2 / 42.0)), torch.sin(th) / th)
    B = torch.where(small, 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0 * (1.0 - th2 / 56.0)), 2.0 * torch.sin(0.5 * th) ** 2 / t2)
    C = torch.where(small, 1.0 / 6.0 - th2 / 120.0 * (1.0 - th2 / 42.0 * (1.0 - th2 / 72.0)), (th - torch.sin(th)) / (t2 * th))
    return A, B, C


def _rt(R, t):
    T = torch.zeros(R.shape[:-2] + (4, 4), dtype=R.dtype, device=R.device)
    T[..., :3, :3], T[..., :3, 3], T[..., 3, 3] = R, t, 1.0
    return T


def exp_se3(xi):
    """[..,6] (omega, v) -> [..,4,4]"""
    w, v = xi[..., :3], xi[..., 3:]
    A, B, C = (c[..., None, None] for c in _abc((w * w).sum(-1)))
    K = hat(w)
    K2 = K @ K
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device)
    return _rt(eye + A * K + B * K2, ((eye + B * K + C * K2) @ v[..., None])[..., 0])


def log_se3(T):
    """[..,4,4] -> [..,6]; the angle in [0, pi) (at pi itself the axis is not defined by R - R^T)"""
    R, t = T[..., :3, :3], T[..., :3, 3]
    w = 0.5 * torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)  # sin th axis
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    s2 = (w * w).sum(-1)
    small = (s2 < 1e-12) & (c > 0)
    s = torch.where(small, torch.ones_like(s2), s2).sqrt()
    k = torch.where(small, 1.0 + s2 / 6.0, torch.atan2(s, c) / s)
    om = k[..., None] * w
    _, B, C = (x[..., None, None] for x in _abc((om * om).sum(-1)))
    K = hat(om)
    V = torch.eye(3, dtype=T.dtype, device=T.device) + B * K + C * (K @ K)
    return torch.cat([om, torch.linalg.solve(V, t[..., None])[..., 0]], -1)


def inverse(T):
    Rt = T[..., :3, :3].transpose(-1, -2)
    return _rt(Rt, -(Rt @ T[..., :3, 3:])[..., 0])


def rotation_of(M):
    """The rotation a 3 x 3 matrix that is only nearly orthonormal (fp32 entries) stands for, as the contract reads it: through
    its unit quaternion (Shepperd's branches)."""
    M = M.to(F64)
    out = torch.empty_like(M)
    flat, res = M.reshape(-1, 3, 3), out.reshape(-1, 3, 3)
    for n, R in enumerate(flat.tolist()):
        tr = R[0][0] + R[1][1] + R[2][2]
        if tr > 0:
            s = 2.0 * math.sqrt(tr + 1.0)
            q = [0.25 * s, (R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s]
        elif R[0][0] > R[1][1] and R[0][0] > R[2][2]:
            s = 2.0 * math.sqrt(1.0 + R[0][0] - R[1][1] - R[2][2])
            q = [(R[2][1] - R[1][2]) / s, 0.25 * s, (R[0][1] + R[1][0]) / s, (R[0][2] + R[2][0]) / s]
        elif R[1][1] > R[2][2]:
            s = 2.0 * math.sqrt(1.0 + R[1][1] - R[0][0] - R[2][2])
            q = [(R[0][2] - R[2][0]) / s, (R[0][1] + R[1][0]) / s, 0.25 * s, (R[1][2] + R[2][1]) / s]
        else:
            s = 2.0 * math.sqrt(1.0 + R[2][2] - R[0][0] - R[1][1])
            q = [(R[1][0] - R[0][1]) / s, (R[0][2] + R[2][0]) / s, (R[1][2] + R[2][1]) / s, 0.25 * s]
        nrm = math.sqrt(sum(x * x for x in q))
        r, x, y, z = (v / nrm for v in q)
        res[n] = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                               [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                               [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]], dtype=F64)
    return out


def from_viewmatrices(vm):
    """float32 [..,4,4] or [..,16] W2C^T -> float64 W2C [..,4,4] on the same device, the rotation read by `rotation_of`"""
    T = vm.detach().reshape(vm.shape[0], 4, 4).transpose(-1, -2).to(F64)
    return _rt(rotation_of(T[..., :3, :3].cpu()).to(T.device), T[..., :3, 3])


def to_viewmatrices(T):
    return T.transpose(-1, -2).to(torch.float32).contiguous()


def omega_of(information, E, device="cpu"):
    """[E,6,6] float64 from None, [E,2] or [E,6,6]"""
    if information is None:
        return torch.eye(6, dtype=F64, device=device).expand(E, 6, 6).clone()
    information = information.to(F64)
    if information.dim() == 2 and information.shape[1] == 2:
        return torch.diag_embed(information[:, [0, 0, 0, 1, 1, 1]])
    information = information.reshape(E, 6, 6)
    return 0.5 * (information + information.transpose(-1, -2))


def residuals(T, edges, Z, delta=None):
    """[E,6]; `delta` [E,12]: the left perturbations (d_i, d_j) of each edge's two poses"""
    Ti, Tj = T[edges[:, 0]], T[edges[:, 1]]
    if delta is not None:
        Ti, Tj = exp_se3(delta[:, :6]) @ Ti, exp_se3(delta[:, 6:]) @ Tj
    return log_se3(inverse(Z) @ Ti @ inverse(Tj))


def huber(s2, delta):
    """(rho, w) of s^2"""
    if delta == INF:
        return s2, torch.ones_like(s2)
    s = s2.clamp_min(1e-300).sqrt()
    inl = s <= delta
    return torch.where(inl, s2, 2.0 * delta * s - delta * delta), torch.where(inl, torch.ones_like(s), delta / s)


def chi2(T, edges, Z, Omega):
    r = residuals(T, edges, Z)
    return torch.einsum("ei,eij,ej->e", r, Omega, r)


def cost(T, edges, Z, Omega, huber_delta=INF):
    return huber(chi2(T, edges, Z, Omega), huber_delta)[0].sum()


def gradient(T, edges, Z, Omega, huber_delta=INF):
    """d cost / d d_k of the update T_k <- Exp(d_k) T_k at d = 0, [K,6]: autograd through Exp, Log and rho"""
    d = torch.zeros((T.shape[0], 6), dtype=F64, device=T.device, requires_grad=True)
    cost(exp_se3(d) @ T, edges, Z, Omega, huber_delta).backward()
    return d.grad


def gradient_norm(T, edges, Z, Omega, fixed, huber_delta=INF):
    return float(gradient(T, edges, Z, Omega, huber_delta)[~fixed].norm())


def jacobians(T, edges, Z):
    """[E,6,12]: d r_e / d (d_i, d_j) at 0 -- the edges are independent, so the Jacobian of the sum over the edges holds each's"""
    zero = torch.zeros((edges.shape[0], 12), dtype=F64, device=T.device)
    J = torch.autograd.functional.jacobian(lambda d: residuals(T, edges, Z, d).sum(0), zero)  # [6,E,12]
    return J.permute(1, 0, 2)


def normal_equations(T, edges, Z, Omega, huber_delta=INF):
    """dense H [6K,6K] and g [6K] of sum J^T (w Omega) J and sum J^T (w Omega) r"""
    K, E = T.shape[0], edges.shape[0]
    r = residuals(T, edges, Z)
    _, w = huber(torch.einsum("ei,eij,ej->e", r, Omega, r), huber_delta)
    J = jacobians(T, edges, Z)
    W = w[:, None, None] * Omega
    He = J.transpose(-1, -2) @ W @ J                      # [E,12,12]
    ge = (J.transpose(-1, -2) @ W @ r[..., None])[..., 0]  # [E,12]
    dof = (edges[:, :, None] * 6 + torch.arange(6, device=T.device)).reshape(E, 12)
    H = torch.zeros((6 * K, 6 * K), dtype=F64, device=T.device)
    g = torch.zeros((6 * K,), dtype=F64, device=T.device)
    H.index_put_((dof[:, :, None].expand(E, 12, 12), dof[:, None, :].expand(E, 12, 12)), He, accumulate=True)
    g.index_put_((dof,), ge, accumulate=True)
    return H, g


def _loose(D, lam, rcond):
    """[K] bool: a pivot of the LDL^T of D + lam diag D that is not above rcond * max diag D (or not positive)"""
    K = D.shape[0]
    diag = torch.diagonal(D, dim1=-2, dim2=-1)
    M = D + lam * torch.diag_embed(diag)
    floor = rcond * diag.max(-1).values
    bad = torch.zeros(K, dtype=torch.bool, device=D.device)
    M = M.clone()
    for j in range(6):
        p = M[:, j, j]
        bad |= ~((p > floor) & (p > 0))
        p = torch.where(bad, torch.ones_like(p), p)
        M = M - M[:, :, j:j + 1] @ M[:, j:j + 1, :] / p[:, None, None]
    return bad


def solve(T, edges, Z, Omega, fixed, iterations=10, huber_delta=INF, damping=1e-4, rcond=1e-12, step_tolerance=1e-9,
          cost_tolerance=1e-12):
    """Levenberg-Marquardt as the header states it.  Returns a dict: T, costs (the accepted costs, the initial one first), trials
    (one (accepted, cost before, candidate cost) per trial), steps (the [K,6] step of every trial), accepted, rejected, loose [K],
    converged, lam."""
    K = T.shape[0]
    lam = min(max(damping, 1e-12), 1e12)
    c = float(cost(T, edges, Z, Omega, huber_delta))
    out = dict(costs=[c], trials=[], steps=[], accepted=0, rejected=0, converged=False)
    loose = torch.zeros(K, dtype=torch.bool, device=T.device)
    H = g = None
    for _ in range(iterations):
        if H is None:
            H, g = normal_equations(T, edges, Z, Omega, huber_delta)
            if not float(g.reshape(K, 6)[~fixed & ~loose].abs().max() if bool((~fixed & ~loose).any()) else 0.0) > 0.0:
                out["converged"] = True
                break
        D = torch.stack([H[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(K)])
        loose = loose | (~fixed & _loose(D, lam, rcond))
        active = ~fixed & ~loose
        if not bool(active.any()):
            out["converged"] = True
            break
        idx = (torch.nonzero(active)[:, 0][:, None] * 6 + torch.arange(6, device=T.device)).reshape(-1)
        Hd = H[idx][:, idx]
        d = torch.zeros((6 * K,), dtype=F64, device=T.device)
        d[idx] = torch.linalg.solve(Hd + lam * torch.diag(torch.diagonal(Hd)), -g[idx])
        d = d.reshape(K, 6)
        Tn = exp_se3(d) @ T
        cn = float(cost(Tn, edges, Z, Omega, huber_delta))
        ok = cn < c
        out["trials"].append((ok, c, cn))
        out["steps"].append(d)
        if ok:
            out["accepted"] += 1
            decrease = (c - cn) / c
            T, c, lam, H = Tn, cn, max(lam / 10.0, 1e-12), None
            out["costs"].append(c)
            step = max(float(d[:, :3].norm(dim=-1).max()), float(d[:, 3:].norm(dim=-1).max()))
            if step < step_tolerance or decrease < cost_tolerance:
                out["converged"] = True
                break
        else:
            out["rejected"] += 1
            lam = min(lam * 10.0, 1e12)
            if lam >= 1e12:
                break
    out.update(T=T, loose=loose, lam=lam)
    return out


# ------------------------------------------------------------------------------------------------------------ the test graphs
def look_at_circle(K, radius=2.0):
    """K keyframes on a circle of `radius` in the world's xz plane, looking at the centre: W2C [K,4,4]"""
    T = torch.zeros((K, 4, 4), dtype=F64)
    for k in range(K):
        a = 2.0 * math.pi * k / K
        pos = torch.tensor([radius * math.cos(a), 0.1 * math.sin(3 * a), radius * math.sin(a)], dtype=F64)
        zc = -pos / pos.norm()
        xc = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=F64), zc)
        xc = xc / xc.norm()
        R = torch.stack([xc, torch.linalg.cross(zc, xc), zc])  # rows: the camera's axes in the world
        T[k] = _rt(R, -R @ pos)
    return T


def ring_graph(K, loops, seed=0, rot_noise=0.02, trans_noise=0.03):
    """The reference graph: `look_at_circle` as truth, K - 1 chain edges (k + 1, k) and `loops` loop edges, each measurement the
    truth's times Exp of Gaussian noise (rot_noise rad, trans_noise m), Omega = diag(100, 100, 100, 25, 25, 25), the initial
    poses chained from the odometry.  Returns dict(truth, T0, edges, Z, Omega, fixed), float64 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    truth = look_at_circle(K)
    pairs = [(k + 1, k) for k in range(K - 1)] + [((K - 1 - 3 * n) % K, (5 * n) % K) for n in range(loops)]
    edges = torch.tensor(pairs, dtype=torch.long)
    E = edges.shape[0]
    noise = torch.randn((E, 6), generator=g, dtype=F64) * torch.tensor([rot_noise] * 3 + [trans_noise] * 3, dtype=F64)
    Z = exp_se3(noise) @ truth[edges[:, 0]] @ inverse(truth[edges[:, 1]])
    T0 = [truth[0]]
    for k in range(K - 1):
        T0.append(Z[k] @ T0[k])  # T_{k+1} = Z T_k
    Omega = torch.diag(torch.tensor([100.0] * 3 + [25.0] * 3, dtype=F64)).expand(E, 6, 6).clone()
    fixed = torch.zeros(K, dtype=torch.bool)
    fixed[0] = True
    return dict(truth=truth, T0=torch.stack(T0), edges=edges, Z=Z, Omega=Omega, fixed=fixed)
