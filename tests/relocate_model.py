"""A sequential numpy / float64 restatement of the fixed-size map upkeep (include/dgr_hip.h: dgr_relocate_*, dgr_position_noise),
written from the stated semantics and not from the kernels: Python integers for the weights, their prefix and the targets, float64
for the new opacity and scale.  The GPU tests compare csrc/relocate.hip with it."""
import math

import numpy as np

ROLES = {"xyz": "xyz", "scaling": "scaling", "rotation": "rotation", "opacity": "opacity"}
MAX_COPIES = 51


def logit_threshold(min_opacity):
    """logit(min_opacity) formed in float64 and rounded once to fp32: what the plan compares the raw opacity with"""
    if min_opacity <= 0:
        return np.float32(-np.inf)
    return np.float32(math.log(min_opacity / (1.0 - min_opacity)))


def sigmoid64(raw):
    return 1.0 / (1.0 + math.exp(-float(raw)))


def weight(raw):
    """w = rint(2^20 o), o in float64; the input is asserted not to sit within 1e-6 of a rounding tie"""
    x = 1048576.0 * sigmoid64(raw)
    assert abs((x - math.floor(x)) - 0.5) > 1e-6, f"2^20 sigmoid({raw}) = {x} sits on a rounding tie"
    return int(np.rint(x))


def new_values(o, N):
    """(o', coeff) of a Gaussian of opacity o split into N copies, before the clamp: o' = 1 - (1 - o)^(1/N), coeff = o / D with
    D = sum_{m=1..N} sum_{k=0..m-1} C(m-1, k) (-1)^k (k+1)^(-1/2) o'^(k+1), all float64"""
    o1 = 1.0 - (1.0 - o) ** (1.0 / N)
    D = 0.0
    for m in range(1, N + 1):
        for k in range(m):
            D += math.comb(m - 1, k) * (-1.0) ** k * (k + 1) ** -0.5 * o1 ** (k + 1)
    return o1, o / D


def new_raw_values(raw, N, min_opacity):
    """(new raw opacity, log(coeff)) in float64: o' clamped to [min_opacity, 1 - 2^-23], then the logit"""
    o1, coeff = new_values(sigmoid64(raw), N)
    c = min(max(o1, min_opacity), 1.0 - 2.0 ** -23)
    return math.log(c / (1.0 - c)), math.log(coeff)


def sample_sources(raw, draws, min_opacity):
    """The integer part.  raw: fp32 [P]; draws: integers [P] in [0, 2^32).  Returns (dead mask, live mask, source int32 [P] with
    -1 at the rows that are not relocated, hits int64 [P], S)."""
    raw = np.asarray(raw, dtype=np.float32).reshape(-1)
    P = raw.shape[0]
    thr = logit_threshold(min_opacity)
    finite = np.isfinite(raw)
    assert not (raw[finite] == thr).any(), "a raw opacity sits on the threshold"
    with np.errstate(invalid="ignore"):
        dead = finite & (raw < thr)
    live = finite & ~dead
    w = [weight(raw[i]) if live[i] else 0 for i in range(P)]
    C, S = [], 0
    for i in range(P):
        C.append(S)
        S += w[i]
    source, hits = np.full(P, -1, dtype=np.int32), np.zeros(P, dtype=np.int64)
    if S > 0:
        live_rows = [i for i in range(P) if w[i] > 0]
        ends = [C[i] + w[i] for i in live_rows]  # increasing
        for r in np.flatnonzero(dead):
            d = int(draws[r])
            assert 0 <= d < 2 ** 32
            t = (d * S) >> 32
            lo, hi = 0, len(ends) - 1  # the first live row whose end lies above t
            while lo < hi:
                mid = (lo + hi) // 2
                if ends[mid] > t:
                    hi = mid
                else:
                    lo = mid + 1
            i = live_rows[lo]
            assert C[i] <= t < C[i] + w[i]
            source[r] = i
            hits[i] += 1
    return dead, live, source, hits, S


def relocate_model(leaves, moments, accs, draws, min_opacity=0.005, roles=None):
    """leaves: name -> float32 array [P, ...]; moments: name -> (exp_avg, exp_avg_sq) for the leaves that have them; accs: name ->
    array with P elements (or None).  Returns a dict: counts (5 ints), source, hits, relocated / hit masks, leaves (float32: every
    copied value bit for bit, the new opacity and scale as the float64 values rounded once), moments, accs."""
    roles = dict(ROLES, **(roles or {}))
    L = {name: np.array(t, dtype=np.float32, copy=True) for name, t in leaves.items()}
    P = L[roles["xyz"]].shape[0]
    raw = L[roles["opacity"]].reshape(P).copy()
    scaling_before = L[roles["scaling"]].copy()
    dead, live, source, hits, S = sample_sources(raw, draws, min_opacity)
    relocated, hit = source >= 0, hits > 0
    new_op, log_coeff = {}, {}
    for i in np.flatnonzero(hit):
        new_op[i], log_coeff[i] = new_raw_values(raw[i], min(int(hits[i]) + 1, MAX_COPIES), min_opacity)
    before = {name: t.copy() for name, t in L.items()}
    for r in np.flatnonzero(relocated):
        s = int(source[r])
        for name in L:
            L[name][r] = before[name][s]
        L[roles["opacity"]].reshape(P)[r] = np.float32(new_op[s])
        L[roles["scaling"]][r] = (scaling_before[s].astype(np.float64) + log_coeff[s]).astype(np.float32)
    for i in np.flatnonzero(hit):
        L[roles["opacity"]].reshape(P)[i] = np.float32(new_op[i])
        L[roles["scaling"]][i] = (scaling_before[i].astype(np.float64) + log_coeff[i]).astype(np.float32)
    M = {}
    for name, pair in moments.items():
        M[name] = tuple(np.array(t, dtype=np.float32, copy=True) for t in pair)
        for t in M[name]:
            t[relocated | hit] = 0.0
    A = {}
    for name, t in accs.items():
        A[name] = None if t is None else np.array(t, dtype=np.float32, copy=True)
        if t is not None:
            A[name].reshape(P)[relocated] = 0.0
    counts = (int(dead.sum()), int(live.sum()), int(relocated.sum()), int(hit.sum()), int(hits.max()) if P else 0)
    return dict(counts=counts, source=source, hits=hits, relocated=relocated, hit=hit, S=S, leaves=L, moments=M, accs=A)


def rotation_matrix(q):
    """3DGS's build_rotation of q / |q|, q = (r, x, y, z), float64"""
    r, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(np.asarray(q, dtype=np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def position_noise_model(scaling_raw, rotation, opacity_raw, noise, lr, noise_scale=5e5, gate_k=100.0, gate_x0=0.995):
    """Returns (delta [P, 3], magnitude [P, 3]) in float64 from the fp32 inputs: delta_c = g sum_j Sigma_cj n_j and magnitude_c =
    g sum_j |Sigma_cj| |n_j|, Sigma = R S^2 R^T, g = noise_scale lr / (1 + exp(-gate_k (1 - o - gate_x0)))."""
    s = np.asarray(scaling_raw, dtype=np.float64)
    n = np.asarray(noise, dtype=np.float64)
    raw = np.asarray(opacity_raw, dtype=np.float64).reshape(-1)
    P = s.shape[0]
    delta, magnitude = np.zeros((P, 3)), np.zeros((P, 3))
    for i in range(P):
        R = rotation_matrix(rotation[i])
        cov = R @ np.diag(np.exp(s[i]) ** 2) @ R.T
        o = 1.0 / (1.0 + math.exp(-raw[i]))
        z = gate_k * (1.0 - o - gate_x0)
        gate = 1.0 / (1.0 + math.exp(-z)) if z >= 0 else math.exp(z) / (1.0 + math.exp(z))
        g = noise_scale * float(lr) * gate
        delta[i] = g * (cov @ n[i])
        magnitude[i] = g * (np.abs(cov) @ np.abs(n[i]))
    return delta, magnitude
