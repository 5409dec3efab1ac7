"""CPU models of the four small step kernels -- the fused sparse Adam and `add_densification_stats` (csrc/optim.hip), the pose
kernels (csrc/pose.hip) and the plain L1 loss (csrc/l1_loss.hip) -- with the inputs and the bars their tests share.

For every operation: a float64 model, a float32 numpy replica that follows the kernel operation for operation, cached input
families (made once: treat them as read-only) and a `*_check` function that measures outputs against the model in units of the
operation's bars.  tests/test_step_model.py runs the replicas and a list of wrong variants ("mutants") of the models through
the checks on the CPU; tests/test_hip_step_kernels.py runs the kernels through the same checks.

Every bar is a count of the kernel's rounded operations, each worth a relative U = 2^-24 (round to nearest; a contracted fma
only removes roundings), and is derived where it is defined.  None was tuned on a kernel's output."""
import functools
import math

import numpy as np

U = 2.0 ** -24      # unit roundoff of float32
TINY = 2.0 ** -149  # the smallest float32 denormal: what an underflowing result may lose

# the launch geometry the shapes below are chosen around (csrc/optim.hip, csrc/l1_loss.hip)
ADAM_GRID_PASS = 256 * 32 * 256   # elements one pass of sparse_adam_kernel's grid-stride loop covers
L1_FORWARD_THREADS = 128 * 256    # threads of l1_partial_kernel: an element past this index is some thread's second term
L1_BACKWARD_PASS = 2048 * 256     # elements one pass of l1_backward_kernel covers


def f32(x):
    """the float32 value nearest to x, as a Python float: what a `float` argument of the C ABI holds"""
    return float(np.float32(x))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


class Report(dict):
    """name -> (worst error as a fraction of its bar, fraction of the elements outside the bar); `exact` lists the names of the
    bit-for-bit checks that failed."""

    def __init__(self):
        super().__init__()
        self.exact = []

    def add(self, name, err, bar):
        err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / bar)  # (a zero bar asks for a zero error)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        self[name] = (float(ratio.max()) if ratio.size else 0.0, float((ratio > 1.0).mean()) if ratio.size else 0.0)

    def require(self, name, ok):
        if not ok:
            self.exact.append(name)

    @property
    def ok(self):
        return not self.exact and all(worst <= 1.0 for worst, _ in self.values())

    def __str__(self):
        s = ", ".join(f"{k} {w:.3g} of its bar" + (f" ({100 * f:.2g} % outside)" if f else "") for k, (w, f) in self.items())
        return s + ("; NOT EXACT: " + ", ".join(self.exact) if self.exact else "")

    def check(self, what=""):
        assert self.ok, f"{what}: {self}"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ================================================= Adam: one step from a given state =================================================
ADAM_SHAPES = [(1, (1,)), (255, (3,)), (257, (4,)), (300, (16, 3)), (1000, (45,))]  # (rows, row shape): one block, a partial
ADAM_LARGE = (43700, (16, 3))  # block, k of 1, 3, 4, 45, 48; and 2 097 600 elements: 448 past one grid pass
ADAM_EPS = (1e-15, 1e-8)
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_CAPTURABLE_STEPS = (1, 2, 10, 1000, 20000)
ADAM_MUTANTS_FORMULA = ("eps_before_bias", "eps_in_sqrt", "no_bias2", "no_bias1", "step_off_by_one")
ADAM_MUTANTS_INDEX = ("row_mod_rows", "visible_lt_0", "first_pass_only")


def adam_hyper(eps, lr=1e-2, betas=(0.9, 0.999)):
    """(lr, beta1, beta2, eps) as the float32 values the kernel receives"""
    return (f32(lr), f32(betas[0]), f32(betas[1]), f32(eps))


@functools.lru_cache(maxsize=None)
def adam_inputs(n):
    """(p, g, m0, v0): float32 [n].  g = +-10^uniform(-12, 3) with every 17th element an exact zero, m0 of both signs over the same
    range, v0 = 10^uniform(-24, 6), every 5th element m0 = v0 = 0 (a row's first step), p standard normal.
    Those are the marginals; jointly, an element's state is at its gradient's scale, as the state of a running optimiser is:
    with g = +-10^e, m0 = +-10^(e + d_m) and v0 = 10^(2 (e + d_v)), d uniform in half a decade either way and the exponent
    wrapped around [-12, 3) (which keeps it uniform).  Drawn independently, a gradient near eps would meet a sqrt(v0) near eps
    -- the regime in which a misplaced eps is visible -- in a few elements per thousand only."""
    rng = np.random.default_rng(1234 + n)
    sign = lambda: rng.choice(np.array([-1.0, 1.0]), n)  # noqa: E731
    e = rng.uniform(-12, 3, n)
    near = lambda: (e + rng.uniform(-0.5, 0.5, n) + 12.0) % 15.0 - 12.0  # noqa: E731
    g = sign() * 10.0 ** e
    m0 = sign() * 10.0 ** near()
    v0 = 10.0 ** (2.0 * near())
    g[16::17] = 0.0
    m0[4::5] = v0[4::5] = 0.0
    return _frozen(*(a.astype(np.float32) for a in (rng.standard_normal(n), g, m0, v0)))


@functools.lru_cache(maxsize=None)
def adam_visible(pattern, rows):
    """int32 [rows] or None.  "mixed": positive radii, zeros and -1 entries (the kernel skips <= 0); "mod7": i % 7 != 0, a period
    that divides neither 256 nor k, so that a wrong row index shows in the second grid pass as well."""
    i = np.arange(rows)
    if pattern == "none":
        return None
    v = {"ones": np.full(rows, 3), "zeros": np.zeros(rows), "mixed": np.where(i % 3 == 0, 0, np.where(i % 5 == 1, -1, i % 11 + 1)),
         "mod7": (i % 7 != 0) * 5}[pattern].astype(np.int32)
    return _frozen(v)[0]


def adam_selected(n, k, visible, mutant=None):
    """bool [n]: the elements the step updates"""
    e = np.arange(n)
    sel = np.ones(n, dtype=bool)
    if visible is not None:
        row = e % len(visible) if mutant == "row_mod_rows" else e // k
        sel = visible[row] >= 0 if mutant == "visible_lt_0" else visible[row] > 0
    if mutant == "first_pass_only":
        sel = sel & (e < ADAM_GRID_PASS)
    return sel


def adam_mutant_differs(mutant, hyper, step):
    """whether a formula mutant is another function at this step at all (decided from the formula, not from any output): the
    bias mutants where the bias they touch is not 1.0 in float64, eps inside the root everywhere"""
    _, b1, b2, _ = hyper
    bias1, bias2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return {"eps_before_bias": bias2 != 1.0, "no_bias2": bias2 != 1.0, "no_bias1": bias1 != 1.0, "eps_in_sqrt": True,
            "step_off_by_one": bias1 != 1.0 or bias2 != 1.0}[mutant]


def adam_update64(m, v, hyper, step, mutant=None):
    """torch.optim.Adam's update lr / bias1 * m / (sqrt(v / bias2) + eps) in float64, or a wrong variant of it"""
    lr, b1, b2, eps = hyper
    t = step + 1 if mutant == "step_off_by_one" else step
    bias1 = 1.0 if mutant == "no_bias1" else 1.0 - b1 ** t
    bias2 = 1.0 if mutant == "no_bias2" else 1.0 - b2 ** t
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if mutant == "eps_before_bias":
        den = (np.sqrt(v) + eps) / math.sqrt(bias2)
    elif mutant == "eps_in_sqrt":
        den = np.sqrt(v / bias2 + eps)
    else:
        den = np.sqrt(v / bias2) + eps
    return lr / bias1 * m / den


def adam_moments64(g, m0, v0, hyper):
    _, b1, b2, _ = hyper
    g, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (g, m0, v0))
    return b1 * m0 + (1.0 - b1) * g, b2 * v0 + (1.0 - b2) * g * g


def adam_model(inputs, k, visible, hyper, step, mutant=None):
    """(p, m, v) float64 [n] after one step; the rows the step skips keep their values"""
    p, g, m0, v0 = (np.asarray(a, dtype=np.float64) for a in inputs)
    sel = adam_selected(len(p), k, visible, mutant)
    with np.errstate(invalid="ignore"):
        m, v = adam_moments64(g, m0, v0, hyper)
        # (a mutant is a wrong UPDATE: it sees the moments a device would return, rounded to float32)
        u = adam_update64(m.astype(np.float32), v.astype(np.float32), hyper, step, mutant)
    return np.where(sel, p - u, p), np.where(sel, m, m0), np.where(sel, v, v0)


def adam_replica32(inputs, k, visible, hyper, step, capturable=False):
    """sparse_adam_kernel in numpy float32, operation for operation (without fma contraction)"""
    p, g, m0, v0 = inputs
    lr, b1, b2, eps = (np.float32(x) for x in hyper)
    one = np.float32(1.0)
    if capturable:  # the corrections formed in float32 from the step count, as the kernel forms them
        st = np.float32(step)
        step_size = lr / (one - np.power(b1, st, dtype=np.float32))
        inv_sqrt_bias2 = one / np.sqrt(one - np.power(b2, st, dtype=np.float32))
    else:  # formed in double on the host, rounded once
        step_size = np.float32(float(lr) / (1.0 - float(b1) ** step))
        inv_sqrt_bias2 = np.float32(1.0 / math.sqrt(1.0 - float(b2) ** step))
    sel = adam_selected(len(p), k, visible)
    with np.errstate(invalid="ignore"):
        m = b1 * m0 + (one - b1) * g
        v = b2 * v0 + (one - b2) * g * g
        p_new = p - step_size * m / (np.sqrt(v) * inv_sqrt_bias2 + eps)
    return np.where(sel, p_new, p), np.where(sel, m, m0), np.where(sel, v, v0)


def adam_p_factor(hyper, step, capturable):
    """The multiple of U |u| the parameter may be off by, besides the final subtraction's U |p - u|.
    Host form, 8: step_size and inv_sqrt_bias2 are each one rounding of a double (2), then step_size * m, sqrtf, * inv_sqrt_bias2,
    + eps and the division are five rounded operations on positive terms (5): 7, and one to spare for sqrtf.
    Capturable form: besides, the two corrections are formed in float32.  A powf off by up to 3 ulp of beta^t (< 4 U beta^t),
    the subtraction from 1 and the division move step_size by < 4 U / (1 - beta1^t) relative (beta^t < 1); for the second
    correction the root halves the same 4 U / (1 - beta2^t): 2 U / (1 - beta2^t)."""
    _, b1, b2, _ = hyper
    return 8.0 + (4.0 / (1.0 - b1 ** step) + 2.0 / (1.0 - b2 ** step) if capturable else 0.0)


def adam_check(inputs, k, visible, hyper, step, p_out, m_out, v_out, capturable=False):
    """Report of one step's outputs (float32 [n]) against the model, in two stages so that cancellation in m is not paid for in p.
      m: |m - m64| <= 3 U (|b1 m0| + |(1 - b1) g|): 1 - b1, its product with g, b1 m0 and the sum are one rounding each, at most three
         of them on either term.
      v: |v - v64| <= 4 U v64 + TINY: (1 - b2) g g is three roundings, b2 v0 one, the sum of the two positive terms one more: at most
         four on either term.
      p: against p - u64 with u64 the float64 update of the moments the DEVICE returned: U |p - u64| for the subtraction and
         adam_p_factor() U |u64| for the update, + TINY.
    The rows the step skips must keep parameter and both moments bit for bit."""
    p, g, m0, v0 = inputs
    _, b1, _, _ = hyper
    sel = adam_selected(len(p), k, visible)
    rep = Report()
    skip = ~sel
    rep.require("skipped rows keep p, m, v", same_bits(p_out[skip], p[skip]) and same_bits(m_out[skip], m0[skip]) and
                same_bits(v_out[skip], v0[skip]))
    p, g, m0, v0, p_out, m_out, v_out = (np.asarray(a, dtype=np.float64)[sel] for a in (p, g, m0, v0, p_out, m_out, v_out))
    m64, v64 = adam_moments64(g, m0, v0, hyper)
    rep.add("m", np.abs(m_out - m64), 3 * U * (np.abs(b1 * m0) + np.abs((1.0 - b1) * g)))
    rep.add("v", np.abs(v_out - v64), 4 * U * v64 + TINY)
    u64 = adam_update64(m_out, v_out, hyper, step)
    target = p - u64
    rep.add("p", np.abs(p_out - target), U * np.abs(target) + adam_p_factor(hyper, step, capturable) * U * np.abs(u64) + TINY)
    return rep


# ================================================= densification statistics =================================================
STATS_ROWS = (1, 256, 257, 5001)  # one row, a full block, one row into the next, many blocks with a partial one
STATS_VIEWS = 5


@functools.lru_cache(maxsize=None)
def stats_inputs(rows):
    """dict(dmeans [V, P, 4] float32 (the kernel reads [:, :3] of it; column 3 is a canary), radii [V, P] int32, accum0, denom0,
    maxr0 float32 [P]).  Gradients +-10^uniform(-6, 2); radii -1 .. 39 with about 30 % zeros; rows with i % 4 == 3 are never seen
    and carry a NaN gradient in every view; every row with radii <= 0 in a view has a NaN gradient in view 0."""
    rng = np.random.default_rng(77 + rows)
    V, P = STATS_VIEWS, rows
    d = rng.choice(np.array([-1.0, 1.0]), (V, P, 4)) * 10.0 ** rng.uniform(-6, 2, (V, P, 4))
    radii = rng.integers(-1, 40, (V, P))
    radii[rng.random((V, P)) < 0.3] = 0
    never = np.arange(P) % 4 == 3
    if P > 1:
        radii[:, never] = np.where(np.arange(V)[:, None] % 2 == 0, 0, -1)
        d[:, never, :2] = np.nan
    else:
        radii[:] = 7  # (the one row is seen)
    d[0, radii[0] <= 0, :2] = np.nan
    accum0 = rng.random(P) * (rng.random(P) < 0.5)
    denom0 = rng.integers(0, 4, P).astype(np.float64)
    maxr0 = rng.integers(0, 20, P).astype(np.float64)
    out = dict(dmeans=d.astype(np.float32), radii=radii.astype(np.int32), accum0=accum0.astype(np.float32),
               denom0=denom0.astype(np.float32), maxr0=maxr0.astype(np.float32))
    _frozen(*out.values())
    return out


def stats_model(inp, views=STATS_VIEWS, dtype=np.float64):
    """(accum, denom, max_radii2D) after `views` views: accumulated in float64 (the model), or in float32 with the kernel's
    operations (the replica, dtype=np.float32)"""
    accum, denom, maxr = (inp[k].astype(dtype) for k in ("accum0", "denom0", "maxr0"))
    for v in range(views):
        seen = inp["radii"][v] > 0
        gx, gy = inp["dmeans"][v, :, 0].astype(dtype), inp["dmeans"][v, :, 1].astype(dtype)
        with np.errstate(invalid="ignore"):
            norm = np.sqrt(gx * gx + gy * gy)
        accum = np.where(seen, accum + norm, accum)
        denom = np.where(seen, denom + dtype(1.0), denom)
        maxr = np.where(seen, np.maximum(maxr, inp["radii"][v].astype(dtype)), maxr)
    return accum, denom, maxr


def stats_check(inp, accum, denom, maxr, views=STATS_VIEWS):
    """accum: |accum - accum64| <= 3 U V max(accum64) per row, the maximum over the views being the last value of a sum of
    non-negative terms: per view gx gx + gy gy is three roundings that the root halves (1.5 U), sqrtf one more -- under 3 U of the
    term -- and the addition U of the running sum; both are at most the row's final sum.  denom and max_radii2D are small
    integers in float32: exact.  A row no view saw keeps all three bit for bit (NaN gradients included).  None skips an output."""
    a64, d64, r64 = stats_model(inp, views)
    rep = Report()
    never = ~(inp["radii"][:views] > 0).any(axis=0)
    if accum is not None:
        rep.add("accum", np.abs(accum.astype(np.float64) - a64), 3 * U * views * a64)
        rep.require("unseen rows keep accum", same_bits(accum[never], inp["accum0"][never]))
    if denom is not None:
        rep.require("denom exact", np.array_equal(denom.astype(np.float64), d64))
    if maxr is not None:
        rep.require("max_radii2D exact", np.array_equal(maxr.astype(np.float64), r64))
    return rep


# ================================================= pose =================================================
POSE_SCALES = (1e-3, 1.0, 1e3)  # |q|: the backward divides by it and projects along q
POSE_RANDOM = 200               # random rotations per scale
TANFOV = (0.6, 0.45)
POSE_MUTANTS = ("no_division_by_norm", "no_projection", "G_transposed", "skew_sign")


@functools.lru_cache(maxsize=None)
def pose_cases():
    """dict(q [N, 4], t [N, 3], dview [N, 4, 4] float32, label: list of N).  Per scale: 200 random unit quaternions, the identity,
    the three 180 degree rotations (r = 0), r = -1 with a 1e-4 vector part about each axis; |t| = 10^uniform(-3, 2); random
    upstream gradients.  Case i + N / 2 is case i with -q (same rotation, same upstream)."""
    rng = np.random.default_rng(99)
    special = [("identity", (1, 0, 0, 0))]
    for a in range(3):
        v = [0.0, 0.0, 0.0]
        v[a] = 1.0
        special.append((f"180 about {'xyz'[a]}", (0.0, *v)))
    for a in range(3):
        v = [0.0, 0.0, 0.0]
        v[a] = 1e-4
        special.append((f"r = -1, 1e-4 about {'xyz'[a]}", (-1.0, *v)))
    q, label = [], []
    for s in POSE_SCALES:
        r = rng.standard_normal((POSE_RANDOM, 4))
        r /= np.linalg.norm(r, axis=1, keepdims=True)
        q += [s * x for x in r] + [s * np.array(x, dtype=np.float64) for _, x in special]
        label += [f"random {i} at |q| = {s:g}" for i in range(POSE_RANDOM)] + [f"{n} at |q| = {s:g}" for n, _ in special]
    q = np.array(q)
    n = len(q)
    d = rng.standard_normal((n, 3))
    t = d / np.linalg.norm(d, axis=1, keepdims=True) * 10.0 ** rng.uniform(-3, 2, (n, 1))
    dview = rng.standard_normal((n, 4, 4))
    q, t, dview = np.concatenate([q, -q]), np.concatenate([t, t]), np.concatenate([dview, dview])
    label = label + ["-q of " + s for s in label]
    return dict(label=label, **dict(zip(("q", "t", "dview"), _frozen(*(a.astype(np.float32) for a in (q, t, dview))))))


def pose_perspec():
    """Proj^T of the symmetric frustum as float32 [4, 4]: the kernel's third input"""
    tx, ty, zn, zf = TANFOV[0], TANFOV[1], 0.01, 100.0
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[2, 2], P[2, 3], P[3, 2] = 1.0 / tx, 1.0 / ty, zf / (zf - zn), -(zf * zn) / (zf - zn), 1.0
    return P.T.astype(np.float32)


@functools.lru_cache(maxsize=None)
def pose_model64():
    """dict(view [N, 4, 4], campos [N, 3], dq [N, 4], dt [N, 3]) float64: `slam.camera_tensors(slam.w2c_from_quat_trans(q, t))`
    on the CPU in float64 with float64 autograd of sum(view * dview) -- the package's own formulation through quat_to_rotmat,
    written independently of the kernel's closed form."""
    import torch
    from dgr_amd import slam
    c = pose_cases()
    out = dict(view=[], campos=[], dq=[], dt=[])
    h = len(c["q"]) // 2  # (the -q half below: R(-q) = R(q), so the same tensors with dq negated)
    for q, t, w in zip(c["q"][:h], c["t"][:h], c["dview"][:h]):
        q64 = torch.tensor(q.astype(np.float64), requires_grad=True)
        t64 = torch.tensor(t.astype(np.float64), requires_grad=True)
        view, _, _, campos = slam.camera_tensors(slam.w2c_from_quat_trans(q64, t64), *TANFOV)
        (view * torch.tensor(w.astype(np.float64))).sum().backward()
        for k, x in (("view", view.detach()), ("campos", campos), ("dq", q64.grad), ("dt", t64.grad)):
            out[k].append(x.numpy().copy())
    out = {k: np.array(v) for k, v in out.items()}
    return {k: np.concatenate([v, -v if k == "dq" else v]) for k, v in out.items()}


def pose_closed_form(q, t, perspec, dview, F=np.float32, mutant=None):
    """pose_forward_kernel and pose_backward_kernel for one case in scalar arithmetic of type F, operation for operation:
    F = np.float32 is the replica, F = np.float64 with `mutant` a wrong variant of the model.  Returns (view, proj, campos, dq, dt)."""
    q, t = [F(x) for x in q], [F(x) for x in t]
    P = [[F(x) for x in row] for row in perspec]
    D = [[F(x) for x in row] for row in dview]
    one, two, zero = F(1.0), F(2.0), F(0.0)
    inv = one / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    qh = [x * inv for x in q]
    r, x, y, z = qh
    d = r * r - (x * x + y * y + z * z)
    R = [[d + two * x * x, two * x * y - two * r * z, two * x * z + two * r * y],
         [two * x * y + two * r * z, d + two * y * y, two * y * z - two * r * x],
         [two * x * z - two * r * y, two * y * z + two * r * x, d + two * z * z]]
    V = [[R[j][i] for j in range(3)] + [zero] for i in range(3)] + [[t[0], t[1], t[2], one]]
    proj = [[zero] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            s = zero
            for k in range(4):
                s = s + V[i][k] * P[k][j]
            proj[i][j] = s
    campos = [-(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]) for i in range(3)]
    # backward
    G = [[D[a][b] if mutant == "G_transposed" else D[b][a] for b in range(3)] for a in range(3)]
    dt = [D[3][a] for a in range(3)]
    v = qh[1:]
    tr = G[0][0] + G[1][1] + G[2][2]
    g = [zero] * 4
    g[0] = two * r * tr + two * (-v[2] * G[0][1] + v[1] * G[0][2] + v[2] * G[1][0] - v[0] * G[1][2] - v[1] * G[2][0] + v[0] * G[2][1])
    skew = [G[2][1] - G[1][2], G[0][2] - G[2][0], G[1][0] - G[0][1]]
    if mutant == "skew_sign":
        skew[0] = G[2][1] + G[1][2]
    for k in range(3):
        gv = zero
        for j in range(3):
            gv = gv + (G[k][j] + G[j][k]) * v[j]
        g[1 + k] = -two * v[k] * tr + two * gv + two * r * skew[k]
    along = qh[0] * g[0] + qh[1] * g[1] + qh[2] * g[2] + qh[3] * g[3]
    if mutant == "no_projection":
        along = zero
    scale = one if mutant == "no_division_by_norm" else inv
    dq = [(g[i] - qh[i] * along) * scale for i in range(4)]
    return tuple(np.array(a, dtype=F) for a in (V, proj, campos, dq, dt))


def pose_outputs(F=np.float32, mutant=None):
    """pose_closed_form over every case: dict(view, proj, campos, dq, dt) of stacked arrays"""
    c, P = pose_cases(), pose_perspec()
    cols = zip(*(pose_closed_form(q, t, P, w, F, mutant) for q, t, w in zip(c["q"], c["t"], c["dview"])))
    return {k: np.array(list(col)) for k, col in zip(("view", "proj", "campos", "dq", "dt"), cols)}


def pose_check(out):
    """Report of dict(view, proj, campos, dq, dt) [N, ...] against pose_model64().  With |q_hat| = 1 every product of two
    components of q_hat is at most 1 in magnitude and carries the two normalisations' and its own rounding.
      view, rotation part: |D| <= 16 U.  An entry is at most six such products (the diagonal: r r, x x, y y, z z and 2 x x) added
         up: the normalisation (the sum of four squares, the root, the reciprocal, the product: under 4 U per component, 8 U per
         product of two, on a rotation whose entries are quadratic forms of magnitude <= 1) and about one U per product and sum.
         The translation row, the zeros and the 1 are copies: exact.
      proj[i][j]: |D| <= 8 U sum_k |V_ik| |P_kj| against the float64 product of the view THE DEVICE RETURNED with the float32
         perspec matrix the kernel was given: four rounded products and four rounded additions (the sum starts from 0).  The
         rotation's own error is the view bar's business.
      campos[i]: |D| <= 8 U sum_j |R_ji| |t_j| + 16 U |t|: three products and two sums on the first term, the rotation's 16 U
         against a vector of length |t| on the second.
      dq: |D| <= 16 U sum |G_ab| / |q|: every component of g is a sum of at most eleven terms 2 q_hat G, the projection adds
         four more; each carries the normalisation's roundings and a handful of its own, against a total of at most
         4 sum|G|: the same 16 U as the rotation, on sum |G| / |q|.
      dt is a copy: exact.
      |q . dq| <= 32 U sum|G|: q . dq = |q| q_hat . dq vanishes exactly; what is left is twice dq's error (|q| cancels).
    And -q is the same rotation: equal view, opposite dq, exactly -- IEEE operations commute with a change of sign (compared
    as values: x - x is +0 for either sign of x)."""
    c, m = pose_cases(), pose_model64()
    q, t, G = c["q"].astype(np.float64), c["t"].astype(np.float64), np.abs(c["dview"].astype(np.float64)[:, :3, :3]).sum((1, 2))
    norm_q = np.linalg.norm(q, axis=1)
    rep = Report()
    view = np.asarray(out["view"], dtype=np.float64)
    rep.add("view", np.abs(view[:, :3, :3] - m["view"][:, :3, :3]).max((1, 2)), 16 * U)
    rest = view.copy()
    rest[:, :3, :3] = 0.0
    want = np.zeros_like(rest)
    want[:, 3, :3], want[:, 3, 3] = t, 1.0
    rep.require("translation row exact", np.array_equal(rest, want))
    P = pose_perspec().astype(np.float64)
    rep.add("proj", np.abs(np.asarray(out["proj"], dtype=np.float64) - view @ P), 8 * U * (np.abs(view) @ np.abs(P)))
    R = m["view"][:, :3, :3]  # view[i][j] = R[j][i]: campos[i] = -sum_j R[j][i] t[j] = -sum_j view[i][j] t[j]
    rep.add("campos", np.abs(np.asarray(out["campos"], dtype=np.float64) - m["campos"]),
            8 * U * np.einsum("nij,nj->ni", np.abs(R), np.abs(t)) + 16 * U * np.linalg.norm(t, axis=1, keepdims=True))
    dq = np.asarray(out["dq"], dtype=np.float64)
    rep.add("dq", np.abs(dq - m["dq"]).max(1), 16 * U * G / norm_q)
    rep.require("dt exact", np.array_equal(np.asarray(out["dt"], dtype=np.float64), m["dt"]))
    rep.add("q . dq", np.abs((q * dq).sum(1)), 32 * U * G)
    h = len(q) // 2
    rep.require("-q: same view", np.array_equal(out["view"][:h], out["view"][h:]))
    rep.require("-q: opposite dq", np.array_equal(out["dq"][:h], -np.asarray(out["dq"][h:])))
    return rep


# ================================================= L1 loss =================================================
L1_FAMILIES = ("dyadic", "random")
# (colour shape, depth shape): one element each; one forward pass with a partial block; the forward's second term (57 600 colour
# elements); the backward's second pass on the colour loop (529 200 > 524 288); and on the depth loop with n_d > n_c (532 900)
L1_SHAPES = [((3, 1, 1), (1, 1, 1)), ((3, 37, 53), (1, 37, 53)), ((3, 120, 160), (1, 120, 160)), ((3, 420, 420), (1, 420, 420)),
             ((1, 8, 8), (1, 730, 730))]
L1_UPSTREAM = 3.0
L1_MUTANTS = ("forward_first_term_only", "backward_first_pass_only", "n_from_color")


@functools.lru_cache(maxsize=None)
def l1_inputs(family, shapes):
    """dict(color, color_obs, depth, depth_obs float32 of `shapes`; w_color, w_depth).
    dyadic: multiples of 1/4 in [0, 4] with a block of exact ties; w_c = n_c 2^-20, w_d = n_d 2^-21, so that k_c = 2^-20 and
            k_d = 2^-21 and every term and every partial sum, in any order, is a small multiple of 2^-23: exact in float32.
    random: uniform values, a block of ties, weights 1 and 0.5."""
    cs, ds = shapes
    rng = np.random.default_rng(5 + 1000 * L1_FAMILIES.index(family) + L1_SHAPES.index(shapes))
    n_c, n_d = math.prod(cs), math.prod(ds)
    if family == "dyadic":
        draw = lambda s: rng.integers(0, 17, s) / 4.0  # noqa: E731
        w_c, w_d = n_c * 2.0 ** -20, n_d * 2.0 ** -21
    else:
        draw = lambda s: rng.random(s) * 4.0  # noqa: E731
        w_c, w_d = 1.0, 0.5
    c, co, d, do = (draw(cs).astype(np.float32), draw(cs).astype(np.float32), draw(ds).astype(np.float32), draw(ds).astype(np.float32))
    co.reshape(-1)[:max(1, n_c // 7):2] = c.reshape(-1)[:max(1, n_c // 7):2]  # ties: sign(0) = 0
    do.reshape(-1)[-max(1, n_d // 9):] = d.reshape(-1)[-max(1, n_d // 9):]
    if n_c == 3:
        co.reshape(-1)[1], co.reshape(-1)[2] = c.reshape(-1)[1] + 0.5, c.reshape(-1)[2] - 0.25  # (not ties only)
    _frozen(c, co, d, do)
    return dict(color=c, color_obs=co, depth=d, depth_obs=do, w_color=f32(w_c), w_depth=f32(w_d))


def l1_scales(inp):
    """(k_c, k_d) as the launcher forms them: float32(w / float32(n))"""
    n_c, n_d = inp["color"].size, inp["depth"].size
    return (np.float32(inp["w_color"]) / np.float32(n_c) if n_c else np.float32(0.0),
            np.float32(inp["w_depth"]) / np.float32(n_d) if n_d else np.float32(0.0))


def l1_model(inp, mutant=None, upstream=L1_UPSTREAM):
    """(loss float64, dcolor, ddepth float32) -- the gradients are exact by construction: float32(up k) sign(x - x_obs), sign(0) = 0,
    `upstream` being the factor the loss is multiplied by downstream.  The mutants drop what a kernel without its grid-stride
    passes would drop (unwritten = NaN)."""
    c, co, d, do = (inp[k].reshape(-1) for k in ("color", "color_obs", "depth", "depth_obs"))
    k_c, k_d = l1_scales(inp)
    ac, ad = np.abs(c.astype(np.float64) - co), np.abs(d.astype(np.float64) - do)
    if mutant == "forward_first_term_only":
        ac, ad = ac[:L1_FORWARD_THREADS], ad[:L1_FORWARD_THREADS]
    loss = float(k_c) * ac.sum() + float(k_d) * ad.sum()
    up = np.float32(upstream)
    dc, dd = (up * k_c) * np.sign(c - co), (up * k_d) * np.sign(d - do)
    if mutant == "backward_first_pass_only":
        dc[L1_BACKWARD_PASS:] = np.nan
        dd[L1_BACKWARD_PASS:] = np.nan
    if mutant == "n_from_color":
        dd[c.size:] = np.nan
    return loss, dc.astype(np.float32).reshape(inp["color"].shape), dd.astype(np.float32).reshape(inp["depth"].shape)


def _xor_reduce64(s):
    """the 64-lane butterfly of __shfl_xor: s [..., 64] -> every lane holds the sum; lane 0 is returned"""
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ off]
    return s[..., 0]


def l1_replica32(inp):
    """l1_partial_kernel + l1_final_kernel in numpy float32: 32 768 threads with their serial terms, the wave butterflies, the
    four waves of a block, the 128 partials"""
    k_c, k_d = l1_scales(inp)
    s = np.zeros(L1_FORWARD_THREADS, dtype=np.float32)
    for k, a, b in ((k_c, inp["color"], inp["color_obs"]), (k_d, inp["depth"], inp["depth_obs"])):
        term = k * np.abs(a.reshape(-1) - b.reshape(-1))
        for lo in range(0, term.size, L1_FORWARD_THREADS):
            part = term[lo:lo + L1_FORWARD_THREADS]
            s[:part.size] += part
    red = _xor_reduce64(s.reshape(128, 4, 64))
    partial = (red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])
    return _xor_reduce64(np.float32(0.0) + partial[:64] + partial[64:])


def l1_loss_bar(inp, loss64):
    """random family: |loss - loss64| <= (ceil(n / 32768) + 24) U loss64 with n = n_c + n_d.  All terms are non-negative, so every
    rounding is relative to at most the total: a thread adds at most ceil(n_c / 32768) + ceil(n_d / 32768) <= ceil(n / 32768) + 1
    terms serially, each term is a subtraction and a product (2) of a k that is itself a rounded quotient (1), and the tree above
    the threads is 6 + 2 + 2 + 6 = 16 additions: ceil(n / 32768) + 20, and four to spare."""
    n = inp["color"].size + inp["depth"].size
    return (math.ceil(n / L1_FORWARD_THREADS) + 24) * U * loss64


def l1_check(inp, family, loss, dcolor, ddepth, upstream=L1_UPSTREAM):
    """Report: the dyadic loss must EQUAL the float64 sum (a dropped or doubly counted element shows), the random one meets
    l1_loss_bar; both gradients bit for bit.  None skips an output."""
    loss64, dc, dd = l1_model(inp, upstream=upstream)
    rep = Report()
    if loss is not None:
        if family == "dyadic":
            rep.require(f"loss {float(loss)!r} == {loss64!r}", float(loss) == loss64)
        else:
            rep.add("loss", abs(float(loss) - loss64), l1_loss_bar(inp, loss64))
    if dcolor is not None:
        rep.require("dcolor bit for bit", same_bits(dcolor, dc))
    if ddepth is not None:
        rep.require("ddepth bit for bit", same_bits(ddepth, dd))
    return rep
