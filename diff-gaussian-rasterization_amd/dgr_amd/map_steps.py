"""The steps that work on the whole Gaussian map, each fused through the C ABI (include/dgr_hip.h states the semantics).

`add_densification_stats` is 3DGS's per-view bookkeeping in one launch (`dgr_densification_stats`, csrc/optim.hip).
`densify_and_prune` is the step that changes P: 3DGS's densify_and_clone, densify_and_split and prune_points over every
leaf, Adam moment and accumulator in three launches (`dgr_densify_plan`, `dgr_densify_apply`) and one host read.
`seed_from_frame` is its sibling: it appends one Gaussian per unexplained pixel of an RGB-D keyframe (`dgr_seed_plan`,
`dgr_seed_apply`).
`relocate_dead` and `inject_position_noise` keep a map of FIXED size healthy (3DGS-MCMC's two steps; `dgr_relocate_plan`,
`dgr_relocate_apply`, `dgr_position_noise`): in place, no host read, capturable.
`transform_map` moves the map after a pose-graph update, every Gaussian by the Sim(3) transform of the keyframe it is anchored to
(`dgr_transform_plan`, `dgr_transform_apply`), and `pose_corrections` forms those transforms from the old and new poses: likewise.
All see the model through `_ModelTable`, enter the library through `_capi.StepCalls` and keep their names in `dgr_amd.optim`.
"""
import collections
import ctypes
import math

import torch

from . import _capi


@torch.no_grad()
def add_densification_stats(dmeans2D, radii, xyz_gradient_accum=None, denom=None, max_radii2D=None):
    """3DGS's per-view densification bookkeeping in one launch (`dgr_densification_stats`): for rows with radii > 0,
    `xyz_gradient_accum += |dmeans2D[:, :2]|`, `denom += 1`, `max_radii2D = max(max_radii2D, radii)`, on the
    tensors' device and its current stream, whichever device is current.
    `dmeans2D`: the `.grad` of the `means2D` tensor handed to the rasterizer ([P, 3]); the three accumulators are float32
    tensors with P elements ([P] or [P, 1]), updated in place; pass None to skip one."""
    P = radii.numel()
    for t in (xyz_gradient_accum, denom, max_radii2D):
        if t is not None and (t.numel() != P or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
            raise RuntimeError("add_densification_stats: accumulators must be contiguous float32 GPU tensors with P elements")
    if (radii.dtype != torch.int32 or not radii.is_cuda or not dmeans2D.is_cuda or dmeans2D.shape != (P, 3) or
            dmeans2D.dtype != torch.float32):
        raise RuntimeError("add_densification_stats: radii must be int32 [P] and dmeans2D float32 [P, 3] on the GPU")
    if any(t is not None and t.device != radii.device for t in (dmeans2D, xyz_gradient_accum, denom, max_radii2D)):
        raise RuntimeError("add_densification_stats: every tensor must be on radii's device")
    ptr = lambda t: None if t is None else t.data_ptr()
    _capi.call("dgr_densification_stats", radii.device, P, dmeans2D.contiguous().data_ptr(), radii.contiguous().data_ptr(),
               ptr(xyz_gradient_accum), ptr(denom), ptr(max_radii2D))


DensifyCounts = collections.namedtuple("DensifyCounts", "rows survivors clones children split")
DEFAULT_ROLES = {"xyz": "xyz", "scaling": "scaling", "rotation": "rotation", "opacity": "opacity"}


def densify_thresholds(grad_threshold, extent, percent_dense=0.01, min_opacity=0.005, max_screen_size=None):
    """The five fp32 thresholds of `dgr_densify_plan`, formed in float64 (ctypes rounds each once to fp32): grad_threshold,
    logit(min_opacity), log(percent_dense * extent), log(0.1 * extent) and max_screen_size -- the last two +inf when
    max_screen_size is None (neither size rule prunes then)."""
    inf = float("inf")
    logit = -inf if min_opacity <= 0 else inf if min_opacity >= 1 else math.log(min_opacity / (1.0 - min_opacity))
    sized = max_screen_size is not None
    return (float(grad_threshold), logit, math.log(percent_dense * extent), math.log(0.1 * extent) if sized else inf,
            float(max_screen_size) if sized else inf)


def _rows_tensor(t, P, what, who):  # `t` detached, checked; no copy
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() < 1 or t.shape[0] != P:
        raise RuntimeError(f"{who}: {what} must be a float32 GPU tensor with {P} rows")
    return t.detach()


def _in_place(t, what, who):
    if not t.is_contiguous():
        raise RuntimeError(f"{who}: {what} is rewritten in place and must be contiguous")
    return t


class _ModelTable:
    """The model as every map step (`who` in the messages) sees it: the leaves by role, P and the device, the checks of the leaves
    and the accumulators, and the table of per-Gaussian tensors that a dgr_*_apply call walks -- every leaf followed by its two
    Adam moments, then the accumulators -- handed over as descriptors, 24 at a time.  As it stands it serves the steps that
    rewrite the tensors in place: a row is (tensor, k, mode) and nothing is copied.  Called in the order the refusals are
    reported in."""
    as_input = staticmethod(lambda t: t)  # what a checked leaf or accumulator becomes before the kernels get it

    def __init__(self, who, params, optimizer, roles, known_roles):
        self.who, self.params, self.optimizer = who, params, optimizer
        self.roles = dict(known_roles, **(roles or {}))
        missing = [r for r in DEFAULT_ROLES if self.roles[r] not in params]
        if missing:
            raise KeyError(f"{who}: params has no entry for {missing} (roles = {self.roles})")
        self.table, self.out, self.moments = [], {}, {}

    def locate(self):  # P and the device, from the xyz leaf
        xyz = self.params[self.roles["xyz"]]
        if not xyz.is_cuda:
            raise RuntimeError(f"{self.who}: the parameters must live on the GPU")
        self.P, self.dev = xyz.shape[0], xyz.device
        return self.P

    def check_leaves(self):  # self.src: the leaves, detached (the opacity leaf's shape is the caller's to check)
        P, roles, as_input = self.P, self.roles, self.as_input
        self.src = {name: as_input(_rows_tensor(t, P, f"params[{name!r}]", self.who)) for name, t in self.params.items()}
        for role, shape in (("xyz", (P, 3)), ("scaling", (P, 3)), ("rotation", (P, 4))):
            if tuple(self.src[roles[role]].shape) != shape:
                raise RuntimeError(f"{self.who}: the {role} leaf must be [P, {shape[1]}]")
        return self.src

    def check_accumulators(self, xyz_gradient_accum, denom, max_radii2D, required=()):  # self.acc: name -> tensor or None
        self.acc = {"xyz_gradient_accum": xyz_gradient_accum, "denom": denom, "max_radii2D": max_radii2D}
        for name, t in self.acc.items():
            if t is None and name not in required:
                continue
            if t is None or t.numel() != self.P:
                raise RuntimeError(f"{self.who}: {name} must have P elements")
            self.acc[name] = self.as_input(_rows_tensor(t, self.P, name, self.who))
        return self.acc

    def add(self, t, tail, k, mode):  # one row of the table: `t` ([P, *tail], k per row) rewritten as `mode` says
        self.table.append((t, k, mode))
        return t

    def check_moments(self, name, t, state):  # the two moments of the leaf `t`, as their rows take them
        for m in state:
            if m.shape != t.shape or m.dtype != torch.float32 or m.device != t.device:
                raise RuntimeError(f"{self.who}: the moments of params[{name!r}] must have its shape, dtype and device")
            _in_place(m, f"a moment of params[{name!r}]", self.who)
        return state

    def carry_empty(self, t, tail):  # a leaf or moment without a value per row (a degree-0 model's [P, 0, 3] f_rest): no kernel sees it
        return t

    def add_leaves(self, fields_of, moment_fields):
        # every leaf as `fields_of(name)` = (mode[, value]) says, each followed by its two moments where the optimiser has them;
        # a leaf of zero width has no row of the table (the C ABI refuses k < 1 and a NULL tensor): it is carried as it is
        add, state_of = self.add, self.optimizer.state if self.optimizer is not None else {}
        for name, t in self.src.items():
            tail = tuple(t.shape[1:])
            k = math.prod(tail)
            state = state_of.get(self.params[name])
            if k == 0:
                self.out[name] = self.carry_empty(t, tail)
                if state is not None:
                    if any(m.shape != t.shape or m.dtype != torch.float32 or m.device != t.device for m in state):
                        raise RuntimeError(f"{self.who}: the moments of params[{name!r}] must have its shape, dtype and device")
                    self.moments[name] = tuple(self.carry_empty(m, tail) for m in state)
                continue
            self.out[name] = add(t, tail, k, *fields_of(name))
            if state is not None:
                self.moments[name] = tuple(add(m, tail, k, *moment_fields) for m in self.check_moments(name, t, state))

    def add_accumulators(self, *fields):  # the accumulators that were given, one value per row: name -> the row's tensor
        return {name: self.add(t, tuple(t.shape[1:]), 1, *fields) for name, t in self.acc.items() if t is not None}

    @staticmethod
    def fill(descs, rows):
        for d, (t, k, mode) in zip(descs, rows):
            d.data, d.k, d.mode = t.data_ptr(), k, mode

    def apply(self, desc_type, max_tensors, call):
        # `call(n, descriptors)`: the step's dgr_*_apply, once per 24 rows of the table (one launch in all for 3DGS's model)
        for i in range(0, len(self.table), max_tensors):
            part = self.table[i:i + max_tensors]
            descs = (desc_type * len(part))()
            self.fill(descs, part)
            call(len(part), descs)


class _ResizeStep(_ModelTable):
    """What the two steps that change P (`densify_and_prune`, `seed_from_frame`) add: the refusal to be recorded, the plan call with
    the one host read, a row (src, dst, k, mode, value) whose `dst` is a new tensor of the new length read from a contiguous
    `src`, and the hand-over to the optimiser."""
    as_input = staticmethod(torch.Tensor.contiguous)

    def refuse_capture(self, abi):
        if abi.capturing():
            raise RuntimeError(f"{self.who} changes the number of Gaussians and reads the new count on the host: it cannot be "
                               "recorded into a hipGraph (call it between replays)")

    def plan(self, nbytes, call, counts_type):  # `call(plan pointer, counts pointer)`: the step's dgr_*_plan
        self.plan_buffer = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        counts_dev = torch.empty(8, dtype=torch.int32, device=self.dev)
        call(self.plan_buffer.data_ptr(), counts_dev.data_ptr())
        counts = counts_type(*counts_dev.tolist()[:5])  # the call's one host synchronisation
        self.P_new = counts.rows
        return counts

    def add(self, src, tail, k, mode, value=None):
        # one row of the table: a new [P_new, *tail] tensor (k per row) filled from `src` (or None) as `mode` (and `value`) say
        dst = torch.empty((self.P_new,) + tail, dtype=torch.float32, device=self.dev)
        self.table.append((src, dst, k, mode, value))
        return dst

    def carry_empty(self, t, tail):  # ... of the new length
        return torch.empty((self.P_new,) + tail, dtype=torch.float32, device=self.dev)

    def check_moments(self, name, t, state):
        return state[0].contiguous(), state[1].contiguous()

    @staticmethod
    def fill(descs, rows):
        for d, (s, t, k, mode, value) in zip(descs, rows):
            d.src, d.dst, d.k, d.mode = _capi.ptr(s), t.data_ptr(), k, mode
            if value is not None:
                d.value = value

    def finish(self):  # the new leaves, `requires_grad` as the old ones', and the optimiser pointed at them
        params, out = self.params, self.out
        for name, t in params.items():
            out[name].requires_grad_(t.requires_grad)
        if self.optimizer is not None:
            self.optimizer.replace_params({params[name]: out[name] for name in params},
                                          {params[name]: self.moments[name] for name in self.moments})
        return out


@torch.no_grad()
def densify_and_prune(params, optimizer, xyz_gradient_accum, denom, max_radii2D, *, grad_threshold, extent,
                      percent_dense=0.01, min_opacity=0.005, max_screen_size=None, noise=None, seed=0, roles=None):
    """3DGS's densify_and_prune (clone, split into two, prune) over the whole model, fused (include/dgr_hip.h:
    dgr_densify_plan / dgr_densify_apply; the semantics are stated there).

    `params`: dict name -> leaf [P, ...]; `roles` says which names are the xyz [P,3], scaling [P,3] (log of scale), rotation
    [P,4] (r, x, y, z) and opacity [P] or [P,1] (logit) leaves, default {"xyz": "xyz", ...}; every other entry is copied
    row-wise.  `optimizer`: a SparseAdam over those leaves (or None): surviving rows keep their moments, new rows start
    from zero, the step count stays, and the optimiser is pointed at the new leaves (`replace_params`).  The accumulators
    are float32 tensors of P elements; `max_radii2D` may be None.  `noise`: [P, 2, 3] standard normals for the two children
    of each ORIGINAL row, or None for the kernel's own generator keyed by `seed`.

    Returns (new params dict, xyz_gradient_accum, denom, max_radii2D, DensifyCounts): leaves with `requires_grad`
    preserved, the three accumulators as zeros of the new length.  One host synchronisation (the read of the counts), so
    the call cannot be recorded into a hipGraph."""
    step = _ResizeStep("densify_and_prune", params, optimizer, roles, DEFAULT_ROLES)
    roles, P = step.roles, step.locate()
    with _capi.StepCalls(step.dev) as abi:
        step.refuse_capture(abi)
        src = step.check_leaves()
        if src[roles["opacity"]].numel() != P:
            raise RuntimeError("densify_and_prune: the opacity leaf must be [P] or [P, 1]")
        acc = step.check_accumulators(xyz_gradient_accum, denom, max_radii2D, required=("xyz_gradient_accum", "denom"))
        if noise is not None:
            if tuple(noise.shape) != (P, 2, 3):
                raise RuntimeError("densify_and_prune: noise must be [P, 2, 3]")
            noise = _rows_tensor(noise, P, "noise", "densify_and_prune").contiguous()
        thresholds = densify_thresholds(grad_threshold, extent, percent_dense, min_opacity, max_screen_size)

        scaling, rotation = src[roles["scaling"]], src[roles["rotation"]]
        counts = step.plan(abi.lib.dgr_densify_plan_bytes(P), lambda plan, counts_dev: abi.call(
            "dgr_densify_plan", P, _capi.ptr(acc["xyz_gradient_accum"]), _capi.ptr(acc["denom"]), _capi.ptr(acc["max_radii2D"]),
            _capi.ptr(src[roles["opacity"]]), _capi.ptr(scaling), *thresholds, plan, counts_dev), DensifyCounts)

        mode_of = {roles["xyz"]: _capi.DENSIFY_XYZ, roles["scaling"]: _capi.DENSIFY_LOG_SCALE}
        step.add_leaves(lambda name: (mode_of.get(name, _capi.DENSIFY_COPY),), (_capi.DENSIFY_ZERO_NEW,))
        zeroed = [step.add(None, tuple(t.shape[1:]) if t is not None else (), 1, _capi.DENSIFY_ZERO) for t in acc.values()]
        step.apply(_capi.DensifyTensor, _capi.DENSIFY_MAX_TENSORS, lambda n, descs: abi.call(
            "dgr_densify_apply", P, counts.rows, step.plan_buffer.data_ptr(), n, descs, _capi.ptr(scaling), _capi.ptr(rotation), _capi.ptr(noise),
            ctypes.c_ulonglong(int(seed) & (2 ** 64 - 1))))
    return step.finish(), zeroed[0], zeroed[1], zeroed[2], counts


SeedCounts = collections.namedtuple("SeedCounts", "rows new valid unseen infront")
SEED_ROLES = dict(DEFAULT_ROLES, f_dc="f_dc")


def seed_constants(fx, fy, *, silhouette_threshold=0.5, depth_error_min=float("inf"), depth_range=(0.0, float("inf")), stride=1,
                   init_opacity=0.5, scale_factor=1.0):
    """The host values of `dgr_seed_plan` / `dgr_seed_apply`, formed in float64 (ctypes rounds each once to fp32): (depth_min,
    depth_max, silhouette_threshold, depth_error_min, pix, opacity_raw) with pix = scale_factor * stride * 0.5 * (1 / fx +
    1 / fy) and opacity_raw = logit(init_opacity)."""
    inf = float("inf")
    logit = -inf if init_opacity <= 0 else inf if init_opacity >= 1 else math.log(init_opacity / (1.0 - init_opacity))
    return (float(depth_range[0]), float(depth_range[1]), float(silhouette_threshold), float(depth_error_min),
            float(scale_factor) * stride * 0.5 * (1.0 / fx + 1.0 / fy), logit)


def _image(t, shape, what):
    """a float32 GPU image with `shape`'s elements whose trailing dimensions are `shape`'s (leading ones of size 1 allowed)"""
    lead = t.dim() - len(shape) if t is not None else 0
    if (t is None or not t.is_cuda or t.dtype != torch.float32 or lead < 0 or tuple(t.shape[lead:]) != tuple(shape) or
            t.numel() != math.prod(shape)):
        raise RuntimeError(f"seed_from_frame: {what} must be a float32 GPU tensor of shape {list(shape)}")
    return t.detach().contiguous()


@torch.no_grad()
def seed_from_frame(params, optimizer, color_obs, depth_obs, viewmatrix, fx, fy, cx, cy, *, opacity_map=None, depth=None,
                    silhouette_threshold=0.5, depth_error_min=float("inf"), depth_range=(0.0, float("inf")), stride=1,
                    init_opacity=0.5, scale_factor=1.0, fill=None, roles=None, xyz_gradient_accum=None, denom=None,
                    max_radii2D=None):
    """Map expansion from an RGB-D keyframe, fused (include/dgr_hip.h: dgr_seed_plan / dgr_seed_apply; the semantics are stated
    there): one new Gaussian per candidate pixel (every `stride`-th of every `stride`-th row) whose `depth_obs` lies inside
    `depth_range` (exclusive) and which the map does not explain -- `opacity_map` (the forward's silhouette) below
    `silhouette_threshold`, or the rendered `depth` more than `depth_error_min` behind the observed one; with neither image,
    every valid candidate (the first frame).  New rows follow the old ones in row-major pixel order.

    `color_obs` [3, H, W], `depth_obs` [H, W], `opacity_map` / `depth` [H, W] or [1, H, W]: float32 on the GPU.  `viewmatrix`:
    16 floats on the GPU holding W2C^T (what the rasterizer takes, what `slam.pose_to_camera` returns): the pose never visits
    the host.  `fx, fy, cx, cy`: pixels; a point on the optical axis lands on pixel (cx, cy).  `depth_error_min`: a float, or a
    one-element float32 GPU tensor (a caller's k * median(error), no host read: `stats.median * 50` of
    `slam.masked_l1_loss(..., return_stats=True)` on this frame is one).
    `params`: dict name -> leaf [P, ...] (P = 0: empty leaves); `roles` as densify_and_prune's plus "f_dc" (the degree-0 SH
    coefficients, [P, 3] or [P, 1, 3]; may be absent from `params`).  A new row is: xyz the pixel unprojected to the world;
    scaling log(depth * scale_factor * stride * (1 / fx + 1 / fy) / 2) in all three components; rotation (1, 0, 0, 0); opacity
    logit(init_opacity); f_dc (rgb - 0.5) / C0; every other leaf `fill.get(name, 0.0)`.  `optimizer`: a SparseAdam over the leaves
    (or None): old rows keep their moments, new rows start from zero, the step count stays (`replace_params`).  The accumulators
    that are given keep their old rows and get zeros for the new ones.

    Returns (params, xyz_gradient_accum, denom, max_radii2D, SeedCounts(rows, new, valid, unseen, infront)), `requires_grad`
    preserved on every leaf.  When no pixel is selected the inputs are returned as they are and the optimiser is untouched.  One
    host synchronisation (the read of the counts), so the call cannot be recorded into a hipGraph."""
    step = _ResizeStep("seed_from_frame", params, optimizer, roles, SEED_ROLES)
    roles = step.roles
    fill = dict(fill or {})
    unknown = [name for name in fill if name not in params or name in roles.values()]
    if unknown:
        raise KeyError(f"seed_from_frame: fill names {unknown}, which are not leaves without a role")
    P = step.locate()
    if int(stride) != stride or stride < 1:
        raise ValueError("seed_from_frame: stride must be an integer >= 1")
    stride = int(stride)
    with _capi.StepCalls(step.dev) as abi:
        step.refuse_capture(abi)
        if depth_obs.dim() < 2:
            raise RuntimeError("seed_from_frame: depth_obs must be [H, W]")
        H, W = depth_obs.shape[-2:]
        depth_obs = _image(depth_obs, (H, W), "depth_obs")
        opacity_map = None if opacity_map is None else _image(opacity_map, (H, W), "opacity_map")
        depth = None if depth is None else _image(depth, (H, W), "depth")
        has_dc = roles["f_dc"] in params
        if has_dc or color_obs is not None:
            color_obs = _image(color_obs, (3, H, W), "color_obs")
        if not viewmatrix.is_cuda or viewmatrix.dtype != torch.float32 or viewmatrix.numel() != 16:
            raise RuntimeError("seed_from_frame: viewmatrix must hold 16 float32 values on the GPU (W2C^T)")
        viewmatrix = viewmatrix.detach().contiguous()
        error_dev = None
        if isinstance(depth_error_min, torch.Tensor):
            if not depth_error_min.is_cuda or depth_error_min.dtype != torch.float32 or depth_error_min.numel() != 1:
                raise RuntimeError("seed_from_frame: a tensor depth_error_min must be one float32 value on the GPU")
            error_dev, depth_error_min = depth_error_min.detach().contiguous(), float("inf")
        plan_bytes = abi.lib.dgr_seed_plan_bytes(W, H, stride)
        if plan_bytes == 0:
            raise RuntimeError(f"seed_from_frame: a {W} x {H} frame at stride {stride} is refused (dgr_seed_plan_bytes)")
        src = step.check_leaves()
        if math.prod(src[roles["opacity"]].shape[1:]) != 1:
            raise RuntimeError("seed_from_frame: the opacity leaf must be [P] or [P, 1]")
        if has_dc and math.prod(src[roles["f_dc"]].shape[1:]) != 3:
            raise RuntimeError("seed_from_frame: the f_dc leaf must be [P, 3] or [P, 1, 3]")
        step.check_accumulators(xyz_gradient_accum, denom, max_radii2D)
        depth_min, depth_max, sil, err_min, pix, opacity_raw = seed_constants(
            fx, fy, silhouette_threshold=silhouette_threshold, depth_error_min=depth_error_min, depth_range=depth_range,
            stride=stride, init_opacity=init_opacity, scale_factor=scale_factor)

        counts = step.plan(plan_bytes, lambda plan, counts_dev: abi.call(
            "dgr_seed_plan", W, H, stride, depth_obs.data_ptr(), _capi.ptr(opacity_map), _capi.ptr(depth), depth_min, depth_max, sil, err_min,
            _capi.ptr(error_dev), P, plan, counts_dev), SeedCounts)
        if counts.new == 0:
            return params, xyz_gradient_accum, denom, max_radii2D, counts

        mode_of = {roles["xyz"]: (_capi.SEED_XYZ, 0.0), roles["scaling"]: (_capi.SEED_LOG_SCALE, 0.0),
                   roles["rotation"]: (_capi.SEED_QUAT_IDENTITY, 0.0), roles["opacity"]: (_capi.SEED_CONST, opacity_raw),
                   roles["f_dc"]: (_capi.SEED_RGB_DC, 0.0)}
        step.add_leaves(lambda name: mode_of.get(name) or (_capi.SEED_CONST, float(fill.get(name, 0.0))),
                        (_capi.SEED_CONST, 0.0))
        grown = step.add_accumulators(_capi.SEED_CONST, 0.0)
        step.apply(_capi.SeedTensor, _capi.SEED_MAX_TENSORS, lambda n, descs: abi.call(
            "dgr_seed_apply", W, H, stride, P, counts.rows, step.plan_buffer.data_ptr(), n, descs, _capi.ptr(color_obs), depth_obs.data_ptr(),
            viewmatrix.data_ptr(), fx, fy, cx, cy, pix))
    return step.finish(), grown.get("xyz_gradient_accum"), grown.get("denom"), grown.get("max_radii2D"), counts


RelocateResult = collections.namedtuple("RelocateResult", "counts source")


def _device_scalar(value, dtype, what, who):
    """(host value, device pointer or None) of an argument that is a Python number or a 1-element `dtype` GPU tensor the kernels read"""
    if isinstance(value, torch.Tensor):
        if not value.is_cuda or value.dtype != dtype or value.numel() != 1:
            raise RuntimeError(f"{who}: a tensor {what} must be one {str(dtype).replace('torch.', '')} value on the GPU")
        return 0, value.data_ptr()
    return value, None


@torch.no_grad()
def relocate_dead(params, optimizer, *, min_opacity=0.005, draws=None, seed=0, step=0, xyz_gradient_accum=None, denom=None,
                  max_radii2D=None, roles=None):
    """3DGS-MCMC's relocation for a map of fixed size, fused and in place (include/dgr_hip.h: dgr_relocate_plan /
    dgr_relocate_apply; the semantics are stated there): every dead Gaussian (opacity below `min_opacity`) is moved onto a live one
    drawn with probability proportional to its opacity, and the opacity and scale of all N copies of a drawn Gaussian are
    recomputed, in float64, so that the rendered result is unchanged.

    `params`, `roles`, the accumulators: as densify_and_prune's (opacity [P] or [P, 1]); every leaf, moment and accumulator must
    be contiguous, because all are rewritten in place: they stay the same tensor objects, P does not change and the optimiser is
    not re-pointed.  `optimizer`: a SparseAdam over the leaves (or None).  Both Adam moments of every leaf are set to 0 at the
    relocated rows AND at the sources they hit -- the project's choice: a stale moment belongs neither to the old place nor to the
    new shape; the accumulators that are given are set to 0 at the relocated rows only.  Every other row keeps its bits.
    `draws`: int64 [P] with one value in [0, 2^32) per row (read at the dead rows), or None for the kernel's Philox generator
    keyed by `seed` with the counter (row, step).  `step`: an int, or a 1-element int32 GPU tensor that the kernels read, so that
    every replay of a recorded graph draws fresh numbers.

    Returns RelocateResult(counts, source), both device tensors: counts int32 [8] = {dead, live, relocated, sources hit, largest
    hits, 0, 0, 0}, source int32 [P] the source row of a relocated row and -1 elsewhere.  No host read and no allocation that
    outlives the call: it can be recorded into a hipGraph, or run between the replays of one without re-recording."""
    who = "relocate_dead"
    work = _ModelTable(who, params, optimizer, roles, DEFAULT_ROLES)
    roles, P = work.roles, work.locate()
    with _capi.StepCalls(work.dev) as abi:
        leaves = work.check_leaves()
        for name, t in leaves.items():
            _in_place(t, f"params[{name!r}]", who)
        opacity, scaling = leaves[roles["opacity"]], leaves[roles["scaling"]]
        if opacity.numel() != P:
            raise RuntimeError(f"{who}: the opacity leaf must be [P] or [P, 1]")
        acc = work.check_accumulators(xyz_gradient_accum, denom, max_radii2D)
        if not 0.0 <= min_opacity < 1.0:
            raise ValueError(f"{who}: min_opacity must lie in [0, 1)")
        if draws is not None and (not draws.is_cuda or draws.dtype != torch.int64 or tuple(draws.shape) != (P,) or
                                  not draws.is_contiguous()):
            raise RuntimeError(f"{who}: draws must be a contiguous int64 GPU tensor [P] of values in [0, 2^32)")
        step, step_dev = _device_scalar(step, torch.int32, "step", who)
        mode_of = {roles["opacity"]: _capi.RELOCATE_OPACITY, roles["scaling"]: _capi.RELOCATE_LOG_SCALE}
        work.add_leaves(lambda name: (mode_of.get(name, _capi.RELOCATE_COPY),), (_capi.RELOCATE_ZERO_TOUCHED,))
        [_in_place(t, name, who) for name, t in acc.items() if t is not None]
        work.add_accumulators(_capi.RELOCATE_ZERO_RELOCATED)

        scratch = torch.empty(abi.lib.dgr_relocate_scratch_bytes(P), dtype=torch.uint8, device=work.dev)
        counts = torch.empty(8, dtype=torch.int32, device=work.dev)
        source = torch.empty(P, dtype=torch.int32, device=work.dev)
        abi.call("dgr_relocate_plan", P, _capi.ptr(opacity), densify_thresholds(0.0, 1.0, min_opacity=min_opacity)[1],
                 _capi.ptr(draws), ctypes.c_ulonglong(int(seed) & (2 ** 64 - 1)), int(step), step_dev, scratch.data_ptr(),
                 counts.data_ptr(), _capi.ptr(source))
        if P:
            work.apply(_capi.RelocateTensor, _capi.RELOCATE_MAX_TENSORS, lambda n, descs: abi.call(
                "dgr_relocate_apply", P, scratch.data_ptr(), n, descs, scaling.data_ptr(), opacity.data_ptr(), float(min_opacity)))
    return RelocateResult(counts, source)


@torch.no_grad()
def inject_position_noise(params, lr, *, noise_scale=5e5, gate_k=100.0, gate_x0=0.995, noise=None, seed=0, step=0, roles=None):
    """3DGS-MCMC's SGLD position noise in one launch, fp32, in place (include/dgr_hip.h: dgr_position_noise): xyz += g Sigma n
    with Sigma = R S^2 R^T of each Gaussian and g = noise_scale * lr / (1 + exp(-gate_k (1 - opacity - gate_x0))): only the
    near-transparent Gaussians move.  `lr`: the position learning rate, a float or a 1-element float32 GPU tensor.  `noise`: [P, 3]
    standard normals, or None for Philox normals keyed by `seed` with the counter (row, step); `step` as relocate_dead's.  The xyz
    leaf must be contiguous; it stays the same tensor.  No host read: capturable."""
    who = "inject_position_noise"
    work = _ModelTable(who, params, None, roles, DEFAULT_ROLES)
    roles, P = work.roles, work.locate()
    with _capi.StepCalls(work.dev) as abi:
        leaves = work.check_leaves()
        if leaves[roles["opacity"]].numel() != P:
            raise RuntimeError(f"{who}: the opacity leaf must be [P] or [P, 1]")
        xyz = _in_place(leaves[roles["xyz"]], f"params[{roles['xyz']!r}]", who)
        if noise is not None:
            if tuple(noise.shape) != (P, 3):
                raise RuntimeError(f"{who}: noise must be [P, 3]")
            noise = _rows_tensor(noise, P, "noise", who).contiguous()
        step, step_dev = _device_scalar(step, torch.int32, "step", who)
        lr, lr_dev = _device_scalar(lr, torch.float32, "lr", who)
        scaling, rotation, opacity = (leaves[roles[r]].contiguous() for r in ("scaling", "rotation", "opacity"))  # (only read)
        abi.call("dgr_position_noise", P, _capi.ptr(xyz), _capi.ptr(scaling), _capi.ptr(rotation), _capi.ptr(opacity), _capi.ptr(noise),
                 ctypes.c_ulonglong(int(seed) & (2 ** 64 - 1)), int(step), step_dev, float(lr), lr_dev, float(noise_scale),
                 float(gate_k), float(gate_x0))


TRANSFORM_ROLES = dict(DEFAULT_ROLES, f_rest="f_rest", shs="shs")
TransformCounts = collections.namedtuple("TransformCounts", "transformed unanchored invalid_transforms anchored_invalid")


class _TransformTable(_ModelTable):
    """The table of `transform_map`: a row is (tensor, k, mode, skip), and only the leaves the transform changes have one."""

    def add(self, t, tail, k, mode, skip=0):
        self.table.append((t, k, mode, skip))
        return t

    @staticmethod
    def fill(descs, rows):
        for d, (t, k, mode, skip) in zip(descs, rows):
            d.data, d.k, d.mode, d.skip = t.data_ptr(), k, mode, skip


@torch.no_grad()
def pose_corrections(old_viewmatrices, new_viewmatrices):
    """The transforms `transform_map` takes, from the keyframes' poses before and after a pose-graph update: both arguments are
    stacks [K, 4, 4] (or [K, 16]) of the rasterizer's viewmatrix W2C^T on the GPU; the result is T_k = C2W_new,k W2C_old,k as
    float32 [K, 4, 4], row-major, old world -> new world: a Gaussian fixed in keyframe k's camera frame stays fixed in it.  Formed in
    float64 torch ops on the device (W2C = [s R | t] is inverted in closed form, so a Sim(3) pose is taken as well as a rigid one);
    no host read."""
    old, new = (m.detach().reshape(-1, 4, 4).transpose(-1, -2).to(torch.float64) for m in (old_viewmatrices, new_viewmatrices))
    if old.shape != new.shape or not old.is_cuda or not new.is_cuda:
        raise RuntimeError("pose_corrections: two stacks of the same number of 4 x 4 viewmatrices on the GPU")
    A, t = new[:, :3, :3], new[:, :3, 3:]
    A_inv = A.transpose(-1, -2) / ((A * A).sum(dim=(1, 2), keepdim=True) / 3.0)  # (s R)^-1 = R^T / s
    c2w = torch.zeros_like(new)
    c2w[:, :3, :3], c2w[:, :3, 3:], c2w[:, 3, 3] = A_inv, -(A_inv @ t), 1.0
    return (c2w @ old).to(torch.float32).contiguous()


@torch.no_grad()
def transform_map(params, optimizer, transforms, *, anchor="anchor", moments="rotate", roles=None):
    """The map correction after a pose-graph update (loop closure, global bundle adjustment), fused and in place (include/dgr_hip.h:
    dgr_transform_plan / dgr_transform_apply; the semantics are stated there): row i of every leaf is moved by transforms[anchor[i]].

    `transforms`: float32 [K, 4, 4] on the GPU, row-major Sim(3) matrices old world -> new world (`pose_corrections` makes them);
    they are read by the kernels, so a recorded call follows a rewritten tensor.  `anchor`: the name of a leaf of `params` ([P] or
    [P, 1], what `seed_from_frame(fill={"anchor": k})` wrote and densify_and_prune / relocate_dead copied), a float32 [P] tensor, or
    None for one global transform (transforms[0]).  A row whose anchor is not an integer in 0 .. K - 1, or whose transform is not a
    similarity (not finite, det <= 0, A^T A / s^2 off the identity by more than 1e-3), keeps its bits.
    `roles` as relocate_dead's, plus "f_rest" ([P, M, 3], M = 0, 3, 8 or 15) and "shs" ([P, M + 1, 3], the DC row stays); either may
    be absent.  xyz -> A x + t, rotation -> q_R (x) q, scaling -> + log s, the SH bands by their rotation matrices; opacity, f_dc
    and every other leaf are invariant.  `moments`: "rotate" takes the Adam moments of those leaves along (exp_avg as a covector,
    exp_avg_sq by the squared matrices: the diagonal of the rotated second moment, the project's choice), "keep" leaves the
    optimiser's state alone.  Everything is rewritten in place: leaves and moments must be contiguous and stay the same tensor
    objects, P does not change, the optimiser is not re-pointed.

    Returns the counts as an int32 [4] device tensor (`TransformCounts` names the fields): rows transformed, rows whose anchor names
    no transform, invalid transforms, rows anchored to an invalid transform.  No host read: it can be recorded into a hipGraph."""
    who = "transform_map"
    if moments not in ("rotate", "keep"):
        raise ValueError(f"{who}: moments must be 'rotate' or 'keep'")
    work = _TransformTable(who, params, optimizer if moments == "rotate" else None, roles, TRANSFORM_ROLES)
    roles, P = work.roles, work.locate()
    with _capi.StepCalls(work.dev) as abi:
        leaves = work.check_leaves()
        if (not isinstance(transforms, torch.Tensor) or not transforms.is_cuda or transforms.dtype != torch.float32 or
                transforms.dim() != 3 or tuple(transforms.shape[1:]) != (4, 4) or not transforms.is_contiguous() or
                transforms.device != work.dev):
            raise RuntimeError(f"{who}: transforms must be a contiguous float32 GPU tensor [K, 4, 4] on the leaves' device")
        K = transforms.shape[0]
        if isinstance(anchor, str):
            if anchor not in params:
                raise KeyError(f"{who}: params has no anchor leaf {anchor!r} (pass a tensor, or None for one global transform)")
            if anchor in (roles[r] for r in roles):
                raise KeyError(f"{who}: the anchor leaf {anchor!r} has a role")
            anchor_t = leaves[anchor]
        else:
            anchor_t = None if anchor is None else _rows_tensor(anchor, P, "anchor", who)
        if anchor_t is not None and (anchor_t.numel() != P or not anchor_t.is_contiguous() or anchor_t.device != work.dev):
            raise RuntimeError(f"{who}: the anchor must be a contiguous float32 [P] or [P, 1] tensor on the leaves' device")
        kind_of = {roles["xyz"]: _capi.TRANSFORM_XYZ, roles["rotation"]: _capi.TRANSFORM_QUAT,
                   roles["scaling"]: _capi.TRANSFORM_LOG_SCALE}
        state_of = work.optimizer.state if work.optimizer is not None else {}
        for name, t in leaves.items():
            kind, skip = kind_of.get(name), 0
            if name in (roles["f_rest"], roles["shs"]):
                skip = 3 if name == roles["shs"] else 0
                if t.dim() != 3 or t.shape[2] != 3 or t.shape[1] - skip // 3 not in (0, 3, 8, 15):
                    raise RuntimeError(f"{who}: params[{name!r}] must be [P, M{' + 1' if skip else ''}, 3] with M = 0, 3, 8 or 15 "
                                       "(the complete bands of degree 1 .. 3)")
                kind = _capi.TRANSFORM_SH if t.shape[1] - skip // 3 else None  # nothing above the DC row: nothing rotates
            if kind is None:
                continue
            tail = tuple(t.shape[1:])
            k = math.prod(tail)
            work.add(_in_place(t, f"params[{name!r}]", who), tail, k, kind + _capi.TRANSFORM_VALUE, skip)
            state = state_of.get(params[name])
            if state is not None and kind != _capi.TRANSFORM_LOG_SCALE:
                m1, m2 = work.check_moments(name, t, state)
                work.add(m1, tail, k, kind + _capi.TRANSFORM_MOMENT1, skip)
                work.add(m2, tail, k, kind + _capi.TRANSFORM_MOMENT2, skip)

        nbytes = abi.lib.dgr_transform_scratch_bytes(K)
        if nbytes == 0:
            raise RuntimeError(f"{who}: {K} transforms are refused (1 .. 2^20)")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=work.dev)
        counts = torch.empty(4, dtype=torch.int32, device=work.dev)
        abi.call("dgr_transform_plan", K, transforms.data_ptr(), scratch.data_ptr(), counts.data_ptr())
        work.apply(_capi.TransformTensor, _capi.TRANSFORM_MAX_TENSORS, lambda n, descs: abi.call(
            "dgr_transform_apply", P, K, scratch.data_ptr(), _capi.ptr(anchor_t), n, descs, counts.data_ptr()))
    return counts
