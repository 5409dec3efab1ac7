"""Fused sparse Adam for the Gaussian parameters.

`torch.optim.Adam` semantics (no weight decay, no amsgrad) with one HIP launch per tensor through the C ABI
(`dgr_sparse_adam`, csrc/optim.hip).  `step(visible=radii)` updates only the Gaussians some view saw -- parameter and
both moments of the other rows are left untouched, as in 3DGS's sparse Adam; `step()` updates every row.

The steps that work on the whole map live in `dgr_amd.map_steps`; their public names are offered here as well.
"""
import torch

from . import _capi
from .map_steps import (DEFAULT_ROLES, SEED_ROLES, TRANSFORM_ROLES, DensifyCounts, RelocateResult, SeedCounts,  # noqa: F401
                        TransformCounts, add_densification_stats, densify_and_prune, densify_thresholds, inject_position_noise,
                        pose_corrections, relocate_dead, seed_constants, seed_from_frame, transform_map)


class SparseAdam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, capturable=False):
        """`params`: tensors [P, ...] or torch-style groups `{"params": [...], "lr": ...}`.  `capturable=True` keeps the
        step count on the device (one extra tiny launch per step) so that `step()` can be recorded into a hipGraph."""
        groups = list(params)
        if groups and isinstance(groups[0], torch.Tensor):
            groups = [{"params": groups}]
        self.param_groups = []
        for g in groups:
            g = dict(g)
            g.setdefault("lr", lr)
            g.setdefault("betas", betas)
            g.setdefault("eps", eps)
            g["params"] = list(g["params"])
            self.param_groups.append(g)
        self.state = {}
        self.steps = 0
        self.capturable = bool(capturable)
        self._step_dev = None

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    @torch.no_grad()
    def step(self, visible=None):
        """visible: a bool or integer tensor with one entry per row on the parameters' device (e.g. the forward's radii; a row is
        updated where > 0; any integer dtype is converted to int32) or None for every row.  Everything is checked on the host
        before the library is loaded: a refused call leaves `steps`, the device step count and `state` as they were.  The launches
        go to the parameters' device and its current stream, whichever device is current."""
        if visible is not None and (not isinstance(visible, torch.Tensor) or visible.is_floating_point() or visible.is_complex()):
            raise RuntimeError("SparseAdam: `visible` must be a bool or integer tensor (e.g. the forward's radii)")
        live = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if visible is not None and any(visible.numel() != p.shape[0] for p in live if p.dim() >= 1):
            raise RuntimeError("SparseAdam: `visible` must have one entry per row")
        for p in live:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.dim() < 1:
                raise RuntimeError("SparseAdam: parameters must be contiguous float32 tensors on the GPU")
            if p.grad.dtype != torch.float32 or p.grad.device != p.device or p.grad.shape != p.shape:
                raise RuntimeError("SparseAdam: a gradient must be a float32 tensor of its parameter's shape and device")
        if visible is not None and any(visible.device != p.device for p in live):
            raise RuntimeError(f"SparseAdam: `visible` is on {visible.device}, not on the parameters' device")
        dev = next(p.device for g in self.param_groups for p in g["params"])
        fresh = (self.capturable and self._step_dev is None) or any(p not in self.state for p in live)
        if fresh and dev.type == "cuda":
            with _capi.on_device(dev):  # (the question is for the parameters' device)
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("SparseAdam: this step() would create the moments or the device step count while a hipGraph "
                                       "is being recorded, and every replay would reset them: take one eager step first, then capture")
        with _capi.StepCalls(dev) as abi:  # (one guard and one stream lookup for all the tensors)
            self.steps += 1
            if self.capturable:
                if self._step_dev is None:
                    self._step_dev = torch.full((1,), self.steps - 1, dtype=torch.int32, device=dev)
                self._step_dev.add_(1)
            if visible is not None:
                if visible.dtype == torch.bool:
                    visible = visible.to(torch.int32)
                elif visible.dtype != torch.int32:  # (the sign test here: a wide value must not wrap into another sign)
                    visible = (visible > 0).to(torch.int32)
                visible = visible.contiguous()
            vis, call = None if visible is None else visible.data_ptr(), abi.call
            entry, step = ("dgr_sparse_adam_capturable", self._step_dev.data_ptr()) if self.capturable else ("dgr_sparse_adam", self.steps)
            for g in self.param_groups:
                b1, b2 = g["betas"]
                for p in g["params"]:
                    if p.grad is None:
                        continue
                    grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                    s = self.state.get(p)
                    if s is None:
                        s = self.state[p] = (torch.zeros_like(p), torch.zeros_like(p))
                    if p.numel() == 0:  # no value to update (a degree-0 model's [P, 0, 3] f_rest): the library refuses k < 1
                        continue
                    rows = p.shape[0]
                    call(entry, rows, p.numel() // max(rows, 1), p.data_ptr(), grad.data_ptr(), s[0].data_ptr(), s[1].data_ptr(),
                         vis, float(g["lr"]), float(b1), float(b2), float(g["eps"]), step)

    def replace_params(self, old_to_new, moments=None):
        """Points the optimiser at new leaves after the number of rows changed (`densify_and_prune`): `old_to_new` maps each
        replaced parameter to its successor, `moments` an old parameter to the successor's (exp_avg, exp_avg_sq).  A
        parameter without moments gets no state (its first step creates it, zeros).  `steps` and the device step count of
        the capturable form are kept: new rows meet the current bias correction, as 3DGS's do."""
        moments = moments or {}
        for g in self.param_groups:
            g["params"] = [old_to_new.get(p, p) for p in g["params"]]
        for old, new in old_to_new.items():
            self.state.pop(old, None)
            if old in moments:
                m, v = moments[old]
                if m.shape != new.shape or v.shape != new.shape:
                    raise RuntimeError("SparseAdam.replace_params: the moments must have the new parameter's shape")
                self.state[new] = (m, v)
