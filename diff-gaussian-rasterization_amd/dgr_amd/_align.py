"""What the three pose aligners share above the C ABI (icp.py, rgbd.py, gicp.py; csrc/gn_step.h is the same tail below it): the
checks of their numbers and [4,4] poses, the scratch of a fused step, and the device buffers of a chain of steps."""
import torch

from . import _capi

INF = float("inf")


def _number(what, name, v, lowest=None):
    """`v` as a float: not NaN, not below `lowest` where one is given"""
    v = float(v)
    if v != v:
        raise ValueError(f"{what}: {name} must not be NaN")
    if lowest is not None and v < lowest:
        raise ValueError(f"{what}: {name} must not be {'negative' if lowest == 0.0 else f'below {lowest}'}, not {v}")
    return v


def _scalars(what, fx, fy, **named):
    """floats, none of them NaN, fx and fy finite and positive, every name of `named` given as (value, lowest allowed or None)"""
    out = {n: _number(what, n, v) for n, v in dict(fx=fx, fy=fy, **{n: v[0] for n, v in named.items()}).items()}
    for n in ("fx", "fy"):
        if not 0.0 < out[n] < INF:
            raise ValueError(f"{what}: {n} must be finite and positive, not {out[n]}")
    for n, (_, lowest) in named.items():
        _number(what, n, out[n], lowest)
    return out


def _pose(what, name, t, layout="W2C^T"):
    """a float32 [4,4] tensor; `layout`: what the message says the sixteen numbers hold"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, not {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, not {t.dtype}")
    if tuple(t.shape) != (4, 4):
        raise ValueError(f"{what}: {name} is [4,4] ({layout}), not {tuple(t.shape)}")
    return t


def _step_scratch(alloc, what, size_symbol, W, H, strides, dev):
    """one zero-filled scratch that serves every stride of `strides` (the ticket at its start is left at zero by every step).
    `alloc`: the calling module's `torch`, here and in _Chain (its tests stand a guard-banded allocator in for that name)"""
    size_of = getattr(_capi.load(), size_symbol)
    sizes = [size_of(W, H, s) for s in sorted(set(strides))]
    if not all(sizes):
        raise ValueError(f"{what}: cannot take a {W} x {H} frame at strides {sorted(set(strides))} (below 2^30 candidates)")
    return alloc.zeros((max(sizes),), dtype=torch.uint8, device=dev)


class _Chain:
    """The device buffers a chain of `iterations` fused steps runs through: `pose` [4,4], every step's output and, in an align
    call, its input too (seeded from `first`); `qt` (quat, trans) and the optional `flags` [n] / `idx` [n], stored by the last step
    only; `stats` [iterations, width], a row per step.  A single step is the chain of one whose pose is the caller's `out`
    (`out_name` in the message) or a new tensor.  `idx`: False where the step's ABI has no such argument, else a length or None."""

    def __init__(self, alloc, what, dev, iterations, width, *, first=None, out=None, out_name=None, flags=None, idx=False):
        self.pose = alloc.empty((4, 4), dtype=torch.float32, device=dev) if out is None else out
        p = self.pose
        if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32 and tuple(p.shape) == (4, 4) and p.is_contiguous()):
            raise ValueError(f"{what}: {out_name} must be a contiguous float32 GPU tensor [4,4]")
        if first is not None:
            self.pose.copy_(first.detach())
        self.qt = alloc.empty((8,), dtype=torch.float32, device=dev)
        self.stats = alloc.empty((iterations, width), dtype=torch.float64, device=dev)
        self.flags = None if flags is None else alloc.empty((flags,), dtype=torch.uint8, device=dev)
        self.has_idx = idx is not False
        self.idx = alloc.empty((idx,), dtype=torch.int32, device=dev) if idx else None

    def tail(self, k):
        """the trailing arguments of step `k`: pose out, quat, trans, stats[k], (idx,) flags -- all but the first and stats[k]
        NULL before the last step"""
        last = k == self.stats.shape[0] - 1
        at_last = [_capi.ptr(t) if last else None for t in (self.qt, self.qt[4:]) + ((self.idx,) if self.has_idx else ()) + (self.flags,)]
        return [self.pose.data_ptr(), *at_last[:2], self.stats[k].data_ptr(), *at_last[2:]]

    def result(self, cls):
        return cls(self.pose, self.qt[:4], self.qt[4:7], self.stats, *((self.idx,) if self.has_idx else ()), self.flags)
