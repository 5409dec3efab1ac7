"""What the GPU tests of the four map steps (tests/test_hip_{densify,seed,relocate,transform}.py) share: the extra leaves and the
generators of leaves and moments, the upload with an optimiser in a known state, and the two checks of what
dgr_amd/map_steps.py's one call path promises about the leaves and the optimiser -- a step that rewrites the rows in place
(relocation, map correction) and a step that returns new tensors (densify-and-prune, map expansion).  Every generator draws in the
order its callers always drew in: the inputs of a case are a function of its seed alone."""
import numpy as np
import torch

import hip_helpers as hh
from dgr_amd.optim import SparseAdam
from util import bits_equal  # noqa: F401  (the map-step tests' one comparison: shape, float32 and bits)

# further per-row tensors with k = 3, 45, 48, 1, 4 elements per row; "label" does not require grad
EXTRAS = {"f_dc": (1, 3), "f_rest": (15, 3), "sh48": (16, 3), "label": (), "aux4": (2, 2)}
STEPS = 3  # the optimiser's step count going in, and coming out


def leaves_of(P, g, extras=EXTRAS):
    L = {"xyz": 3.0 * torch.randn((P, 3), generator=g), "scaling": 0.7 * torch.randn((P, 3), generator=g) - 2.0,
         "rotation": torch.randn((P, 4), generator=g), "opacity": 2.0 * torch.randn((P, 1), generator=g)}
    for name, shape in extras.items():
        L[name] = torch.randn((P,) + shape, generator=g)
    return L


def moments_of(L, g, names=None, floor=None):
    """a pair (exp_avg ~ N(0, 1), exp_avg_sq ~ U[0, 1) + floor) per leaf of `names` (all), drawn leaf by leaf in L's order"""
    second = (lambda t: torch.rand(t.shape, generator=g)) if floor is None else (lambda t: torch.rand(t.shape, generator=g) + floor)
    return {name: (torch.randn(t.shape, generator=g), second(t)) for name, t in L.items() if names is None or name in names}


def on_device(L, M, optimizer=True, frozen=("label",), grouped=None):
    """Uploads the CPU leaves L (torch or numpy), every one but `frozen` requiring grad, and builds a SparseAdam with one group per
    leaf of `grouped` (all, in L's order), the moments M = {name: (exp_avg, exp_avg_sq)} as its state and STEPS steps taken.
    Returns (params, optimiser or None, the moments on the device by name, the record the two checks below compare with)."""
    d = hh.dev()
    up = lambda t: (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(d)  # noqa: E731
    params = {name: up(t).requires_grad_(name not in frozen) for name, t in L.items()}
    opt, moments = None, {}
    grouped = [name for name in L if grouped is None or name in grouped]
    if optimizer:
        opt = SparseAdam([{"params": [params[name]], "lr": 1e-3} for name in grouped])
        for name, (m, v) in M.items():
            moments[name] = opt.state[params[name]] = (up(m), up(v))
        opt.steps = STEPS
    before = dict(leaves={name: (p, p.data_ptr()) for name, p in params.items()}, frozen=frozen, grouped=grouped, moments=moments)
    return params, opt, moments, before


def _assert_optimizer(before, leaves, opt):
    assert opt.steps == STEPS and len(opt.state) == len(before["moments"])
    assert len(opt.param_groups) == len(before["grouped"])
    assert all(len(g["params"]) == 1 and g["params"][0] is leaves[name] for g, name in zip(opt.param_groups, before["grouped"]))


def assert_in_place(before, params, opt):
    """after a step that rewrites rows in place: every leaf is the tensor it was, at its address, still a leaf with its
    requires_grad; the optimiser has its step count, its groups in order and, as state, the very moment tensors it was given"""
    for name, (p, address) in before["leaves"].items():
        assert params[name] is p and p.data_ptr() == address and p.is_leaf, name
        assert p.requires_grad == (name not in before["frozen"]), name
    if opt is not None:
        _assert_optimizer(before, params, opt)
        assert all(opt.state[params[name]][i] is pair[i] for name, pair in before["moments"].items() for i in (0, 1))


def assert_rebuilt(before, out, opt):
    """after a step that returns new tensors: every output is a leaf with its input's requires_grad; the optimiser has its step
    count, its groups rebound to the outputs in order and state for exactly the leaves that had moments"""
    for name, p in out.items():
        assert p.requires_grad == (name not in before["frozen"]) and p.is_leaf, name
    if opt is not None:
        _assert_optimizer(before, out, opt)
        assert all(out[name] in opt.state for name in before["moments"])
