"""A degree-0 model as 3DGS builds it, for the map-step tests: f_dc [P, 1, 3] and f_rest [P, 0, 3].  A leaf without a value per
row, and its two Adam moments, take no part in any kernel (the C ABI refuses k < 1 and a NULL tensor; tests/test_step_modules.py
shows that none leaves Python) and come back with the new number of rows.  What the GPU tests hold: every other leaf, moment,
accumulator and count carries the bits of the same call on the model without f_rest -- calls that the tests around them hold to
their float64 models -- and the optimiser goes on stepping, also from a recorded graph."""
import torch

from dgr_amd.optim import SparseAdam

NAMES = ("xyz", "f_dc", "opacity", "scaling", "rotation")


def model(L, device, with_rest):
    """`L`: leaves on the CPU, NAMES among them.  The leaves on `device` in 3DGS's order, f_rest behind f_dc if `with_rest`."""
    params = {}
    for name in NAMES:
        params[name] = L[name].to(device).requires_grad_()
        if name == "f_dc" and with_rest:
            params["f_rest"] = torch.zeros((L["xyz"].shape[0], 0, 3), device=device, requires_grad=True)
    return params


def set_grads(params):
    for p in params.values():
        p.grad = torch.sin(3.0 * p.detach())  # (a function of the value alone: the same bits in both runs)


def stepped_adam(params, capturable):
    """a SparseAdam over every leaf that has taken one step"""
    opt = SparseAdam([{"params": [p], "lr": 1e-3} for p in params.values()], capturable=capturable)
    set_grads(params)
    opt.step()
    assert all(p in opt.state for p in params.values())
    return opt


def step_again(opt, params, capturable):
    """one more step on the leaves as they are now; the capturable form also recorded into a graph and replayed twice"""
    set_grads(params)
    opt.step()
    if capturable:
        dev = params["xyz"].device
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                opt.step()
        torch.cuda.current_stream(dev).wait_stream(side)
        for _ in range(2):
            graph.replay()
    torch.cuda.synchronize()


def snapshot(params, opt, **others):
    """name -> a CPU copy of every leaf but f_rest, of its two moments and of `others`"""
    got = {}
    for name in NAMES:
        got[name] = params[name]
        got[name + ".exp_avg"], got[name + ".exp_avg_sq"] = opt.state[params[name]]
    got.update(others)
    torch.cuda.synchronize()
    return {name: t.detach().cpu().clone() if isinstance(t, torch.Tensor) else t for name, t in got.items()}


def check_rest(params, opt, rows):
    rest = params["f_rest"]
    assert tuple(rest.shape) == (rows, 0, 3) and rest.dtype == torch.float32 and rest.requires_grad and rest.is_leaf and rest.is_cuda
    assert [tuple(m.shape) for m in opt.state[rest]] == [(rows, 0, 3)] * 2
    assert list(params) == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    assert all(g["params"][0] is p for g, p in zip(opt.param_groups, params.values()))
    assert all(p.shape[0] == rows for p in params.values())


def assert_same_bits(a, b):
    assert set(a) == set(b)
    for name in a:
        if isinstance(a[name], torch.Tensor):
            assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype, name
            assert torch.equal(a[name].contiguous().view(torch.int32), b[name].contiguous().view(torch.int32)), name
        else:
            assert a[name] == b[name], name
