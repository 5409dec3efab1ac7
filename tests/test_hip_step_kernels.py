"""The fused sparse Adam, add_densification_stats (csrc/optim.hip), the pose kernels (csrc/pose.hip) and the plain L1 loss (csrc/l1_loss.hip) against
their float64 models, at the shapes that reach every grid-stride pass and on inputs that tell a subtly wrong kernel from a right
one.  Models, inputs and bars: tests/step_model.py; that they can do so: tests/test_step_model.py (no GPU needed).  Every test
prints what it measured, in units of its bars, before it asserts."""
import math

import numpy as np
import pytest
import torch

import step_model as sm

pytestmark = pytest.mark.gpu

_ids = lambda s: "x".join(map(str, s[0] if isinstance(s[0], tuple) else (s[0],) + s[1]))  # noqa: E731


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _gpu(a):
    """a device copy of a (read-only) numpy array"""
    return torch.from_numpy(np.array(a)).to(_dev())


# ================================================= Adam =================================================
def adam_step(rows, row_shape, pattern, eps, step, capturable, visible_dtype=torch.int32):
    """One SparseAdam step from the state of sm.adam_inputs -- m0 and v0 written into opt.state, the step count set -- with a NaN
    gradient in every row the step must skip.  Returns the flat float32 (p, m, v) and the arguments of sm.adam_check."""
    from dgr_amd.optim import SparseAdam
    dev, k = _dev(), math.prod(row_shape)
    inp = sm.adam_inputs(rows * k)
    hyper, visible = sm.adam_hyper(eps), sm.adam_visible(pattern, rows)
    g = inp[1].copy().reshape(rows, k)
    if visible is not None:
        g[visible <= 0, 0] = np.nan
    shape = (rows,) + tuple(row_shape)
    p, m, v = (_gpu(a).view(shape) for a in (inp[0], inp[2], inp[3]))
    p.requires_grad_()
    p.grad = _gpu(g).view(shape)
    opt = SparseAdam([p], lr=hyper[0], betas=hyper[1:3], eps=hyper[3], capturable=capturable)
    opt.state[p] = (m, v)
    opt.steps = step - 1
    if capturable:
        opt._step_dev = torch.full((1,), step - 1, dtype=torch.int32, device=dev)
    vis = None
    if visible is not None:
        vis = _gpu(visible)
        vis = vis > 0 if visible_dtype == torch.bool else vis.to(visible_dtype)
    opt.step(visible=vis)
    assert opt.steps == step and (not capturable or int(opt._step_dev) == step)
    out = tuple(_np(t).reshape(-1) for t in (p, m, v))
    return out, (inp, k, visible, hyper, step)


def check_both_forms(rows, row_shape, pattern, eps, step):
    for capturable in (False, True):
        out, args = adam_step(rows, row_shape, pattern, eps, step, capturable)
        rep = sm.adam_check(*args, *out, capturable=capturable)
        print(f"{'capturable' if capturable else 'host'} form, {rows} x {row_shape}, visible {pattern}, eps {eps}, step {step}: {rep}")
        rep.check("capturable form" if capturable else "host form")
        if pattern == "zeros":
            assert all(sm.same_bits(o, i) for o, i in zip(out, (args[0][0], args[0][2], args[0][3])))


@pytest.mark.parametrize("pattern", ["none", "ones", "zeros", "mixed"])
@pytest.mark.parametrize("shape", sm.ADAM_SHAPES, ids=_ids)
def test_adam_shapes_and_visible_patterns(shape, pattern):
    check_both_forms(*shape, pattern, 1e-15, 2)


@pytest.mark.parametrize("step", sm.ADAM_STEPS)
@pytest.mark.parametrize("eps", sm.ADAM_EPS)
def test_adam_one_step_from_a_given_state(eps, step):
    out, args = adam_step(*sm.ADAM_SHAPES[-1], "mixed", eps, step, False)
    rep = sm.adam_check(*args, *out)
    print(f"host form, eps {eps}, step {step}: {rep}")
    rep.check("host form")


@pytest.mark.parametrize("step", sm.ADAM_CAPTURABLE_STEPS)
@pytest.mark.parametrize("eps", sm.ADAM_EPS)
def test_capturable_adam_forms_its_bias_corrections_on_the_device(eps, step):
    """The parameter bar allows a device powf that is off by up to 3 ulp (sm.adam_p_factor); the host form's bar is printed
    beside it as a figure."""
    out, args = adam_step(*sm.ADAM_SHAPES[-1], "none", eps, step, True)
    rep = sm.adam_check(*args, *out, capturable=True)
    print(f"capturable form, eps {eps}, step {step}: {rep}; against the host form's bar: p {sm.adam_check(*args, *out)['p'][0]:.3g}")
    rep.check("capturable form")


@pytest.mark.parametrize("pattern", ["mod7", "none"])
def test_adam_second_grid_pass(pattern):
    """2 097 600 elements: the last 448 are updated by the second pass of the grid-stride loop only, with visible[e / k] read
    there too."""
    check_both_forms(*sm.ADAM_LARGE, pattern, 1e-15, 2)


def test_adam_visible_dtypes_agree():
    """bool, int32 and the wider or narrower integer types (converted on the way in) select the same rows: the same bits"""
    want, _ = adam_step(*sm.ADAM_SHAPES[3], "mixed", 1e-15, 2, False, torch.int32)
    for dtype in (torch.bool, torch.int64, torch.int16, torch.int8):
        got, _ = adam_step(*sm.ADAM_SHAPES[3], "mixed", 1e-15, 2, False, dtype)
        assert all(sm.same_bits(a, b) for a, b in zip(got, want)), dtype


# ---- refusals that need GPU parameters: no launch can happen, whether or not the check is in place ----
@pytest.fixture
def no_library(monkeypatch):
    from dgr_amd import _capi
    monkeypatch.setattr(_capi, "load", lambda: pytest.fail("the library was loaded before the step was refused"))


def _fresh_optimizer(capturable):
    from dgr_amd.optim import SparseAdam
    p = torch.zeros((6, 3), device=_dev(), requires_grad=True)
    p.grad = torch.ones_like(p)
    return SparseAdam([p], capturable=capturable), p


@pytest.mark.parametrize("capturable", [False, True])
def test_adam_refuses_a_cpu_visible_and_keeps_its_state(no_library, capturable):
    opt, p = _fresh_optimizer(capturable)
    for visible, match in ((torch.ones(6, dtype=torch.int32), "device"), (torch.ones(6, dtype=torch.bool), "device"),
                           (torch.ones(6, device=_dev()), "bool or integer"), (torch.ones(7, dtype=torch.int64, device=_dev()), "per row")):
        with pytest.raises(RuntimeError, match=match):
            opt.step(visible=visible)
        assert opt.steps == 0 and opt._step_dev is None and opt.state == {}
    assert float(p.detach().abs().sum()) == 0.0


@pytest.mark.parametrize("capturable", [False, True])
def test_adam_refuses_a_first_step_inside_a_capture(no_library, capturable):
    """zeros_like (the moments) and torch.full (the step count) would be recorded: every replay would reset them"""
    opt, p = _fresh_optimizer(capturable)
    dev = _dev()
    counter = torch.zeros(1, device=dev)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            counter.add_(1.0)  # (so that the recorded graph is not empty)
            with pytest.raises(RuntimeError, match="one eager step first"):
                opt.step()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert opt.steps == 0 and opt._step_dev is None and opt.state == {}


# ================================================= densification statistics =================================================
@pytest.mark.parametrize("column", [False, True], ids=["[P]", "[P,1]"])
@pytest.mark.parametrize("rows", sm.STATS_ROWS)
def test_densification_stats(rows, column):
    """Five views in a row; dmeans2D is a non-contiguous [:, :3] slice of a [P, 4] tensor; a row a view did not see keeps its three
    values bit for bit through that view, NaN gradient or not."""
    from dgr_amd.optim import add_densification_stats
    inp = sm.stats_inputs(rows)
    shape = (rows, 1) if column else (rows,)
    accum, denom, maxr = (_gpu(inp[k]).view(shape) for k in ("accum0", "denom0", "maxr0"))
    for v in range(sm.STATS_VIEWS):
        before = [_np(t).reshape(-1) for t in (accum, denom, maxr)]
        d4 = _gpu(inp["dmeans"][v])
        add_densification_stats(d4[:, :3], _gpu(inp["radii"][v]), accum, denom, maxr)
        unseen = inp["radii"][v] <= 0
        assert all(sm.same_bits(_np(t).reshape(-1)[unseen], b[unseen]) for t, b in zip((accum, denom, maxr), before)), v
    rep = sm.stats_check(inp, *(_np(t).reshape(-1) for t in (accum, denom, maxr)))
    print(f"{rows} rows: {rep}")
    rep.check("five views")


@pytest.mark.parametrize("skip", [0, 1, 2], ids=["no accum", "no denom", "no max_radii2D"])
def test_densification_stats_optional_outputs(skip):
    from dgr_amd.optim import add_densification_stats
    inp = sm.stats_inputs(257)
    outs = [_gpu(inp[k]) for k in ("accum0", "denom0", "maxr0")]
    outs[skip] = None
    for v in range(sm.STATS_VIEWS):
        add_densification_stats(_gpu(inp["dmeans"][v])[:, :3], _gpu(inp["radii"][v]), *outs)
    sm.stats_check(inp, *(None if t is None else _np(t) for t in outs)).check("optional outputs")


# ================================================= pose =================================================
def test_pose_kernels_against_the_float64_model():
    """Every case of sm.pose_cases through slam.pose_to_camera and its backward: random rotations at |q| = 1e-3, 1, 1e3, the
    identity, the 180 degree rotations, r = -1, and -q of each."""
    from dgr_amd import slam
    c = sm.pose_cases()
    qs, ts, ws = (_gpu(c[k]) for k in ("q", "t", "dview"))
    got = dict(view=[], proj=[], campos=[], dq=[], dt=[])
    for q, t, w in zip(qs, ts, ws):
        q, t = q.clone().requires_grad_(), t.clone().requires_grad_()
        view, proj, perspec, campos = slam.pose_to_camera(q, t, *sm.TANFOV)
        assert view.requires_grad and not proj.requires_grad and not campos.requires_grad
        (view * w).sum().backward()
        for k, x in (("view", view.detach()), ("proj", proj), ("campos", campos), ("dq", q.grad), ("dt", t.grad)):
            got[k].append(x)
    assert np.array_equal(_np(perspec), sm.pose_perspec())  # (the model's third input is the kernel's)
    rep = sm.pose_check({k: _np(torch.stack(v)) for k, v in got.items()})
    print(f"{len(qs)} poses: {rep}")
    rep.check("pose")


# ================================================= L1 loss =================================================
_l1_ids = lambda s: "x".join(map(str, s[0])) + "+" + "x".join(map(str, s[1]))  # noqa: E731


def _l1_tensors(inp):
    return tuple(_gpu(inp[k]) for k in ("color", "depth", "color_obs", "depth_obs"))


def l1_abi(inp, upstream, use_color=True, use_depth=True):
    """dgr_l1_loss_forward / _backward through ctypes, the gradient images pre-filled with NaN (an element no thread writes stays
    NaN instead of holding whatever the allocator left there).  upstream None: a NULL pointer.  Returns (loss, dcolor, ddepth)."""
    from dgr_amd import _capi
    lib, dev = _capi.load(), _dev()
    c, d, co, do = _l1_tensors(inp)
    dc, dd = torch.full_like(c, float("nan")), torch.full_like(d, float("nan"))
    n_c, n_d = (c.numel() if use_color else 0), (d.numel() if use_depth else 0)
    ptr = lambda t, use: t.data_ptr() if use else None  # noqa: E731
    buf = torch.full((lib.dgr_l1_loss_scratch_floats() + 1,), float("nan"), dtype=torch.float32, device=dev)
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=dev)
    st = _capi.stream_handle(dev.index)
    images = (n_c, ptr(c, use_color), ptr(co, use_color), n_d, ptr(d, use_depth), ptr(do, use_depth), inp["w_color"], inp["w_depth"])
    assert lib.dgr_l1_loss_forward(st, *images, buf[1:].data_ptr(), buf.data_ptr()) == 0, _capi.last_error()
    assert lib.dgr_l1_loss_backward(st, *images, None if up is None else up.data_ptr(), ptr(dc, use_color), ptr(dd, use_depth)) == 0, \
        _capi.last_error()
    return _np(buf)[0], _np(dc), _np(dd)


@pytest.mark.parametrize("shapes", sm.L1_SHAPES, ids=_l1_ids)
@pytest.mark.parametrize("family", sm.L1_FAMILIES)
def test_l1_loss_and_its_gradients(family, shapes):
    """slam.l1_loss and its backward (upstream 3.0), then the same through the C ABI into NaN-filled gradient images: the dyadic
    loss EQUALS the float64 sum, the random one meets its bar, both gradient images bit for bit."""
    from dgr_amd import slam
    inp = sm.l1_inputs(family, shapes)
    c, d, co, do = _l1_tensors(inp)
    c.requires_grad_(), d.requires_grad_()
    loss = slam.l1_loss(c, d, co, do, inp["w_color"], inp["w_depth"])
    (sm.L1_UPSTREAM * loss).backward()
    rep = sm.l1_check(inp, family, _np(loss), _np(c.grad), _np(d.grad))
    print(f"{family} {shapes}: {rep or 'exact'}")
    rep.check("autograd")
    sm.l1_check(inp, family, *l1_abi(inp, sm.L1_UPSTREAM)).check("C ABI")


@pytest.mark.parametrize("shapes", [sm.L1_SHAPES[1], sm.L1_SHAPES[4]], ids=_l1_ids)
@pytest.mark.parametrize("family", sm.L1_FAMILIES)
def test_l1_abi_null_arguments(family, shapes):
    """upstream = NULL means 1; n_color = 0 with NULL colour pointers and n_depth = 0 with NULL depth pointers leave the other
    term (and the other image untouched: it stays NaN)."""
    inp = sm.l1_inputs(family, shapes)
    sm.l1_check(inp, family, *l1_abi(inp, None), upstream=1.0).check("upstream = NULL")
    empty = np.zeros((0,), dtype=np.float32)
    loss, dc, dd = l1_abi(inp, sm.L1_UPSTREAM, use_color=False)
    assert np.isnan(dc).all()
    sm.l1_check(dict(inp, color=empty, color_obs=empty), family, loss, None, dd).check("n_color = 0")
    loss, dc, dd = l1_abi(inp, sm.L1_UPSTREAM, use_depth=False)
    assert np.isnan(dd).all()
    sm.l1_check(dict(inp, depth=empty, depth_obs=empty), family, loss, dc, None).check("n_depth = 0")


def test_l1_loss_refuses_mismatched_gpu_images():
    from dgr_amd import slam
    c, d = torch.zeros((3, 4, 5), device=_dev()), torch.zeros((1, 4, 5), device=_dev())
    with pytest.raises(ValueError, match="differ in shape"):
        slam.l1_loss(c, d, c.reshape(3, 5, 4), d)
    with pytest.raises(ValueError, match="GPU tensors"):
        slam.l1_loss(c, d, c, d.cpu())
    with pytest.raises(ValueError, match="float32"):
        slam.l1_loss(c, d.double(), c, d.double())
