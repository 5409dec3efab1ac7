"""slam.ssim / slam.l1_ssim_loss (csrc/ssim.hip) on the GPU against the float64 model of tests/ssim_model.py.

Parity is measured, not fixed in advance: e_hip is the distance of the HIP result from the float64 model, e_32 that of the float32
CPU restatement of the same lines (the yardstick), and the bar of an input kind is 2 x the largest e_32 of that kind over the six
shapes (the project's ref-parity convention; a separable two-pass sum and a direct 121-tap sum round in different
orders, so equality with the yardstick cannot be expected).  Every figure is printed before it is asserted; with
DGR_SSIM_MEASURED=<file> they are appended there (profiles/ssim/measured.txt holds one such run)."""
import os
import sys

import pytest
import torch

from dgr_amd import slam

import ssim_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the loss of the parity test: colour and depth weights of the mapping example, 3DGS's lambda
W_COLOR, W_DEPTH, LAMBDA = 1.0, 0.5, 0.2
QUANTITIES = ("ssim", "ssim_grad", "loss", "loss_grad")


def _record(line):
    print(line)
    path = os.environ.get("DGR_SSIM_MEASURED")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _depth_pair(shape):
    g = torch.Generator().manual_seed(99 + sum(shape))
    s = (shape[0], 1, shape[2], shape[3])
    return 1.0 + torch.rand(s, generator=g), 1.0 + torch.rand(s, generator=g)


def _errors(got, ref64):
    """(|ssim - ssim64|, max|g - g64| / max|g64|, |loss - loss64|, the same for the loss's colour gradient)"""
    out = []
    for value, grad in (("ssim", "ssim_grad"), ("loss", "loss_grad")):
        out.append(abs(float(got[value].double().cpu()) - float(ref64[value])))
        out.append(float((got[grad].double().cpu() - ref64[grad]).abs().max()) / float(ref64[grad].abs().max()))
    return out


def _hip(x, y, d, do):
    xg, yg = x.to(DEV).requires_grad_(), y.to(DEV)
    s = slam.ssim(xg, yg)
    s.backward()
    xl, dl = x.to(DEV).requires_grad_(), d.to(DEV).requires_grad_()
    loss = slam.l1_ssim_loss(xl, dl, yg, do.to(DEV), W_COLOR, W_DEPTH, LAMBDA)
    loss.backward()
    return dict(ssim=s.detach(), ssim_grad=xg.grad, loss=loss.detach(), loss_grad=xl.grad, depth_grad=dl.grad)


def _cpu(x, y, d, do, dtype):
    a = M.model(x, y, dtype=dtype)
    b = M.model(x, y, d, do, W_COLOR * (1 - LAMBDA), W_COLOR * LAMBDA, W_DEPTH, dtype=dtype)
    return dict(ssim=a["ssim"], ssim_grad=a["grad"], loss=b["loss"], loss_grad=b["grad"], depth_grad=b["grad_depth"])


@pytest.fixture(scope="module")
def parity():
    """{(kind, shape): (e_hip[4], e_32[4])}: the model, the yardstick and the kernels run once for all parity tests."""
    table = {}
    for kind in M.KINDS:
        for shape in M.SHAPES:
            x, y = M.inputs(kind, shape)
            d, do = _depth_pair(shape)
            ref64 = _cpu(x, y, d, do, torch.float64)
            got = _hip(x, y, d, do)
            table[kind, shape] = (_errors(got, ref64), _errors(_cpu(x, y, d, do, torch.float32), ref64))
            # the depth term's gradient is w / n sign(d - d_obs): exact in any precision
            assert torch.allclose(got["depth_grad"].cpu().double(), ref64["depth_grad"], rtol=1e-6, atol=0)
    torch.cuda.synchronize()
    return table


@pytest.mark.parametrize("kind", M.KINDS)
def test_parity_with_the_float64_model(parity, kind):
    bars = [2 * max(parity[kind, s][1][q] for s in M.SHAPES) for q in range(4)]
    _record(f"# {kind}: bar = 2 x max e_32 over the six shapes: " + ", ".join(f"{n} {b:.3e}" for n, b in zip(QUANTITIES, bars)))
    worst = []
    for shape in M.SHAPES:
        e_hip, e_32 = parity[kind, shape]
        for q, name in enumerate(QUANTITIES):
            ratio = e_hip[q] / bars[q]
            _record(f"{kind:10s} {str(shape):18s} {name:9s} e_hip {e_hip[q]:.3e}  e_32 {e_32[q]:.3e}  e_hip/bar {ratio:.3f}")
            worst.append((ratio, shape, name))
    assert all(b > 0 for b in bars), bars
    assert max(worst)[0] <= 1.0, max(worst)


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_identical_images():
    x = _rand((2, 3, 37, 53), 1)
    ref = x.clone()
    s = slam.ssim(x, ref)
    assert abs(1.0 - float(s)) <= 1e-6, float(s)
    # the L1 term is exactly 0 and so is its gradient wherever the images tie: lambda = 0 leaves nothing else
    xr = x.clone().requires_grad_()
    loss = slam.l1_ssim_loss(xr, None, ref, None, 1.0, 0.5, 0.0)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not xr.grad.any()
    # ties in part of the image: zero gradient exactly there
    y = ref.clone()
    y[:, :, :, 20:] += 0.25
    xr = x.clone().requires_grad_()
    slam.l1_ssim_loss(xr, None, y, None, 1.0, 0.5, 0.0).backward()
    assert not xr.grad[:, :, :, :20].any() and bool((xr.grad[:, :, :, 20:] < 0).all())


def test_ssim_is_symmetric_in_its_arguments():
    for kind in M.KINDS:
        x, y = (t.to(DEV) for t in M.inputs(kind, (2, 3, 17, 33)))
        a, b = float(slam.ssim(x, y)), float(slam.ssim(y, x))
        assert abs(a - b) <= 1e-6, (kind, a, b)


def _close(a, b, rtol):
    """max|a - b| <= rtol max|b| (rtol of scale)"""
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= rtol * scale, (float((a - b).abs().max()), scale)


@pytest.mark.parametrize("with_depth", [True, False], ids=["depth", "no-depth"])
def test_composition_from_ssim_and_torch_ops(with_depth):
    shape, w_c, w_d, lam = (2, 3, 37, 53), 0.7, 0.4, 0.3
    c0, co = _rand(shape, 2), _rand(shape, 3)
    d0, do = (_rand((2, 1, 37, 53), 4), _rand((2, 1, 37, 53), 5)) if with_depth else (None, None)

    def leaves():
        return c0.clone().requires_grad_(), (d0.clone().requires_grad_() if with_depth else None)

    c, d = leaves()
    loss = slam.l1_ssim_loss(c, d, co, do, w_c, w_d, lam)
    (3.0 * loss).backward()
    c2, d2 = leaves()
    want = w_c * ((1 - lam) * (c2 - co).abs().mean() + lam * (1 - slam.ssim(c2, co)))
    if with_depth:
        want = want + w_d * (d2 - do).abs().mean()
    (3.0 * want).backward()
    assert abs(float(loss) - float(want)) <= 2e-6 * abs(float(want)), (float(loss), float(want))
    _close(c.grad, c2.grad, 1e-5)
    if with_depth:
        _close(d.grad, d2.grad, 1e-5)


def test_lambda_zero_is_l1_loss():
    shape = (2, 3, 37, 53)
    c0, co, d0, do = _rand(shape, 6), _rand(shape, 7), _rand((2, 1, 37, 53), 8), _rand((2, 1, 37, 53), 9)
    c, d = c0.clone().requires_grad_(), d0.clone().requires_grad_()
    a = slam.l1_ssim_loss(c, d, co, do, 1.0, 0.5, 0.0)
    a.backward()
    c2, d2 = c0.clone().requires_grad_(), d0.clone().requires_grad_()
    b = slam.l1_loss(c2, d2, co, do, 1.0, 0.5)
    b.backward()
    assert abs(float(a) - float(b)) <= 2e-6 * float(b)
    assert torch.allclose(c.grad, c2.grad, rtol=1e-6, atol=0) and torch.allclose(d.grad, d2.grad, rtol=1e-6, atol=0)


def test_a_stack_is_the_mean_of_its_views():
    V, shape = 3, (3, 3, 37, 53)
    c0, co, d0, do = _rand(shape, 10), _rand(shape, 11), _rand((V, 1, 37, 53), 12), _rand((V, 1, 37, 53), 13)
    c, d = c0.clone().requires_grad_(), d0.clone().requires_grad_()
    whole = slam.l1_ssim_loss(c, d, co, do)
    whole.backward()
    per_view = []
    for k in range(V):
        ck, dk = c0[k].clone().requires_grad_(), d0[k].clone().requires_grad_()
        loss = slam.l1_ssim_loss(ck, dk, co[k], do[k])
        loss.backward()
        per_view.append(float(loss))
        _close(c.grad[k], ck.grad / V, 1e-5)
        _close(d.grad[k], dk.grad / V, 1e-5)
    mean = sum(per_view) / V
    assert abs(float(whole) - mean) <= 2e-6 * mean, (float(whole), mean)


def test_two_calls_give_the_same_bits():
    shape = (4, 3, 48, 64)
    c0, co, d0, do = _rand(shape, 14), _rand(shape, 15), _rand((4, 1, 48, 64), 16), _rand((4, 1, 48, 64), 17)
    runs = []
    for _ in range(2):
        c, d = c0.clone().requires_grad_(), d0.clone().requires_grad_()
        loss = slam.l1_ssim_loss(c, d, co, do)
        loss.backward()
        runs.append((loss.detach().clone(), c.grad, d.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][1]).all() and runs[0][1].abs().max() > 0


def test_inference_form_gives_the_same_loss_and_no_gradient():
    """Without a gradient to form, the forward runs with want_maps = 0 on a scratch that ends before the maps: same bits."""
    shape = (2, 3, 37, 53)
    c0, co = _rand(shape, 18), _rand(shape, 19)
    a = slam.l1_ssim_loss(c0, None, co, None)
    with torch.no_grad():
        b = slam.l1_ssim_loss(c0.clone().requires_grad_(), None, co, None)
    c = slam.l1_ssim_loss(c0.clone().requires_grad_(), None, co, None)
    assert not a.requires_grad and not b.requires_grad and c.requires_grad
    assert torch.equal(a, c.detach()) and torch.equal(b, c.detach())


def test_replayed_from_a_hipgraph():
    shape = (2, 3, 37, 53)
    c, d = _rand(shape, 20).requires_grad_(), _rand((2, 1, 37, 53), 21).requires_grad_()
    co, do = _rand(shape, 22), _rand((2, 1, 37, 53), 23)

    def step():
        c.grad = d.grad = None
        loss = slam.l1_ssim_loss(c, d, co, do)
        loss.backward()
        return loss.detach(), c.grad, d.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    new = [_rand(shape, 24), _rand((2, 1, 37, 53), 25), _rand(shape, 26), _rand((2, 1, 37, 53), 27)]
    with torch.no_grad():
        for dst, src in zip((c, d, co, do), new):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    ce, de = new[0].clone().requires_grad_(), new[1].clone().requires_grad_()
    loss = slam.l1_ssim_loss(ce, de, new[2], new[3])
    loss.backward()
    for a, b in zip(replayed, (loss.detach(), ce.grad, de.grad)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("fused", [False, True], ids=["eager", "fused"])
def test_mapping_loop_with_the_ssim_loss(fused):
    """examples/mapping.py --ssim 0.2: the L1 + D-SSIM loop goes down and leaves finite gradients.  Only the direction is asserted
    (nobody has measured what ratio such a loop reaches in this many iterations); the ratio is recorded."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from mapping import mapping_loop
    iters, keyframes = 40, 3
    (l0, l1), pc, _ = mapping_loop(torch.device(DEV), 8000, 192, 144, keyframes, iters, fused=fused, ssim_lambda=0.2)
    _record(f"mapping_loop ssim_lambda=0.2 {'fused' if fused else 'eager'}: loss {l0:.4e} -> {l1:.4e}, ratio {l1 / l0:.3f}")
    assert l1 < l0, (l0, l1)
    for name, leaf in pc.leaves().items():
        assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()), name
