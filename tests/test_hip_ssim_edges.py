"""The SSIM / L1 + D-SSIM kernels (csrc/ssim.hip) where tests/test_hip_ssim.py cannot see: the three derivative maps and the
gradient per pixel with the forward and the backward judged apart, the two reduction loops past their first trip, an image feature
at every column and row phase of the 32 x 16 tile, the independence of the planes, what include/dgr_hip.h promises about the
scratch, and the largest shapes the entry point accepts.  The cases and what makes each of them a case live in
tests/ssim_model.py and are asserted without a GPU in tests/test_ssim_abi.py.

Every assertion is one of two kinds.  Bit equality where the same instruction sequence sees the same operands (a shifted patch, a
plane alone or in a stack, upstream NULL or 1, a strided input or its copy).  Or the project's parity convention:
the distance from the float64 model of tests/ssim_model.py, against the bar 2 x the largest distance e_32 of the float32 CPU
restatement of the same lines over the test's own cases, computed at run time; every figure is printed before it is asserted and,
with DGR_SSIM_MEASURED=<file>, appended there (profiles/ssim/measured.txt holds one such run)."""
import numpy as np
import pytest
import torch

from dgr_amd import _capi, slam

import ssim_model as M
from test_hip_guarded_buffers import GuardedTorch
from test_hip_ssim import _record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SSIM_ONLY = (0.0, -1.0, 0.0)   # loss = SSIM - 1: dL_dimg is dSSIM/dimg
MAPPING = (0.8, 0.2, 0.5)      # l1_ssim_loss(w_color=1, w_depth=0.5, lambda_dssim=0.2)
HEADER = 4                     # scratch[0..3]: mean SSIM, mean|img - ref|, mean|depth - depth_obs|, maps flag


def _floats(shape):
    n = _capi.load().dgr_ssim_scratch_floats(*shape)
    assert n > 0, shape
    return n


def _forward(alloc, x, y, d=None, do=None, weights=SSIM_ONLY, want_maps=1, floats=None):
    """dgr_ssim_loss_forward on contiguous device tensors -> (scratch, loss), both from `alloc`.empty"""
    shape = tuple(x.shape)
    scratch = alloc.empty(_floats(shape) if floats is None else floats, dtype=torch.float32, device=DEV)
    loss = alloc.empty(1, dtype=torch.float32, device=DEV)
    _capi.call("dgr_ssim_loss_forward", x.device, *shape, x.data_ptr(), y.data_ptr(), 0 if d is None else d.numel(), _capi.ptr(d),
               _capi.ptr(do), *weights, scratch.data_ptr(), int(want_maps), loss.data_ptr())
    return scratch, loss


def _backward(alloc, x, y, scratch, d=None, do=None, weights=SSIM_ONLY, upstream=None):
    """dgr_ssim_loss_backward -> (dL_dimg, dL_ddepth), both from `alloc`.empty and NaN before the call"""
    dimg = alloc.empty(tuple(x.shape), dtype=torch.float32, device=DEV).fill_(float("nan"))
    dd = None if d is None else alloc.empty(tuple(d.shape), dtype=torch.float32, device=DEV).fill_(float("nan"))
    _capi.call("dgr_ssim_loss_backward", x.device, *x.shape, x.data_ptr(), y.data_ptr(), 0 if d is None else d.numel(), _capi.ptr(d),
               _capi.ptr(do), *weights, scratch.data_ptr(), _capi.ptr(upstream), dimg.data_ptr(), _capi.ptr(dd))
    return dimg, dd


def _maps_of(scratch, shape):
    """the three maps: the last 3 n floats of the scratch (include/dgr_hip.h)"""
    n = int(np.prod(shape))
    return scratch[scratch.numel() - 3 * n:].view(3, *shape)


def _dist(got, ref64, scale=None):
    """max|got - ref64| / max|ref64| (or / scale)"""
    return float((got.detach().double().cpu() - ref64).abs().max()) / (float(ref64.abs().max()) if scale is None else scale)


# ---- 1. per-pixel parity of the maps and the gradient, forward and backward apart ----------------------------------------------
QUANTITIES = ("map_mu1", "map_s1", "map_s12", "grad", "grad_bwd", "ssim")
ZERO_WHEN_SAME = ("map_mu1", "grad", "grad_bwd")   # analytically 0 with ref == img: judged against the "rand" case's scale


def _parity_case(x, y, scales=None):
    """({quantity: e_hip}, {quantity: e_32}, {quantity: max|model64|}) of one input pair.  "grad" is the kernels' forward and
    backward together; "grad_bwd" the backward kernel alone, fed the model's maps rounded to float32 (its yardstick is "grad"'s);
    "ssim" an absolute distance.  `scales` replaces the case's own scale where given."""
    shape, n = tuple(x.shape), x.numel()
    ref = M.model(x, y)
    m64 = dict(zip(QUANTITIES[:3], M.maps(x, y)), grad=ref["grad"], grad_bwd=ref["grad"])
    cpu = M.model(x, y, dtype=torch.float32)
    m32 = dict(zip(QUANTITIES[:3], M.maps(x, y, torch.float32)), grad=cpu["grad"], grad_bwd=cpu["grad"])
    xg, yg = x.to(DEV), y.to(DEV)
    scratch, loss = _forward(torch, xg, yg)
    got = dict(zip(QUANTITIES[:3], _maps_of(scratch, shape)))
    got["grad"] = _backward(torch, xg, yg, scratch)[0]
    fed = torch.zeros_like(scratch)
    fed[HEADER - 1] = 1.0  # the header's flag: maps present
    fed[fed.numel() - 3 * n:] = torch.stack(M.maps(x, y)).to(torch.float32).flatten().to(DEV)
    got["grad_bwd"] = _backward(torch, xg, yg, fed)[0]
    own = {q: float(m64[q].abs().max()) for q in QUANTITIES[:5]}
    scale = dict(own, **(scales or {}))
    e_hip = {q: _dist(got[q], m64[q], scale[q]) for q in QUANTITIES[:5]}
    e_32 = {q: _dist(m32[q], m64[q], scale[q]) for q in QUANTITIES[:5]}
    e_hip["ssim"] = abs(float(scratch[0].double().cpu()) - float(ref["ssim"]))
    e_32["ssim"] = abs(float(cpu["ssim"]) - float(ref["ssim"]))
    assert abs(float(loss) - (float(scratch[0]) - 1.0)) <= 1.2e-7  # (weights (0, -1, 0): the loss is SSIM - 1, rounded once)
    return e_hip, e_32, own


@pytest.fixture(scope="module")
def parity():
    """{(kind, shape): (e_hip, e_32)}: the model, the yardstick and the kernels run once"""
    table, rand_scale = {}, {}
    for kind in M.EDGE_KINDS:  # ("rand" first: its scales serve "same")
        for shape in M.EDGE_SHAPES:
            x, y = M.edge_inputs(kind, shape)
            scales = {q: rand_scale[shape][q] for q in ZERO_WHEN_SAME} if kind == "same" else None
            e_hip, e_32, own = _parity_case(x, y, scales)
            if kind == "rand":
                rand_scale[shape] = own
            table[kind, shape] = (e_hip, e_32)
    torch.cuda.synchronize()
    return table


def _bars(parity, kind):
    return {q: 2 * max(parity[kind, s][1][q] for s in M.EDGE_SHAPES) for q in QUANTITIES}


@pytest.mark.parametrize("kind", M.EDGE_KINDS)
def test_maps_and_gradient_per_pixel(parity, kind):
    """Each of the three maps the forward writes, the gradient of forward + backward, and the gradient of the backward alone from
    the model's maps, against the float64 model.  (Mean SSIM is recorded here and not asserted: with ref == img the yardstick is
    exact and its bar 0; tests/test_hip_ssim.py::test_identical_images holds it to 1e-6.)"""
    bars = _bars(parity, kind)
    _record(f"# edges {kind}: bar = 2 x max e_32 over the nine edge shapes: " + ", ".join(f"{q} {bars[q]:.3e}" for q in QUANTITIES))
    worst = []
    for shape in M.EDGE_SHAPES:
        e_hip, e_32 = parity[kind, shape]
        for q in QUANTITIES:
            ratio = e_hip[q] / bars[q] if bars[q] > 0 else float("inf") if e_hip[q] > 0 else 0.0
            _record(f"edges {kind:10s} {str(shape):16s} {q:8s} e_hip {e_hip[q]:.3e}  e_32 {e_32[q]:.3e}  e_hip/bar {ratio:.3f}")
            if q != "ssim":
                worst.append((ratio, shape, q))
    assert all(bars[q] > 0 for q in QUANTITIES[:5]), bars
    assert max(worst)[0] <= 1.0, sorted(worst, reverse=True)[:5]


# ---- 2. the reduction loops past their first trip -----------------------------------------------------------------------------
def test_the_tile_sum_past_one_trip():
    """ssim_final_kernel adds the workgroups' slots 256 at a time: 255, 256 and 257 one-tile planes, 260 one-pixel planes and 378
    tiles of a larger stack, every plane random so that every slot holds a different value.  Mean SSIM and scratch[1], under the
    bar as tests/test_hip_ssim.py forms it: 2 x the largest e_32 over the test's own cases (one case's e_32 can be 0)."""
    rows = []
    for shape in M.TILE_SHAPES:
        x, y = M.edge_inputs("rand", shape)
        ref, cpu = M.model(x, y), M.model(x, y, dtype=torch.float32)
        l1_64 = float((x.double() - y.double()).abs().mean())
        l1_32 = float((x - y).abs().mean())
        scratch, loss = _forward(torch, x.to(DEV), y.to(DEV), weights=MAPPING[:2] + (0.0,))
        head = scratch[:HEADER].double().cpu()
        assert float(head[2]) == 0.0 and float(head[3]) == 1.0, head
        loss64 = MAPPING[0] * l1_64 + MAPPING[1] * (1.0 - float(ref["ssim"]))
        loss32 = float(torch.tensor(MAPPING[0]) * (x - y).abs().mean() + torch.tensor(MAPPING[1]) * (1 - cpu["ssim"]))
        rows.append((shape, (abs(float(head[0]) - float(ref["ssim"])), abs(float(head[1]) - l1_64), abs(float(loss) - loss64)),
                     (abs(float(cpu["ssim"]) - float(ref["ssim"])), abs(l1_32 - l1_64), abs(loss32 - loss64))))
    names = ("ssim", "mean_l1", "loss")
    bars = [2 * max(r[2][q] for r in rows) for q in range(3)]
    _record("# tile sum: bar = 2 x max e_32 over the five tile-count cases: " + ", ".join(f"{n} {b:.3e}" for n, b in zip(names, bars)))
    worst = []
    for shape, e_hip, e_32 in rows:
        for q, name in enumerate(names):
            _record(f"tiles {M.tiles_of(shape):4d} {str(shape):16s} {name:8s} e_hip {e_hip[q]:.3e}  e_32 {e_32[q]:.3e}  "
                    f"e_hip/bar {e_hip[q] / bars[q]:.3f}")
            worst.append((e_hip[q] / bars[q], shape, name))
    assert all(b > 0 for b in bars), bars
    assert max(worst)[0] <= 1.0, max(worst)


def test_the_depth_sum_past_one_trip():
    """depth_partial_kernel walks the depth image 32768 elements at a time; the C ABI and the Python surface leave n_depth free of
    the colour shape.  Ties and the largest differences sit on the last element of the first trip, the first of the second and the
    last of all.  Loss and scratch[2] against the model; dL_ddepth = w_depth / n_depth sign(d - d_obs) upstream per element."""
    x, y = M.edge_inputs("rand", (1, 1, 5, 7))
    xg, yg = x.to(DEV), y.to(DEV)
    up = 1.75
    upstream = torch.tensor([up], dtype=torch.float32, device=DEV)
    rows = []
    for n in M.DEPTH_COUNTS:
        for variant in ("ties", "peaks"):
            d, do, special = M.depth_pair(n, variant)
            dg, dog = d.to(DEV), do.to(DEV)
            ref = M.model(x, y, d, do, *MAPPING)
            cpu = M.model(x, y, d, do, *MAPPING, dtype=torch.float32)
            dl1_64, dl1_32 = float((d.double() - do.double()).abs().mean()), float((d - do).abs().mean())
            scratch, loss = _forward(torch, xg, yg, dg, dog, MAPPING)
            dimg, dd = _backward(torch, xg, yg, scratch, dg, dog, MAPPING, upstream)
            rows.append((n, variant, (abs(float(loss) - float(ref["loss"])), abs(float(scratch[2]) - dl1_64)),
                         (abs(float(cpu["loss"]) - float(ref["loss"])), abs(dl1_32 - dl1_64))))
            want = MAPPING[2] / n * torch.sign(d.double() - do.double()) * up
            got = dd.cpu()
            assert torch.allclose(got.double(), want, rtol=1e-6, atol=0), (n, variant)
            ties = d == do
            assert not got[ties].any() and bool((got[~ties] != 0).all()) and int(ties.sum()) >= (len(special) if variant == "ties" else 0)
            if variant == "ties":
                assert bool(ties[special].all())
            # the Python surface on the same arrays: the same bits
            xl, dl = xg.clone().requires_grad_(), dg.clone().requires_grad_()
            py_loss = slam.l1_ssim_loss(xl, dl, yg, dog, 1.0, MAPPING[2], 0.2)
            (up * py_loss).backward()
            assert torch.equal(py_loss.detach().reshape(1), loss) and torch.equal(dl.grad, dd) and torch.equal(xl.grad, dimg)
    names = ("loss", "mean_dl1")
    bars = [2 * max(r[3][q] for r in rows) for q in range(2)]
    _record("# depth sum: bar = 2 x max e_32 over the eight depth cases: " + ", ".join(f"{n} {b:.3e}" for n, b in zip(names, bars)))
    worst = []
    for n, variant, e_hip, e_32 in rows:
        for q, name in enumerate(names):
            _record(f"depth n_depth {n:6d} {variant:6s} {name:8s} e_hip {e_hip[q]:.3e}  e_32 {e_32[q]:.3e}  e_hip/bar {e_hip[q] / bars[q]:.3f}")
            worst.append((e_hip[q] / bars[q], n, variant, name))
    assert all(b > 0 for b in bars), bars
    assert max(worst)[0] <= 1.0, max(worst)


# ---- 3. every tile phase, bit for bit -----------------------------------------------------------------------------------------
def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def test_a_patch_at_every_tile_phase_gives_the_same_bits():
    """A 13 x 19 random patch pair on a constant canvas, its corner at every column of a 32-wide tile, every row of a 16-high one
    and eight mixed placements.  A pixel's map values depend on its 11 x 11 neighbourhood and its gradient on 21 x 21, formed by the
    same instruction sequence whichever lane and tile own the pixel: over the patch and a 10-pixel margin dSSIM/dimg carries the
    bits of the first placement, shifted.  The sums of m and |img - ref| see the same multiset of addends and run in double, so mean
    SSIM and the loss stay within one float32 ulp."""
    (oy, ox), (h, w), m = M.PATCH_ORIGIN, M.PATCH_HW, M.MARGIN
    patch = M.patch_pair()

    def run(dy, dx):
        img, ref = (t.to(DEV) for t in M.placed(M.CANVAS_HW, patch, oy + dy, ox + dx))
        leaf = img.clone().requires_grad_()
        s = slam.ssim(leaf, ref)
        s.backward()
        loss = slam.l1_ssim_loss(img, None, ref, None)
        window = leaf.grad[0, 0, oy + dy - m:oy + dy + h + m, ox + dx - m:ox + dx + w + m]
        return window.cpu(), float(s.detach()), float(loss)

    g0, s0, l0 = run(0, 0)
    assert g0.shape == (h + 2 * m, w + 2 * m) and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    differ, worst_value = [], 0.0
    for dy, dx in M.PHASES[1:]:
        g, s, loss = run(dy, dx)
        bad = int((g.view(torch.int32) != g0.view(torch.int32)).sum())
        if bad:
            differ.append((dy, dx, bad, float((g - g0).abs().max()) / float(g0.abs().max())))
        worst_value = max(worst_value, abs(s - s0) / _ulp32(s0), abs(loss - l0) / _ulp32(l0))
    _record(f"tile phases: {len(M.PHASES) - 1} placements, {len(differ)} with a gradient bit changed; mean SSIM and loss move by at most "
            f"{worst_value:.2f} ulp")
    assert not differ, differ  # (dy, dx, elements whose bits differ, largest difference / max|grad|)
    assert worst_value <= 1.0, worst_value


# ---- 4. planes are independent ------------------------------------------------------------------------------------------------
def _ssim_grad(x, y):
    leaf = x.clone().requires_grad_()
    slam.ssim(leaf, y).backward()
    return leaf.grad


def test_planes_are_independent():
    """A plane's gradient in a [2,2,37,53] stack is its gradient alone over 4, bit for bit: the only difference is the factor
    1 / (float)n with n four times larger, and a power of two commutes with rounding.  NaN and Inf in one plane leave the other
    three planes' bits alone."""
    shape = (2, 2, 37, 53)
    x, y = (t.to(DEV) for t in M.edge_inputs("rand", shape))
    whole = _ssim_grad(x, y)
    assert bool(torch.isfinite(whole).all())
    for v in range(2):
        for c in range(2):
            alone = _ssim_grad(x[v, c][None].contiguous(), y[v, c][None].contiguous())
            assert float(alone.abs().max()) > 0
            assert torch.equal(whole[v, c], alone[0] / 4), (v, c)
    poisoned = x.clone()
    poisoned[1, 0] = float("nan")
    poisoned[1, 0, ::2, ::3] = float("inf")
    poisoned[1, 0, 1::4, 1::5] = float("-inf")
    got = _ssim_grad(poisoned, y)
    for v, c in ((0, 0), (0, 1), (1, 1)):
        assert torch.equal(got[v, c], whole[v, c]), (v, c)


# ---- 5. the header's promises and memory safety -------------------------------------------------------------------------------
def _depth_for(shape, seed=0):
    g = torch.Generator().manual_seed(77 + sum(shape) + seed)
    s = (shape[0], 1, shape[2], shape[3])
    return (1.0 + torch.rand(s, generator=g)).to(DEV), (1.0 + torch.rand(s, generator=g)).to(DEV)


def test_inference_form_on_a_scratch_that_ends_before_the_maps():
    """want_maps = 0 with the scratch cut where the maps would begin, between guards: nothing outside is written and the loss has
    the bits of the want_maps = 1 call."""
    for shape in ((2, 2, 37, 53), (1, 1, 16, 32), (1, 1, 1, 1)):
        x, y = (t.to(DEV) for t in M.edge_inputs("rand", shape))
        d, do = _depth_for(shape)
        full_scratch, full_loss = _forward(torch, x, y, d, do, MAPPING, want_maps=1)
        guarded = GuardedTorch()
        short = _floats(shape) - 3 * x.numel()
        scratch, loss = _forward(guarded, x, y, d, do, MAPPING, want_maps=0, floats=short)
        assert guarded.check() == 2
        assert torch.equal(loss, full_loss) and torch.equal(scratch[:HEADER - 1], full_scratch[:HEADER - 1])
        assert float(scratch[HEADER - 1]) == 0.0 and float(full_scratch[HEADER - 1]) == 1.0


def test_inference_form_leaves_the_maps_alone_and_poisons_a_backward():
    """want_maps = 0 on a full-size scratch: the map region keeps the byte pattern it held, and a backward called on that scratch
    fills dL_dimg with NaN, every element, whatever the weights."""
    shape = (2, 2, 37, 53)
    x, y = (t.to(DEV) for t in M.edge_inputs("rand", shape))
    n = x.numel()
    for weights in (MAPPING[:2] + (0.0,), SSIM_ONLY):
        scratch = torch.empty(_floats(shape), dtype=torch.float32, device=DEV)
        scratch.view(torch.uint8).fill_(0x5A)
        loss = torch.empty(1, dtype=torch.float32, device=DEV)
        _capi.call("dgr_ssim_loss_forward", x.device, *shape, x.data_ptr(), y.data_ptr(), 0, None, None, *weights,
                   scratch.data_ptr(), 0, loss.data_ptr())
        assert bool((scratch[scratch.numel() - 3 * n:].view(torch.uint8) == 0x5A).all())
        assert float(scratch[HEADER - 1]) == 0.0 and bool(torch.isfinite(loss).all())
        dimg = torch.zeros_like(x)
        _capi.call("dgr_ssim_loss_backward", x.device, *shape, x.data_ptr(), y.data_ptr(), 0, None, None, *weights,
                   scratch.data_ptr(), None, dimg.data_ptr(), None)
        assert bool(torch.isnan(dimg).all())


@pytest.mark.parametrize("shape", M.EDGE_SHAPES + M.TILE_SHAPES[-1:], ids=str)
def test_forward_and_backward_stay_inside_their_buffers(shape):
    """want_maps = 1 with the scratch, the loss and both gradient images between guard regions: no byte outside them changes, and
    every element inside the gradients is written."""
    x, y = (t.to(DEV) for t in M.edge_inputs("rand", shape))
    d, do = _depth_for(shape)
    guarded = GuardedTorch()
    scratch, loss = _forward(guarded, x, y, d, do, MAPPING)
    assert guarded.check() == 2
    dimg, dd = _backward(guarded, x, y, scratch, d, do, MAPPING)
    assert guarded.check() == 2
    assert bool(torch.isfinite(dimg).all()) and bool(torch.isfinite(dd).all()) and bool(torch.isfinite(loss).all())
    assert bool(torch.isfinite(_maps_of(scratch, shape)).all())


def test_upstream_null_means_one():
    shape = (2, 2, 37, 53)
    x, y = (t.to(DEV) for t in M.edge_inputs("rand", shape))
    d, do = _depth_for(shape)
    scratch, _ = _forward(torch, x, y, d, do, MAPPING)
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    a = _backward(torch, x, y, scratch, d, do, MAPPING, None)
    b = _backward(torch, x, y, scratch, d, do, MAPPING, one)
    two = _backward(torch, x, y, scratch, d, do, MAPPING, 2 * one)
    for p, q, r in zip(a, b, two):
        assert float(p.abs().max()) > 0 and torch.equal(p, q) and torch.equal(r, 2 * p)


def test_a_strided_image_gives_the_bits_of_its_copy():
    shape = (2, 2, 37, 53)
    g = torch.Generator().manual_seed(31)
    wide = torch.rand(shape[:3] + (2 * shape[3],), generator=g).to(DEV)
    ref = torch.rand(shape, generator=g).to(DEV)
    strided = wide[..., ::2].detach().requires_grad_()
    assert not strided.is_contiguous()
    copy = strided.detach().contiguous().requires_grad_()
    values = []
    for leaf in (strided, copy):
        s = slam.ssim(leaf, ref)
        loss = slam.l1_ssim_loss(leaf, None, ref, None)
        (s + loss).backward()
        values.append((s.detach(), loss.detach(), leaf.grad))
    for a, b in zip(*values):
        assert torch.equal(a, b)
    assert float(values[0][2].abs().max()) > 0


# ---- 6. the largest shapes the entry point accepts ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.LIMIT_SHAPES, ids=str)
def test_the_largest_accepted_shapes(parity, shape):
    """n_images * channels = 65535 (the grid's z) and a height and a width of 2^20 (65536 workgroups along the grid's y, 32768 along
    x): forward and backward succeed (_capi.call raises on any other result), and mean SSIM and the gradient meet the "rand" bar of
    the per-pixel test.  The model's gradient is its three-map form, which tests/test_ssim_abi.py pins to float64 autograd on these
    shapes."""
    bars = _bars(parity, "rand")
    x, y = M.edge_inputs("rand", shape)
    ssim64, grad64 = float(M.ssim_map(x.double(), y.double()).mean()), M.analytic_grad(x, y)
    xg, yg = x.to(DEV), y.to(DEV)
    scratch, loss = _forward(torch, xg, yg)
    dimg, _ = _backward(torch, xg, yg, scratch)
    torch.cuda.synchronize()
    e_ssim, e_grad = abs(float(scratch[0].double().cpu()) - ssim64), _dist(dimg, grad64)
    _record(f"limit {str(shape):20s} ssim e_hip {e_ssim:.3e}  e_hip/bar {e_ssim / bars['ssim']:.3f}   grad e_hip {e_grad:.3e}  "
            f"e_hip/bar {e_grad / bars['grad']:.3f}")
    assert bars["ssim"] > 0 and bars["grad"] > 0
    assert e_ssim <= bars["ssim"] and e_grad <= bars["grad"], (e_ssim, e_grad, bars)
