"""The SSIM loss entry points (include/dgr_hip.h: dgr_ssim_*) and their Python surface without a GPU: declared, exported and
bound; the scratch size; every argument error refused with a message before any device call; and the formula the backward kernel
implements, pinned against autograd in float64."""
import ctypes as C

import pytest
import torch

from dgr_amd import _capi, slam

import ssim_model as M
from abi_checks import FAKE, assert_entry_points, refused

NAMES = ("dgr_ssim_scratch_floats", "dgr_ssim_loss_forward", "dgr_ssim_loss_backward")


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_ssim_loss_forward": 16, "dgr_ssim_loss_backward": 17})
    assert _capi._SIGS["dgr_ssim_scratch_floats"][0] is C.c_long


def test_scratch_size():
    f = _capi.load().dgr_ssim_scratch_floats
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8), (1, 3, -8, 8), (65536, 1, 8, 8),
                (256, 256, 8, 8)):
        assert f(*bad) == 0, bad
    assert f(65535, 1, 1, 1) > 0 and f(255, 257, 1, 1) > 0
    base = (2, 3, 40, 70)
    for shape in (base, (1, 1, 1, 1), (4, 3, 480, 640), (1, 3, 1080, 1920), (8, 3, 4000, 6000)):
        n = shape[0] * shape[1] * shape[2] * shape[3]
        assert 3 * n < f(*shape) <= 3 * n + n // 16 + 1024, shape   # the maps, and partial sums that stay a small share
    for dim in range(4):  # monotone in each dimension (also across a tile boundary: 32 -> 33 columns, 16 -> 17 rows)
        sizes = []
        for v in (1, 2, 16, 17, 32, 33, 100):
            shape = list(base)
            shape[dim] = v
            sizes.append(f(*shape))
        assert all(b > a for a, b in zip(sizes, sizes[1:])), (dim, sizes)


def _forward(shape=(1, 3, 8, 8), img=FAKE, ref=FAKE, n_depth=0, depth=None, depth_obs=None, scratch=FAKE, loss=FAKE):
    return _capi.load().dgr_ssim_loss_forward(None, *shape, img, ref, n_depth, depth, depth_obs, 0.8, 0.2, 0.5, scratch, 1, loss)


def _backward(shape=(1, 3, 8, 8), img=FAKE, ref=FAKE, n_depth=0, depth=None, depth_obs=None, scratch=FAKE, dimg=FAKE, ddepth=None):
    return _capi.load().dgr_ssim_loss_backward(None, *shape, img, ref, n_depth, depth, depth_obs, 0.8, 0.2, 0.5, scratch, None,
                                               dimg, ddepth)


CASES = [
    (dict(img=None), "img or ref is NULL"),
    (dict(ref=None), "img or ref is NULL"),
    (dict(scratch=None), "scratch is NULL"),
    (dict(scratch=FAKE + 4), "16-byte aligned"),
    (dict(shape=(0, 3, 8, 8)), "must be positive"),
    (dict(shape=(1, 0, 8, 8)), "must be positive"),
    (dict(shape=(1, 3, -1, 8)), "must be positive"),
    (dict(shape=(1, 3, 8, 0)), "must be positive"),
    (dict(n_depth=-1), "n_depth is negative"),
    (dict(n_depth=64, depth=None, depth_obs=FAKE), "NULL depth or depth_obs"),
    (dict(n_depth=64, depth=FAKE, depth_obs=None), "NULL depth or depth_obs"),
    (dict(shape=(65536, 1, 8, 8)), "at most 65535"),
    (dict(shape=(300, 300, 8, 8)), "at most 65535"),
]
IDS = ["img-null", "ref-null", "scratch-null", "scratch-misaligned", "V=0", "C=0", "H<0", "W=0", "n_depth<0", "depth-null",
       "depth_obs-null", "V-too-large", "VC-too-large"]


@pytest.mark.parametrize("case, text", CASES, ids=IDS)
def test_forward_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_forward(**case), "dgr_ssim_loss_forward", text)


@pytest.mark.parametrize("case, text", CASES, ids=IDS)
def test_backward_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_backward(**case), "dgr_ssim_loss_backward", text)


def test_null_outputs_are_refused():
    refused(_forward(loss=None), "dgr_ssim_loss_forward", "loss is NULL")
    refused(_backward(dimg=None), "dgr_ssim_loss_backward", "dL_dimg is NULL")
    refused(_backward(n_depth=64, depth=FAKE, depth_obs=FAKE, ddepth=None), "dgr_ssim_loss_backward", "NULL dL_ddepth")


def test_python_surface_refuses_what_it_cannot_read():
    """Every check runs on the host, the device check last: CPU tensors reach each of them and never the library."""
    r = torch.rand
    x, y = r(3, 8, 8), r(3, 8, 8)
    for fn in (slam.ssim, lambda a, b: slam.l1_ssim_loss(a, None, b, None)):
        with pytest.raises(ValueError, match="GPU tensors"):
            fn(x, y)
        with pytest.raises(ValueError, match="GPU tensors"):
            fn(x[None], y[None])
        with pytest.raises(ValueError, match="float32"):
            fn(x.double(), y.double())
        with pytest.raises(ValueError, match="float32"):
            fn(x, y.half())
        with pytest.raises(ValueError, match="must be a tensor"):
            fn(x, None)
        for a, b, text in ((r(3, 8, 8), r(3, 8, 9), "differ in shape"), (r(3, 8, 8), r(1, 3, 8, 8), "differ in shape"),
                           (r(8, 8), r(8, 8), r"\[C,H,W\] or \[V,C,H,W\]"), (r(1, 2, 3, 8, 8), r(1, 2, 3, 8, 8), r"\[C,H,W\]"),
                           (r(0, 3, 8, 8), r(0, 3, 8, 8), "cannot read"), (r(300, 300, 2, 2), r(300, 300, 2, 2), "cannot read")):
            with pytest.raises(ValueError, match=text):
                fn(a, b)
    with pytest.raises(ValueError, match="together or both None"):
        slam.l1_ssim_loss(x, r(1, 8, 8), y, None)
    with pytest.raises(ValueError, match="differ in shape"):
        slam.l1_ssim_loss(x, r(1, 8, 8), y, r(1, 8, 7))
    with pytest.raises(ValueError, match="float32"):
        slam.l1_ssim_loss(x, r(1, 8, 8).double(), y, r(1, 8, 8).double())
    with pytest.raises(ValueError, match="GPU tensors"):
        slam.l1_ssim_loss(x, r(1, 8, 8), y, r(1, 8, 8))


def test_three_map_gradient_is_the_autograd_gradient():
    """The formula the backward kernel implements, against float64 autograd of the model, on every parity case."""
    for kind in M.KINDS:
        for shape in M.SHAPES:
            x, y = M.inputs(kind, shape)
            auto = M.model(x, y)["grad"]
            ana = M.analytic_grad(x, y)
            scale = float(auto.abs().max())
            assert scale > 0 and float((ana - auto).abs().max()) <= 1e-10 * scale, (kind, shape)


def test_maps_recombined_are_the_autograd_gradient_on_the_edge_shapes():
    """`maps()` recombined by `grad_from_maps` (= analytic_grad), against float64 autograd, at the same bound, on the shapes and
    kinds of tests/test_hip_ssim_edges.py.  With ref == img the gradient is 0 analytically and float64 leaves rounding noise on
    both sides: the scale is then that of the "rand" case of the shape."""
    shapes = M.EDGE_SHAPES + M.TILE_SHAPES + ((1, 1) + M.CANVAS_HW,)
    for shape in shapes:
        for kind in M.EDGE_KINDS:
            x, y = M.edge_inputs(kind, shape)
            auto = M.model(x, y)["grad"]
            three = M.maps(x, y)
            assert all(t.shape == auto.shape and t.dtype == torch.float64 for t in three)
            ana = M.grad_from_maps(x, y, three)
            assert torch.equal(ana, M.analytic_grad(x, y))
            scale = float(auto.abs().max()) if kind != "same" else float(M.model(*M.edge_inputs("rand", shape))["grad"].abs().max())
            assert scale > 0 and float((ana - auto).abs().max()) <= 1e-10 * scale, (kind, shape)
    for shape in M.LIMIT_SHAPES:
        x, y = M.edge_inputs("rand", shape)
        auto, ana = M.model(x, y)["grad"], M.analytic_grad(x, y)
        scale = float(auto.abs().max())
        assert scale > 0 and float((ana - auto).abs().max()) <= 1e-10 * scale, shape


def test_the_edge_cases_are_where_they_are_meant_to_be():
    """What makes each case of tests/test_hip_ssim_edges.py a case, from the constants of csrc/ssim.hip: a 32 x 16 tile, 256
    threads in the one-workgroup sum, 128 x 256 threads in the depth sum, an 11-tap window."""
    tiles = [M.tiles_of(s) for s in M.EDGE_SHAPES]
    assert tiles[:3] == [1, 2, 2] and M.tiles_of((1, 1, 16, 32)) == 1
    assert M.tiles_of((2, 2, 37, 53)) == 4 * 3 * 2 and 37 % 2 == 1  # an odd height: the last thread row's second output is outside
    assert all(min(s[2:]) < 11 for s in M.EDGE_SHAPES[3:8])  # smaller than the window
    # the tile loop of the final sum: below, at and past one trip of 256, each plane of the first four a tile of its own
    assert [M.tiles_of(s) for s in M.TILE_SHAPES] == [255, 256, 257, 260, 378]
    assert [M.tiles_of(s) > M.FINAL_THREADS for s in M.TILE_SHAPES] == [False, False, True, True, True]
    assert max(M.tiles_of(s) for s in M.SHAPES) < M.FINAL_THREADS  # (what tests/test_hip_ssim.py reaches)
    # the depth loop: below, at and past one trip, and past two
    assert [n > M.DEPTH_THREADS for n in M.DEPTH_COUNTS] == [False, False, True, True] and M.DEPTH_COUNTS[1] == M.DEPTH_THREADS
    assert M.DEPTH_COUNTS[3] > 2 * M.DEPTH_THREADS
    for n in M.DEPTH_COUNTS:
        for variant in ("ties", "peaks"):
            d, d_obs, special = M.depth_pair(n, variant)
            assert special[-1] == n - 1 and set(special) <= {M.DEPTH_THREADS - 1, M.DEPTH_THREADS, n - 1}
            gap = (d - d_obs).abs()
            others = torch.ones(n, dtype=torch.bool)
            others[special] = False
            assert bool((gap[others] <= 0.5).all()) and bool((gap[others] > 0).all())
            assert bool((gap[special] == (0.0 if variant == "ties" else 8.0)).all())
    # the limits: accepted by the scratch size, and one more is not
    f = _capi.load().dgr_ssim_scratch_floats
    for V, C_, H, W in M.LIMIT_SHAPES:
        assert f(V, C_, H, W) > 3 * V * C_ * H * W
    assert f(65536, 1, 1, 1) == 0 and f(1, 1, (1 << 20) + 1, 1) == 0 and f(1, 1, 1, (1 << 20) + 1) == 0
    # the tile-phase scene: every column phase of a 32-wide tile, every row phase of a 16-high one; the patch stays 20 pixels
    # (a gradient's 10 + its margin's 10) from the canvas border, so no placement sees the zero padding
    (H, W), (h, w), (oy, ox) = M.CANVAS_HW, M.PATCH_HW, M.PATCH_ORIGIN
    assert {dx for dy, dx in M.PHASES if dy == 0} == set(range(32)) and {dy for dy, dx in M.PHASES if dx == 0} == set(range(16))
    assert len(M.PHASES) == 32 + 15 + 8 == len(set(M.PHASES)) and sum(1 for dy, dx in M.PHASES if dy and dx) == 8
    for dy, dx in M.PHASES:
        assert oy + dy >= 2 * M.MARGIN and ox + dx >= 2 * M.MARGIN
        assert H - (oy + dy + h) >= 2 * M.MARGIN and W - (ox + dx + w) >= 2 * M.MARGIN, (dy, dx)
    img, ref = M.placed(M.CANVAS_HW, M.patch_pair(), oy + 3, ox + 5)
    px, py = M.patch_pair()
    assert img.shape == ref.shape == (1, 1, H, W)
    assert torch.equal(img[0, 0, oy + 3:oy + 3 + h, ox + 5:ox + 5 + w], px) and torch.equal(ref[0, 0, oy + 3:oy + 3 + h, ox + 5:ox + 5 + w], py)
    assert int((img != 0.5).sum()) <= h * w and int((ref != 0.4).sum()) <= h * w and float(img[0, 0, 0, 0]) == 0.5


def test_the_model_shifts_with_the_patch():
    """The premise of the tile-phase test, in the model: moving the patch moves the gradient around it and changes nothing else."""
    (oy, ox), (h, w), m = M.PATCH_ORIGIN, M.PATCH_HW, M.MARGIN
    patch = M.patch_pair()
    base = M.model(*M.placed(M.CANVAS_HW, patch, oy, ox))
    moved = M.model(*M.placed(M.CANVAS_HW, patch, oy + 15, ox + 31))
    a = base["grad"][0, 0, oy - m:oy + h + m, ox - m:ox + w + m]
    b = moved["grad"][0, 0, oy + 15 - m:oy + 15 + h + m, ox + 31 - m:ox + 31 + w + m]
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
    assert abs(float(base["ssim"]) - float(moved["ssim"])) <= 1e-12


def test_the_model_is_3dgs_ssim():
    """Spot values that follow from the definition: identical images give 1; the window sums to 1 and is symmetric."""
    g = M.window_1d().double()
    assert abs(float(g.sum()) - 1) < 1e-7 and torch.equal(g, g.flip(0)) and float(g[5]) == float(g.max())
    x, _ = M.inputs("rand", (1, 3, 17, 33))
    assert abs(float(M.model(x, x)["ssim"]) - 1) < 1e-12
    x, y = M.inputs("rand", (2, 3, 17, 33))
    per_view = [float(M.model(x[k], y[k])["ssim"]) for k in range(2)]
    assert abs(float(M.model(x, y)["ssim"]) - sum(per_view) / 2) < 1e-12
