"""The masked-loss entry points (include/dgr_hip.h: dgr_masked_loss_*) and their Python surface without a GPU: declared, exported
and bound; the scratch size; every argument error refused with a message before any device call; and the gradient formula of the
CPU model (tests/masked_loss_model.py), which the GPU tests compare the backward kernel with, pinned against float64 autograd."""
import ctypes as C

import pytest
import torch

from dgr_amd import _capi, slam

import masked_loss_model as M
from abi_checks import FAKE, assert_entry_points, refused

NAMES = ("dgr_masked_loss_scratch_bytes", "dgr_masked_loss_forward", "dgr_masked_loss_backward")
NAN, INF = float("nan"), float("inf")


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_masked_loss_forward": 14, "dgr_masked_loss_backward": 16})
    assert _capi._SIGS["dgr_masked_loss_scratch_bytes"][0] is C.c_size_t
    assert C.sizeof(_capi.MaskedLossParams) == 36
    assert hasattr(slam, "masked_l1_loss") and slam.MaskedLossStats._fields == ("mask", "median", "base", "kept")


def test_scratch_size():
    f = _capi.load().dgr_masked_loss_scratch_bytes
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -8), (65536, 8, 8), (1, 1 << 15, (1 << 15) + 1),
                (1, 1 << 20, 1 << 20)):
        assert f(*bad) == 0, bad
    assert f(65535, 1, 1) > 0 and f(1, 1 << 15, 1 << 15) > 0
    for V, H, W in ((1, 1, 1), (3, 33, 65), (1, 480, 640), (4, 1080, 1920)):
        n = V * H * W
        # the stats, three 2048-bin histograms per view, the mask bytes, and partial sums that stay a small share
        assert f(V, H, W) % 16 == 0 and n + 3 * 2048 * 4 * V < f(V, H, W) <= n + n // 16 + (3 * 2048 * 4 + 64) * V + 256
    base = (2, 40, 70)
    for dim in range(3):  # monotone in each dimension: never smaller, and larger across 16 pixels (the mask bytes are padded to 16)
        sizes = []
        for v in (1, 2, 16, 17, 32, 33, 100, 5000):
            shape = list(base)
            shape[dim] = v
            sizes.append(f(*shape))
        assert all(b > a for a, b in zip(sizes, sizes[1:])), (dim, sizes)
    assert f(1, 1, 1) <= f(1, 1, 2) <= f(1, 1, 17) and f(1, 1, 1) < f(1, 1, 17)


def _params(lo=0.0, hi=INF, sil=0.99, factor=10.0, reject=1, mask_color=1, reduction=0, w_color=1.0, w_depth=0.5):
    return _capi.MaskedLossParams(lo, hi, sil, factor, reject, mask_color, reduction, w_color, w_depth)


def _forward(shape=(1, 3, 8, 8), color=FAKE, color_obs=FAKE, depth=FAKE, depth_obs=FAKE, params=True, scratch=FAKE, loss=FAKE, **p):
    return _capi.load().dgr_masked_loss_forward(None, *shape, color, color_obs, depth, depth_obs, None, None,
                                                _params(**p) if params else None, scratch, loss)


def _backward(shape=(1, 3, 8, 8), color=FAKE, color_obs=FAKE, depth=FAKE, depth_obs=FAKE, params=True, scratch=FAKE, dcolor=FAKE,
              ddepth=FAKE, **p):
    return _capi.load().dgr_masked_loss_backward(None, *shape, color, color_obs, depth, depth_obs, None, None,
                                                 _params(**p) if params else None, scratch, None, dcolor, ddepth)


CASES = [
    (dict(color=None), "color or color_obs is NULL"),
    (dict(color_obs=None), "color or color_obs is NULL"),
    (dict(depth=None), "depth or depth_obs is NULL"),
    (dict(depth_obs=None), "depth or depth_obs is NULL"),
    (dict(params=False), "params is NULL"),
    (dict(scratch=None), "scratch is NULL"),
    (dict(scratch=FAKE + 4), "16-byte aligned"),
    (dict(shape=(0, 3, 8, 8)), "must be positive"),
    (dict(shape=(1, 0, 8, 8)), "must be positive"),
    (dict(shape=(1, 3, -1, 8)), "must be positive"),
    (dict(shape=(1, 3, 8, 0)), "must be positive"),
    (dict(shape=(65536, 3, 8, 8)), "at most 65535"),
    (dict(shape=(1, 3, 1 << 16, 1 << 16)), "at most 2^30"),
    (dict(lo=NAN), "depth_lo or depth_hi is NaN"),
    (dict(hi=NAN), "depth_lo or depth_hi is NaN"),
    (dict(sil=NAN), "silhouette_threshold is NaN"),
    (dict(factor=NAN), "outlier_factor is NaN"),
    (dict(factor=NAN, reject=0), "outlier_factor is NaN"),
    (dict(factor=-1.0), "outlier_factor is negative"),
    (dict(reduction=2), "unknown reduction"),
    (dict(reduction=-1), "unknown reduction"),
]
IDS = ["color-null", "color_obs-null", "depth-null", "depth_obs-null", "params-null", "scratch-null", "scratch-misaligned", "V=0",
       "C=0", "H<0", "W=0", "V-too-large", "HW-too-large", "lo-nan", "hi-nan", "threshold-nan", "factor-nan", "factor-nan-unused",
       "factor-negative", "reduction=2", "reduction<0"]


@pytest.mark.parametrize("case, text", CASES, ids=IDS)
def test_forward_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_forward(**case), "dgr_masked_loss_forward", text)


@pytest.mark.parametrize("case, text", CASES, ids=IDS)
def test_backward_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_backward(**case), "dgr_masked_loss_backward", text)


def test_null_outputs_are_refused():
    refused(_forward(loss=None), "dgr_masked_loss_forward", "loss is NULL")
    refused(_backward(dcolor=None, ddepth=None), "dgr_masked_loss_backward", "both NULL")


def test_python_surface_refuses_what_it_cannot_read():
    """Every check runs on the host, the device check last: CPU tensors reach each of them and never the library."""
    r = torch.rand
    c, d = r(3, 8, 8), r(1, 8, 8)
    f = slam.masked_l1_loss
    with pytest.raises(ValueError, match="GPU tensors"):
        f(c, d, c, d)
    with pytest.raises(ValueError, match="GPU tensors"):
        f(c[None], d[None], c[None], d[None], d[None], torch.ones(1, 1, 8, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match="GPU tensors"):
        f(c, d[0], c, d[0], d[0], torch.ones(8, 8, dtype=torch.uint8), outlier_factor=None, reduction="mean", mask_color=False)
    with pytest.raises(ValueError, match="float32"):
        f(c.double(), d, c.double(), d)
    with pytest.raises(ValueError, match="float32"):
        f(c, d, c, d.half())
    with pytest.raises(ValueError, match="must be a tensor"):
        f(c, d, c, None)
    with pytest.raises(ValueError, match="differ in shape"):
        f(c, d, r(3, 8, 9), d)
    with pytest.raises(ValueError, match="differ in shape"):
        f(c, d, c, r(1, 8, 7))
    with pytest.raises(ValueError, match=r"\[C,H,W\] or \[V,C,H,W\]"):
        f(r(8, 8), d, r(8, 8), d)
    for bad_depth in (r(1, 8, 9), r(2, 8, 8), r(1, 1, 8, 8), r(64)):
        with pytest.raises(ValueError, match="does not match color"):
            f(c, bad_depth, c, bad_depth)
    with pytest.raises(ValueError, match="does not match color"):
        f(c[None], d, c[None], d)
    for bad in (r(1, 8, 9), r(3, 8, 8), r(1, 1, 8, 8)):
        with pytest.raises(ValueError, match="opacity_map .* does not have the depth's shape"):
            f(c, d, c, d, bad)
    with pytest.raises(ValueError, match="opacity_map must be a float32 tensor"):
        f(c, d, c, d, d.double())
    with pytest.raises(ValueError, match="mask must be a uint8 or bool tensor"):
        f(c, d, c, d, None, d)
    with pytest.raises(ValueError, match="mask .* does not have the depth's pixel shape"):
        f(c, d, c, d, None, torch.ones(1, 8, 9, dtype=torch.bool))
    for bad in ("max", "none", None, 1):
        with pytest.raises(ValueError, match="reduction must be 'sum' or 'mean'"):
            f(c, d, c, d, reduction=bad)
    for kw in (dict(outlier_factor=NAN), dict(outlier_factor=-1.0), dict(depth_range=(NAN, 1.0)), dict(silhouette_threshold=NAN)):
        with pytest.raises(ValueError, match="must not be NaN"):
            f(c, d, c, d, **kw)


def test_model_gradient_is_the_autograd_gradient():
    """The formula the backward kernel implements (w / N sign(.) [K]) against float64 autograd of the model's own loss with the
    mask held fixed, for both reductions and both colour forms."""
    for family in M.FAMILIES:
        for shape in M.SHAPES[:5]:
            x = M.inputs(family, shape)
            for kw in (dict(), dict(reduction="mean"), dict(mask_color=False, reduction="mean", w_color=0.7, w_depth=1.3)):
                m = M.model(**x, **kw)
                # (where depth is NaN the model's gradient is 0 -- the pixel is outside K -- and autograd's is NaN times 0)
                dc, dd = M.autograd_grads(x["color"], torch.nan_to_num(x["depth"], nan=0.0, posinf=1e30, neginf=-1e30),
                                          x["color_obs"], x["depth_obs"], m["mask"], **kw)
                assert torch.allclose(dc, m["dcolor"], rtol=1e-14, atol=0) and torch.allclose(dd, m["ddepth"], rtol=1e-14, atol=0), \
                    (family, shape, kw)


def test_the_model_follows_the_definition():
    """Spot values that follow from the header's definition."""
    one = lambda v: torch.full((1, 1, 1, 1), v)
    c = torch.zeros(1, 3, 1, 1)
    m = M.model(c + 0.5, one(1.25), c, one(1.0), w_color=1.0, w_depth=1.0)
    assert float(m["loss"]) == 1.75 and m["median"].tolist() == [0.25] and m["base"].tolist() == m["kept"].tolist() == [1]
    m = M.model(c + 0.5, one(1.25), c, one(0.0))  # a hole: nothing kept, the colour term masked away with it
    assert float(m["loss"]) == 0.0 and m["median"].tolist() == [0.0] and m["base"].tolist() == [0]
    m = M.model(c + 0.5, one(1.25), c, one(0.0), mask_color=False, reduction="mean")
    assert float(m["loss"]) == 0.5
    # the lower median of an even count, and <= at a zero median
    d_obs = torch.ones(1, 1, 1, 4)
    d = d_obs + torch.tensor([0.0, 0.25, 0.5, 4.0]).view(1, 1, 1, 4)
    m = M.model(torch.zeros(1, 1, 1, 4), d, torch.zeros(1, 1, 1, 4), d_obs, outlier_factor=2.0)
    assert m["median"].tolist() == [0.25] and m["kept"].tolist() == [3] and m["mask"].view(-1).tolist() == [True, True, True, False]
    m = M.model(torch.zeros(1, 1, 1, 4), d_obs, torch.zeros(1, 1, 1, 4), d_obs, outlier_factor=0.0)
    assert m["median"].tolist() == [0.0] and m["kept"].tolist() == [4]
    x = M.inputs("dyadic", (1, 3, 480, 640))
    m = M.model(**x, w_color=1.0, w_depth=1.0)
    assert float(m["loss"].float()) == float(m["loss"]) and 0 < int(m["kept"][0]) < int(m["base"][0])  # exact in fp32
    assert int(M.model(**M.inputs("random", (3, 3, 33, 65)))["base"][1]) == 0
