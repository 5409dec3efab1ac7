"""The contribution-statistics entry points (include/dgr_hip.h: dgr_contribution_scratch_bytes, dgr_contribution_stats) and their
Python surface without a GPU: declared, exported and bound; the params struct's layout against the header text; the scratch
size; every argument error refused with a message before any device call; the keyword-only arguments and the ValueErrors of the
Python side."""
import ctypes as C
import re

import pytest
import torch

from dgr_amd import _capi, contrib, slam

from abi_checks import FAKE, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_contribution_scratch_bytes", "dgr_contribution_stats")
NAN = float("nan")
FIELDS = [("min_pixels", "int"), ("weight_min", "float"), ("frame_id", "int")]


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_contribution_scratch_bytes": 1, "dgr_contribution_stats": 19})
    assert _capi._SIGS["dgr_contribution_scratch_bytes"][0] is C.c_size_t


def test_params_struct_matches_the_header_text():
    body = header_text().split("} dgr_contribution_params;")[0].rsplit("typedef struct dgr_contribution_params {", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == FIELDS
    P = _capi.ContributionParams
    assert [(n, {C.c_float: "float", C.c_int: "int"}[t]) for n, t in P._fields_] == fields
    assert C.sizeof(P) == 12 and [getattr(P, n).offset for n, _ in fields] == [0, 4, 8]


def test_the_header_states_the_semantics():
    text = header_text()
    doc = text[text.index("per-Gaussian contribution statistics"):text.index("typedef struct dgr_contribution_params")]
    for word in ("n_contrib", "power <= 0", "15/255", "floor(w 2^32)", "min_pixels", "weight_min", "frame_id", "overflowed",
                 "three launches", "hipGraph", "alpha_mode"):
        assert word in doc, word


def test_scratch_size():
    f = _capi.load().dgr_contribution_scratch_bytes
    for bad in (-1, 1 << 28, 1 << 40):
        assert f(bad) == 0, bad
    last = 0
    for P in (0, 1, 63, 64, 65, 1000, 100000, (1 << 28) - 1):
        n = f(P)
        # an int32, a float32 and an int64 per Gaussian, each plane aligned; a loose upper bound against a runaway layout
        assert n % 16 == 0 and 16 * P <= n <= 16 * P + 2048 and n > 0, P
        assert n >= last
        last = n


def _stats(P=100, W=64, H=48, R=500, geom=FAKE, binning=FAKE, img=FAKE, params=True, scratch=FAKE, n_touched=FAKE, max_weight=FAKE,
           sum_weight=FAKE, touched_total=None, max_weight_total=None, sum_weight_total=None, views=None, last_seen=None, counts=FAKE,
           min_pixels=1, weight_min=0.0, frame_id=0):
    p = _capi.ContributionParams(min_pixels, weight_min, frame_id) if params else None
    return _capi.load().dgr_contribution_stats(None, P, W, H, R, geom, binning, img, p, scratch, n_touched, max_weight, sum_weight,
                                               touched_total, max_weight_total, sum_weight_total, views, last_seen, counts)


@pytest.mark.parametrize("case, text", [
    (dict(params=False), "params is NULL"),
    (dict(P=-1), "P must be"), (dict(P=1 << 28), "P must be"),
    (dict(W=0), "width and height"), (dict(H=0), "width and height"), (dict(W=-5), "width and height"), (dict(H=-1), "width and height"),
    (dict(W=1 << 16, H=1 << 15), "width and height"),
    (dict(R=-1), "R is negative"),
    (dict(geom=None), "state buffers"), (dict(binning=None), "state buffers"), (dict(img=None), "state buffers"),
    (dict(min_pixels=-1), "min_pixels is negative"),
    (dict(weight_min=NAN), "weight_min is NaN or negative"), (dict(weight_min=-0.5), "weight_min is NaN or negative"),
    (dict(scratch=None, n_touched=None), "scratch is NULL"), (dict(scratch=None, max_weight=None), "scratch is NULL"),
    (dict(scratch=None, sum_weight=None), "scratch is NULL"),
    (dict(scratch=None, n_touched=None, max_weight=None, sum_weight=None, views=FAKE), "scratch is NULL"),
    (dict(scratch=FAKE + 8), "scratch is not 16-byte aligned"), (dict(scratch=FAKE + 4, n_touched=None), "scratch is not 16-byte aligned"),
    (dict(n_touched=FAKE + 2), "4-byte aligned"), (dict(max_weight=FAKE + 1), "4-byte aligned"), (dict(views=FAKE + 2), "4-byte aligned"),
    (dict(last_seen=FAKE + 3), "4-byte aligned"), (dict(max_weight_total=FAKE + 2), "4-byte aligned"), (dict(counts=FAKE + 2), "4-byte aligned"),
    (dict(sum_weight=FAKE + 4), "8-byte aligned"), (dict(touched_total=FAKE + 4), "8-byte aligned"),
    (dict(sum_weight_total=FAKE + 4), "8-byte aligned"),
    (dict(n_touched=None, max_weight=None, sum_weight=None, counts=None), "nothing to write"),
    (dict(P=0, geom=None, binning=None, img=None, scratch=None, n_touched=None, max_weight=None, sum_weight=None, counts=None),
     "nothing to write"),
    (dict(weight_min=NAN, touched_total=FAKE, max_weight_total=FAKE, sum_weight_total=FAKE, views=FAKE, last_seen=FAKE),
     "weight_min is NaN or negative"),
])
def test_contribution_stats_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_stats(**case), "dgr_contribution_stats", text)


def test_no_gaussians_need_no_state_buffers_and_no_scratch():
    """P = 0: the buffers and the scratch may be NULL; the next refusal is the one asked for"""
    refused(_stats(P=0, geom=None, binning=None, img=None, scratch=None, n_touched=None, max_weight=None, sum_weight=None,
                   min_pixels=-1), "dgr_contribution_stats", "min_pixels is negative")


def test_python_surface():
    keyword_only(slam.contribution_stats, ["geomBuffer", "binningBuffer", "imageBuffer", "P", "H", "W", "R"],
                 dict(into=None, min_pixels=1, weight_min=0.0, frame_id=0))
    keyword_only(slam.render_contributions, ["viewpoint_camera", "pc", "pipe", "bg_color"],
                 dict(scaling_modifier=1.0, override_color=None, gt_depth=None, variant="light", into=None, min_pixels=1,
                      weight_min=0.0, frame_id=0), required=("viewmatrix", "fov", "HW"))
    assert slam.ContributionStats._fields == ("n_touched", "max_weight", "sum_weight", "counts")
    assert slam.contribution_stats is contrib.contribution_stats and slam.render_contributions is contrib.render_contributions
    assert slam.ContributionStats is contrib.ContributionStats and slam.ContributionAccumulator is contrib.ContributionAccumulator


def test_the_accumulator_and_the_q32_view_on_the_host():
    acc = slam.ContributionAccumulator(5, "cpu")
    assert [t.dtype for t in acc.tensors()] == [torch.int64, torch.float32, torch.int64, torch.int32, torch.int32]
    assert all(tuple(t.shape) == (5,) for t in acc.tensors()) and (acc.last_seen == -1).all()
    acc.views += torch.tensor([0, 1, 2, 3, 0], dtype=torch.int32)
    acc.sum_weight_total[1] = 3 << 31
    assert acc.observed().tolist() == [False, True, True, True, False] and acc.observed(3).tolist() == [False, False, False, True, False]
    assert acc.sum_weight_float().tolist() == [0.0, 1.5, 0.0, 0.0, 0.0] and acc.sum_weight_float().dtype == torch.float64
    acc.reset()
    assert not acc.views.any() and not acc.sum_weight_total.any() and (acc.last_seen == -1).all()
    st = slam.ContributionStats(torch.tensor([2], dtype=torch.int32), torch.tensor([0.5]), torch.tensor([1 << 30]), torch.zeros(4, dtype=torch.int32))
    assert st.sum_weight_float().tolist() == [0.25]
    with pytest.raises(ValueError, match="must not be negative"):
        slam.ContributionAccumulator(-1, "cpu")


def test_python_surface_refuses_what_it_cannot_read():
    """Every check runs on the host, the device check last: CPU tensors reach each of them and never the library."""
    f = slam.contribution_stats
    b = torch.zeros(1 << 16, dtype=torch.uint8)
    ok = dict(P=10, H=48, W=64, R=100)
    with pytest.raises(ValueError, match="GPU tensors"):
        f(b, b, b, **ok)
    with pytest.raises(ValueError, match="GPU tensors"):
        f(b, b, b, **ok, into=slam.ContributionAccumulator(10, "cpu"), min_pixels=3, weight_min=0.5, frame_id=4)
    with pytest.raises(ValueError, match="geomBuffer must be a tensor"):
        f(None, b, b, **ok)
    with pytest.raises(ValueError, match="binningBuffer must be a 1-D uint8"):
        f(b, b.float(), b, **ok)
    with pytest.raises(ValueError, match="imageBuffer must be a 1-D uint8"):
        f(b, b, b.reshape(2, -1), **ok)
    for bad in (-1, 1 << 28):
        with pytest.raises(ValueError, match="P must be"):
            f(b, b, b, bad, 48, 64, 100)
    for H, W in ((0, 64), (48, 0), (-1, 64)):
        with pytest.raises(ValueError, match="H and W must be positive"):
            f(b, b, b, 10, H, W, 100)
    with pytest.raises(ValueError, match="R must not be negative"):
        f(b, b, b, 10, 48, 64, -1)
    with pytest.raises(ValueError, match="min_pixels must not be negative"):
        f(b, b, b, **ok, min_pixels=-1)
    with pytest.raises(ValueError, match="weight_min must not be NaN"):
        f(b, b, b, **ok, weight_min=NAN)
    with pytest.raises(ValueError, match="weight_min must not be negative"):
        f(b, b, b, **ok, weight_min=-0.1)
    with pytest.raises(ValueError, match="into must be a ContributionAccumulator"):
        f(b, b, b, **ok, into=torch.zeros(10))
    with pytest.raises(ValueError, match="into holds 11 Gaussians"):
        f(b, b, b, **ok, into=slam.ContributionAccumulator(11, "cpu"))
    with pytest.raises(ValueError, match="unknown variant"):
        slam.render_contributions(None, None, None, None, viewmatrix=torch.eye(4), fov=(1.0, 1.0), HW=(48, 64), variant="dense")
