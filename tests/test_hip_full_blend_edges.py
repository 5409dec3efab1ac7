"""The full variant's blend kernels (csrc/render_full.hip) at the edges of their batch loops.

The forward stages a tile's list 256 positions at a time: it blends the terminating Gaussian before the pixel stops, keeps final_T,
n_valid, n_contrib and first_contrib (absolute, 1-based), flushes an earlier batch's tag bytes as a full batch and the last one's
up to the list's end, zeroes the never-staged tail and sums num_related through a status word.  The backward stages 128 positions
(64 under deterministic_grads) from min(range, the tile's last contributor) towards the front: it carries T and three recurrences
across batches, finds the pixel's front-most contributor by its position relative to the batch (its three sums reach dL_dview
alone), cuts each pixel at its own last contributor and pairs neighbouring entries of different halves of a quadrant.

The scenes (tests/full_blend_scenes.py; tests/test_full_blend_scenes.py checks on the CPU that they are what they claim): one tile
with exactly 128 / 129 / 256 / 257 / 512 entries, one tile whose right half meets its first contributor beyond position 128 (and
beyond 256 in a second variant) while its left half ends before 256, a ragged 70x41 frame, an opaque 48x48 frame whose tiles
finish early.  Each on both lane mappings.

Forward: the integer state, final_T, uncertainty and num_related are the oracle's bits, first_contrib the float64 model's, colour
and depth within 1e-6 max(1, |ref|); every tag byte is written; a second forward into the same buffers gives the same bits.
Backward: judged as tests/ref_parity.py judges, with the oracle in the reference's seat -- e_hip <= max(2 e_oracle, 1e-5) per
tensor, distances to the float64 model (fp64_model.torch_full) relative to the tensor's largest value, no element and no row left
out (the float oracle and the C-math oracle decide every pixel of these scenes alike); dL_dview also element by element.
The measured table: profiles/full_blend_edges/measured.txt.
"""
import numpy as np
import pytest
import torch

import fp64_model as M
import full_blend_scenes as S
import hip_helpers as hh
from hip_helpers import forced_lane_lists as lane_lists  # noqa: F401  (fixtures)
from dgr_amd import _capi
from full_blend_scenes import FWD_BATCH
from ref_parity import BAR_GRAD, BAR_IMAGE, GRADS, SANITY, scale_distance
from test_hip_absgrad import check_against
from test_hip_fwd_blend_edges import assert_every_tag_byte_is_written
from test_hip_live_lists import raw_state

pytestmark = pytest.mark.gpu

ATOMICS_BAR = 2e-5   # of a tensor's largest value: the same sums in another order of float atomics
ALL = list(S.SCENES)
FRONT = ["exact129", "exact257", "shadowed", "shadowed272"]          # where the front-most pair's sums are judged on their own
DETERMINISTIC = ["exact129", "exact257", "shadowed", "shadowed272", "opaque"]
EXTRAS = ["exact257", "shadowed"]                                     # absgrad and silhouette
LISTS = {0: " (h)", 1: " (q)"}                                        # the lane mapping in the printed table: half-wave / quadrant lists


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------ forward
STATE = ("ranges", "point_list", "n_contrib", "n_valid", "first_contrib", "final_T")


def forward_state(s, d):
    out = {k: hh.hip_state(k, s, d) for k in STATE}
    out["half_tags"] = raw_state("half_tags", s, d, d["num_rendered"], np.uint8)
    for k in ("num_rendered", "num_related", "color", "depth", "uncertainty", "radii"):
        out[k] = d[k]
    return out


def presized_forward(s, deg, capacity, bufs=None):
    """dgr_full_forward_presized into caller-owned buffers (`bufs`: an earlier call's, reused as they are -- nothing cleared);
    returns (the dict hip_full_forward returns, bufs)"""
    lib, dev = _capi.load(), hh.dev()
    P, W, H = s.P, s.W, s.H
    if bufs is None:
        u8 = dict(dtype=torch.uint8, device=dev)
        bufs = dict(geom=torch.empty(lib.dgr_geometry_bytes(P), **u8), binning=torch.empty(lib.dgr_binning_bytes(capacity, W, H), **u8),
                    img=torch.empty(lib.dgr_image_bytes(W, H), **u8), status=torch.full((4,), -7, dtype=torch.int32, device=dev),
                    color=torch.empty((3, H, W), device=dev), depth=torch.empty((1, H, W), device=dev),
                    uncertainty=torch.empty((1, H, W), device=dev), radii=torch.empty(P, dtype=torch.int32, device=dev))
    inp = [hh.T(a) for a in (s.bg, s.means, s.shs, s.opac, s.scales, s.rots, s.view, s.proj, s.campos, s.gt)]
    bg, means, shs, opac, scales, rots, view, proj, campos, gt = (t.data_ptr() for t in inp)
    p = _capi.ptr
    rc = lib.dgr_full_forward_presized(_capi.stream_handle(), p(bufs["geom"]), p(bufs["binning"]), capacity, p(bufs["img"]), p(bufs["status"]),
                                       P, deg, s.shs.shape[1], bg, W, H, means, shs, None, opac, scales, 1.0, rots, None, view, proj, campos,
                                       s.tanfovx, s.tanfovy, 0, p(bufs["color"]), p(bufs["depth"]), gt, p(bufs["uncertainty"]), p(bufs["radii"]))
    assert rc == 0, _capi.last_error()
    torch.cuda.synchronize()
    status = bufs["status"].tolist()
    assert status[1] == 0 and status[2] == 0, status
    d = dict(num_rendered=status[0], num_related=status[3], geom=bufs["geom"], binning=bufs["binning"], img=bufs["img"])
    d.update({k: bufs[k].cpu().numpy() for k in ("color", "depth", "uncertainty", "radii")})
    return d, bufs


@pytest.mark.parametrize("name", ALL)
def test_forward(oracle, lane_lists, name):
    s, deg = S.scene(name)
    st, ref = S.oracle_full_forward(oracle, name)
    model = S.references(oracle, name)[3]
    _, d = hh.hip_full_forward(s, deg)
    got = forward_state(s, d)
    assert got["num_rendered"] == ref["num_rendered"] and got["num_related"] == ref["num_related"]
    assert np.array_equal(got["radii"], ref["radii"])
    for k, mine in (("ranges", "ranges"), ("point_list", "point_list"), ("n_contrib", "n_contrib"), ("n_valid_contrib", "n_valid")):
        assert np.array_equal(got[mine], st.get(k)), k
    assert np.array_equal(bits(got["final_T"].view(np.float32)), bits(st.get("final_T")))
    assert np.array_equal(bits(got["uncertainty"]), bits(ref["uncertainty"]))
    assert np.array_equal(got["first_contrib"].reshape(s.H, s.W), model["first_contrib"])
    assert np.array_equal(got["n_valid"].reshape(s.H, s.W), model["n_valid"])
    for k in ("color", "depth"):
        a, b = got[k].astype(np.float64), ref[k].astype(np.float64)
        err = float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
        print(f"{name + LISTS[lane_lists]:<16} forward {k:<6} max |hip - oracle| / max(1, |oracle|) = {err:.2e}")
        assert a.shape == b.shape and err <= BAR_IMAGE, k
    # tag bytes: every list entry's byte is written; behind the last walked forward batch they are zero
    ranges = got["ranges"].reshape(-1, 2).astype(np.int64)
    tags = got["half_tags"]
    assert_every_tag_byte_is_written(s, d, tags, ranges)
    if name == "opaque":
        last = S.tile_max(s, got["n_contrib"].reshape(s.H, s.W)).reshape(-1)
        early = 0
        for tile, (lo, hi) in enumerate(ranges):
            walked = FWD_BATCH * -(-int(last[tile]) // FWD_BATCH)
            if hi - lo > walked:
                early += 1
                assert not tags[lo + walked:hi].any(), tile
        assert early > 0
    # twice into the same buffers (nothing cleared in between; the status words start as garbage): the same bits, and
    # num_related is this frame's, not the sum of two
    one, bufs = presized_forward(s, deg, ref["num_rendered"])
    first = forward_state(s, one)
    two, _ = presized_forward(s, deg, ref["num_rendered"], bufs)
    second = forward_state(s, two)
    for k, v in got.items():
        for other in (first, second):
            assert np.array_equal(np.asarray(v), np.asarray(other[k])), k


# ------------------------------------------------------------------------------------------ backward
def hip_grads(s, deg, out, grads, lean=False, **kw):
    gC, gD, gU = grads
    g = hh.hip_full_backward_raw(s, deg, out, grads=(gC, gD, None if lean else gU), **kw)
    torch.cuda.synchronize()
    d = {n: v.cpu().numpy() for n, v in zip(hh.GRAD_NAMES, g[:9])}
    assert d["dL_dview"].shape == (4, 4) and not d["dL_dview"].reshape(-1)[[3, 7, 11, 15]].any()
    if len(g) > 9:
        d["absgrad"] = g[9].cpu().numpy()
    return d


def judge(case, g_hip, g_or, g64, only=None, extra_abs=None):
    """Per tensor of ref_parity.GRADS the float64 model has: e_hip <= max(2 e_oracle, BAR_GRAD), every element counted.  A tensor
    whose float64 gradient is all zero is all zero on both sides.  dL_dview also element by element:
    |hip - fp64| <= 1e-5 max |fp64| + 2 |oracle - fp64|.  `extra_abs` {tensor: absolute error of the oracle}: stands in for
    e_oracle where the oracle cannot run the form (see test_silhouette)."""
    failures = []
    for k in GRADS:
        if k not in g64 or (only is not None and k not in only):
            continue
        b = np.asarray(g64[k], np.float64)
        a = np.asarray(g_hip[k], np.float64).reshape(b.shape)
        scale = float(np.abs(b).max())
        if scale == 0.0:
            assert not a.any() and (g_or is None or not np.asarray(g_or[k]).any()), f"{case} {k}: not zero where float64 is"
            print(f"{case:<40} {k:<14} all zero")
            continue
        e_hip = scale_distance(a, b)
        if g_or is not None:
            o = np.asarray(g_or[k], np.float64).reshape(b.shape)
            e_or = scale_distance(o, b)
        else:
            e_or = float(extra_abs[k]) / scale
        print(f"{case:<40} {k:<14} e_oracle {e_or:9.2e}  e_hip {e_hip:9.2e}")
        assert e_or <= SANITY, f"{case} {k}: the oracle is {e_or:.2e} from the float64 model"
        if e_hip > max(2.0 * e_or, BAR_GRAD):
            failures.append(f"{case} {k}: e_hip {e_hip:.2e}, e_oracle {e_or:.2e}, bar {BAR_GRAD:.0e}")
        if k == "dL_dview" and g_or is not None:
            room = BAR_GRAD * scale + 2.0 * np.abs(o - b)
            worst = float((np.abs(a - b) - room).max())
            print(f"{case:<40} {'dL_dview/elem':<14} max (|hip - fp64| - room) / scale {worst / scale:9.2e}")
            if worst > 0:
                failures.append(f"{case} dL_dview: an element is {worst / scale:.2e} of scale beyond 1e-5 max|ref| + 2 |oracle - fp64|")
    assert not failures, "; ".join(failures)


def atomics_equal(case, a, b, names=hh.GRAD_NAMES):
    """two calls that compute the same sums: within ATOMICS_BAR of each tensor's largest value"""
    for k in names:
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        scale = float(np.abs(y).max())
        if scale == 0.0:
            assert not x.any(), f"{case} {k}"
            continue
        err = float(np.abs(x - y).max()) / scale
        print(f"{case:<40} {k:<14} max |a - b| / max |b| {err:9.2e}")
        assert err <= ATOMICS_BAR, f"{case} {k}: {err:.2e}"


def forward_on_the_oracles_decisions(oracle, name, cmath=False):
    s, deg = S.scene(name)
    st, ref = S.oracle_full_forward(oracle, name, cmath)
    out, d = hh.hip_full_forward(s, deg)
    assert np.array_equal(d["radii"], ref["radii"]) and d["num_rendered"] == ref["num_rendered"]
    assert np.array_equal(hh.hip_state("point_list", s, d), st.get("point_list"))
    assert np.array_equal(hh.hip_state("n_contrib", s, d), st.get("n_contrib"))
    assert np.array_equal(hh.hip_state("n_valid", s, d), st.get("n_valid_contrib"))
    return s, deg, out


@pytest.mark.parametrize("name", ALL)
def test_backward_default(oracle, lane_lists, name):
    s, deg, out = forward_on_the_oracles_decisions(oracle, name)
    grads, g_or, g64, _ = S.references(oracle, name, "default")
    judge(f"{name} default{LISTS[lane_lists]}", hip_grads(s, deg, out, grads), g_or, g64)


@pytest.mark.parametrize("name", ALL)
def test_backward_lean(oracle, lane_lists, name):
    s, deg, out = forward_on_the_oracles_decisions(oracle, name)
    grads, g_or, g64, _ = S.references(oracle, name, "lean")
    lean = hip_grads(s, deg, out, grads, lean=True)
    zero = hip_grads(s, deg, out, grads)   # (an explicit all-zero uncertainty gradient)
    assert not grads[2].any()
    atomics_equal(f"{name} lean vs zero image{LISTS[lane_lists]}", lean, zero)
    judge(f"{name} lean{LISTS[lane_lists]}", lean, g_or, g64)


@pytest.mark.parametrize("name", FRONT)
def test_backward_depth_only(oracle, lane_lists, name):
    """gC = 0 and no uncertainty gradient: the front-most pair's sums are the only pose terms"""
    s, deg, out = forward_on_the_oracles_decisions(oracle, name)
    grads, g_or, g64, _ = S.references(oracle, name, "depth")
    assert not grads[0].any() and np.abs(g64["dL_dview"]).max() > 0
    judge(f"{name} depth only{LISTS[lane_lists]}", hip_grads(s, deg, out, grads, lean=True), g_or, g64)


@pytest.mark.parametrize("name", DETERMINISTIC)
def test_backward_deterministic(oracle, lane_lists, name):
    grads, g_or, g64, _ = S.references(oracle, name, "default")
    with _capi.thread_options(deterministic_grads=1):
        s, deg, out = forward_on_the_oracles_decisions(oracle, name)
        a = hip_grads(s, deg, out, grads)
        b = hip_grads(s, deg, out, grads)
    for k in hh.GRAD_NAMES:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    judge(f"{name} deterministic{LISTS[lane_lists]}", a, g_or, g64)


@pytest.mark.parametrize("name", EXTRAS)
def test_absgrad(oracle, lane_lists, name):
    s, deg, out = forward_on_the_oracles_decisions(oracle, name)
    st, ref = S.oracle_full_forward(oracle, name)
    grads, g_or, g64, _ = S.references(oracle, name, "default")
    plain = hip_grads(s, deg, out, grads)
    ab = hip_grads(s, deg, out, grads, absgrad=True)
    atomics_equal(f"{name} absgrad vs plain{LISTS[lane_lists]}", ab, plain)
    pairs = []
    loss, _, img = M.torch_full(s, deg, ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"),
                                tuple(np.asarray(g, np.float64) for g in grads), pairs=pairs)
    loss.backward()
    want = M.absgrad_of_pairs(pairs, img["_idx"], s.P, s.W, s.H)
    assert ab["absgrad"].shape == (s.P, 3)
    check_against(ab["absgrad"], want, ref["radii"], f"{name} absgrad")


def silhouette_grads64(oracle, name, gA):
    """float64 gradients of sum gA * (1 - T_final), the exact silhouette term: the colour loss of a second call with colour 0
    everywhere (SH degree 0: C0 sh_0 + 1/2 = 0), background (1, 0, 0) and colour gradient (-gA, 0, 0) -- same decisions, same
    leaves (tests/test_hip_silhouette.py).  No SH gradient (the fake colours') and no pose gradient: with the reference's pose
    gradient (pose_grad = 0) no background share reaches dL_dview (include/dgr_hip.h)."""
    s, deg = S.scene(name)
    assert deg == 0
    st, ref = S.oracle_full_forward(oracle, name)
    zero = np.zeros((s.H, s.W))
    sh0 = np.zeros_like(np.asarray(s.shs, np.float64))
    sh0[:, 0, :] = -0.5 / M.C0
    s2 = s._replace(bg=np.array([1.0, 0.0, 0.0], np.float32), shs=sh0)
    g, _ = S.grads64(s2, deg, st, ref, (np.stack([-np.asarray(gA, np.float64), zero, zero]), zero, zero))
    assert np.abs(g["dL_dview"]).max() <= 1e-12 * np.abs(g["dL_dmeans3D"]).max()
    g["dL_dsh"] = np.zeros_like(g["dL_dsh"])
    g["dL_dview"] = np.zeros((4, 4))
    return g


@pytest.mark.parametrize("name", EXTRAS)
def test_silhouette(oracle, lane_lists, name):
    """A silhouette image on top of the default form.  The oracle has no silhouette term: the image enters the kernel through one
    per-pixel constant (bg_term), every sum is the default form's, so the oracle's ABSOLUTE error on the default form stands in
    for e_oracle."""
    s, deg, out = forward_on_the_oracles_decisions(oracle, name)
    grads, g_or, g64, _ = S.references(oracle, name, "default")
    gA = (np.random.default_rng(3).normal(0.0, 1.0, (s.H, s.W)) / (s.W * s.H) ** 0.5).astype(np.float32)
    extra = silhouette_grads64(oracle, name, gA)
    both = {k: g64[k] + extra[k] for k in g64}
    err_or = {k: float(np.abs(np.asarray(g_or[k], np.float64).reshape(g64[k].shape) - g64[k]).max()) for k in g64}
    got = hip_grads(s, deg, out, grads, silhouette=gA)
    assert scale_distance(got["dL_dmeans3D"], g64["dL_dmeans3D"]) > 1e-3   # (the image does reach the gradients)
    judge(f"{name} default + silhouette{LISTS[lane_lists]}", got, None, both, extra_abs=err_or)


@pytest.mark.parametrize("alpha_mode", [1, 2])
def test_lean_call_equals_the_zero_image_call_in_the_other_alpha_modes(oracle, lane_lists, alpha_mode):
    """launch_render_bwd_full has no lean instance for alpha_mode 1 and 2: a NULL image reads as zero there.  Mode 2 (glibc's expf
    restated) is also judged, against the C-math oracle and the float64 model on its decisions."""
    name = "exact257"
    s, deg = S.scene(name)
    grads = S.pixel_grads(name, "lean")
    with _capi.thread_options(alpha_mode=alpha_mode):
        if alpha_mode == 2:
            s, deg, out = forward_on_the_oracles_decisions(oracle, name, cmath=True)
        else:
            out, _ = hh.hip_full_forward(s, deg)
        lean = hip_grads(s, deg, out, grads, lean=True)
        zero = hip_grads(s, deg, out, grads)
    atomics_equal(f"{name} alpha_mode {alpha_mode} lean vs zero{LISTS[lane_lists]}", lean, zero)
    if alpha_mode == 2:
        _, g_or, g64, _ = S.references(oracle, name, "lean", cmath=True)
        judge(f"{name} alpha_mode 2 lean{LISTS[lane_lists]}", lean, g_or, g64)
