"""The light forward's live lists and the backward that walks them.

When the forward blend flushes a staged batch it writes the entries somebody blended (tag byte != 0) compacted, in tile-list
order, as {Gaussian id, list position << 8 | tag byte} from the tile's range start on, and the tile's live count into a per-tile
word (csrc/render_common.h: live_list).  The light backward stages from that array alone: a batch is 128 live entries (64 in the
deterministic kernel), and a tile nobody blended returns before its first barrier.

  * the exported list against the exported tag bytes, tile by tile: same positions, ids and tags, in order, and the count;
  * gradients against the oracle at the bars of tests/test_hip_light_parity.py (1e-5 of each tensor's scale, no outlier rows),
    in every backward mode, with a tile of more than 128 live entries (two backward batches) in the frame;
  * deterministic_grads: two runs, the same bits;
  * lazy mode: an overflowed frame is NaN, its backward walks nothing and does not fault.
"""
import numpy as np
import pytest
import torch

from dgr_amd import _capi
from dgr_amd.synth import cluster_scene, heavy_tail_scene
from util import assert_grad_close, make_scene, mask_flipped_pixels
import hip_helpers as hh
from hip_helpers import deterministic, lazy, set_lane_lists as lane_lists  # noqa: F401  (fixtures)
from test_hip_light_parity import GRAD_NAMES, IMAGES, check_backward

pytestmark = pytest.mark.gpu


def raw_state(name, s, d, n, dtype):
    """`n` elements of a state array as dgr_state_export hands them out (names hip_helpers.hip_state has no layout for)"""
    lib = _capi.load()
    tdt = {np.uint8: torch.uint8, np.uint32: torch.int32}[dtype]
    dst = torch.zeros(max(n, 1), dtype=tdt, device=hh.dev())
    got = lib.dgr_state_export(_capi.stream_handle(), name.encode(), s.P, s.W, s.H, d["num_rendered"], hh.binning_capacity(d, s.W, s.H),
                               _capi.ptr(d["geom"]), _capi.ptr(d["binning"]), _capi.ptr(d["img"]), dst.data_ptr())
    assert got >= 0, _capi.last_error()
    torch.cuda.synchronize()
    return dst[:n].cpu().numpy().view(dtype)


def tiles_of(s):
    return ((s.W + 15) // 16) * ((s.H + 15) // 16)


def live_state(s, d):
    R, tiles = d["num_rendered"], tiles_of(s)
    tags = raw_state("half_tags", s, d, R, np.uint8)
    live = raw_state("live_list", s, d, 2 * R, np.uint32).reshape(R, 2)
    counts = raw_state("live_counts", s, d, tiles, np.uint32)
    ranges = hh.hip_state("ranges", s, d).reshape(tiles, 2).astype(np.int64)
    return tags, live, counts, ranges


def assert_live_list_is_the_tagged_entries(s, d):
    """For every tile: the live entries are, in order, the list positions whose tag byte is non-zero, with their id and tag."""
    tags, live, counts, ranges = live_state(s, d)
    plist = hh.hip_state("point_list", s, d)
    assert counts.shape[0] == ranges.shape[0]
    for tile, (lo, hi) in enumerate(ranges):
        pos = np.nonzero(tags[lo:hi])[0]
        n = int(counts[tile])
        assert n == pos.size, (tile, n, pos.size)
        e = live[lo:lo + n]
        assert np.array_equal(e[:, 1] >> 8, pos.astype(np.uint32)), tile
        assert np.array_equal(e[:, 1] & 0xFF, tags[lo:hi][pos].astype(np.uint32)), tile
        assert np.array_equal(e[:, 0], plist[lo:hi][pos]), tile
    return tags, counts, ranges


def opaque_scene(P=3000, W=64, H=48, seed=3):
    """big, nearly opaque splats: every pixel's transmittance falls below 1e-4 after a few entries of lists that are thousands long"""
    s = make_scene(P, W, H, seed)
    return s._replace(scales=(s.scales * 8.0).astype(np.float32), opac=np.full_like(s.opac, 0.99))


def test_small_scene():
    s = make_scene(2000, 64, 48, 1)
    _, d = hh.hip_forward(s, 0)
    tags, counts, ranges = assert_live_list_is_the_tagged_entries(s, d)
    assert counts.sum() > 0 and counts.sum() == np.count_nonzero(tags)


def test_a_list_of_several_forward_batches_and_more_than_one_backward_batch():
    s = make_scene(6000, 64, 48, 2)
    _, d = hh.hip_forward(s, 3)
    tags, counts, ranges = assert_live_list_is_the_tagged_entries(s, d)
    assert (ranges[:, 1] - ranges[:, 0]).max() > 3 * 256  # the running base crosses several flushes
    assert counts.max() > 128                             # ... and the backward stages such a tile in two batches


def test_an_opaque_scene_whose_tiles_finish_early():
    s = opaque_scene()
    _, d = hh.hip_forward(s, 3)
    tags, counts, ranges = assert_live_list_is_the_tagged_entries(s, d)
    nc = hh.hip_state("n_contrib", s, d).reshape(s.H, s.W)
    gx = (s.W + 15) // 16
    early = 0
    for tile, (lo, hi) in enumerate(ranges):
        tx, ty = tile % gx, tile // gx
        last = int(nc[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].max())
        if hi - lo > 256 and last <= 256:  # nothing behind the first forward batch was blended (or even staged)
            early += 1
            assert not tags[lo + 256:hi].any() and counts[tile] <= 256
    assert early > 0


def test_empty_tiles():
    s = make_scene(40, 256, 256, 4)
    _, d = hh.hip_forward(s, 0)
    tags, counts, ranges = assert_live_list_is_the_tagged_entries(s, d)
    empty = ranges[:, 1] == ranges[:, 0]
    assert empty.any() and not counts[empty].any()
    g = hh.hip_backward(s, 0, hh.hip_forward(s, 0)[0])  # (tiles without a live entry return at once)
    assert all(np.isfinite(v).all() for v in g.values())


def test_both_lane_mappings_by_the_frame(lane_lists):
    """a clustered frame of small splats walks half-wave lists, a heavy-tailed one quadrant lists (the frame's own flag)"""
    lane_lists(2)
    flags = []
    for s in (cluster_scene(make_scene(20000, 320, 200, 3)),
              heavy_tail_scene(make_scene(30000, 640, 480, 4), frac=0.05, sigma_px=(10, 200), seed=9)):
        _, d = hh.hip_forward(s, 3)
        assert_live_list_is_the_tagged_entries(s, d)
        flags.append(int(hh.hip_state("sched_flag", s, d)[0] >> 2) & 1)
    assert flags == [0, 1]


@pytest.mark.parametrize("lists", [0, 1])
def test_either_lane_mapping_forced(lane_lists, lists):
    lane_lists(lists)
    s = make_scene(20000, 320, 200, 3)
    _, d = hh.hip_forward(s, 3)
    assert_live_list_is_the_tagged_entries(s, d)


@pytest.fixture
def tight_cull():
    _capi.load()
    _capi.set_option("tight_cull", 1)
    yield
    _capi.set_option("tight_cull", 0)


def test_tight_cull(tight_cull):
    s = make_scene(10000, 256, 256, 0)
    _, d = hh.hip_forward(s, 3)
    assert_live_list_is_the_tagged_entries(s, d)


# ------------------------------------------------------------------------------------------ gradients against the oracle
DENSE = (6000, 64, 48, 3, 2)   # tiles with more than 128 live entries: two backward batches (asserted below)
USUAL = (20000, 320, 200, 3, 0)


def assert_two_backward_batches(s, d):
    counts = raw_state("live_counts", s, d, tiles_of(s), np.uint32)
    assert counts.max() > 128


@pytest.mark.parametrize("case", [DENSE, USUAL])
@pytest.mark.parametrize("mode", [(False, False), (True, False), (False, True)], ids=["mapping+pose", "mapping", "tracking"])
def test_backward_against_the_oracle(oracle, case, mode):
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    d, _, _ = check_backward(oracle, s, deg, track_off=mode[0], map_off=mode[1], what=f"live lists P={P}")
    if case == DENSE:
        assert_two_backward_batches(s, d)


def masked_grads(oracle, s, deg):
    """check_backward's preparation: forward on both sides, pixel gradients of O(1) sums, threshold flips masked"""
    W, H = s.W, s.H
    grads = tuple(g * (W * H) ** 0.5 for g in (s.gC, s.gD, s.gM, s.gV))
    out, d = hh.hip_forward(s, deg)
    st, ref = hh.oracle_forward(oracle, s, deg)
    grads, _ = mask_flipped_pixels(grads, hh.hip_state("n_contrib", s, d), st.get("n_contrib"), W, H, "live lists",
                                   images=[(d[k], ref[k]) for k in IMAGES], median_margin=oracle.light_median_margin(st, ref["opacity_map"]))
    return out, d, st, ref, grads


def assert_gradients(g, gr, label, view=True):
    for k in GRAD_NAMES:
        assert_grad_close(g[k], gr[k], f"{k} [{label}]", rel_to_max=1e-5, elem_rtol=1e-3, elem_frac=1e-4, outlier_rows=0)
    if view:
        assert_grad_close(g["dL_dview"], gr["dL_dview"], f"dL_dview [{label}]", rel_to_max=1e-5, elem_rtol=1e-3, elem_frac=0.0)


@pytest.mark.parametrize("case", [DENSE, USUAL])
@pytest.mark.parametrize("track_off", [False, True])
def test_lean_loss(oracle, case, track_off):
    """no gradient image for the median depth and the variance: the lean kernel, against the oracle fed zero images"""
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    out, d, st, ref, (gC, gD, gM, gV) = masked_grads(oracle, s, deg)
    zero = np.zeros_like(gM)
    gr = hh.oracle_backward(oracle, st, s, deg, ref["opacity_map"], track_off=track_off, grads=(gC, gD, zero, zero))
    g = hh.hip_backward(s, deg, out, track_off=track_off, grads=(gC, gD, None, None), alphas=ref["opacity_map"])
    assert_gradients(g, gr, "lean", view=not track_off)


@pytest.mark.parametrize("case", [DENSE, USUAL])
@pytest.mark.parametrize("lean", [False, True])
def test_absgrad_kernel(oracle, case, lean):
    """the absgrad instances: the ordinary gradients meet the oracle's bars, the absolute sums bound them"""
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    out, d, st, ref, (gC, gD, gM, gV) = masked_grads(oracle, s, deg)
    zero = np.zeros_like(gM)
    gr = hh.oracle_backward(oracle, st, s, deg, ref["opacity_map"], grads=(gC, gD, zero, zero) if lean else (gC, gD, gM, gV))
    raw = hh.hip_backward_raw(s, deg, out, grads=(gC, gD, None, None) if lean else (gC, gD, gM, gV), alphas=ref["opacity_map"], absgrad=True)
    g = {n: v.cpu().numpy() for n, v in zip(hh.GRAD_NAMES, list(raw[:8]) + [torch.sum(raw[8], dim=0)])}
    assert_gradients(g, gr, "absgrad")
    ab = raw[-1].cpu().numpy().astype(np.float64)
    assert ab.shape == g["dL_dmeans2D"].shape
    m = np.abs(g["dL_dmeans2D"][:, :2].astype(np.float64))
    assert np.all(ab[:, :2] >= m - 1e-5 * max(m.max(), 1e-30)) and ab[:, :2].max() > 0


@pytest.mark.parametrize("case", [DENSE, USUAL])
@pytest.mark.parametrize("map_off", [False, True])
def test_silhouette_image(oracle, case, map_off):
    """dL/d(opacity_map) enters the blend backward as the background term does (render_light.hip: SILHOUETTE): a zero background
    with the silhouette image -<bg, dL/dcolour> is the oracle's backward with that background."""
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    out, d, st, ref, grads = masked_grads(oracle, s, deg)
    gr = hh.oracle_backward(oracle, st, s, deg, ref["opacity_map"], map_off=map_off, grads=grads)
    sil = -(s.bg[:, None, None].astype(np.float32) * grads[0]).sum(axis=0).astype(np.float32)
    g = hh.hip_backward(s, deg, out, map_off=map_off, grads=grads, alphas=ref["opacity_map"], bg=np.zeros(3, np.float32), silhouette=sil)
    if map_off:
        assert_grad_close(g["dL_dview"], gr["dL_dview"], "dL_dview [silhouette, tracking]", rel_to_max=1e-5, elem_rtol=1e-3, elem_frac=0.0)
    else:
        assert_gradients(g, gr, "silhouette")


def test_batched_backward(oracle):
    from test_hip_batch import batch_backward, batch_forward, one_view_dict, scenes
    P, W, H, deg, seed, V = 6000, 64, 48, 3, 2, 3
    ss = scenes(P, W, H, V, seed)
    out, cams = batch_forward(ss, deg)
    grads, alphas, ref_sum, ref_view, ref_m2d = [], [], None, [], []
    for v, s in enumerate(ss):
        st, ref = hh.oracle_forward(oracle, s, deg)
        ov = one_view_dict(out, v)
        d = {"color": ov[1].cpu().numpy(), "depth": ov[2].cpu().numpy(), "depth_median": ov[3].cpu().numpy(), "opacity_map": ov[5].cpu().numpy()}
        dv = {"num_rendered": ov[0], "geom": ov[7], "binning": ov[8], "img": ov[9]}
        assert_live_list_is_the_tagged_entries(s, dv)
        assert_two_backward_batches(s, dv)
        g = tuple(x * (W * H) ** 0.5 for x in (s.gC, s.gD, s.gM, s.gV))
        g, _ = mask_flipped_pixels(g, hh.hip_state("n_contrib", s, dv), st.get("n_contrib"), W, H, f"live lists, batch view {v}",
                                   images=[(d[k], ref[k]) for k in IMAGES], median_margin=oracle.light_median_margin(st, ref["opacity_map"]))
        gr = hh.oracle_backward(oracle, st, s, deg, ref["opacity_map"], grads=g)
        grads.append(g)
        alphas.append(ref["opacity_map"])
        ref_view.append(gr["dL_dview"])
        ref_m2d.append(gr["dL_dmeans2D"])
        ref_sum = {k: gr[k].astype(np.float64) + (0.0 if ref_sum is None else ref_sum[k]) for k in gr}
    g = batch_backward(ss, deg, out, cams, grads, alphas=alphas)
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"):
        assert_grad_close(g[k], ref_sum[k].reshape(g[k].shape), k, rel_to_max=1e-5, elem_rtol=1e-3, elem_frac=1e-4, outlier_rows=0)
    for v in range(V):
        assert_grad_close(g["dL_dmeans2D"][v], ref_m2d[v], f"dL_dmeans2D[{v}]", rel_to_max=1e-5, elem_rtol=1e-3, elem_frac=1e-4, outlier_rows=0)
        assert_grad_close(g["dL_dview"][v], ref_view[v], f"dL_dview[{v}]", rel_to_max=1e-5, elem_rtol=1e-3, elem_frac=0.0)


# ------------------------------------------------------------------------------------------ determinism, lazy mode
@pytest.mark.parametrize("case", [DENSE, USUAL])
@pytest.mark.parametrize("mode", [dict(), dict(map_off=True), dict(track_off=True)], ids=["mapping+pose", "tracking", "mapping"])
def test_deterministic_grads_two_runs_the_same_bits(deterministic, oracle, case, mode):
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    out, _ = hh.hip_forward(s, deg)
    a = hh.hip_backward(s, deg, out, **mode)
    b = hh.hip_backward(s, deg, out, **mode)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert any(v.any() for v in a.values())
    check_backward(oracle, s, deg, what="live lists, deterministic", **mode)  # (the 64-entry batches of the deterministic kernel)


def forget(L, key):
    for d in (L._capacity_cache, L._last_status, L._unsettled):
        d.pop(key, None)


def test_an_overflowed_lazy_frame_is_nan_and_its_backward_walks_nothing(lazy):
    """A lazy forward whose binning buffer is too small leaves every tile list empty: NaN images (never a plausible empty frame),
    no live entry anywhere -- the backward over that state returns at once, adds nothing and does not fault -- and the overflow
    is raised before the optimizer step.  (The sequence of tests/test_hip_lazy_safety.py.)"""
    L = lazy
    from dgr_amd.multiview import make_settings

    def leaves(s, scale=1.0):
        return [hh.T(a).requires_grad_() for a in (s.means, s.shs, s.opac, s.scales * np.float32(scale), s.rots, s.view)]

    def step(rast, lv, s):
        m2 = torch.zeros((s.P, 3), device=hh.dev(), requires_grad=True)
        o = rast(means3D=lv[0], means2D=m2, opacities=lv[2], shs=lv[1], scales=lv[3], rotations=lv[4], viewmatrix=lv[5], gt_depth=hh.T(s.gt))
        torch.autograd.backward([o[0], o[2], o[3], o[4]], [hh.T(s.gC), hh.T(s.gD[None]), hh.T(s.gM[None]), hh.T(s.gV[None])])
        return o

    # A shape of this test's own, forgotten before and after: the capacity a shape has learned lives in the module, keyed by
    # (device, P, H, W), and only grows -- behind another test that enlarged the same shape the big frame below would simply fit.
    # (3x the splats: 42 475 instances against the 1.5 * 13 510 + 4096 a lazy forward sizes its buffer with.)
    s = make_scene(4100, 104, 72, 13)
    key = (hh.dev().index, s.P, s.H, s.W)
    forget(L, key)
    try:
        rast = L.GaussianRasterizer(make_settings(s, 3, hh.dev()))
        for _ in range(3):                                   # the first call is strict and teaches the capacity; then lazy
            o = step(rast, leaves(s), s)
        L.check_async_errors()
        assert key not in L._unsettled and torch.isfinite(o[0]).all()
        big = leaves(s, 3.0)                                 # three times the instances: past the capacity
        o = step(rast, big, s)
        torch.cuda.synchronize()
        assert torch.isnan(o[0]).all() and torch.isnan(o[2]).all() and torch.isnan(o[5]).all()
        for leaf in big[:5]:
            assert leaf.grad is not None and not leaf.grad.any()
        with pytest.raises(RuntimeError, match="overflow"):
            L.check_async_errors()
        o1 = step(rast, leaves(s, 3.0), s)                   # strict again, and right
        assert torch.isfinite(o1[0]).all()
    finally:
        forget(L, key)
