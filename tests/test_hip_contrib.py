"""Per-Gaussian contribution statistics (include/dgr_hip.h: dgr_contribution_stats; dgr_amd.contrib) on the GPU: against the
float64 model of tests/contrib_model.py on the forward's own state (its records and its decisions), against identities that need
no model (the full forward's n_valid, the exported tag bytes, the light forward's median-pixel counts, the alpha image),
bit-equality under both lane mappings and between runs, alpha modes 1 and 2, the fold into an accumulator, NULL per-view pointers,
an overflowed frame, a hipGraph replay and `render_contributions` over both variants and bindings.

Tolerances.  n_touched is exact wherever the model has no ambiguous pair (contrib_model: a decision within 1e-6 of its
threshold).  max_weight and sum_weight 2^-32 stand within max(2 |float32 replay - float64|, floor) of the float64 value, floors
1e-6 and 1e-6 n_touched, over the Gaussians that do not blend at or behind an ambiguous pair; the conditions (at most 2 % with
an ambiguous pair, at most 10 % left out) are asserted, and were checked on the CPU oracle's forward state for every scene here
(at most 0.12 % and 1.6 %).  The model reads the render records the forward left, as the replay does: the distance between the
forward's fp32 projection and a float64 one (a few ulp of a pixel coordinate, about 1e-6 in a weight) is the forward's, pinned
by the parity tests, and no part of what is checked here."""
import functools

import numpy as np
import pytest
import torch

import contrib_model as cm
import hip_helpers as hh
from hip_helpers import binding, forced_lane_lists as lane_lists  # noqa: F401  (fixtures)
from dgr_amd import _capi, slam
from dgr_amd.synth import make_scene
from test_slam_render import Model
from util import one_tile_scene

pytestmark = pytest.mark.gpu

ID_MASK = (1 << 28) - 1
Q32 = 2.0 ** -32


def opaque_scene(P, W, H, seed):
    """big, nearly opaque splats: every pixel finishes after a few entries of lists that are thousands long"""
    s = make_scene(P, W, H, seed)
    return s._replace(scales=(s.scales * 8.0).astype(np.float32), opac=np.full_like(s.opac, 0.99))


SCENES = {
    "one_tile_255": ("light", lambda: one_tile_scene(255)), "one_tile_256": ("light", lambda: one_tile_scene(256)),
    "one_tile_257": ("light", lambda: one_tile_scene(257)), "one_tile_512": ("light", lambda: one_tile_scene(512)),
    "ragged": ("light", lambda: make_scene(6000, 70, 41, 6)), "opaque": ("light", lambda: opaque_scene(3000, 48, 48, 3)),
    "full": ("full", lambda: make_scene(3000, 96, 64, 7)),
}


def forward(s, variant):
    """(the state buffers and R, the forward's dict of numpy arrays)"""
    if variant == "light":
        out, d = hh.hip_forward(s, 3)
        return (out[7], out[8], out[9], out[0]), d
    out, d = hh.hip_full_forward(s, 3)
    return (out[6], out[7], out[8], out[0]), d


def stats_of(s, state, **kw):
    geom, binning, img, R = state
    st = slam.contribution_stats(geom, binning, img, s.P, s.H, s.W, R, **kw)
    torch.cuda.synchronize()
    return st


def host(st):
    return [t.cpu().numpy() for t in st]


@functools.lru_cache(maxsize=None)
def case(name):
    """A scene, its forward, the forward's decisions, the kernel's statistics and the model's: computed once, never modified."""
    variant, make = SCENES[name]
    s = make()
    state, d = forward(s, variant)
    n_touched, max_weight, sum_weight, counts = host(stats_of(s, state))
    dec = (d["radii"] > 0, hh.hip_state("point_list", s, d) & ID_MASK, hh.hip_state("ranges", s, d), hh.hip_state("n_contrib", s, d))
    tags = hh.hip_state("contribution_tags", s, d)
    extra = {"n_valid": hh.hip_state("n_valid", s, d)} if variant == "full" else {}
    geom = cm.records(hh.hip_state("means2D", s, d), hh.hip_state("conic_opacity", s, d))  # the records the replay read
    return dict(s=s, variant=variant, d=d, dec=dec, tags=tags, n_touched=n_touched, max_weight=max_weight, sum_weight=sum_weight,
                counts=counts, model=cm.stats(s, geom, *dec[1:]), **extra)


def assert_identities(s, variant, d, point_list, tags, n_touched, max_weight, sum_weight, counts, n_valid=None):
    """what holds exactly, whatever the model says"""
    assert n_touched.dtype == np.int32 and max_weight.dtype == np.float32 and sum_weight.dtype == np.int64
    assert (n_touched >= 0).all() and (sum_weight >= 0).all() and (max_weight >= 0).all() and (max_weight <= 0.99).all()
    by_tag = np.zeros(s.P, bool)
    by_tag[point_list[tags != 0]] = True
    assert np.array_equal(n_touched > 0, by_tag)  # blended by some pixel <=> some list entry of it carries a tag
    assert np.array_equal(n_touched > 0, max_weight > 0) and np.array_equal(n_touched > 0, sum_weight > 0)
    assert (max_weight.astype(np.float64) <= sum_weight * Q32 + Q32).all()
    assert counts.tolist() == [int((n_touched > 0).sum()), int((n_touched > 0).sum()), 0, 0]  # (min_pixels 1, weight_min 0)
    n_pairs = int(n_touched.astype(np.int64).sum())
    assert n_pairs > 0
    if variant == "full":
        assert n_pairs == int(n_valid.astype(np.int64).sum()) == int(d["num_related"])
        alpha_image = d["uncertainty"]
    else:
        assert (n_touched >= d["gau_related_pixels"].reshape(-1)).all()
        alpha_image = d["opacity_map"]
    # each fp32 add of the alpha image rounds once on a partial sum of at most 1; each truncation loses less than 2^-32
    total, image = float((sum_weight * Q32).sum()), float(alpha_image.astype(np.float64).sum())
    print(f"sum of sum_weight {total:.9f}, of the alpha image {image:.9f}, |difference| {abs(total - image):.3e}, bound {n_pairs * 2.0 ** -24:.3e}")
    assert abs(total - image) <= n_pairs * 2.0 ** -24


@pytest.mark.parametrize("name", list(SCENES))
def test_exact_identities(name):
    c = case(name)
    assert_identities(c["s"], c["variant"], c["d"], c["dec"][1], c["tags"], c["n_touched"], c["max_weight"], c["sum_weight"],
                      c["counts"], c.get("n_valid"))


@pytest.mark.parametrize("name", list(SCENES))
def test_n_touched_against_the_model(name):
    c = case(name)
    m, got = c["model"], c["n_touched"].astype(np.int64)
    ambiguous_share, _ = cm.conditions(m)
    diff = np.abs(got - m.count)
    print(f"{name}: touched {int((m.count > 0).sum())}, pairs {m.n_pairs}, with an ambiguous pair {ambiguous_share:.4f}, "
          f"largest |difference| {int(diff.max())}")
    assert ambiguous_share <= 0.02
    assert (m.count > 0).sum() > 0
    assert np.array_equal(got[m.ambiguous == 0], m.count[m.ambiguous == 0])
    assert (diff <= m.ambiguous).all()


def weight_errors(c):
    m = c["model"]
    _, left_out = cm.conditions(m)
    keep = ~m.tainted & (m.count > 0)
    tol_max, tol_sum = cm.tolerances(m)
    err_max = np.abs(c["max_weight"].astype(np.float64) - m.max)
    err_sum = np.abs(c["sum_weight"] * Q32 - m.sum)
    return left_out, keep, err_max, tol_max, err_sum, tol_sum


@pytest.mark.parametrize("name", list(SCENES))
def test_max_weight_against_the_model(name):
    """Measured on the MI355X: profiles/contrib/measured.txt."""
    left_out, keep, err, tol, _, _ = weight_errors(case(name))
    print(f"{name}: left out {left_out:.4f}, kept {int(keep.sum())}, largest |max_weight - model| {err[keep].max():.3e}, "
          f"above the tolerance {int((err > tol)[keep].sum())}, largest excess {np.max((err - tol)[keep]):.3e}")
    assert left_out <= 0.10 and keep.sum() > 0
    assert (err <= tol)[keep].all()


@pytest.mark.parametrize("name", list(SCENES))
def test_sum_weight_against_the_model(name):
    left_out, keep, _, _, err, tol = weight_errors(case(name))
    print(f"{name}: left out {left_out:.4f}, kept {int(keep.sum())}, largest |sum_weight 2^-32 - model| {err[keep].max():.3e}, "
          f"above the tolerance {int((err > tol)[keep].sum())}, largest excess {np.max((err - tol)[keep]):.3e}")
    assert left_out <= 0.10 and keep.sum() > 0
    assert (err <= tol)[keep].all()


@pytest.mark.parametrize("name", ["one_tile_257", "ragged", "full"])
def test_the_statistics_do_not_depend_on_the_tags_granularity(name, lane_lists):  # noqa: F811
    """a forward that walked quadrant lists sets both half bits of a quadrant, one that walked half-wave lists sets one: the
    replay folds them, so both give the same bits"""
    variant, make = SCENES[name]
    s = make()
    a = host(stats_of(s, forward(s, variant)[0]))
    _capi.set_option("lane_lists", 1 - lane_lists)
    b = host(stats_of(s, forward(s, variant)[0]))
    assert int(a[0].sum()) > 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["ragged", "full"])
def test_two_runs_give_equal_bits(name):
    variant, make = SCENES[name]
    s = make()
    state, _ = forward(s, variant)
    a, b = host(stats_of(s, state)), host(stats_of(s, state))
    for x, y, z in zip(a, b, [case(name)[k] for k in ("n_touched", "max_weight", "sum_weight", "counts")]):
        assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.parametrize("name", ["ragged", "full"])
@pytest.mark.parametrize("alpha_mode", [1, 2])
def test_alpha_modes_against_their_own_forward(name, alpha_mode):
    variant, make = SCENES[name]
    s = make()
    with _capi.thread_options(alpha_mode=alpha_mode):
        state, d = forward(s, variant)
        got = host(stats_of(s, state))
    pl, tags = hh.hip_state("point_list", s, d) & ID_MASK, hh.hip_state("contribution_tags", s, d)
    assert_identities(s, variant, d, pl, tags, *got, hh.hip_state("n_valid", s, d) if variant == "full" else None)


def two_views():
    return [make_scene(6000, 70, 41, 6, k) for k in (0, 1)]


def torch_fold(acc, st, min_pixels, weight_min, frame_id):
    """the fold in torch operations"""
    touched, mx, sm, views, last = acc
    obs = (st.n_touched >= min_pixels) & (st.max_weight >= weight_min)
    return (touched + st.n_touched.long(), torch.maximum(mx, st.max_weight), sm + st.sum_weight, views + obs.int(),
            torch.where(obs, torch.full_like(last, frame_id), last)), obs


@pytest.mark.parametrize("min_pixels, weight_min", [(1, 0.0), (5, 0.0), (1, 0.3), (5, 0.3)])
def test_two_views_folded_into_one_accumulator(min_pixels, weight_min):
    views = two_views()
    acc = slam.ContributionAccumulator(views[0].P, hh.dev())
    want = tuple(t.clone() for t in acc.tensors())
    assert (acc.last_seen == -1).all() and not acc.observed().any()
    for k, s in enumerate(views):
        st = stats_of(s, forward(s, "light")[0], into=acc, min_pixels=min_pixels, weight_min=weight_min, frame_id=7 + k)
        want, obs = torch_fold(want, st, min_pixels, weight_min, 7 + k)
        assert st.counts.tolist() == [int((st.n_touched > 0).sum()), int(obs.sum()), 0, 0]
        assert 0 < int(obs.sum()) and (weight_min == 0.0 and min_pixels == 1 or int(obs.sum()) < int((st.n_touched > 0).sum()))
    for got, w in zip(acc.tensors(), want):
        assert got.dtype == w.dtype and torch.equal(got, w)
    assert torch.equal(acc.observed(2), want[3] >= 2) and int(acc.observed(2).sum()) > 0
    assert torch.equal(acc.sum_weight_float(), want[2].double() * Q32)
    acc.reset()
    assert not any(bool(t.any()) for t in acc.tensors()[:4]) and (acc.last_seen == -1).all()


def call_abi(s, state, params, scratch, per_view, acc, counts):
    geom, binning, img, R = state
    p = _capi.ptr
    _capi.call("dgr_contribution_stats", hh.dev(), s.P, s.W, s.H, int(R), p(geom), p(binning), p(img), _capi.ContributionParams(*params),
               p(scratch), *(p(t) for t in per_view), *(p(t) for t in acc), p(counts))
    torch.cuda.synchronize()


def test_null_per_view_pointers_give_the_same_accumulators():
    views = two_views()
    P, dev = views[0].P, hh.dev()
    a, b = slam.ContributionAccumulator(P, dev), slam.ContributionAccumulator(P, dev)
    nbytes = _capi.load().dgr_contribution_scratch_bytes(P)
    assert nbytes >= 16 * P
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
    counts = torch.full((4,), -1, dtype=torch.int32, device=dev)
    for k, s in enumerate(views):
        state = forward(s, "light")[0]
        st = stats_of(s, state, into=a, min_pixels=2, weight_min=0.1, frame_id=k)
        call_abi(s, state, (2, 0.1, k), scratch, (None, None, None), b.tensors(), counts)
        assert torch.equal(counts, st.counts)
        # ... and any one of them alone, the accumulators and the counts absent
        only = torch.empty((P,), dtype=torch.float32, device=dev)
        call_abi(s, state, (2, 0.1, k), scratch, (None, only, None), (None,) * 5, None)
        assert torch.equal(only, st.max_weight)
    for x, y in zip(a.tensors(), b.tensors()):
        assert torch.equal(x, y)
    assert int(a.views.sum()) > 0


def presized_light(s, cap, k=None):
    """a presized light forward (precomputed colours) with binning capacity `cap`, through the C ABI: (state, status, inputs, alpha)"""
    lib, dev = _capi.load(), hh.dev()
    P, W, H = s.P, s.W, s.H
    u8 = lambda n: torch.empty((n,), dtype=torch.uint8, device=dev)  # noqa: E731
    f = lambda *sh: torch.empty(sh, device=dev)  # noqa: E731
    if k is None:
        k = dict(bg=hh.T(s.bg), means=hh.T(s.means), opac=hh.T(s.opac), scales=hh.T(s.scales), rots=hh.T(s.rots), view=hh.T(s.view),
                 proj=hh.T(s.proj), campos=hh.T(s.campos), gt=hh.T(s.gt), colors=torch.full((P, 3), 0.5, device=dev),
                 geom=u8(lib.dgr_geometry_bytes(P)), binning=u8(lib.dgr_binning_bytes(cap, W, H)), img=u8(lib.dgr_image_bytes(W, H)),
                 status=torch.zeros(4, dtype=torch.int32, device=dev), color=f(3, H, W), depth=f(1, H, W), median=f(1, H, W),
                 var=f(1, H, W), alpha=f(1, H, W), unc=f(P, 1), radii=torch.empty(P, dtype=torch.int32, device=dev),
                 px=torch.empty((P, 1), dtype=torch.int32, device=dev))
    p = _capi.ptr
    rc = lib.dgr_light_forward_presized(
        _capi.stream_handle(), p(k["geom"]), p(k["binning"]), cap, p(k["img"]), p(k["status"]), P, 1, 0, p(k["bg"]), W, H, p(k["means"]),
        None, p(k["colors"]), p(k["opac"]), p(k["scales"]), 1.0, p(k["rots"]), None, p(k["view"]), p(k["proj"]), p(k["campos"]),
        s.tanfovx, s.tanfovy, 0, p(k["color"]), p(k["depth"]), p(k["median"]), p(k["alpha"]), p(k["gt"]), p(k["var"]), p(k["unc"]),
        p(k["px"]), p(k["radii"]))
    assert rc == 0, _capi.last_error()
    return k


def test_an_overflowed_frame_is_all_zero_and_is_not_folded():
    s = make_scene(3000, 96, 64, 7)
    cap = 1000
    k = presized_light(s, cap)
    torch.cuda.synchronize()
    status = k["status"].tolist()
    assert status[0] > cap and status[1] == 1, status
    acc = slam.ContributionAccumulator(s.P, hh.dev())
    for n, t in enumerate(acc.tensors()):
        t.fill_(3 + n)
    before = [t.clone() for t in acc.tensors()]
    # (min_pixels 0: a frame that was rendered would have "observed" every Gaussian)
    st = stats_of(s, (k["geom"], k["binning"], k["img"], cap), into=acc, min_pixels=0, weight_min=0.0, frame_id=99)
    assert not st.n_touched.any() and not st.max_weight.any() and not st.sum_weight.any()
    assert st.counts.tolist() == [0, 0, 1, 0]
    for got, w in zip(acc.tensors(), before):
        assert torch.equal(got, w)
    # and the same call with room for everything is a view like any other
    k2 = presized_light(s, status[0])
    st2 = stats_of(s, (k2["geom"], k2["binning"], k2["img"], status[0]), into=acc, min_pixels=0, weight_min=0.0, frame_id=99)
    assert st2.counts.tolist() == [int((st2.n_touched > 0).sum()), s.P, 0, 0] and int(st2.n_touched.sum()) > 0
    assert torch.equal(acc.views, before[3] + 1) and (acc.last_seen == 99).all()


def test_a_recorded_call_follows_the_moved_gaussians():
    s = make_scene(3000, 96, 64, 7)
    moved = s._replace(means=(s.means + np.float32(0.05) * np.random.default_rng(0).standard_normal(s.means.shape)).astype(np.float32))
    cap = 4 * 65536
    acc = slam.ContributionAccumulator(s.P, hh.dev())
    k = presized_light(s, cap)
    eager = {}
    for name, scene in (("moved", moved), ("first", s)):
        k["means"].copy_(hh.T(scene.means))
        presized_light(s, cap, k)
        eager[name] = host(stats_of(s, (k["geom"], k["binning"], k["img"], cap)))
    assert k["status"].tolist()[1] == 0 and not np.array_equal(eager["first"][0], eager["moved"][0])
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        def step():
            presized_light(s, cap, k)
            return slam.contribution_stats(k["geom"], k["binning"], k["img"], s.P, s.H, s.W, cap, into=acc, frame_id=5)
        step()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            st = step()
    acc.reset()
    for n, name in enumerate(("first", "moved", "first")):
        k["means"].copy_(hh.T((s if name == "first" else moved).means))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(host(st), eager[name]):
            assert np.array_equal(got, want)
        assert int(acc.views.max()) == n + 1 and int(acc.last_seen.max()) == 5
    assert torch.equal(acc.touched_total.cpu(), torch.from_numpy(2 * eager["first"][0].astype(np.int64) + eager["moved"][0]))


def test_no_gaussians():
    s = make_scene(0, 32, 32, 1)
    state, _ = forward(s, "light")
    acc = slam.ContributionAccumulator(0, hh.dev())
    st = stats_of(s, state, into=acc)
    assert st.n_touched.numel() == 0 and st.max_weight.numel() == 0 and st.sum_weight.numel() == 0
    assert st.counts.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("variant", ["light", "full"])
def test_a_frame_with_every_gaussian_culled(variant):
    s = make_scene(500, 64, 48, 2)
    view = np.asarray(s.view, np.float64).reshape(4, 4)
    fwd = view[:3, 2]  # camera-space z = m . fwd + view[3, 2]: mirrored behind the camera
    z = s.means.astype(np.float64) @ fwd + view[3, 2]
    s = s._replace(means=(s.means - 2.0 * z[:, None] * fwd[None] / (fwd @ fwd)).astype(np.float32))
    state, d = forward(s, variant)
    assert not d["radii"].any() and d["num_rendered"] == 0
    acc = slam.ContributionAccumulator(s.P, hh.dev())
    st = stats_of(s, state, into=acc)
    assert not st.n_touched.any() and not st.max_weight.any() and not st.sum_weight.any() and st.counts.tolist() == [0, 0, 0, 0]
    assert not acc.views.any() and (acc.last_seen == -1).all()


@pytest.mark.parametrize("variant", ["light", "full"])
def test_render_contributions_renders_what_render_renders(variant, binding):  # noqa: F811
    s = make_scene(3000, 96, 64, 7)
    dev = hh.dev()
    pc = Model(s, dev)
    kw = dict(viewmatrix=hh.T(s.view), fov=(s.tanfovx, s.tanfovy), HW=(s.H, s.W), gt_depth=hh.T(s.gt), variant=variant)
    bg = hh.T(s.bg)
    with torch.no_grad():
        want = slam.render(None, pc, None, bg, **kw)
    acc = slam.ContributionAccumulator(s.P, dev)
    res, st = slam.render_contributions(None, pc, None, bg, **kw, into=acc, frame_id=3)
    torch.cuda.synchronize()
    assert set(res) == set(want)
    # the images and the integer outputs bit for bit (gau_uncertainty is a sum of float atomics: not the same bits run after run)
    for name, w in want.items():
        if name == "gau_uncertainty":
            assert torch.allclose(res[name], w, rtol=1e-4, atol=1e-6), name
        elif name != "viewspace_points":
            assert res[name].dtype == w.dtype and torch.equal(res[name], w), name
    assert res["viewspace_points"] is None
    # the statistics are those of the view: against the alpha image and the frustum test
    touched = st.n_touched > 0
    assert int(touched.sum()) > 0 and bool((res["visibility_filter"] | ~touched).all())
    assert int(touched.sum()) < int(res["visibility_filter"].sum())  # (occluded and sub-threshold Gaussians pass radii > 0)
    n_pairs = int(st.n_touched.long().sum())
    assert abs(float(st.sum_weight_float().sum()) - float(res["opacity_map"].double().sum())) <= n_pairs * 2.0 ** -24
    assert torch.equal(acc.views, touched.int()) and torch.equal(acc.last_seen, torch.where(touched, 3, -1).int())
    if variant == "full":
        assert torch.equal(st.n_touched.cpu(), torch.from_numpy(case("full")["n_touched"]))
