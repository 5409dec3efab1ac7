"""slam.tsdf_integrate and slam.extract_mesh on the GPU against the float64 numpy model (tests/tsdf_model.py).

Integrate.  Outside the model's `ambiguous` mask (samples within 1e-3 px of a pixel boundary, 1e-5 of the near plane or of the
truncation: at most 3 % of them, tests/test_tsdf_model.py) the weights are equal exactly and tsdf and colour stand within
max(2 e32, floor): e32 = the largest |integrate32 - integrate| of the case (what float32 costs in numpy's operation order; the
factor 2 covers another equally valid order or fused multiply-adds), floor = 8 float32 epsilons of the value's size: the update
(x w + t weight) / (w + weight) is two products, a sum and a quotient, half an epsilon each of a result of size <= 1: two
epsilons per view, and the averaging lets at most a few views' worth survive: 8 eps = 9.5e-7 for the colours in [0, 1], twice
that for the tsdf, whose range [-1, 1] has size 2.
Figures measured on the MI355X: profiles/tsdf/measured.txt.
The view loop and the brick culling (tests/tsdf_model.py: MANY_CASES, CULLING) go through the same comparison: scenes of up to 513
views of which a few see the lattice, at every line of the loop (a ballot's high half, waves 1-3, a later chunk, a partial one), and
poses at which the culling decides (cameras inside the lattice, rolled, a near plane across it, a principal point outside the image,
fx != fy); a view fused under a wrong number would fuse a constant image or miss a rendered one.  Where every view is live the
model's ambiguous share has no bound: there the bits of one call are held against those of calls of at most five views.

Extraction.  From volumes written directly as analytic distance fields over the truncation, with irrational centres and radii
(no value is exactly 0): the triangle count per cell equals the model's (the sign decisions are taken on the same float32
values); vertices within 4 eps (|coordinate| + voxel): t = v_A / (v_A - v_B) is a difference of two values of opposite sign and
a quotient (an epsilon of t <= 1, times the edge's length: one voxel), p_A and p_B one rounding each, their difference one, and
the final fused multiply-add one (half an epsilon of the coordinate each); colours within 4 eps of their size by the same count."""
import functools

import numpy as np
import pytest
import torch

import tsdf_model as M
from dgr_amd import fusion, slam

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
FLOOR = 8 * EPS
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def make_volume(s, volume=None, color_volume=None, with_color=True):
    vol = slam.TsdfVolume(s["origin"], s["voxel"], s["dims"], color=with_color, device=DEV)
    if volume is not None:
        vol.volume.copy_(T(volume))
    if color_volume is not None:
        vol.color.copy_(T(color_volume))
    return vol


def fuse(vol, s, views=slice(None), with_color=True, mask=None, **opts):
    return slam.tsdf_integrate(vol, T(s["depth"][views]), T(s["views"][views]), s["fx"], s["fy"], s["cx"], s["cy"],
                               color=T(s["color"][views]) if with_color else None, mask_image=None if mask is None else T(mask[views]), **opts)


def host(vol):
    torch.cuda.synchronize()
    return vol.volume.cpu().numpy(), None if vol.color is None else vol.color.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


pattern = M.pattern


def check_against_model(name, s, volume=None, color_volume=None, with_color=True, mask=None, **opts):
    """fuse on the GPU and in the model; assert the comparison of the module's docstring; returns the GPU's (volume, colour)"""
    m64 = M.run(s, M.integrate, None if volume is None else volume.copy(), None if color_volume is None else color_volume.copy(),
                with_color, mask=mask, **opts)
    m32 = M.run(s, M.integrate32, None if volume is None else volume.copy(), None if color_volume is None else color_volume.copy(),
                with_color, mask=mask, **opts)
    vol64, col64, amb, touched = m64
    assert amb.mean() <= 0.03
    vol = make_volume(s, volume, color_volume if with_color or color_volume is not None else None, with_color or color_volume is not None)
    fuse(vol, s, with_color=with_color, mask=mask, **opts)
    got, gcol = host(vol)
    keep = ~amb
    e32 = float(np.abs(m32[0][..., 0] - vol64[..., 0])[keep].max(initial=0.0))
    err = float(np.abs(got[..., 0] - vol64[..., 0])[keep].max(initial=0.0))
    line = f"tsdf-measured {name}: samples {amb.size} ambiguous {amb.mean():.4f} touched {touched.mean():.4f} e32 {e32:.3e} kernel-vs-model tsdf {err:.3e}"
    assert np.array_equal(got[..., 1][keep].astype(np.float64), vol64[..., 1][keep]), name
    assert err <= max(2 * e32, 2 * FLOOR), (name, err, e32)  # (2 FLOOR: the tsdf's range [-1, 1] has size 2)
    if with_color:
        c32 = float(np.abs(m32[1][..., :3] - col64[..., :3])[keep].max(initial=0.0))
        cerr = float(np.abs(gcol[..., :3] - col64[..., :3])[keep].max(initial=0.0))
        line += f" colour e32 {c32:.3e} kernel-vs-model colour {cerr:.3e}"
        assert cerr <= max(2 * c32, FLOOR), (name, cerr, c32)
        assert not gcol[..., 3].any() or color_volume is not None
    print(line)
    # what no view updated keeps its bits
    start = np.zeros_like(got) if volume is None else volume
    still = keep & ~touched
    assert np.array_equal(bits(got)[still], bits(start)[still]), name
    return got, gcol, touched, amb


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_integrate_equals_the_model(name):
    check_against_model(name, M.scene(**M.CASES[name]))


def test_views_in_one_call_equal_the_same_views_in_several_calls_bit_for_bit():
    s = M.scene(V=5)
    start = pattern(s)
    runs = []
    for split in ([slice(0, 5)], [slice(v, v + 1) for v in range(5)], [slice(0, 2), slice(2, 5)], [slice(0, 5)]):
        vol = make_volume(s, *start)
        for part in split:
            fuse(vol, s, part)
        runs.append(host(vol))
    for got in runs[1:]:  # (the last one: two runs of the same call)
        assert np.array_equal(bits(got[0]), bits(runs[0][0])) and np.array_equal(bits(got[1]), bits(runs[0][1]))
    assert not np.array_equal(bits(runs[0][0]), bits(start[0]))


def test_samples_no_view_reaches_keep_their_bits():
    """a pose that sees only part of the lattice, over a volume that is recognisably not empty"""
    s = M.scene(V=2)
    s["views"] = np.stack([M.pose(0.0, 0.45, 0.0, [0.1, 0.0, 0.3]), M.pose(0.1, 0.5, 0.0, [0.0, 0.1, 0.35])])
    frames = [M.render_scene(p, s["H"], s["W"], s["fx"], s["fy"], s["cx"], s["cy"]) for p in s["views"]]
    s.update(depth=np.stack([f[0] for f in frames]), color=np.stack([f[1] for f in frames]))
    start = pattern(s)
    got, gcol, touched, amb = check_against_model("partial-view", s, *start)
    still = ~amb & ~touched
    assert 0.2 < still.mean() < 0.9 and touched.mean() > 0.05
    assert np.array_equal(bits(gcol)[still], bits(start[1])[still])
    assert (bits(got)[touched & ~amb] != bits(start[0])[touched & ~amb]).any()


@pytest.mark.parametrize("name, opts", [
    ("max-weight", dict(max_weight=2.0)), ("weight-half", dict(weight=0.5)), ("depth-range", dict(depth_range=(1.7, 3.0))),
    ("near-2", dict(near=1.98)), ("no-colour", dict(with_color=False)),
])
def test_options(name, opts):
    s = M.scene(V=3)
    got, _, touched, amb = check_against_model(name, s, **opts)
    w = got[..., 1][~amb]
    if name == "max-weight":
        assert w.max() == 2.0 and (w == 2.0).mean() > 0.2
    if name == "weight-half":
        assert set(np.unique(w)) == {0.0, 0.5, 1.0, 1.5}
    if name in ("depth-range", "near-2"):
        full = M.run(s)[3]
        assert touched.sum() < 0.8 * full.sum()


def test_mask_image_excludes_pixels_at_or_below_the_threshold():
    s = M.scene(V=3)
    rng = np.random.default_rng(2)
    mask = rng.uniform(0.9, 1.0, s["depth"].shape).astype(np.float32)
    mask[:, ::3, ::2] = np.float32(0.99)  # exactly the threshold: excluded
    _, _, touched, _ = check_against_model("mask", s, mask=mask)
    assert touched.sum() < 0.8 * M.run(s)[3].sum()


def test_color_none_leaves_the_colour_volume_untouched():
    s = M.scene(V=3)
    start = pattern(s)
    _, gcol, touched, _ = check_against_model("colour-kept", s, *start, with_color=False)
    assert np.array_equal(bits(gcol), bits(start[1])) and touched.any()


def test_views_that_see_nothing_change_nothing():
    s = M.scene(V=2)
    start = pattern(s)
    behind = dict(s, views=np.stack([M.pose(0.0, 0.0, 0.0, [0.0, 0.0, -10.0]), M.pose(0.1, 3.0, 0.0, [0.0, 0.0, 0.0])]))
    for name, scene, opts in (("behind", behind, {}), ("near", s, dict(near=100.0))):
        vol = make_volume(s, *start)
        fuse(vol, scene, **opts)
        got = host(vol)
        assert np.array_equal(bits(got[0]), bits(start[0])) and np.array_equal(bits(got[1]), bits(start[1])), name


def test_nan_and_inf_inputs_end_in_skipped_updates():
    """NaN and Inf depths and a NaN pose: those views change nothing, so the finite view's result stands alone, bit for bit"""
    s = M.scene(V=4)
    s["depth"][1] = np.nan
    s["depth"][2] = np.inf
    s["views"][3] = np.nan
    s["depth"][0][5:9, 7:30] = np.nan  # and holes in the finite view itself
    s["depth"][0][20:22, 3:50] = np.inf
    start = pattern(s)
    vol = make_volume(s, *start)
    fuse(vol, s)
    got = host(vol)
    alone = make_volume(s, *start)
    fuse(alone, s, slice(0, 1))
    want = host(alone)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.isfinite(got[0]).all() and not np.array_equal(bits(got[0]), bits(start[0]))
    mixed = dict(s, views=s["views"].copy())
    mixed["views"][3] = M.MAIN_POSES[3]
    mixed["views"][3][1, 2] = np.nan  # one NaN entry: x and z survive in part; nothing may fault
    fuse(make_volume(s, *start), mixed)
    torch.cuda.synchronize()


def test_integrate_captured_into_a_graph_equals_eager():
    s, other = M.scene(V=3), M.scene(V=3)
    other["depth"] = (other["depth"] * np.float32(1.03)).astype(np.float32)
    eager = {}
    for name, sc in (("first", s), ("other", other)):
        vol = make_volume(s)
        fuse(vol, sc)
        eager[name] = host(vol)
    assert not np.array_equal(bits(eager["first"][0]), bits(eager["other"][0]))
    vol = make_volume(s)
    depth, color, views = T(s["depth"]), T(s["color"]), T(s["views"])
    step = lambda: slam.tsdf_integrate(vol, depth, views, s["fx"], s["fy"], s["cx"], s["cy"], color=color)  # noqa: E731
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            step()
    for name, sc in (("other", other), ("first", s)):
        vol.reset()
        depth.copy_(T(sc["depth"]))
        graph.replay()
        got = host(vol)
        assert np.array_equal(bits(got[0]), bits(eager[name][0])) and np.array_equal(bits(got[1]), bits(eager[name][1])), name


# ---- the view loop (chunks of 256 views, a ballot per wave of 64) and the brick culling; the scenes and the conditions under which
# they say something: tests/tsdf_model.py, tests/test_tsdf_model.py

def same_bits(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def fused(s, start, calls, **opts):
    """the (volume, colour) after one fuse() per entry of `calls` (index lists or slices), from `start`"""
    vol = make_volume(s, *start)
    for part in calls:
        fuse(vol, s, part, **opts)
    return host(vol)


MANY_GPU = ["64-high-half", "65-wave-1", "256-waves-1-3", "257-second-chunk", "257-first-chunk-blind", "513-three-chunks"]


@pytest.mark.parametrize("name", MANY_GPU)
def test_many_views_equal_the_model(name):
    s = M.many_case(name)
    check_against_model("many " + name, s, *M.pattern(s), **M.MANY_OPTS)


@pytest.mark.parametrize("name", ["257-second-chunk", "257-first-chunk-blind", "513-three-chunks"])
def test_many_views_in_one_call_equal_the_live_views_alone_bit_for_bit(name):
    s = M.many_case(name)
    start = M.pattern(s)
    whole = fused(s, start, [slice(None)], **M.MANY_OPTS)
    assert same_bits(fused(s, start, [s["live"]], **M.MANY_OPTS), whole)
    assert same_bits(fused(s, start, [[v] for v in s["live"]], **M.MANY_OPTS), whole)
    assert not np.array_equal(bits(whole[0]), bits(start[0])) and not np.array_equal(bits(whole[1]), bits(start[1]))
    changed = (bits(whole[0]) != bits(start[0])).any(axis=-1)
    print(f"tsdf-measured many {name} bits: views {len(s['views'])} live {len(s['live'])} samples {changed.size} changed {changed.mean():.4f}; "
          f"one call = the live views in one call = a call per live view")


def test_three_hundred_live_views_equal_sixty_calls_of_five():
    s = M.many_view_scene(live=range(M.ALL_LIVE["V"]), **M.ALL_LIVE)
    start = M.pattern(s)
    whole = fused(s, start, [slice(None)], max_weight=4.0)
    assert same_bits(fused(s, start, [slice(v, v + 5) for v in range(0, 300, 5)], max_weight=4.0), whole)
    assert same_bits(fused(s, start, [slice(0, 256), slice(256, 300)], max_weight=4.0), whole)
    first = fused(s, start, [slice(0, 256)], max_weight=4.0)
    assert not same_bits(whole, start) and not np.array_equal(bits(whole[0]), bits(first[0])) and not np.array_equal(bits(whole[1]), bits(first[1]))
    changed = (bits(whole[0]) != bits(start[0])).any(axis=-1)
    print(f"tsdf-measured all-live 300: samples {changed.size} changed {changed.mean():.4f} changed by views 256.. "
          f"{(bits(whole[0]) != bits(first[0])).any(axis=-1).mean():.4f}")


@pytest.mark.parametrize("name", sorted(M.CULLING))
def test_culling_scenes_equal_the_model(name):
    s, opts = M.culling_case(name)
    start = M.pattern(s)
    _, _, touched, amb = check_against_model("culling " + name, s, *start, **opts)
    share = M.brick_shares(touched)
    assert (share == 0).sum() >= 5 and ((share > 0) & (share < 1)).sum() >= 5
    _, gcol, _, _ = check_against_model("culling " + name + " no-colour", s, *start, with_color=False, **opts)
    assert np.array_equal(bits(gcol), bits(start[1]))


def test_a_graph_replay_with_many_views():
    s, other = M.many_case("257-second-chunk"), M.many_case("257-moved")
    assert other["live"] == [1, 65, 256] and other["dims"] == s["dims"]
    start = M.pattern(s)
    eager = {name: fused(sc, start, [slice(None)], **M.MANY_OPTS) for name, sc in (("first", s), ("moved", other))}
    assert not same_bits(eager["first"], eager["moved"])
    vol = make_volume(s, *start)
    depth, color, views = T(s["depth"]), T(s["color"]), T(s["views"])
    step = lambda: slam.tsdf_integrate(vol, depth, views, s["fx"], s["fy"], s["cx"], s["cy"], color=color, **M.MANY_OPTS)  # noqa: E731
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            step()
    for name, sc in (("moved", other), ("first", s)):
        vol.volume.copy_(T(start[0]))
        vol.color.copy_(T(start[1]))
        depth.copy_(T(sc["depth"]))
        color.copy_(T(sc["color"]))
        views.copy_(T(sc["views"]))
        graph.replay()
        got = host(vol)
        print(f"tsdf-measured graph replay 257 views, live {sc['live']}: changed {(bits(got[0]) != bits(start[0])).any(axis=-1).mean():.4f}")
        assert same_bits(got, eager[name]), name


def test_the_wrapper_takes_strided_inputs_of_many_views():
    """every other view of a 514-view batch, as strided tensors: 257 views, the same bits as from contiguous copies"""
    s = M.many_case("257-second-chunk")
    start = M.pattern(s)
    want = fused(s, start, [slice(None)], **M.MANY_OPTS)

    def strided(a):
        wide = torch.full((2 * a.shape[0],) + a.shape[1:], float("nan"), dtype=torch.float32, device=DEV)
        wide[::2] = T(a)
        return wide[::2]
    depth, color, views = strided(s["depth"]), strided(s["color"]), strided(s["views"])
    assert not depth.is_contiguous() and not color.is_contiguous() and not views.is_contiguous()
    vol = make_volume(s, *start)
    slam.tsdf_integrate(vol, depth, views, s["fx"], s["fy"], s["cx"], s["cy"], color=color, **M.MANY_OPTS)
    got = host(vol)
    print(f"tsdf-measured strided 257 of 514 views: changed {(bits(got[0]) != bits(start[0])).any(axis=-1).mean():.4f}")
    assert same_bits(got, want)


# ---- extraction

H_MESH, TRUNC_MESH = 0.05, 0.2
R43_FRAC = 0.2
C_IRR = np.array([np.sqrt(2.0) - 1.4, np.pi - 3.15, np.e - 2.7])  # (0.0142, -0.0084, 0.0183)


def mesh_case(name):
    """-> (dims, origin, distance function, min_weight, zero-weight slab or None)"""
    def centred(dims, frac=0.33, c_off=(0.0, 0.0, 0.0)):
        ext = H_MESH * (np.array(dims) - 1)
        origin = tuple(-ext / 2)
        return dims, origin, M.sphere_sdf(C_IRR + np.array(c_off), float(frac * ext.min() * np.sqrt(1.01)))
    if name == "2x2x2":
        return (2, 2, 2), (0.0, 0.0, 0.0), M.sphere_sdf(C_IRR * 0.3, 0.7 * H_MESH * np.sqrt(1.1))
    if name in ("9x7x5", "33x9x9", "34x9x9"):
        return centred(tuple(int(n) for n in name.split("x")))
    if name == "43x43x43":
        return centred((43, 43, 43), R43_FRAC)
    if name == "torus":
        return (41, 40, 21), (-1.0, -0.975, -0.5), M.torus_sdf(C_IRR, 0.2 * np.e, 0.1 * np.sqrt(3.0))
    if name == "one-block":  # a sample of the lattice's first z layer inside a sphere smaller than a voxel: cells of block 0 only
        origin = np.array([-0.8, -0.2, -0.2])
        return (34, 9, 9), tuple(origin), M.sphere_sdf(origin + H_MESH * np.array([5.013, 3.021, 0.017]), 0.45 * H_MESH)
    if name == "nothing":
        return (12, 11, 10), (0.0, 0.0, 0.0), (lambda X, Y, Z: 1.0 + 0.0 * X)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def mesh_reference(name, slab=False):
    dims, origin, fn = mesh_case(name)
    vol = M.sdf_volume(dims, origin, H_MESH, TRUNC_MESH, fn)
    assert not (vol[..., 0] == 0).any()
    if slab:
        vol[:, dims[1] // 2, :, 1] = 0.0
    rng = np.random.default_rng(11)
    col = np.concatenate([rng.uniform(0.0, 1.0, vol.shape[:3] + (3,)), np.zeros(vol.shape[:3] + (1,))], axis=-1).astype(np.float32)
    counts, tris, tcol = M.triangles(vol, origin, H_MESH, color=col)
    for a in (vol, col, counts, tris, tcol):
        a.setflags(write=False)
    return dims, origin, vol, col, counts, tris, tcol


def gpu_mesh(dims, origin, vol, col, **kw):
    v = slam.TsdfVolume(origin, H_MESH, dims, truncation=TRUNC_MESH, color=col is not None, device=DEV)
    v.volume.copy_(T(vol))
    if col is not None:
        v.color.copy_(T(col))
    mesh = slam.extract_mesh(v, **kw)
    torch.cuda.synchronize()
    return v, mesh


def per_cell_counts(vertices, dims, origin):
    """the triangles of each cell, from where their centroids lie (a triangle lies inside its cell)"""
    tri = vertices.reshape(-1, 3, 3).astype(np.float64)
    idx = np.floor((tri.mean(axis=1) - np.array(origin)) / H_MESH).astype(np.int64)
    idx = np.clip(idx, 0, np.array(dims) - 2)
    lin = (idx[:, 2] * (dims[1] - 1) + idx[:, 1]) * (dims[0] - 1) + idx[:, 0]
    return lin


@pytest.mark.parametrize("name", ["2x2x2", "9x7x5", "33x9x9", "34x9x9", "43x43x43", "torus", "one-block"])
def test_extraction_equals_the_model(name):
    dims, origin, vol, col, counts, tris, tcol = mesh_reference(name)
    _, mesh = gpu_mesh(dims, origin, vol, col)
    Tn = int(counts.sum())
    assert Tn > 0 and mesh.count.tolist() == [Tn] and mesh.flags.tolist() == [0]
    assert tuple(mesh.vertices.shape) == (3 * Tn, 3) and tuple(mesh.colors.shape) == (3 * Tn, 3)
    got, gcol = mesh.vertices.cpu().numpy().reshape(-1, 3, 3), mesh.colors.cpu().numpy().reshape(-1, 3, 3)
    # ordered by cell: the model's cell of every triangle, in order, is the kernel's
    want_cells = np.repeat(np.arange(counts.size), counts)
    assert np.array_equal(per_cell_counts(tris, dims, origin), want_cells)
    assert np.array_equal(per_cell_counts(got, dims, origin), want_cells)  # the count per cell, and the order of the cells
    tol = 4 * EPS * (np.abs(tris) + H_MESH)
    err = np.abs(got - tris)
    cerr = np.abs(gcol - tcol)
    print(f"tsdf-measured mesh {name}: cells {counts.size} triangles {Tn} vertex error {err.max():.3e} = {(err / (np.abs(tris) + H_MESH)).max() / EPS:.2f} eps "
          f"(|coordinate| + voxel); colour error {cerr.max():.3e} = {cerr.max() / EPS:.2f} eps")
    assert (err <= tol).all()
    assert (cerr <= 4 * EPS).all()
    if name == "one-block":
        assert counts[:256].sum() == Tn and counts.size > 2048


def surface_invariants(vertices):
    """-> (every undirected edge belongs to exactly two triangles that traverse it in opposite directions, V - E + F, 6 x volume)"""
    tri = vertices.reshape(-1, 3, 3)
    uniq, inv = np.unique(np.ascontiguousarray(tri).view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    v = inv.reshape(-1, 3)
    directed = np.concatenate([v[:, [0, 1]], v[:, [1, 2]], v[:, [2, 0]]])
    de, dn = np.unique(directed, axis=0, return_counts=True)
    rev = {tuple(e) for e in de.tolist()}
    closed = bool((dn == 1).all()) and all((b, a) in rev for a, b in rev)
    undirected = np.unique(np.sort(directed, axis=1), axis=0)
    t64 = tri.astype(np.float64)
    vol6 = float(np.einsum("ij,ij->i", t64[:, 0], np.cross(t64[:, 1], t64[:, 2])).sum())
    return closed, len(uniq) - len(undirected) + len(tri), vol6


@pytest.mark.parametrize("name, euler", [("43x43x43", 2), ("torus", 0)])
def test_the_surface_is_closed_and_oriented(name, euler):
    dims, origin, vol, col, counts, tris, _ = mesh_reference(name)
    _, mesh = gpu_mesh(dims, origin, vol, None)
    closed, chi, vol6 = surface_invariants(mesh.vertices.cpu().numpy())
    assert closed and chi == euler and vol6 > 0
    if name == "43x43x43":
        # A piecewise-linear level set of a smooth distance field is second order: along an edge or inside a tetrahedron of
        # diameter sqrt(3) h, linear interpolation of f = |p - c| - R is off by at most (sqrt(3) h)^2 / 8 max |f''| = 3 h^2 / (8 R),
        # and |grad f| = 1 turns that into the surface's displacement.  Over the area 4 pi R^2: 1.5 pi R h^2; a third more for the
        # higher-order terms: 2 pi R h^2.
        R = float(R43_FRAC * H_MESH * 42 * np.sqrt(1.01))
        dv = abs(vol6 / 6 - 4.0 / 3.0 * np.pi * R ** 3)
        print(f"tsdf-measured mesh volume {name}: {vol6 / 6:.6f} analytic {4.0 / 3.0 * np.pi * R ** 3:.6f} difference {dv:.3e} bound {2 * np.pi * R * H_MESH ** 2:.3e}")
        assert dv <= 2 * np.pi * R * H_MESH ** 2


def test_min_weight_opens_the_surface_at_a_slab_of_zero_weights():
    dims, origin, vol, col, counts, tris, _ = mesh_reference("43x43x43", True)
    full = mesh_reference("43x43x43")[4].reshape(42, 42, 42)
    cells = counts.reshape(42, 42, 42)
    y = dims[1] // 2
    assert full[:, y - 1:y + 1].sum() > 0 and not cells[:, y - 1:y + 1].any() and np.array_equal(np.delete(cells, [y - 1, y], axis=1), np.delete(full, [y - 1, y], axis=1))
    _, mesh = gpu_mesh(dims, origin, vol, None)
    got = mesh.vertices.cpu().numpy()
    assert mesh.count.tolist() == [int(counts.sum())]
    assert np.array_equal(per_cell_counts(got, dims, origin), np.repeat(np.arange(counts.size), counts))
    assert not surface_invariants(got)[0]  # open exactly there
    _, low = gpu_mesh(dims, origin, vol, None, min_weight=0.0)
    assert low.count.tolist() == [int(full.sum())]


def test_a_capacity_below_the_need_is_reported_and_respected(monkeypatch):
    from test_hip_guarded_buffers import GuardedTorch
    dims, origin, vol, col, counts, tris, _ = mesh_reference("34x9x9")
    _, full = gpu_mesh(dims, origin, vol, col)
    Tn = int(counts.sum())
    guarded = GuardedTorch()
    monkeypatch.setattr(fusion, "torch", guarded)
    for cap in (Tn // 2, 1, 0, Tn, Tn + 7):
        _, part = gpu_mesh(dims, origin, vol, col, max_triangles=cap)
        assert guarded.check() >= 3
        n = min(cap, Tn)
        assert part.count.tolist() == [Tn] and part.flags.tolist() == [1 if cap < Tn else 0], cap
        assert tuple(part.vertices.shape) == (3 * cap, 3)
        assert torch.equal(part.vertices[:3 * n], full.vertices[:3 * n]) and torch.equal(part.colors[:3 * n], full.colors[:3 * n]), cap


def test_a_volume_without_a_crossing_gives_an_empty_mesh():
    dims, origin, fn = mesh_case("nothing")
    vol = M.sdf_volume(dims, origin, H_MESH, TRUNC_MESH, fn)
    for d, v in ((dims, vol), ((5, 1, 4), vol[:4, :1, :5]), ((1, 1, 1), vol[:1, :1, :1])):
        _, mesh = gpu_mesh(d, origin, np.ascontiguousarray(v), None)
        assert mesh.count.tolist() == [0] and mesh.flags.tolist() == [0] and tuple(mesh.vertices.shape) == (0, 3) and mesh.colors is None


def test_two_extractions_give_equal_bits_and_a_captured_one_equals_eager():
    dims, origin, vol, col, counts, tris, _ = mesh_reference("43x43x43")
    v, a = gpu_mesh(dims, origin, vol, col)
    _, b = gpu_mesh(dims, origin, vol, col)
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.colors, b.colors)
    cap = int(counts.sum()) + 5
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        slam.extract_mesh(v, max_triangles=cap)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            mesh = slam.extract_mesh(v, max_triangles=cap)
    small = mesh_reference("43x43x43", True)
    for vol_now, ref in ((small[2], None), (vol, a)):
        v.volume.copy_(T(vol_now))
        graph.replay()
        torch.cuda.synchronize()
        n = int(mesh.count.item())
        if ref is None:
            assert n == int(small[4].sum()) and mesh.flags.tolist() == [0]
        else:
            assert n == int(counts.sum()) and torch.equal(mesh.vertices[:3 * n], ref.vertices) and torch.equal(mesh.colors[:3 * n], ref.colors)


def test_end_to_end_the_fused_sphere_lies_on_the_sphere():
    s = M.scene(V=3)
    vol = make_volume(s)
    fuse(vol, s)
    mesh = slam.extract_mesh(vol, min_weight=1.0)
    v = mesh.vertices.cpu().numpy().astype(np.float64)
    assert len(v) > 3000 and mesh.flags.tolist() == [0] and np.isfinite(v).all()
    r = v - M.SPHERE_C
    dist = np.abs(np.linalg.norm(r, axis=1) - M.SPHERE_R)
    # The sphere's part of the mesh: the vertices whose nearest point of the sphere faces at least one of the fused cameras, that
    # is, the part of the sphere the views measured.  Behind each view's silhouette a projective TSDF also closes the band of
    # negative samples against the free space that view sees past the rim: a wall along the tangent rays, up to a truncation
    # behind the tangent circle, which belongs to no measured surface (and leaves the sphere by up to sqrt(R^2 + trunc^2) - R).
    n = r / np.linalg.norm(r, axis=1, keepdims=True)
    facing = np.zeros(len(v), dtype=bool)
    for view in s["views"]:
        m = view.astype(np.float64).T
        eye = -m[:3, :3].T @ m[:3, 3]
        to_eye = eye - (M.SPHERE_C + M.SPHERE_R * n)
        facing |= (to_eye * n).sum(axis=1) > 0.0
    print(f"tsdf-measured end-to-end: {len(v) // 3} triangles, {facing.mean():.3f} of the vertices on the measured part of the sphere, largest "
          f"distance from the sphere there {dist[facing].max():.4f} (voxel {s['voxel']}), mean {dist[facing].mean():.4f}; elsewhere {dist[~facing].max():.4f}")
    assert facing.mean() > 0.7 and (dist[facing] <= s["voxel"]).all()
    c = mesh.colors.cpu().numpy()
    assert c.min() >= 0.0 and c.max() <= 1.0
