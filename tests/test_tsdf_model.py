"""The numpy model of the TSDF steps (tests/tsdf_model.py) on its own, without a GPU: the fused values of a plane and a sphere
against their analytic distance fields; the share of samples next to a decision in every scene the GPU tests use; float32 against
float64 outside that mask; marching tetrahedra against analytic surfaces (closed, Euler characteristic, volume, orientation); and
what keeps the GPU tests of the view loop and the brick culling from passing vacuously: blind views that touch nothing, live views
that each touch something and whose order shows, bricks left out and bricks cut in every culling scene."""
import numpy as np
import pytest

import tsdf_model as M


def test_a_fused_plane_has_its_zero_level_on_the_plane():
    """one view along +z of the plane z = 2: sdf = 2 - z for every sample the image sees, whatever its pixel"""
    dims, origin, h = (12, 10, 30), (-0.3, -0.25, 1.5), 0.04
    depth = np.full((1, 48, 64), 2.0, dtype=np.float32)
    vol, _, amb, touched = M.integrate(np.zeros((30, 10, 12, 2), np.float32), None, origin, h, 0.16, depth, M.pose(0, 0, 0, [0, 0, 0])[None],
                                       60.0, 60.0, 31.3, 23.6)
    _, _, Z = M.lattice(origin, h, dims)
    want = np.minimum(1.0, (2.0 - Z) / np.float64(np.float32(0.16)))
    seen = Z <= 2.0 + 0.16 - 1e-4
    assert touched[seen].all() and not touched[Z > 2.0 + 0.16 + 1e-4].any()
    assert np.abs(vol[..., 0] - want)[touched].max() < 1e-12 and (vol[..., 1][touched] == 1.0).all()
    k = np.argmin(np.where(touched[:, 5, 6], np.abs(vol[:, 5, 6, 0]), np.inf))
    assert abs(Z[k, 5, 6] - 2.0) <= h / 2 + 1e-9


def test_a_fused_sphere_has_its_zero_level_on_the_sphere():
    s = M.scene(V=1)
    vol, col, amb, touched = M.run(s)
    X, Y, Z = M.lattice(s["origin"], s["voxel"], s["dims"])
    dist = np.sqrt((X - M.SPHERE_C[0]) ** 2 + (Y - M.SPHERE_C[1]) ** 2 + (Z - M.SPHERE_C[2]) ** 2) - M.SPHERE_R
    trunc = 4 * s["voxel"]
    near = touched & (np.abs(vol[..., 0]) < 0.25) & (Z < 2.3)
    assert near.sum() > 200
    # the projective distance bounds the true one from above (a ray is no shorter than the normal); a nearest pixel is off by
    # half a pixel's footprint z / fx at most, which the sphere's slope towards its rim turns into depth: a pixel, generously
    foot = 2.6 / s["fx"]
    assert (np.abs(dist[near]) <= 0.25 * trunc + 2 * foot).all()
    inside, outside = touched & (dist < -2 * foot) & (Z < 2.3), touched & (dist > 2 * foot) & (Z < M.SPHERE_C[2])
    assert (vol[..., 0][inside] < 0).all() and (vol[..., 0][outside] > 0).all()
    front = touched & (np.abs(dist) < foot) & (Z < M.SPHERE_C[2] - 0.3)  # (the cap the camera faces, away from the silhouette)
    assert front.sum() > 50 and (col[..., 2][front] > 0.5).mean() > 0.9  # the sphere's own blue


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_few_samples_sit_next_to_a_decision(name):
    """the cap under which the GPU comparison says something: at most 3 % of the samples are left out of it; outside the mask
    float32 and float64 take the same decisions"""
    s = M.scene(**M.CASES[name])
    v64, c64, amb, touched = M.run(s)
    assert amb.mean() <= 0.03, amb.mean()
    v32, c32, _, _ = M.run(s, M.integrate32)
    assert np.array_equal(v32[..., 1][~amb], v64[..., 1][~amb])
    assert np.abs(v32[..., 0] - v64[..., 0])[~amb].max(initial=0.0) < 5e-6
    assert np.abs(c32 - c64)[~amb].max(initial=0.0) < 5e-6
    print(name, "ambiguous", amb.mean(), "touched", touched.mean(), "e32", np.abs(v32[..., 0] - v64[..., 0])[~amb].max(initial=0.0))


def _edges(tris):
    """{directed edge (key a, key b): count} with vertices keyed by their float32 bits"""
    keys = [[tuple(np.float32(p).view(np.uint32).tolist()) for p in t] for t in tris]
    out = {}
    for k in keys:
        for i in range(3):
            e = (k[i], k[(i + 1) % 3])
            out[e] = out.get(e, 0) + 1
    return keys, out


@pytest.mark.parametrize("shape, euler", [("sphere", 2), ("torus", 0)])
def test_marching_tetrahedra_closes_the_surface(shape, euler):
    dims, origin, h = (21, 20, 19), (-0.52, -0.5, -0.47), 0.05
    fn = M.sphere_sdf((0.0123, -0.0071, 0.0049), np.sqrt(0.1)) if shape == "sphere" else M.torus_sdf((0.0123, -0.0071, 0.0049), 0.1 * np.e, 0.1 * np.sqrt(2))
    vol = M.sdf_volume(dims, origin, h, 0.2, fn)
    counts, tris, _ = M.triangles(vol, origin, h)
    assert counts.sum() == len(tris) > 500
    keys, edges = _edges(tris)
    assert all(n == 1 for n in edges.values()) and all((b, a) in edges for a, b in edges)  # every edge once in each direction
    verts = {k for t in keys for k in t}
    nondegenerate = [t for t in keys if len(set(t)) == 3]
    assert len(nondegenerate) == len(keys)
    assert len(verts) - len(edges) // 2 + len(keys) == euler
    vol6 = sum(np.dot(t[0], np.cross(t[1], t[2])) for t in tris)  # divergence theorem: 6 V, positive with outward normals
    if shape == "sphere":
        assert abs(vol6 / 6 - 4 / 3 * np.pi * 0.1 ** 1.5) < 3 * 4 * np.pi * 0.1 * h * h


def test_min_weight_and_empty_volumes():
    dims, origin, h = (9, 7, 5), (-0.2, -0.15, -0.1), 0.05
    vol = M.sdf_volume(dims, origin, h, 0.2, M.sphere_sdf((0.01, 0.02, 0.003), 0.09))
    counts, tris, _ = M.triangles(vol, origin, h)
    assert counts.shape == (8 * 6 * 4,) and counts.sum() > 0
    vol[:, 3, :, 1] = 0.0
    c2, t2, _ = M.triangles(vol, origin, h)
    cells = c2.reshape(4, 6, 8)
    assert not cells[:, 2:4, :].any() and np.array_equal(cells[:, :2], counts.reshape(4, 6, 8)[:, :2])
    assert M.triangles(np.ones((3, 3, 3, 2), np.float32), origin, h)[0].sum() == 0
    assert M.triangles(np.ones((1, 3, 3, 2), np.float32), origin, h)[1].shape == (0, 3, 3)


# ---- the scenes for the integrate kernel's view loop and brick culling: the conditions under which the GPU tests say something

EPS = float(np.finfo(np.float32).eps)


def _fused(s, fn=M.integrate, **opts):
    start = M.pattern(s)
    return M.run(s, fn, start[0].copy(), start[1].copy(), **opts)


def _gpu_tolerance(v64, v32, amb):
    """what tests/test_hip_tsdf.py's check_against_model allows the tsdf: max(2 e32, 2 FLOOR), FLOOR = 8 eps"""
    return max(2 * float(np.abs(v32[..., 0] - v64[..., 0])[~amb].max(initial=0.0)), 2 * 8 * EPS)


@pytest.mark.parametrize("name", sorted(M.MANY_CASES))
def test_many_view_scenes_show_a_wrong_view_number(name):
    s = M.many_case(name)
    V, live = M.MANY_CASES[name]
    assert len(s["views"]) == V and s["live"] == sorted(live) and 1 <= len(live) <= 8
    assert len({v.tobytes() for v in s["views"]}) == V  # no two poses are equal
    blind = M.blind_views(s)
    assert (s["depth"][blind] == np.float32(M.BLIND_DEPTH)).all() and (s["color"][blind] == np.float32(M.BLIND_COLOR)).all()
    if blind:
        _, _, amb, touched = _fused(M.sub_scene(s, blind), **M.MANY_OPTS)
        assert not touched.any() and not amb.any()
        kinds = {k % len(M.BLIND_KINDS) for k in blind}
        assert len(kinds) >= min(len(M.BLIND_KINDS), 4)
    v64, c64, amb, touched = _fused(s, **M.MANY_OPTS)
    assert amb.mean() <= 0.03, amb.mean()
    v32, c32, _, _ = _fused(s, M.integrate32, **M.MANY_OPTS)
    assert np.array_equal(v32[..., 1][~amb], v64[..., 1][~amb])
    for v in s["live"]:
        assert M.run(M.sub_scene(s, [v]), **M.MANY_OPTS)[3].any(), v
    print(name, "ambiguous", amb.mean(), "touched", touched.mean())
    if len(live) >= 2:  # (a single live view has no order)
        back, _, amb_back, _ = _fused(M.sub_scene(s, s["live"][::-1]), **M.MANY_OPTS)
        alone, _, amb_alone, _ = _fused(M.sub_scene(s, s["live"]), **M.MANY_OPTS)
        assert np.array_equal(alone, v64) and np.array_equal(amb_alone, amb) and np.array_equal(amb_back, amb)  # (the blind views: nothing)
        assert np.abs(back[..., 0] - v64[..., 0])[~amb].max() > 100 * _gpu_tolerance(v64, v32, amb)


def test_every_view_of_the_all_live_scene_touches_a_sample():
    s = M.many_view_scene(live=range(M.ALL_LIVE["V"]), **M.ALL_LIVE)
    assert len({v.tobytes() for v in s["views"]}) == 300
    for v in range(300):
        assert M.run(M.sub_scene(s, [v]))[3].any(), v


@pytest.mark.parametrize("name", sorted(M.CULLING))
def test_culling_scenes_leave_bricks_out_and_cut_bricks(name):
    s, opts = M.culling_case(name)
    assert s["dims"] == (130, 10, 12) and len(s["views"]) == 2
    v64, c64, amb, touched = _fused(s, **opts)
    assert amb.mean() <= 0.03, amb.mean()
    v32, c32, _, _ = _fused(s, M.integrate32, **opts)
    assert np.array_equal(v32[..., 1][~amb], v64[..., 1][~amb])
    share = M.brick_shares(touched)
    assert share.shape == (12, 3, 3)
    untouched, partly = int((share == 0).sum()), int(((share > 0) & (share < 1)).sum())
    print(name, "ambiguous", amb.mean(), "touched", touched.mean(), "bricks untouched", untouched, "partly", partly, "of", share.size)
    assert untouched >= 5 and partly >= 5
    for v in range(2):
        assert M.run(M.sub_scene(s, [v]), **opts)[3].any(), v
    if name in ("inside", "minus-x"):
        near = opts.get("near", 0.05)
        for view in s["views"]:
            z = M.brick_corner_depths(s, view)
            assert ((z.min(axis=-1) < near) & (z.max(axis=-1) > near)).any()
            assert ((z.min(axis=-1) < 0.0) & (z.max(axis=-1) > near)).any()  # (and of 0: where the side planes' signs turn)
