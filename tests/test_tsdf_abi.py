"""The TSDF entry points (include/dgr_hip.h: dgr_tsdf_integrate, dgr_mesh_scratch_bytes, dgr_mesh_plan, dgr_mesh_emit) and their
Python surface without a GPU: declared, exported and bound; the two descriptors' layouts against the header text; every argument
error refused with its message before any device call (FAKE pointers: nothing is dereferenced); the scratch size.  One test is
marked gpu: the entry point with 65 536 views."""
import ctypes as C
import re

import pytest
import torch

from dgr_amd import _capi, fusion, slam

from abi_checks import FAKE, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_tsdf_integrate", "dgr_mesh_scratch_bytes", "dgr_mesh_plan", "dgr_mesh_emit")
NAN, INF = float("nan"), float("inf")


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_tsdf_integrate": 12, "dgr_mesh_scratch_bytes": 1, "dgr_mesh_plan": 8, "dgr_mesh_emit": 9})
    assert _capi._SIGS["dgr_mesh_scratch_bytes"][0] is C.c_size_t


def _header_fields(name):
    body = header_text().split("} %s;" % name)[0].rsplit("typedef struct %s {" % name, 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_descriptors_match_the_header_text():
    assert _header_fields("dgr_tsdf_grid") == [("nx", "int"), ("ny", "int"), ("nz", "int"), ("origin[3]", "float"), ("voxel_size", "float")]
    G = _capi.TsdfGrid
    assert C.sizeof(G) == 28 and [(n, getattr(G, n).offset) for n, _ in G._fields_] == [("nx", 0), ("ny", 4), ("nz", 8), ("origin", 12), ("voxel_size", 24)]
    fields = _header_fields("dgr_tsdf_params")
    assert fields == [(n, "float") for n in ("fx", "fy", "cx", "cy", "truncation", "weight", "max_weight", "depth_min", "depth_max",
                                             "near_z", "mask_threshold")]
    P = _capi.TsdfParams
    assert [(n, "float") for n, t in P._fields_ if t is C.c_float] == fields
    assert C.sizeof(P) == 44 and [getattr(P, n).offset for n, _ in fields] == list(range(0, 44, 4))


def test_the_header_states_the_semantics():
    text = header_text()
    doc = text[text.index("TSDF fusion of rendered views"):text.index("typedef struct dgr_tsdf_grid")]
    for word in ("x the fastest", "ONE launch", "read once and written at most once", "floor(u + 0.5)", "sdf < -truncation", "index order",
                 "hipGraph", "Kuhn", "{0, a, a|b, 7}", "tsdf < 0", "v_A / (v_A - v_B)", "Degenerate", "2^31", "bit 0"):
        assert word in doc, word


def _grid(nx=8, ny=8, nz=8, voxel=0.1):
    return _capi.TsdfGrid(nx, ny, nz, (C.c_float * 3)(0.0, 0.0, 0.0), voxel)


def _integrate(grid=True, volume=FAKE, color=FAKE, V=2, W=64, H=48, depth=FAKE, image=FAKE, mask=None, views=FAKE, params=True,
               fx=60.0, fy=60.0, truncation=0.2, **g):
    p = _capi.TsdfParams(fx, fy, 31.5, 23.5, truncation, 1.0, INF, 0.0, INF, 0.05, 0.99) if params else None
    return _capi.load().dgr_tsdf_integrate(None, _grid(**g) if grid else None, volume, color, V, W, H, depth, image, mask, views, p)


@pytest.mark.parametrize("case, text", [
    (dict(grid=False), "grid is NULL"), (dict(params=False), "params is NULL"),
    (dict(nx=0), "must be positive"), (dict(ny=-1), "must be positive"), (dict(nz=0), "must be positive"),
    (dict(nx=2048, ny=1024, nz=1024), "fewer than 2^31 samples"), (dict(nx=1 << 16, ny=1 << 16, nz=1), "fewer than 2^31 samples"),
    (dict(voxel=0.0), "voxel_size must be finite and positive"), (dict(voxel=-0.1), "voxel_size must be finite and positive"),
    (dict(voxel=NAN), "voxel_size must be finite and positive"), (dict(voxel=INF), "voxel_size must be finite and positive"),
    (dict(V=0), "n_views must be at least 1"), (dict(V=-3), "n_views must be at least 1"),
    (dict(W=0), "width and height"), (dict(H=0), "width and height"), (dict(H=-2), "width and height"), (dict(W=1 << 16, H=1 << 15), "width and height"),
    (dict(volume=None), "volume is NULL"), (dict(depth=None), "depth is NULL"), (dict(views=None), "viewmatrices is NULL"),
    (dict(color=None), "go together"), (dict(image=None), "go together"),
    (dict(volume=FAKE + 4), "not 8-byte aligned"), (dict(color=FAKE + 8), "not 16-byte aligned"),
    (dict(depth=FAKE + 2), "not 4-byte aligned"), (dict(mask=FAKE + 1), "not 4-byte aligned"), (dict(views=FAKE + 3), "not 4-byte aligned"),
    (dict(fx=0.0), "fx and fy"), (dict(fy=-1.0), "fx and fy"), (dict(fx=NAN), "fx and fy"), (dict(fy=INF), "fx and fy"),
    (dict(truncation=0.0), "truncation must be finite and positive"), (dict(truncation=NAN), "truncation must be finite and positive"),
    (dict(truncation=INF), "truncation must be finite and positive"), (dict(truncation=-0.2), "truncation must be finite and positive"),
])
def test_integrate_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_integrate(**case), "dgr_tsdf_integrate", text)


def _plan(grid=True, volume=FAKE, min_weight=1.0, max_triangles=100, scratch=FAKE, count=FAKE, flags=FAKE, **g):
    return _capi.load().dgr_mesh_plan(None, _grid(**g) if grid else None, volume, min_weight, max_triangles, scratch, count, flags)


def _emit(grid=True, volume=FAKE, color=FAKE, min_weight=1.0, max_triangles=100, scratch=FAKE, vertices=FAKE, colors=FAKE, **g):
    return _capi.load().dgr_mesh_emit(None, _grid(**g) if grid else None, volume, color, min_weight, max_triangles, scratch, vertices, colors)


@pytest.mark.parametrize("case, text", [
    (dict(grid=False), "grid is NULL"), (dict(nx=0), "must be positive"), (dict(nx=2048, ny=1024, nz=1024), "fewer than 2^31 samples"),
    (dict(voxel=NAN), "voxel_size must be finite and positive"),
    (dict(volume=None), "volume is NULL"), (dict(volume=FAKE + 4), "not 8-byte aligned"), (dict(min_weight=NAN), "min_weight is NaN"),
    (dict(max_triangles=-1), "max_triangles is negative"), (dict(scratch=None), "scratch is NULL or not 16-byte aligned"),
    (dict(scratch=FAKE + 8), "scratch is NULL or not 16-byte aligned"), (dict(count=None), "count or flags is NULL"),
    (dict(flags=None), "count or flags is NULL"), (dict(count=FAKE + 2), "not 4-byte aligned"),
])
def test_mesh_plan_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_plan(**case), "dgr_mesh_plan", text)


@pytest.mark.parametrize("case, text", [
    (dict(grid=False), "grid is NULL"), (dict(nz=-4), "must be positive"), (dict(nx=1 << 11, ny=1 << 10, nz=1 << 10), "fewer than 2^31 samples"),
    (dict(voxel=0.0), "voxel_size must be finite and positive"),
    (dict(volume=None), "volume is NULL"), (dict(color=FAKE + 4), "not 16-byte aligned"), (dict(min_weight=NAN), "min_weight is NaN"),
    (dict(max_triangles=-1), "max_triangles is negative"), (dict(scratch=None), "scratch is NULL or not 16-byte aligned"),
    (dict(vertices=None), "vertices is NULL"), (dict(color=None), "volume without colour"), (dict(vertices=FAKE + 2), "not 4-byte aligned"),
])
def test_mesh_emit_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_emit(**case), "dgr_mesh_emit", text)


def test_scratch_size_grows_with_the_grid():
    f = _capi.load().dgr_mesh_scratch_bytes
    assert f(None) == 0 and f(_grid(nx=2048, ny=1024, nz=1024)) == 0 and f(_grid(nx=0)) == 0 and f(_grid(voxel=NAN)) == 0
    last = 0
    for n in (1, 2, 9, 33, 34, 43, 256, 1024):
        b = f(_grid(nx=n, ny=n, nz=n))
        cells = max(n - 1, 0) ** 3
        # a record per 256-cell block and a header; a loose upper bound against a runaway layout
        assert b % 8 == 0 and 0 < b <= 64 + 16 * ((cells + 255) // 256) and b >= 8 * ((cells + 255) // 256) and b >= last, n
        last = b


def test_python_surface():
    keyword_only(slam.tsdf_integrate, ["vol", "depth", "viewmatrices", "fx", "fy", "cx", "cy"],
                 dict(color=None, mask_image=None, mask_threshold=0.99, weight=1.0, depth_range=(0.0, INF), near=0.05, max_weight=INF))
    keyword_only(slam.extract_mesh, ["vol"], dict(min_weight=1.0, max_triangles=None))
    keyword_only(slam.TsdfVolume.__init__, ["self", "origin", "voxel_size", "dims"], dict(truncation=None, color=True))
    assert slam.TsdfMesh._fields == ("vertices", "colors", "count", "flags")
    assert slam.tsdf_integrate is fusion.tsdf_integrate and slam.extract_mesh is fusion.extract_mesh
    assert slam.TsdfVolume is fusion.TsdfVolume and slam.TsdfMesh is fusion.TsdfMesh


def test_the_volume_on_the_host():
    v = slam.TsdfVolume((-1.0, -0.9, 1.3), 0.05, (40, 36, 28), device="cpu")
    assert tuple(v.volume.shape) == (28, 36, 40, 2) and tuple(v.color.shape) == (28, 36, 40, 4) and v.truncation == pytest.approx(0.2)
    assert v.volume.dtype == v.color.dtype == torch.float32 and not v.volume.any() and not v.color.any()
    v.volume += 1.0
    v.color += 2.0
    ptrs = v.volume.data_ptr(), v.color.data_ptr()
    v.reset()
    assert not v.volume.any() and not v.color.any() and ptrs == (v.volume.data_ptr(), v.color.data_ptr())
    g = v.grid()
    assert (g.nx, g.ny, g.nz) == (40, 36, 28) and list(g.origin) == pytest.approx([-1.0, -0.9, 1.3]) and g.voxel_size == pytest.approx(0.05)
    assert slam.TsdfVolume((0, 0, 0), 0.1, (2, 2, 2), color=False, truncation=0.25, device="cpu").color is None
    b = slam.TsdfVolume.from_bounds((-1.0, 0.0, 0.5), (1.0, 0.5, 0.5), 0.25, device="cpu")
    assert b.dims == (9, 3, 1) and b.origin == (-1.0, 0.0, 0.5)
    assert slam.TsdfVolume.from_bounds((0, 0, 0), (1.01, 1, 1), 0.5, device="cpu").dims == (4, 3, 3)
    for bad, match in ((dict(dims=(0, 2, 2)), "dims must be positive"), (dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=NAN), "voxel_size"),
                       (dict(truncation=-1.0), "truncation"), (dict(dims=(2048, 1024, 1024)), "2\\^31"), (dict(origin=(0, NAN, 0)), "origin"),
                       (dict(dims=(2, 2)), "three entries")):
        kw = dict(origin=(0, 0, 0), voxel_size=0.1, dims=(2, 2, 2), device="meta")
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            slam.TsdfVolume(kw.pop("origin"), kw.pop("voxel_size"), kw.pop("dims"), **kw)
    with pytest.raises(ValueError, match="hi >= lo"):
        slam.TsdfVolume.from_bounds((0, 0, 0), (1, -1, 1), 0.5, device="cpu")


def test_python_surface_refuses_what_it_cannot_read():
    """every check runs on the host, the device check last: CPU tensors reach each of them and never the library"""
    v = slam.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    d, m = torch.ones(2, 6, 8), torch.eye(4).repeat(2, 1, 1)
    ok = dict(fx=10.0, fy=10.0, cx=4.0, cy=3.0)
    f = slam.tsdf_integrate
    with pytest.raises(ValueError, match="must live on the GPU"):
        f(v, d, m, **ok)
    with pytest.raises(ValueError, match="must live on the GPU"):
        f(v, d[0], m[0], **ok, color=torch.ones(3, 6, 8), mask_image=torch.ones(6, 8))
    with pytest.raises(ValueError, match="must be a TsdfVolume"):
        f(None, d, m, **ok)
    with pytest.raises(ValueError, match=r"depth must be \[V, H, W\]"):
        f(v, torch.ones(2, 3, 6, 8), m, **ok)
    with pytest.raises(ValueError, match="viewmatrices must be float32"):
        f(v, d, m[:1], **ok)
    with pytest.raises(ValueError, match="depth must be float32"):
        f(v, d.double(), m, **ok)
    with pytest.raises(ValueError, match="color must be float32"):
        f(v, d, m, **ok, color=torch.ones(2, 6, 8))
    with pytest.raises(ValueError, match="mask_image must be float32"):
        f(v, d, m, **ok, mask_image=torch.ones(2, 6, 9))
    with pytest.raises(ValueError, match="color=False"):
        f(slam.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), color=False, device="cpu"), d, m, **ok, color=torch.ones(2, 3, 6, 8))
    with pytest.raises(ValueError, match="fx and fy"):
        f(v, d, m, fx=0.0, fy=10.0, cx=4.0, cy=3.0)
    with pytest.raises(ValueError, match="must live on the GPU"):
        slam.extract_mesh(v)
    with pytest.raises(ValueError, match="must be a TsdfVolume"):
        slam.extract_mesh(v.volume)
    with pytest.raises(ValueError, match="min_weight must not be NaN"):
        slam.extract_mesh(v, min_weight=NAN)
    with pytest.raises(ValueError, match="max_triangles must be"):
        slam.extract_mesh(v, max_triangles=-1)


def test_python_surface_takes_more_views_than_a_chunk():
    """V > 256 passes every shape check (the device check, the last one, is what refuses CPU tensors); a wrong V anywhere is named"""
    v = slam.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    ok = dict(fx=10.0, fy=10.0, cx=4.0, cy=3.0)
    for V in (257, 600):
        d, m, c, k = torch.ones(V, 6, 8), torch.eye(4).repeat(V, 1, 1), torch.ones(V, 3, 6, 8), torch.ones(V, 6, 8)
        with pytest.raises(ValueError, match="must live on the GPU"):
            slam.tsdf_integrate(v, d, m, **ok, color=c, mask_image=k)
        with pytest.raises(ValueError, match="must live on the GPU"):  # strided: every other view of a batch twice as long
            slam.tsdf_integrate(v, d.repeat(2, 1, 1)[::2], m.repeat(2, 1, 1)[::2], **ok, color=c.repeat(2, 1, 1, 1)[::2])
        with pytest.raises(ValueError, match=rf"viewmatrices must be float32 \[{V}, 4, 4\]"):
            slam.tsdf_integrate(v, d, m[:256], **ok)
        with pytest.raises(ValueError, match=rf"color must be float32 \[{V}, 3, 6, 8\]"):
            slam.tsdf_integrate(v, d, m, **ok, color=c[:V - 1])
        with pytest.raises(ValueError, match=rf"mask_image must be float32 \[{V}, 6, 8\]"):
            slam.tsdf_integrate(v, d, m, **ok, mask_image=k[:256])


@pytest.mark.gpu
def test_sixty_five_thousand_blind_views_in_one_call_leave_the_sample_alone():
    """n_views = 65 536 through the C ABI (256 chunks of the view loop), a 1 x 1 x 1 lattice, a 1 x 1 image: DGR_OK, the bits kept"""
    import numpy as np
    import tsdf_model as M
    V, dev = 1 << 16, torch.device("cuda:0")
    origin, voxel = (0.011, -0.017, 1.47), 0.05
    kinds = np.stack([M.pose(rx, ry, 0.0, t) for rx, ry, t in M.BLIND_KINDS])
    one = np.full((len(kinds), 1, 1), M.BLIND_DEPTH, dtype=np.float32)
    start = np.array([[[[0.375, 1.25]]]], dtype=np.float32), np.array([[[[0.25, 0.5, 0.75, 0.0]]]], dtype=np.float32)
    model = M.integrate(start[0], start[1], origin, voxel, 0.2, one, kinds, 0.9, 0.9, 0.1, -0.1, color=np.repeat(one[:, None], 3, axis=1))
    assert not model[3].any() and not model[2].any()  # blind in the model, and not next to a decision
    views = torch.from_numpy(np.ascontiguousarray(np.tile(kinds, (V // len(kinds) + 1, 1, 1))[:V])).to(dev)
    depth = torch.full((V, 1, 1), M.BLIND_DEPTH, dtype=torch.float32, device=dev)
    image = torch.full((V, 3, 1, 1), M.BLIND_COLOR, dtype=torch.float32, device=dev)
    volume, color = torch.from_numpy(start[0]).to(dev), torch.from_numpy(start[1]).to(dev)
    grid = _capi.TsdfGrid(1, 1, 1, (C.c_float * 3)(*origin), voxel)
    params = _capi.TsdfParams(0.9, 0.9, 0.1, -0.1, 0.2, 1.0, INF, 0.0, INF, 0.05, 0.99)
    rc = _capi.load().dgr_tsdf_integrate(_capi.stream_handle(0), grid, volume.data_ptr(), color.data_ptr(), V, 1, 1, depth.data_ptr(),
                                         image.data_ptr(), None, views.data_ptr(), params)
    assert rc == _capi.DGR_OK, _capi.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(volume.cpu().numpy().view(np.uint32), start[0].view(np.uint32))
    assert np.array_equal(color.cpu().numpy().view(np.uint32), start[1].view(np.uint32))
    # and with the last view the one that sees it, the sample is that view's: the loop reached view 65 535
    views[V - 1] = torch.from_numpy(M.pose(0.0, 0.0, 0.0, [0.0, 0.0, 0.0])).to(dev)
    rc = _capi.load().dgr_tsdf_integrate(_capi.stream_handle(0), grid, volume.data_ptr(), color.data_ptr(), V, 1, 1, depth.data_ptr(),
                                         image.data_ptr(), None, views.data_ptr(), params)
    assert rc == _capi.DGR_OK, _capi.last_error()
    torch.cuda.synchronize()
    # depth 2 is more than a truncation in front of z = 1.47: t = 1, (x w + t) / (w + 1) with w = 1.25; two products, a sum and a
    # quotient of values <= 1, half an epsilon each: 2 eps
    got, gcol, eps = volume.cpu().numpy().astype(np.float64), color.cpu().numpy().astype(np.float64), float(np.finfo(np.float32).eps)
    print(f"tsdf-measured 65536 views, the last one live: weight {got[0, 0, 0, 1]} tsdf error {abs(got[0, 0, 0, 0] - (0.375 * 1.25 + 1.0) / 2.25):.3e} "
          f"(bound {2 * eps:.3e})")
    assert got[0, 0, 0, 1] == 2.25 and abs(got[0, 0, 0, 0] - (0.375 * 1.25 + 1.0) / 2.25) <= 2 * eps
    assert np.abs(gcol[0, 0, 0, :3] - (start[1][0, 0, 0, :3].astype(np.float64) * 1.25 + M.BLIND_COLOR) / 2.25).max() <= 2 * eps and gcol[0, 0, 0, 3] == 0.0
