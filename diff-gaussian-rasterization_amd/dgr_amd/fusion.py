"""TSDF fusion of rendered views, mesh extraction and ray-casting on the device (C ABI: dgr_tsdf_integrate, dgr_mesh_plan,
dgr_mesh_emit, dgr_tsdf_bricks, dgr_tsdf_raycast): the surface a dense RGB-D SLAM run hands over at the end -- what CG-SLAM,
SplaTAM, MonoGS and the Point-SLAM family get from Open3D on the host: depth and colour rendered at the keyframe poses, fused
into a truncated signed distance volume, its zero level as a triangle mesh (marching tetrahedra), and the volume seen from any
pose (depth, normals, colour: KinectFusion's model frame)."""
import math as _math
from typing import NamedTuple as _NamedTuple

import torch

from . import _capi

_INF = float("inf")


class TsdfVolume:
    """A dense lattice of `dims` = (Nx, Ny, Nz) samples, sample (ix, iy, iz) at origin + voxel_size (ix, iy, iz), x fastest:
    `volume` float32 [Nz, Ny, Nx, 2] = (tsdf in [-1, 1], weight >= 0) and, with `color`, `color` float32 [Nz, Ny, Nx, 4] =
    (r, g, b, 0).  Plain tensors: keep, save or zero them.  `truncation` defaults to 4 voxels.  Nx Ny Nz < 2^31."""

    def __init__(self, origin, voxel_size, dims, *, truncation=None, color=True, device="cuda"):
        origin, dims, voxel_size = tuple(float(v) for v in origin), tuple(int(v) for v in dims), float(voxel_size)
        if len(origin) != 3 or len(dims) != 3:
            raise ValueError(f"TsdfVolume: origin and dims have three entries each, not {len(origin)} and {len(dims)}")
        if not all(_math.isfinite(v) for v in origin):
            raise ValueError(f"TsdfVolume: origin must be finite, not {origin}")
        if not (_math.isfinite(voxel_size) and voxel_size > 0.0):
            raise ValueError(f"TsdfVolume: voxel_size must be finite and positive, not {voxel_size}")
        if min(dims) < 1:
            raise ValueError(f"TsdfVolume: dims must be positive, not {dims}")
        if dims[0] * dims[1] * dims[2] >= 1 << 31:
            raise ValueError(f"TsdfVolume: dims {dims} hold 2^31 samples or more")
        truncation = 4.0 * voxel_size if truncation is None else float(truncation)
        if not (_math.isfinite(truncation) and truncation > 0.0):
            raise ValueError(f"TsdfVolume: truncation must be finite and positive, not {truncation}")
        self.origin, self.voxel_size, self.dims, self.truncation = origin, voxel_size, dims, truncation
        self.device = torch.device(device)
        nx, ny, nz = dims
        self.volume = torch.zeros((nz, ny, nx, 2), dtype=torch.float32, device=self.device)
        self.color = torch.zeros((nz, ny, nx, 4), dtype=torch.float32, device=self.device) if color else None

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size, **kw):
        """the smallest lattice with a sample at `lo` whose samples reach `hi` on every axis"""
        lo, hi, voxel_size = tuple(float(v) for v in lo), tuple(float(v) for v in hi), float(voxel_size)
        if len(lo) != 3 or len(hi) != 3 or not all(h >= l for l, h in zip(lo, hi)):
            raise ValueError(f"TsdfVolume.from_bounds: lo and hi must be three-vectors with hi >= lo, not {lo} and {hi}")
        if not (_math.isfinite(voxel_size) and voxel_size > 0.0):
            raise ValueError(f"TsdfVolume: voxel_size must be finite and positive, not {voxel_size}")
        dims = tuple(int(_math.ceil((h - l) / voxel_size - 1e-9)) + 1 for l, h in zip(lo, hi))
        return cls(lo, voxel_size, dims, **kw)

    def reset(self):
        """back to empty (in place: a captured graph keeps pointing at the same tensors)"""
        self.volume.zero_()
        if self.color is not None:
            self.color.zero_()

    def grid(self):
        return _capi.TsdfGrid(*self.dims, (_capi._f * 3)(*self.origin), self.voxel_size)


class TsdfMesh(_NamedTuple):
    """An unindexed triangle list on the device: `vertices` float32 [3 T, 3]; `colors` float32 [3 T, 3] or None; `count` int32
    [1] = the triangles the volume needs; `flags` int32 [1], bit 0 = they did not fit `max_triangles`."""
    vertices: torch.Tensor
    colors: torch.Tensor
    count: torch.Tensor
    flags: torch.Tensor


def _image(what, name, t, shape, dev):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, not {type(t).__name__}")
    if t.dtype != torch.float32 or tuple(t.shape) != shape:
        raise ValueError(f"{what}: {name} must be float32 {list(shape)}, not {t.dtype} {list(t.shape)}")
    if t.device != dev:
        raise ValueError(f"{what}: {name} is on {t.device}, the volume on {dev}")
    return t.contiguous()


def tsdf_integrate(vol, depth, viewmatrices, fx, fy, cx, cy, *, color=None, mask_image=None, mask_threshold=0.99, weight=1.0,
                   depth_range=(0.0, _INF), near=0.05, max_weight=_INF):
    """Fuses V views into `vol` (a TsdfVolume) in ONE launch: every sample is read once and written at most once, whatever V is.
    `depth` [V, H, W] (or [H, W] with a [4, 4] pose), `color` [V, 3, H, W] or None (the colour volume then stays as it is),
    `mask_image` [V, H, W] or None (a render's opacity_map: pixels at or below `mask_threshold` are not fused), `viewmatrices`
    [V, 4, 4] = W2C^T, pixel (x, y) at depth d = ((x - cx) / fx d, (y - cy) / fy d, d) as in keyframe_overlap and icp_align.
    Per sample and view, in order: skip unless z > near, the nearest pixel is inside the image, depth_range[0] < d <
    depth_range[1] and the mask passes; sdf = d - z, skip if sdf < -truncation; t = min(1, sdf / truncation); tsdf = (tsdf w + t
    weight) / (w + weight), colour likewise, w = min(w + weight, max_weight) (include/dgr_hip.h: dgr_tsdf_integrate).
    No atomics, the same bits on every run, nothing read on the host: capturable into a hipGraph.  Returns `vol`."""
    what = "tsdf_integrate"
    if not isinstance(vol, TsdfVolume):
        raise ValueError(f"{what}: vol must be a TsdfVolume, not {type(vol).__name__}")
    if not isinstance(depth, torch.Tensor) or not isinstance(viewmatrices, torch.Tensor):
        raise ValueError(f"{what}: depth and viewmatrices must be tensors")
    if depth.dim() == 2 and viewmatrices.dim() == 2:
        depth, viewmatrices = depth[None], viewmatrices[None]
        color = color[None] if isinstance(color, torch.Tensor) and color.dim() == 3 else color
        mask_image = mask_image[None] if isinstance(mask_image, torch.Tensor) and mask_image.dim() == 2 else mask_image
    if depth.dim() != 3 or depth.size(0) < 1 or depth.size(1) < 1 or depth.size(2) < 1:
        raise ValueError(f"{what}: depth must be [V, H, W] with V, H, W >= 1, not {list(depth.shape)}")
    V, H, W = (int(n) for n in depth.shape)
    dev = vol.device
    depth = _image(what, "depth", depth, (V, H, W), dev)
    viewmatrices = _image(what, "viewmatrices", viewmatrices, (V, 4, 4), dev)
    if color is not None:
        if vol.color is None:
            raise ValueError(f"{what}: color given, but the volume was made with color=False")
        color = _image(what, "color", color, (V, 3, H, W), dev)
    if mask_image is not None:
        mask_image = _image(what, "mask_image", mask_image, (V, H, W), dev)
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    if not (_math.isfinite(fx) and _math.isfinite(fy) and fx > 0.0 and fy > 0.0):
        raise ValueError(f"{what}: fx and fy must be finite and positive, not {(fx, fy)}")
    lo, hi = (float(v) for v in depth_range)
    params = _capi.TsdfParams(fx, fy, cx, cy, vol.truncation, float(weight), float(max_weight), lo, hi, float(near),
                              float(mask_threshold))
    if dev.type != "cuda":
        raise ValueError(f"{what}: the volume must live on the GPU (there is no CPU fallback)")
    p = _capi.ptr
    _capi.call("dgr_tsdf_integrate", dev, vol.grid(), p(vol.volume), p(vol.color) if color is not None else None, V, W, H, p(depth),
               p(color), p(mask_image), p(viewmatrices), params)
    return vol


def extract_mesh(vol, *, min_weight=1.0, max_triangles=None):
    """The zero level of `vol` by marching tetrahedra (Kuhn's six-tetrahedron split of every cell: no ambiguous cases, watertight
    across cells).  A cell counts when its 8 samples have weight >= `min_weight`; a sample is inside when tsdf < 0; triangle
    normals point towards free space; vertices are not welded, but equal points have equal bits (include/dgr_hip.h: dgr_mesh_plan).
    Three launches: count, scan, emit.  `max_triangles=None`: the count is read on the host (the step's only synchronisation) and
    the outputs are allocated exactly.  With a capacity nothing is read: capturable; `count` then says what was needed and bit 0
    of `flags` whether it did not fit.  Returns TsdfMesh."""
    what = "extract_mesh"
    if not isinstance(vol, TsdfVolume):
        raise ValueError(f"{what}: vol must be a TsdfVolume, not {type(vol).__name__}")
    min_weight = float(min_weight)
    if min_weight != min_weight:
        raise ValueError(f"{what}: min_weight must not be NaN")
    if max_triangles is not None:
        max_triangles = int(max_triangles)
        if max_triangles < 0 or max_triangles >= 1 << 31:
            raise ValueError(f"{what}: max_triangles must be 0 .. 2^31 - 1, not {max_triangles}")
    dev = vol.device
    if dev.type != "cuda":
        raise ValueError(f"{what}: the volume must live on the GPU (there is no CPU fallback)")
    grid = vol.grid()
    nbytes = _capi.load().dgr_mesh_scratch_bytes(grid)
    if nbytes == 0:
        raise ValueError(f"{what}: the library refuses a grid of {vol.dims} samples")
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    words = torch.empty((2,), dtype=torch.int32, device=dev)
    count, flags = words[:1], words[1:]
    p = _capi.ptr
    with _capi.StepCalls(dev) as abi:
        cap = (1 << 31) - 1 if max_triangles is None else max_triangles
        abi.call("dgr_mesh_plan", grid, p(vol.volume), min_weight, cap, p(scratch), count.data_ptr(), flags.data_ptr())
        if max_triangles is None:
            cap = int(count.item())
        vertices = torch.empty((3 * cap, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((3 * cap, 3), dtype=torch.float32, device=dev) if vol.color is not None else None
        abi.call("dgr_mesh_emit", grid, p(vol.volume), p(vol.color), min_weight, cap, p(scratch), p(vertices), p(colors))
    return TsdfMesh(vertices, colors, count, flags)


class TsdfRaycast(_NamedTuple):
    """A ray-cast of the volume: `depth` float32 [V, H, W] (0 without a hit), `vnmap` float32 [V, H, W, 4] = (normal in the camera
    frame, depth), what depth_normals writes and icp_step reads, or None; `color` float32 [V, 3, H, W] or None; `flags` uint8
    [V, H, W] or None: bit 0 a hit, bit 1 the ray ended unseen (inside the surface or behind unmeasured space), bit 2 a hit
    without a normal.  With a [4, 4] pose the leading V is dropped."""
    depth: torch.Tensor
    vnmap: torch.Tensor
    color: torch.Tensor
    flags: torch.Tensor


def _min_weight(what, min_weight):
    min_weight = float(min_weight)
    if min_weight != min_weight:
        raise ValueError(f"{what}: min_weight must not be NaN")
    return min_weight


def _brick_shape(dims):
    return tuple(-(-(n - 1) // 8) for n in reversed(dims))


def tsdf_bricks(vol, *, min_weight=1.0):
    """The map of live bricks that lets tsdf_raycast jump over empty space: uint8 [ceil((Nz-1)/8), ceil((Ny-1)/8), ceil((Nx-1)/8)],
    1 iff the brick of 8 x 8 x 8 cells holds a cell whose 8 weights are >= `min_weight` and that has a corner with tsdf <= 0
    (only such a cell can end a ray).  One launch, exact, no atomics, capturable.  Build it again after the volume changed."""
    what = "tsdf_bricks"
    if not isinstance(vol, TsdfVolume):
        raise ValueError(f"{what}: vol must be a TsdfVolume, not {type(vol).__name__}")
    min_weight = _min_weight(what, min_weight)
    dev = vol.device
    if dev.type != "cuda":
        raise ValueError(f"{what}: the volume must live on the GPU (there is no CPU fallback)")
    bricks = torch.empty(_brick_shape(vol.dims), dtype=torch.uint8, device=dev)
    if _capi.load().dgr_tsdf_brick_bytes(vol.grid()) != bricks.numel():
        raise ValueError(f"{what}: the library refuses a grid of {vol.dims} samples")
    _capi.call("dgr_tsdf_bricks", dev, vol.grid(), _capi.ptr(vol.volume), min_weight, _capi.ptr(bricks))
    return bricks


def tsdf_raycast(vol, viewmatrices, fx, fy, cx, cy, H, W, *, depth_range=(0.05, _INF), step=None, min_weight=1.0, bricks="build",
                 normals=True, color=None, return_flags=False):
    """The volume seen from V poses in one launch, one lane per ray: `viewmatrices` [V, 4, 4] = W2C^T (or [4, 4]: the results then
    lose their leading V), pixel (x, y) at depth z = the camera point ((x - cx) / fx z, (y - cy) / fy z, z), as in tsdf_integrate.
    The ray is sampled at z_k = depth_range[0] + k step < depth_range[1] (`step` in metres of depth, None = half a voxel); a
    sample counts when its cell's 8 weights are >= `min_weight`, and its value is the trilinear interpolant.  The first sample
    with a value <= 0 ends the ray: a hit when the sample before it counts and is > 0 (depth by linear interpolation between the
    two, normal from central differences of the interpolant a voxel either side, turned to the camera, colour by trilinear
    interpolation), otherwise no depth (flags bit 1).  include/dgr_hip.h: dgr_tsdf_raycast.
    `bricks`: "build" makes the map of live bricks first (tsdf_bricks: two launches in all), a tensor from tsdf_bricks reuses one
    (same volume, same min_weight), None marches every sample; the results are the same bits either way.  `normals=False` leaves
    vnmap out, `color` (None: as the volume has one) the colour, `return_flags` adds the flags.  Nothing is read on the host:
    capturable.  Returns TsdfRaycast(depth, vnmap, color, flags)."""
    what = "tsdf_raycast"
    if not isinstance(vol, TsdfVolume):
        raise ValueError(f"{what}: vol must be a TsdfVolume, not {type(vol).__name__}")
    if not isinstance(viewmatrices, torch.Tensor):
        raise ValueError(f"{what}: viewmatrices must be a tensor, not {type(viewmatrices).__name__}")
    single = viewmatrices.dim() == 2
    if single:
        viewmatrices = viewmatrices[None]
    if viewmatrices.dim() != 3 or viewmatrices.size(0) < 1:
        raise ValueError(f"{what}: viewmatrices must be [V, 4, 4] with V >= 1 or [4, 4], not {list(viewmatrices.shape)}")
    V, H, W = int(viewmatrices.size(0)), int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"{what}: H and W must be positive, not {(H, W)}")
    dev = vol.device
    viewmatrices = _image(what, "viewmatrices", viewmatrices, (V, 4, 4), dev)
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    if not (_math.isfinite(fx) and _math.isfinite(fy) and fx > 0.0 and fy > 0.0):
        raise ValueError(f"{what}: fx and fy must be finite and positive, not {(fx, fy)}")
    lo, hi = (float(v) for v in depth_range)
    if not _math.isfinite(lo) or hi != hi:
        raise ValueError(f"{what}: depth_range must start at a finite depth and not end at NaN, not {(lo, hi)}")
    step = 0.5 * vol.voxel_size if step is None else float(step)
    if not (_math.isfinite(step) and step > 0.0):
        raise ValueError(f"{what}: step must be finite and positive, not {step}")
    min_weight = _min_weight(what, min_weight)
    color = vol.color is not None if color is None else bool(color)
    if color and vol.color is None:
        raise ValueError(f"{what}: color asked for, but the volume was made with color=False")
    if isinstance(bricks, torch.Tensor):
        if bricks.dtype != torch.uint8 or tuple(bricks.shape) != _brick_shape(vol.dims) or bricks.device != dev:
            raise ValueError(f"{what}: bricks must be the uint8 {list(_brick_shape(vol.dims))} tensor tsdf_bricks returns for this "
                             f"volume, not {bricks.dtype} {list(bricks.shape)} on {bricks.device}")
        bricks = bricks.contiguous()
    elif bricks is not None and bricks != "build":
        raise ValueError(f"{what}: bricks must be \"build\", None or a tensor from tsdf_bricks, not {bricks!r}")
    if dev.type != "cuda":
        raise ValueError(f"{what}: the volume must live on the GPU (there is no CPU fallback)")
    if isinstance(bricks, str):
        bricks = tsdf_bricks(vol, min_weight=min_weight)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    vnmap = torch.empty((V, H, W, 4), dtype=torch.float32, device=dev) if normals else None
    color_out = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev) if color else None
    flags = torch.empty((V, H, W), dtype=torch.uint8, device=dev) if return_flags else None
    params = _capi.RaycastParams(fx, fy, cx, cy, lo, hi, step, min_weight)
    p = _capi.ptr
    _capi.call("dgr_tsdf_raycast", dev, vol.grid(), p(vol.volume), p(vol.color) if color else None,
               p(bricks), V, W, H, p(viewmatrices), params, p(depth), p(vnmap), p(color_out), p(flags))
    if single:
        depth, vnmap, color_out, flags = (None if t is None else t[0] for t in (depth, vnmap, color_out, flags))
    return TsdfRaycast(depth, vnmap, color_out, flags)
