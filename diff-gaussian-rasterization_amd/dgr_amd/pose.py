"""Camera and pose helpers: the projection matrix, (quaternion, translation) -> the rasterizer's camera tensors, and the small
tensors kept between calls.  The rasterizer takes W2C^T (cuda_rasterizer/auxiliary.h:58-77 reads 16 floats column-major):
`viewmatrix` here is always the transpose of the world-to-camera matrix, rotation entry R[j][i] at [i][j] and the translation in
the last ROW; `projmatrix` is W2C^T Proj^T and the camera centre is -(R^T t).  dgr_amd.slam states the whole convention."""
import torch

from . import _capi


_proj_cache = {}


def projection_matrix(tanfovx, tanfovy, znear=0.01, zfar=100.0, device=None, dtype=torch.float32):
    """Proj (row-major math, z forward, as 3DGS `getProjectionMatrix` with symmetric frustum).  Cached per argument set
    (treat the result as read-only): building it copies host scalars to the device, which a hipGraph capture forbids,
    so a captured step finds the matrix its eager warm-up made."""
    key = (float(tanfovx), float(tanfovy), float(znear), float(zfar), str(device), dtype)
    P = _proj_cache.get(key)
    if P is None:
        P = torch.zeros((4, 4), dtype=dtype)
        P[0, 0] = 1.0 / tanfovx
        P[1, 1] = 1.0 / tanfovy
        P[2, 2] = zfar / (zfar - znear)
        P[2, 3] = -(zfar * znear) / (zfar - znear)
        P[3, 2] = 1.0
        P = _proj_cache[key] = P.to(device) if device is not None else P
    return P


_const_cache = {}


def _constants(device, dtype):
    """(identity, Levi-Civita tensor, bottom row) on `device`, built once (host -> device copies are not capturable)."""
    key = (str(device), dtype)
    c = _const_cache.get(key)
    if c is None:
        eps = torch.zeros((3, 3, 3), dtype=dtype)
        for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            eps[i, j, k], eps[i, k, j] = 1.0, -1.0
        c = _const_cache[key] = (torch.eye(3, dtype=dtype).to(device), eps.to(device),
                                 torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=dtype).to(device))
    return c


def quat_to_rotmat(q):
    """Unit quaternion (r, x, y, z) -> 3x3 rotation, differentiable (q is normalised here).
    R = (r^2 - |v|^2) I + 2 v v^T + 2 r [v]x in a dozen tensor operations (a tracking loop is launch-bound)."""
    eye, eps, _ = _constants(q.device, q.dtype)
    q = q / q.norm()
    r, v = q[0], q[1:]
    cross = -(eps * v).sum(-1)  # [v]x: cross[i][j] = -eps[i][j][k] v[k]
    return (r * r - (v * v).sum()) * eye + 2.0 * v.unsqueeze(1) * v.unsqueeze(0) + (2.0 * r) * cross


def w2c_from_quat_trans(q, t):
    """World-to-camera 4x4 from a quaternion and a translation (both differentiable leaves of a tracking step)."""
    top = torch.cat([quat_to_rotmat(q), t.reshape(3, 1)], dim=1)
    return torch.cat([top, _constants(q.device, q.dtype)[2]], dim=0)


def _small_matmul(a, b):
    """a @ b for 3x3 / 4x4 operands as one broadcast multiply and one sum: a BLAS call for sixteen numbers costs more
    host time on ROCm (≈1.5 ms: handle and heuristics) than the whole render."""
    return (a.unsqueeze(-1) * b.unsqueeze(-3)).sum(-2)


def camera_tensors(w2c, tanfovx, tanfovy, znear=0.01, zfar=100.0):
    """(viewmatrix, projmatrix, perspec_matrix, campos) for the rasterizer from a world-to-camera matrix.
    `viewmatrix` stays attached to `w2c`'s graph; the other three are detached (see the module docstring)."""
    P = projection_matrix(tanfovx, tanfovy, znear, zfar, device=w2c.device, dtype=w2c.dtype)
    viewmatrix = w2c.transpose(0, 1).contiguous()
    with torch.no_grad():
        perspec = P.transpose(0, 1).contiguous()
        projmatrix = _small_matmul(w2c.transpose(0, 1), P.transpose(0, 1)).contiguous()
        campos = (-(w2c[:3, :3] * w2c[:3, 3:4]).sum(0)).contiguous()  # -(R^T t)
    return viewmatrix, projmatrix, perspec, campos


class _PoseToCamera(torch.autograd.Function):
    """(quaternion, translation) -> (viewmatrix, projmatrix, campos) in one launch, dL/dviewmatrix -> (dL/dq, dL/dt) in
    another (C ABI: dgr_pose_forward / dgr_pose_backward).  Same function as
    `camera_tensors(w2c_from_quat_trans(q, t), ...)`: only `viewmatrix` carries a gradient."""

    @staticmethod
    def forward(ctx, q, t, perspec):
        q, t, perspec = q.contiguous(), t.contiguous(), perspec.contiguous()
        out = torch.empty((35,), dtype=torch.float32, device=q.device)
        view, proj, campos = out[:16].view(4, 4), out[16:32].view(4, 4), out[32:35]
        _capi.call("dgr_pose_forward", q.device, q.data_ptr(), t.data_ptr(), perspec.data_ptr(), view.data_ptr(), proj.data_ptr(),
                   campos.data_ptr())
        ctx.save_for_backward(q)
        ctx.mark_non_differentiable(proj, campos)
        return view, proj, campos

    @staticmethod
    def backward(ctx, dview, _dproj, _dcampos):
        (q,) = ctx.saved_tensors
        grads = torch.empty((7,), dtype=torch.float32, device=q.device)
        dview = dview.contiguous()
        _capi.call("dgr_pose_backward", q.device, q.data_ptr(), dview.data_ptr(), grads.data_ptr(), grads[4:].data_ptr())
        return grads[:4], grads[4:], None


# ---- tensors kept between calls (_Kept, below) are made by kernels of whichever stream was current at their first use.  A
# later call on ANOTHER stream (dgr_amd.multiview.ViewStreams: a stream per view) must not read them before those kernels have
# finished: every entry carries a stamp -- the creating stream and an event recorded behind the kernels that wrote the
# tensors -- and a consumer on a different stream waits for that event once (per stream).  While a hipGraph is being recorded
# nothing is stored.  The keys of the camera caches are (id, _version) of the source tensors: an in-place `viewmatrix.data = ...`
# swap changes neither and is NOT supported for cached poses -- assign a new tensor, or update it in place with copy_().
class _Stamp:
    __slots__ = ("device", "stream", "event", "seen")

    def __init__(self, device):
        self.device = device
        st = torch.cuda.current_stream(device)
        self.stream = int(st.cuda_stream)
        self.event = torch.cuda.Event()
        self.event.record(st)
        self.seen = {self.stream}

    def order(self):
        # (the raw handle first: building a Stream object per call costs more than the tensors the cache saves)
        index = self.device.index
        h = torch._C._cuda_getCurrentRawStream(index if index is not None else torch.cuda.current_device())
        if h not in self.seen:
            torch.cuda.current_stream(self.device).wait_event(self.event)
            if len(self.seen) < 64:
                self.seen.add(h)


class _Kept:
    """A few values (tensors, or tuples of them) kept between calls: at most `limit` entries, the oldest dropped first."""
    __slots__ = ("limit", "entries")

    def __init__(self, limit):
        self.limit, self.entries = limit, {}  # key -> (value, _Stamp or None)

    def get(self, key):
        """The value kept under `key`, with its device's current stream ordered behind the kernels that made it; else None."""
        hit = self.entries.get(key)
        if hit is None:
            return None
        if hit[1] is not None:
            hit[1].order()
        return hit[0]

    def put(self, key, value, device):
        """Keeps `value`, which the current stream of `device` has just made -- unless that stream is being recorded into a
        hipGraph (a replay re-derives it).  Returns `value`."""
        cuda = device.type == "cuda"
        if not (cuda and torch.cuda.is_current_stream_capturing()):
            if len(self.entries) >= self.limit:
                self.entries.pop(next(iter(self.entries)))
            self.entries[key] = (value, _Stamp(device) if cuda else None)
        return value


_PERSPEC = _Kept(32)  # (tanfovx, tanfovy, znear, zfar, device) -> Proj^T: a constant of the sensor, built once


def _perspec_cached(tanfovx, tanfovy, znear, zfar, device):
    key = (float(tanfovx), float(tanfovy), float(znear), float(zfar), device)
    m = _PERSPEC.get(key)
    if m is None:
        m = projection_matrix(tanfovx, tanfovy, znear, zfar, device=device).transpose(0, 1).contiguous()
        _PERSPEC.put(key, m, m.device)
    return m


def pose_to_camera(q, t, tanfovx, tanfovy, znear=0.01, zfar=100.0):
    """(viewmatrix, projmatrix, perspec_matrix, campos) from a quaternion (r, x, y, z) and a translation, float32 GPU
    tensors: the fused form of `camera_tensors(w2c_from_quat_trans(q, t), tanfovx, tanfovy)` (2 launches for forward +
    backward instead of ~40 elementwise torch kernels).  The perspec_matrix is a symmetric frustum's (principal point at the
    image centre); an off-centre camera goes through `render(viewpoint_camera=...)` with its own `projection_matrix`."""
    for x, n, name in ((q, 4, "q"), (t, 3, "t")):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.numel() != n:
            raise ValueError(f"pose_to_camera: {name} must be a float32 tensor of {n} elements")
    if not q.is_cuda or t.device != q.device:
        raise ValueError("pose_to_camera: q and t must be on one GPU (there is no CPU fallback)")
    perspec = _perspec_cached(tanfovx, tanfovy, znear, zfar, q.device)
    view, proj, campos = _PoseToCamera.apply(q, t, perspec)
    return view, proj, perspec, campos


def _matmul_fixed_order(a, b):
    """a @ b for [..., n, 4] @ [4, m] with the four products of every entry added in index order by elementwise kernels
    (see _campos: the result must not depend on whether `a` is one matrix or a slice of a stack).  Four launches."""
    r = a[..., :, 0:1] * b[0]
    for k in (1, 2, 3):
        r = torch.addcmul(r, a[..., :, k:k + 1], b[k])
    return r


def _campos(vm):
    """Camera centre -(R^T t) from viewmatrix = W2C^T ([4,4] or [V,4,4]), with the three products added in a fixed order
    by elementwise kernels: a `sum()` reduction picks its summation order from the tensor's layout and alignment, so the
    same pose gave cameras one ulp apart as a [4,4] tensor and as a slice of a [V,4,4] one.  Three launches."""
    nt = -vm[..., 3, 0:3]
    r = vm[..., :3, 0] * nt[..., 0:1]
    r = torch.addcmul(r, vm[..., :3, 1], nt[..., 1:2])
    return torch.addcmul(r, vm[..., :3, 2], nt[..., 2:3]).contiguous()


def _cameras_of(vm, perspec_src, tanfovx, tanfovy, znear, zfar):
    """(perspec, vm, projmatrix, campos) of `vm` = W2C^T, one pose [4,4] or a stack [V,4,4], detached; `perspec_src`: the
    camera's own Proj^T, or None for the symmetric frustum of the fov.  The operations of _matmul_fixed_order and _campos in
    their fixed order: a stack's cameras are those of its poses one by one, bit for bit.  Call it under no_grad."""
    perspec = perspec_src if perspec_src is not None else _perspec_cached(tanfovx, tanfovy, znear, zfar, vm.device)
    perspec = perspec.to(vm.device, torch.float32)
    return perspec, vm, _matmul_fixed_order(vm, perspec).contiguous(), _campos(vm)
