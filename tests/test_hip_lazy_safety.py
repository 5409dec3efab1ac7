"""Lazy status mode (DGR_SYNC_MODE=lazy: no host wait inside a forward) when the instance count GROWS under it.

The capacity a lazy forward renders with is a guess (1.5 x the largest count seen for the shape).  A frame past it has empty tile
lists; before round 9 it looked like a frame (background colour, zero depth) for up to lazy_depth + 1 forwards.  Now
  * its images are NaN (the blend kernels see the overflow flag), its backward yields zero gradients,
  * check_async_errors() -- the call to make before optimizer.step() -- raises,
  * the shape runs strict until its count has settled, and a count that grows by more than 25 % between two reads (or comes
    within 20 % of the capacity) sends the shape to strict BEFORE anything overflows.
The second half of the file runs these guards, and a frame whose count grows WITHIN the capacity (its backward must get an R of
at least its count: the capacity, not the largest count seen before it), on every call path of both variants: the compiled
autograd node, the Python autograd Function over the compiled and over the ctypes binding, and the batches over both.
Reference behaviour for comparison: the reference sizes its binning buffer after a blocking read of num_rendered in every
forward (L/cuda_rasterizer/rasterizer_impl.cu:287-296) and so never overflows.
"""
import numpy as np
import pytest
import torch

from util import make_scene
import hip_helpers as hh
from hip_helpers import lazy  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _leaves(s, scale=1.0):
    T = hh.T
    return [T(a).requires_grad_() for a in (s.means, s.shs, s.opac, s.scales * np.float32(scale), s.rots, s.view)]


def _step(rast, leaves, s, backward=True):
    m2 = torch.zeros((s.P, 3), device=hh.dev(), requires_grad=True)
    o = rast(means3D=leaves[0], means2D=m2, opacities=leaves[2], shs=leaves[1], scales=leaves[3], rotations=leaves[4],
             viewmatrix=leaves[5], gt_depth=hh.T(s.gt))
    if backward:
        torch.autograd.backward([o[0], o[2]], [hh.T(s.gC), hh.T(s.gD[None])])
    return o


def test_an_overflowed_lazy_forward_is_nan_not_an_empty_frame_and_raises_before_the_step(lazy):
    L = lazy
    from dgr_amd.multiview import make_settings
    s = make_scene(4000, 96, 64, 11)
    key = (hh.dev().index, s.P, s.H, s.W)
    rast = L.GaussianRasterizer(make_settings(s, 3, hh.dev()))
    for _ in range(3):                                   # the first call is strict and teaches the capacity; then lazy
        o = _step(rast, _leaves(s), s)
    L.check_async_errors()
    assert key not in L._unsettled and torch.isfinite(o[0]).all()
    R0 = L._capacity_cache[key]
    # the same P, every splat three times as large: three times the instances on this small frame, past 1.5 R0 + 4096
    big = _leaves(s, 3.0)
    o = _step(rast, big, s)
    assert torch.isnan(o[0]).all() and torch.isnan(o[2]).all() and torch.isnan(o[5]).all()      # colour, depth, alpha image
    for leaf in big[:5]:
        assert leaf.grad is not None and not leaf.grad.any()          # empty lists: nothing accumulates
    with pytest.raises(RuntimeError, match="overflow"):                # ... and this is what stands in front of optimizer.step()
        L.check_async_errors()
    assert key in L._unsettled
    # the shape is unsettled: the next forwards are strict (exact count, retried inside the call) and therefore right
    o1 = _step(rast, _leaves(s, 3.0), s)
    assert torch.isfinite(o1[0]).all() and L._capacity_cache[key] > 1.5 * R0 + 4096
    _, d_ref = hh.hip_forward(s._replace(scales=s.scales * np.float32(3.0)), 3)   # (the `_C` call: strict as well, here)
    assert np.array_equal(o1[0].detach().cpu().numpy(), d_ref["color"])
    for _ in range(4):                                    # steady count: three settled reads and the shape is lazy again
        _step(rast, _leaves(s, 3.0), s)
    L.check_async_errors()
    assert key not in L._unsettled
    n_before = len(L._pending_status)
    _step(rast, _leaves(s, 3.0), s)
    assert len(L._pending_status) == n_before + 1          # a lazy forward leaves a status word to be read later


def test_a_growing_count_sends_the_shape_to_strict_before_it_overflows(lazy):
    L = lazy
    from dgr_amd.multiview import make_settings
    s = make_scene(4000, 256, 192, 12)
    key = (hh.dev().index, s.P, s.H, s.W)
    rast = L.GaussianRasterizer(make_settings(s, 3, hh.dev()))
    scale = 1.0
    counts, strict_at = [], []
    for it in range(7):
        o = _step(rast, _leaves(s, scale), s)
        assert torch.isfinite(o[0]).all(), f"iteration {it}: a frame rendered past its capacity"
        L.check_async_errors()                           # (before the optimiser step of a real loop)
        counts.append(L._last_status[key][0] if key in L._last_status else L._capacity_cache[key])
        if key in L._unsettled:
            strict_at.append(it)
        scale *= 1.25                                     # ~50 % more instances per iteration
    assert counts[-1] > 3 * counts[0]
    assert strict_at and strict_at[0] <= 2, strict_at      # the growth was noticed at the first lazy read


# ------------------------------------------------------------------------------------------------------------------------------
# The same contract on every call path.  A lazy forward never learns its own count: it bins into a guessed capacity, and its
# backward must still get an R >= the frame's count (deterministic_grads sizes the instance-major row buffer by R; rows past it
# come back NaN -- csrc/render_light.hip: det_gather_kernel).  The growth guard (_unsettled) must hold on every path as well.
# Paths: (variant, binding), the one-view ones through GaussianRasterizer, the batches through the batch classes.
PATHS = [("light", "node"), ("light", "function"), ("light", "debug"), ("light", "ctypes"), ("light", "batch"),
         ("light", "batch-ctypes"), ("full", "node"), ("full", "function"), ("full", "ctypes"), ("full", "batch"),
         ("full", "batch-ctypes")]
V = 2  # views of a batch
GROW = 1.03  # frame B = frame A with every scale x GROW: R0 < R1 <= 1.1 R0 on every view (asserted below)


class Path:
    """forward + backward of one call path; `step(s, scale, grads)` renders frame `s` with its scales x `scale` from fresh
    leaves, back-propagates `grads` (colour, depth; per view for a batch) and returns (images, {leaf: .grad}).  `scenes`: the
    V cameras of a batch (view_index 0 .. V-1 over the same Gaussians), or the one camera."""

    def __init__(self, variant, binding, scenes):
        from dgr_amd import batch as B
        from dgr_amd import batch_full as BF
        from dgr_amd import full as F
        from dgr_amd import light as L
        self.variant, self.binding, self.ss = variant, binding, scenes
        self.batch = binding.startswith("batch")
        s, T = scenes[0], hh.T
        self.key = (hh.dev().index, s.P, s.H, s.W)
        if self.batch:
            self.views, projs, campos, self.gts = (T(np.stack([getattr(x, n) for x in scenes])) for n in ("view", "proj", "campos", "gt"))
            rs = B.BatchRasterizationSettings(image_height=s.H, image_width=s.W, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=T(s.bg),
                                              scale_modifier=1.0, viewmatrices=self.views, projmatrices=projs, sh_degree=3,
                                              campos=campos, prefiltered=False, debug=False, perspec_matrix=T(s.persp),
                                              track_off=False, map_off=False)
            self.rast = (B.GaussianRasterizerBatch if variant == "light" else BF.GaussianRasterizerBatchFull)(rs)
        elif variant == "light":
            from dgr_amd.multiview import make_settings
            self.rast = L.GaussianRasterizer(make_settings(s, 3, hh.dev(), debug=binding == "debug"))
        else:
            self.rast = F.GaussianRasterizer(F.GaussianRasterizationSettings(
                image_height=s.H, image_width=s.W, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=T(s.bg), scale_modifier=1.0,
                viewmatrix=T(s.view), projmatrix=T(s.proj), sh_degree=3, campos=T(s.campos), prefiltered=False,
                perspec_matrix=T(s.persp)))

    def grads_of(self, gs=None):
        """the incoming colour / depth gradients (pixel sums of O(1)); `gs`: [(gC, gD)] per view instead of the scenes' own"""
        gs = gs or [(x.gC * (x.W * x.H) ** 0.5, x.gD * (x.W * x.H) ** 0.5) for x in self.ss]
        if self.batch:
            return hh.T(np.stack([g[0] for g in gs])), hh.T(np.stack([g[1][None] for g in gs]))
        return hh.T(gs[0][0]), hh.T(gs[0][1][None])

    def step(self, scale, grads, backward=True):
        s, T, dev = self.ss[0], hh.T, hh.dev()
        lv = {n: T(a).requires_grad_() for n, a in (("means3D", s.means), ("sh", s.shs), ("opacity", s.opac),
                                                    ("scales", s.scales * np.float32(scale)), ("rotations", s.rots))}
        lv["means2D"] = torch.zeros((V, s.P, 3) if self.batch else (s.P, 3), device=dev, requires_grad=True)
        lv["view"] = (self.views if self.batch else T(s.view)).clone().requires_grad_()
        kw = dict(means3D=lv["means3D"], means2D=lv["means2D"], opacities=lv["opacity"], shs=lv["sh"], scales=lv["scales"],
                  rotations=lv["rotations"])
        if self.batch:
            o = self.rast(**kw, viewmatrices=lv["view"], gt_depths=self.gts)
        else:
            o = self.rast(**kw, viewmatrix=lv["view"], gt_depth=T(s.gt))
        if backward:
            torch.autograd.backward([o[0], o[2]], list(grads))
        return o, lv

    def read(self, o, lv):
        torch.cuda.synchronize()
        return [o[0].detach().cpu().numpy(), o[2].detach().cpu().numpy()], {k: v.grad.cpu().numpy() for k, v in lv.items()}


@pytest.fixture(params=PATHS, ids=["-".join(p) for p in PATHS])
def path(request, monkeypatch):
    """selects the call path; saves and restores the lazy-mode state of the shapes the tests use, and deterministic_grads"""
    from dgr_amd import _capi
    from dgr_amd import full as F
    from dgr_amd import light as L
    variant, binding = request.param
    if binding in ("node", "function", "debug", "batch") and L._C is not L._CompiledC:
        pytest.skip("compiled extension not loaded (DGR_BINDING=ctypes or not built)")
    if binding == "function":
        monkeypatch.setattr(L, "_USE_NODE", False)
    if binding in ("ctypes", "batch-ctypes"):
        monkeypatch.setattr(L, "_C", L._CtypesC)
        monkeypatch.setattr(F, "_C", F._CtypesC)
    _capi.load()
    det = _capi.get_option("deterministic_grads")
    try:
        L.check_async_errors()  # (whatever earlier tests left unread is theirs)
    except RuntimeError:
        L._pending_status.clear()
    state = [{k: (v.copy() if isinstance(v, list) else v) for k, v in d.items()}
             for d in (L._capacity_cache, L._last_status, L._unsettled)]
    yield variant, binding
    L._pending_status.clear()
    for d, saved in zip((L._capacity_cache, L._last_status, L._unsettled), state):
        d.clear()
        d.update(saved)
    _capi.set_option("deterministic_grads", det)


def _forget(L, key):
    for d in (L._capacity_cache, L._last_status, L._unsettled):
        d.pop(key, None)


def _growth_scenes(variant, binding):
    P, W, H, seed = 8000, 256, 160, 21
    return [make_scene(P, W, H, seed, view_index=v) for v in range(V if binding.startswith("batch") else 1)]


def _strict_then_lazy(p, L, monkeypatch, grads):
    """Frame A then frame B (scales x GROW), strict, then lazily: A (strict: learns R0), A (lazy), B (lazy).  Returns strict B,
    lazy B (each (images, grads)), R0, R1."""
    key = p.key
    monkeypatch.setenv("DGR_SYNC_MODE", "strict")
    _forget(L, key)
    p.read(*p.step(1.0, grads))
    R0 = L._capacity_cache[key]
    ref = p.read(*p.step(GROW, grads))
    R1 = L._capacity_cache[key]
    assert R0 < R1 <= 1.1 * R0, (R0, R1)  # (a frame that grew, below the growth trigger and far below the capacity)
    monkeypatch.setenv("DGR_SYNC_MODE", "lazy")
    _forget(L, key)
    p.read(*p.step(1.0, grads))
    assert L._capacity_cache[key] == R0 and not L._pending_status
    p.read(*p.step(1.0, grads))
    assert L._pending_status
    L.check_async_errors()
    assert key not in L._unsettled and L._capacity_cache[key] == R0
    o, lv = p.step(GROW, grads, backward=False)
    assert len(L._pending_status) == (V if p.batch else 1), "frame B did not run lazily"
    torch.autograd.backward([o[0], o[2]], list(grads))
    got = p.read(o, lv)
    L.check_async_errors()
    assert L._capacity_cache[key] == R1  # the count read back for B
    if not p.batch:
        assert L._last_status[key][0] == R1
    return ref, got, R0, R1


def test_a_frame_that_grows_within_the_capacity_gets_the_strict_frames_deterministic_gradients(path, monkeypatch):
    """Deterministic sums depend on the tile order only, not on R: lazy B must give strict B's bits, and finite ones."""
    from dgr_amd import _capi
    from dgr_amd import light as L
    p = Path(*path, _growth_scenes(*path))
    _capi.set_option("deterministic_grads", 1)
    (ref_img, ref_g), (img, g), R0, R1 = _strict_then_lazy(p, L, monkeypatch, p.grads_of())
    for a, b in zip(img, ref_img):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for k in ref_g:
        assert np.isfinite(g[k]).all(), f"{k}: {int((~np.isfinite(g[k])).sum())} non-finite values (R0 {R0}, R1 {R1})"
        assert np.array_equal(g[k].view(np.uint32), ref_g[k].view(np.uint32)), (k, int((g[k] != ref_g[k]).sum()))
        assert np.abs(ref_g[k]).max() > 0, k


def test_a_frame_that_grows_within_the_capacity_with_the_atomic_backward(path, monkeypatch):
    from dgr_amd import _capi
    from dgr_amd import light as L
    from util import assert_grad_close
    p = Path(*path, _growth_scenes(*path))
    _capi.set_option("deterministic_grads", 0)
    (ref_img, ref_g), (img, g), _, _ = _strict_then_lazy(p, L, monkeypatch, p.grads_of())
    for a, b in zip(img, ref_img):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for k in ref_g:
        assert np.isfinite(g[k]).all(), k
        assert_grad_close(g[k].reshape(-1, g[k].shape[-1]), ref_g[k].reshape(-1, ref_g[k].shape[-1]), k, rel_to_max=1e-5)


@pytest.mark.parametrize("variant", ["light", "full"])
def test_the_grown_frames_deterministic_gradients_against_the_oracle(oracle, monkeypatch, variant):
    """Anchors the bit-equality above to the float64 oracle (the bars of tests/test_hip_deterministic.py): strict frame B through
    GaussianRasterizer with deterministic_grads."""
    from dgr_amd import _capi
    from dgr_amd import light as L
    from util import assert_grad_close, mask_flipped_pixels
    monkeypatch.setenv("DGR_SYNC_MODE", "strict")
    s = _growth_scenes(variant, "node")[0]
    sB = s._replace(scales=s.scales * np.float32(GROW))
    gC, gD = (x * (s.W * s.H) ** 0.5 for x in (s.gC, s.gD))
    z = np.zeros_like(gD)
    if variant == "light":
        out, d = hh.hip_forward(sB, 3)
        st, ref = hh.oracle_forward(oracle, sB, 3)
        (gC, gD, _, _), _ = mask_flipped_pixels((gC, gD, z, z), hh.hip_state("n_contrib", sB, d), st.get("n_contrib"), s.W, s.H,
                                                "lazy growth", images=[(d[k], ref[k]) for k in ("color", "depth", "opacity_map")])
        gr = hh.oracle_backward(oracle, st, sB, 3, ref["opacity_map"], grads=(gC, gD, z, z))
        bar = 2e-6
    else:
        _, _, gr = hh.oracle_full(oracle, sB, 3, grads=(gC, gD, z))
        bar = 4e-6
    p = Path(variant, "ctypes" if L._C is not L._CompiledC else "node", [s])
    with _capi.thread_options(deterministic_grads=1):
        _, g = p.read(*p.step(GROW, p.grads_of([(gC, gD)])))
    for k, name in (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("sh", "dL_dsh"), ("opacity", "dL_dopacity"),
                    ("scales", "dL_dscales"), ("rotations", "dL_drotations")):
        assert_grad_close(g[k], gr[name], name, rel_to_max=bar, elem_rtol=2e-3, elem_frac=1e-3)
    assert_grad_close(g["view"], np.asarray(gr["dL_dview"]).reshape(4, 4), "dL_dview", rel_to_max=bar, elem_rtol=1e-3, elem_frac=0.0)


def _drain_overflow(L):
    """check_async_errors raises for the overflowed forward; a batch left one such word per view"""
    with pytest.raises(RuntimeError, match="overflow"):
        L.check_async_errors()
    while L._pending_status:
        try:
            L._check_oldest()
        except RuntimeError as e:
            assert "overflow" in str(e)


def _guarded_step(p, L, scale, grads):
    """one step with every earlier status word read first: a strict forward (the shape unsettled) posts none, a lazy one one
    per view"""
    L.check_async_errors()
    lazy = p.key in L._capacity_cache and p.key not in L._unsettled
    o, lv = p.step(scale, grads)
    posted = len(L._pending_status)
    assert posted == ((V if p.batch else 1) if lazy else 0), (p.key in L._unsettled, posted)
    return o, lv


def test_the_growth_guard_after_an_overflow_on_every_path(path, monkeypatch):
    """tests/test_hip_lazy_safety.py's first test on every call path: NaN images, zero gradients, check_async_errors raises,
    the shape runs strict -- observably: no status word posted -- until three settled reads, then lazily again."""
    from dgr_amd import light as L
    variant, binding = path
    p = Path(variant, binding, [make_scene(4000, 96, 64, 11, view_index=v) for v in range(V if binding.startswith("batch") else 1)])
    key = p.key
    grads = p.grads_of()
    monkeypatch.setenv("DGR_SYNC_MODE", "lazy")
    _forget(L, key)
    for _ in range(3):  # the first call is strict and teaches the capacity; then lazy
        o, _ = p.step(1.0, grads)
    L.check_async_errors()
    assert key not in L._unsettled and torch.isfinite(o[0]).all()
    R0 = L._capacity_cache[key]
    o, lv = p.step(3.0, grads)  # every splat three times as large: past 1.5 R0 + 4096 on every view
    assert torch.isnan(o[0]).all() and torch.isnan(o[2]).all()
    for k in ("means3D", "sh", "opacity", "scales", "rotations"):
        assert lv[k].grad is not None and not lv[k].grad.any(), k
    _drain_overflow(L)
    assert key in L._unsettled
    o1, _ = _guarded_step(p, L, 3.0, grads)  # strict: exact count, retried inside the call, therefore right
    assert torch.isfinite(o1[0]).all() and L._capacity_cache[key] > 1.5 * R0 + 4096
    s3 = p.ss[0]._replace(scales=p.ss[0].scales * np.float32(3.0))
    _, d_ref = hh.hip_forward(s3, 3) if variant == "light" else hh.hip_full_forward(s3, 3)  # (the `_C` call: strict here too)
    assert np.array_equal((o1[0][0] if p.batch else o1[0]).detach().cpu().numpy(), d_ref["color"])
    strict = 0
    for _ in range(4):  # steady count: three settled reads and the shape is lazy again
        strict += p.key in L._unsettled
        _guarded_step(p, L, 3.0, grads)
    L.check_async_errors()
    assert key not in L._unsettled, L._unsettled.get(key)
    assert 1 <= strict <= 3
    _guarded_step(p, L, 3.0, grads)  # lazy: one status word per view
    L.check_async_errors()


def test_a_growing_count_sends_the_shape_to_strict_before_it_overflows_on_every_path(path, monkeypatch):
    from dgr_amd import light as L
    variant, binding = path
    p = Path(variant, binding, [make_scene(4000, 256, 192, 12, view_index=v) for v in range(V if binding.startswith("batch") else 1)])
    key = p.key
    grads = p.grads_of()
    monkeypatch.setenv("DGR_SYNC_MODE", "lazy")
    _forget(L, key)
    scale = 1.0
    counts, strict_at = [], []
    for it in range(7):
        o, _ = _guarded_step(p, L, scale, grads)
        assert torch.isfinite(o[0]).all(), f"iteration {it}: a frame rendered past its capacity"
        L.check_async_errors()
        counts.append(L._capacity_cache[key])
        if key in L._unsettled:
            strict_at.append(it)
        scale *= 1.25  # ~50 % more instances per iteration
    assert counts[-1] > 3 * counts[0]
    assert strict_at and strict_at[0] <= 2, strict_at


@pytest.mark.parametrize("variant", ["light", "full"])
def test_a_captured_batch_replayed_on_a_grown_frame(monkeypatch, variant):
    """examples/mapping.py --graph --fused: a batch step captured on frame A (deterministic_grads), frame B's scales written into
    the captured input in place, replayed.  The replay bins into the capacity the capture was carved with, which its backward
    must get as R: finite gradients, the bits of an eager strict B."""
    from dgr_amd import _capi
    from dgr_amd import batch as B
    from dgr_amd import batch_full as BF
    from dgr_amd import light as L
    if L._C is not L._CompiledC:
        pytest.skip("compiled extension not loaded (DGR_BINDING=ctypes or not built)")
    M = B if variant == "light" else BF
    ss = _growth_scenes(variant, "batch")
    s, T, E = ss[0], hh.T, hh.E
    H, W = s.H, s.W
    key = (hh.dev().index, s.P, H, W)
    views, projs, campos, gts = (T(np.stack([getattr(x, n) for x in ss])) for n in ("view", "proj", "campos", "gt"))
    gC = T(np.stack([x.gC for x in ss])) * (W * H) ** 0.5
    gD = T(np.stack([x.gD[None] for x in ss])) * (W * H) ** 0.5
    gM = torch.zeros_like(gD)
    means, shs, opac, rots, bg, persp, e0 = T(s.means), T(s.shs), T(s.opac), T(s.rots), T(s.bg), T(s.persp), E()
    scales = T(s.scales)
    scales_B = T(s.scales * np.float32(GROW))

    def step():
        out = M._forward_batch(bg, means, e0, opac, scales, rots, 1.0, e0, views, gts, projs, s.tanfovx, s.tanfovy, H, W, shs, 3,
                               campos, False)
        if variant == "light":
            g = B._backward_batch(bg, means, out[6], e0, scales, rots, 1.0, e0, views, projs, s.tanfovx, s.tanfovy, gC, gD, gM,
                                  gM, gts, shs, 3, campos, out[7], out[8], out[9], out[5], persp, False, False, True, True,
                                  num_rendered=out[0])
        else:
            g = BF._backward_batch(bg, means, out[4], e0, scales, rots, 1.0, e0, views, projs, s.tanfovx, s.tanfovy, gC, gD, None,
                                   gts, shs, 3, campos, out[5], out[6], out[7], persp, True, True, out[0])
        return [out[1]] + [x for x in g if x is not None]

    saved = [{k: (v.copy() if isinstance(v, list) else v) for k, v in d.items()} for d in (L._capacity_cache, L._last_status, L._unsettled)]
    try:
        with _capi.thread_options(deterministic_grads=1):
            monkeypatch.setenv("DGR_SYNC_MODE", "strict")
            _forget(L, key)
            scales.copy_(scales_B)
            ref = [t.clone() for t in step()]
            torch.cuda.synchronize()
            R1 = L._capacity_cache[key]
            monkeypatch.setenv("DGR_SYNC_MODE", "lazy")
            _forget(L, key)
            scales.copy_(T(s.scales))
            step()  # (strict: learns frame A's count)
            step()  # (lazy)
            L.check_async_errors()
            assert L._capacity_cache[key] < R1  # (frame A's count: B grew)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                step()
                side.synchronize()
                with torch.cuda.graph(graph, stream=side):
                    res = step()
            L.check_async_errors()
            scales.copy_(scales_B)
            graph.replay()
            torch.cuda.synchronize()
            L.check_captured_status()
            assert len(res) == len(ref)
            for i, (a, b) in enumerate(zip(res, ref)):
                assert torch.isfinite(a).all(), (i, int((~torch.isfinite(a)).sum()))
                assert torch.equal(a, b), (i, float((a - b).abs().max()))
            del graph
    finally:
        L._pending_status.clear()
        for d, sv in zip((L._capacity_cache, L._last_status, L._unsettled), saved):
            d.clear()
            d.update(sv)
