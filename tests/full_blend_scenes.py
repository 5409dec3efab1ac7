"""The scenes of tests/test_hip_full_blend_edges.py (the full variant's blend kernels at the edges of their batch loops) and what
tests/test_full_blend_scenes.py checks about them on the CPU.

The full forward stages a tile's list FWD_BATCH = 256 positions at a time, the full backward BWD_BATCH = 128 positions (64 under
deterministic_grads), walking from min(range, the tile's last contributor) towards the front.

  exact(K)    one tile of a 32x32 frame with exactly K entries, walked to its end: K = 128 / 129 are the backward's batch edges
              (129 = 2 * 64 + 1 the deterministic form's), 256 / 257 the forward's, 512 two forward and four backward batches;
  shadowed    one tile, 384 entries in two groups: the nearer 192 on pixel columns 3 .. 5, the farther 192 on columns 10 .. 12.
              The right half's front-most contributors lie beyond list position 128 (another backward batch than position 0),
              the left half's last contributors before 256;
  shadowed272 the same with 272 nearer Gaussians: the right half's front-most contributors lie beyond 256 (another forward
              batch, and the third backward batch from the front);
  ragged      70x41, SH degree 3, background != 0: right-edge and bottom-edge tiles of more than one forward batch;
  opaque      48x48, SH degree 3: tiles that finish before their last forward batch and whose backward walks half the list at most.
"""
from types import SimpleNamespace

import numpy as np

from util import make_scene, one_tile_scene

FWD_BATCH, BWD_BATCH, BWD_BATCH_DET = 256, 128, 64
EXACT_K = (128, 129, 256, 257, 512)
SPREAD = (0.5, 13.5)   # the centres' pixel range on an axis the scenes below spread them over (the rectangles stay inside tile 0)


def exact(K):
    """one_tile_scene(K) with the centres spread over the tile: at its default (pixels 5 .. 10) no entry lives in the upper half of
    the upper quadrants or the lower half of the lower ones alone, and the backward's paired steps would have nothing to pair"""
    return one_tile_scene(K, groups=[(K, SPREAD, SPREAD, None)])


def shadowed(K=384, near=None):
    """`near` Gaussians (default K / 2) at depth 1 .. 3 on columns 3 .. 5, the others behind them on columns 10 .. 12.  With the
    halves equal the far group starts at list position 192, and too few pixels meet their first Gaussian of it beyond 256 (16
    at the best of 40 seeds); near = 272 with the depth ranges shifted to 1 .. 4 and 4.5 .. 6 is the variant that puts them there."""
    if near is None:
        near, zn, zf = K // 2, (1.0, 3.0), (3.5, 6.0)
    else:
        zn, zf = (1.0, 4.0), (4.5, 6.0)
    return one_tile_scene(K, groups=[(near, (3.0, 5.0), SPREAD, zn), (K - near, (10.0, 12.0), SPREAD, zf)])


def ragged():
    return make_scene(6000, 70, 41, 6)


def opaque():
    from test_hip_live_lists import opaque_scene
    return opaque_scene(3000, 48, 48, 3)


# name -> (builder, SH degree)
SCENES = {f"exact{K}": ((lambda K=K: exact(K)), 0) for K in EXACT_K}
SCENES.update(shadowed=(shadowed, 0), shadowed272=((lambda: shadowed(near=272)), 0), ragged=(ragged, 3), opaque=(opaque, 3))
ONE_TILE = tuple(f"exact{K}" for K in EXACT_K) + ("shadowed", "shadowed272")

_cache = {}


def scene(name):
    """(scene, SH degree), built once"""
    if ("scene", name) not in _cache:
        build, deg = SCENES[name]
        _cache["scene", name] = (build(), deg)
    return _cache["scene", name]


def oracle_full_forward(O, name, cmath=False):
    """(state, outputs) of the oracle's full forward on a scene, computed once per build of the oracle; nobody changes them"""
    key = ("oracle", name, bool(cmath))
    if key not in _cache:
        s, deg = scene(name)
        O.use_cmath(cmath)
        try:
            _cache[key] = O.full_forward(s.bg, s.means, None, s.opac, s.scales, s.rots, 1.0, None, s.view, s.gt, s.proj, s.tanfovx,
                                         s.tanfovy, s.H, s.W, s.shs, deg, s.campos)
        finally:
            O.use_cmath(False)
    return _cache[key]


def tile_lengths(s, st):
    gx, gy = (s.W + 15) // 16, (s.H + 15) // 16
    r = st.get("ranges").reshape(-1, 2).astype(np.int64)
    return (r[:, 1] - r[:, 0]).reshape(gy, gx)


def tile_max(s, img):
    """[gy, gx]: the maximum of an [H, W] image over each 16x16 tile"""
    gx, gy = (s.W + 15) // 16, (s.H + 15) // 16
    a = np.zeros((gy * 16, gx * 16), np.int64)
    a[:s.H, :s.W] = np.asarray(img).reshape(s.H, s.W)
    return a.reshape(gy, 16, gx, 16).max((1, 3))


def contributors(O, s, st):
    """The oracle's per-pixel contributors, re-derived from its float32 state with its own operations (oracle/dgr_oracle.cpp:
    render_forward; the exponential through the function its blend loop calls): per non-empty tile a namespace(tile, x0, y0,
    valid [n, 16, 16] bool: entry k of the tile's list is blended by pixel (y0 + i, x0 + j)).  Pixels outside the frame blend
    nothing."""
    f32 = np.float32
    W, H = s.W, s.H
    gx = (W + 15) // 16
    pl = st.get("point_list").astype(np.int64)
    xy = st.get("means2D").reshape(-1, 2)
    co = st.get("conic_opacity").reshape(-1, 4)
    nc = st.get("n_contrib").reshape(H, W).astype(np.int64)
    out = []
    for tile, (lo, hi) in enumerate(st.get("ranges").reshape(-1, 2).astype(np.int64)):
        if hi <= lo:
            continue
        x0, y0 = (tile % gx) * 16, (tile // gx) * 16
        ids = pl[lo:hi]
        px = (x0 + np.arange(16)).astype(f32)[None, None, :]
        py = (y0 + np.arange(16)).astype(f32)[None, :, None]
        dx = xy[ids, 0][:, None, None] - px
        dy = xy[ids, 1][:, None, None] - py
        a, b, c, o = (co[ids, k][:, None, None] for k in range(4))
        power = f32(-0.5) * (a * dx * dx + c * dy * dy) - b * dx * dy
        assert power.dtype == f32
        alpha = np.minimum(f32(0.99), o * O.exp_as_the_oracle_calls_it(np.minimum(power, f32(0))).reshape(power.shape))
        last = np.zeros((16, 16), np.int64)
        hh, ww = min(16, H - y0), min(16, W - x0)
        last[:hh, :ww] = nc[y0:y0 + hh, x0:x0 + ww]
        valid = (power <= 0) & (alpha >= f32(15.0) / f32(255.0)) & (np.arange(hi - lo)[:, None, None] < last[None])
        out.append(SimpleNamespace(tile=tile, x0=x0, y0=y0, valid=valid))
    return out


def first_and_count(s, tiles):
    """([H, W] first_contrib: the 1-based list position of each pixel's front-most contributor, 0 for none; [H, W] n_valid) of
    `contributors`' tiles"""
    first, count = np.zeros((s.H, s.W), np.int64), np.zeros((s.H, s.W), np.int64)
    for t in tiles:
        hh, ww = min(16, s.H - t.y0), min(16, s.W - t.x0)
        any_ = t.valid.any(0)
        f = np.where(any_, t.valid.argmax(0) + 1, 0)
        first[t.y0:t.y0 + hh, t.x0:t.x0 + ww] = f[:hh, :ww]
        count[t.y0:t.y0 + hh, t.x0:t.x0 + ww] = t.valid.sum(0)[:hh, :ww]
    return first, count


def split_neighbours(t, batch=BWD_BATCH):
    """The most neighbouring entry pairs living in DIFFERENT halves that a quadrant's list of one backward batch of the tile has:
    the backward stages positions [hi - batch, hi) from the tile's last contributor down; a quadrant's list is the staged entries
    some pixel of the 8x8 quadrant blended, an entry lives in the upper half (rows 0 .. 3), the lower half (rows 4 .. 7) or both
    (csrc/render_common.h: build_paired_lists)."""
    total = int((t.valid.any((1, 2)).nonzero()[0].max() + 1) if t.valid.any() else 0)
    best = 0
    for hi in range(total, 0, -batch):
        lo = max(0, hi - batch)
        for q in range(4):
            y, x = (q >> 1) * 8, (q & 1) * 8
            up = t.valid[lo:hi, y:y + 4, x:x + 8].any((1, 2))
            dn = t.valid[lo:hi, y + 4:y + 8, x:x + 8].any((1, 2))
            kind = (up + 2 * dn)[up | dn]
            best = max(best, int(np.count_nonzero(kind[:-1] * kind[1:] == 2)))
    return best


# ------------------------------------------------------------------------------------------ the backward's references
FORMS = ("default", "lean", "depth")   # all three pixel-gradient images / no uncertainty gradient / the depth image's alone


def pixel_grads(name, form="default"):
    """(gC, gD, gU) float32: fp64_model.scaled_grads(s, "full"), rounded once for every party; `lean` and `depth` have gU = 0 (the
    kernels are handed no image), `depth` has gC = 0 as well"""
    import fp64_model as M
    s, _ = scene(name)
    gC, gD, gU = (np.asarray(g, np.float32) for g in M.scaled_grads(s, "full"))
    if form != "default":
        gU = np.zeros_like(gU)
    if form == "depth":
        gC = np.zeros_like(gC)
    return gC, gD, gU


def grads64(s, deg, st, ref, grads):
    """The float64 model's gradients on the decisions of an oracle state, keyed as ref_parity.GRADS (no entry for dL_dcolors and
    dL_dcov3D: intermediates of the model, every consumer of which is judged); and the model's images"""
    import fp64_model as M
    loss, leaves, img = M.torch_full(s, deg, ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"),
                                     tuple(np.asarray(g, np.float64) for g in grads))
    loss.backward()
    gv = sum(leaves[k].grad for k in ("view_ndc", "view_depth", "view_campos") if leaves[k].grad is not None).numpy().reshape(-1).copy()
    gv[[3, 7, 11, 15]] = 0.0   # never written by the reference (quirk F7)
    m2 = np.zeros((s.P, 3))
    m2[img["_idx"], :2] = img["_pix"].grad.numpy() * np.array([0.5 * s.W, 0.5 * s.H])
    g = dict(dL_dmeans2D=m2, dL_dopacity=leaves["opacities"].grad.numpy(), dL_dmeans3D=leaves["means3D"].grad.numpy(),
             dL_dsh=leaves["shs"].grad.numpy(), dL_dscales=leaves["scales"].grad.numpy(), dL_drotations=leaves["rotations"].grad.numpy(),
             dL_dview=gv.reshape(4, 4))
    return g, {k: v for k, v in img.items() if not k.startswith("_")}


def references(O, name, form="default", cmath=False):
    """(pixel gradients, the oracle's gradients, the float64 model's, the model's images) of one scene and form; `cmath`: the
    C-math oracle and the model on ITS decisions.  Computed once, shared by the tests, changed by nobody."""
    key = ("refs", name, form, bool(cmath))
    if key not in _cache:
        s, deg = scene(name)
        st, ref = oracle_full_forward(O, name, cmath)
        grads = pixel_grads(name, form)
        # (the state remembers the build it was made by: its backward is that build's)
        g_or = O.full_backward(st, s.bg, s.means, None, s.scales, s.rots, 1.0, None, s.view, s.gt, s.proj, s.tanfovx, s.tanfovy,
                               *grads, s.shs, deg, s.campos, s.persp)
        g64, img = grads64(s, deg, st, ref, grads)
        _cache[key] = (grads, g_or, g64, img)
    return _cache[key]
