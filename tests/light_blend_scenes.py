"""The scenes of tests/test_hip_light_blend_edges.py (the light blend backward at the edges of its live-entry batches) and what
tests/test_light_blend_scenes.py checks about them on the CPU.

The light backward (csrc/render_light.hip: render_bwd_light_body) walks a tile's LIVE entries -- the list entries some pixel
blended, compacted by the forward as {Gaussian id, list position << 8 | tag} -- from the back, BWD_BATCH = 128 at a time (64 under
deterministic_grads).  Where its lists are paired (the mapping instances on half-wave lists) the batches are of equal size,
per = min(128, int(total / nbatch) + 1): 129 live entries go as 65 + 64, 257 as 86 + 86 + 85.  T, S and the median's threshold
are carried from batch to batch, and a pixel's cut is taken on the entry's list POSITION, which the live record carries.

  live<L>          full_blend_scenes.exact(L) (live129: the same at another seed, SEED_129): one tile of a 32x32 frame whose L list
                   entries are all live.  64 / 65 and 128 / 129 are the deterministic and the default batch and one past it,
                   256 / 257 two batches and one past them (three equal ones of 86 + 86 + 85), 385 three and one past
                   (97 + 97 + 97 + 94);
  sparse<L>of<K>   exact(K) with K - L Gaussians at opacity 0.02 -- below 15/255: listed, never blended -- spread through the
                   list: L live entries whose live index is not their list position;
  two_tiles        129 Gaussians on tile 0 and 257 on tile 3: the second tile's live list starts at the odd offset 129;
  opaque<L>of<K>   K Gaussians, all but L of them dead as above, the others at opacity 0.9 .. 0.99: pixels finish (T < 1e-4) before the
                   list's end, so that live entries BEHIND a pixel's last contributor pass its alpha test and only the cut on the list
                   position keeps them out -- in every scene above a pixel's last contributor is simply its deepest entry that
                   passes, and a kernel without the cut (or with the cut on the live index) computes the same.

Everything here is computed once and changed by nobody.
"""
from types import SimpleNamespace

import numpy as np

import ref_parity as rp
from full_blend_scenes import BWD_BATCH, BWD_BATCH_DET, SPREAD, _cache, contributors, exact, split_neighbours  # noqa: F401
from util import one_tile_scene

LIVE_L = (64, 65, 128, 129, 256, 257, 385)
SPARSE = ((65, 200), (129, 400), (257, 512))
DEAD_OPACITY = 0.02   # < 15/255: alpha = min(0.99, o G) never reaches the blend threshold
FORMS = ("default", "lean", "no_median", "no_var")   # all four pixel-gradient images / neither of the last two / one of them missing


# The seeds of the 129-live tiles (util.one_tile_scene's; every other scene keeps its default, 5).  In batches of 128 such a tile
# leaves ONE entry, the front-most, to its second batch: a pixel's median fires there when that entry alone takes T to 0.5 or
# below, and its last contributor lies there when the pixel blends nothing else.  Both are rare -- of the seeds 0 .. 299 three
# (live129), seven (sparse129of400), five of 0 .. 199 (two_tiles) and eight of 0 .. 119 (opaque129of320) have a pixel of each
# kind -- and these are the first of them (opaque129of320: the first with two pixels of each kind);
# tests/test_light_blend_scenes.py asserts the counts.
SEED_129 = {"live129": 27, "sparse129of400": 32, "two_tiles": 10, "opaque129of320": 42}


def spread_tile(K, seed=5, spread=SPREAD):
    """full_blend_scenes.exact(K) -- which it is at the default seed and spread -- for any seed"""
    return exact(K) if (seed, spread) == (5, SPREAD) else one_tile_scene(K, seed=seed, groups=[(K, spread, spread, None)])


def sparse(L, K, seed=5):
    s = spread_tile(K, seed)
    opac = s.opac.copy()
    opac[np.random.default_rng(11).permutation(K)[:K - L]] = DEAD_OPACITY
    return s._replace(opac=opac)


def opaque(K, dead, spread, seed=5):
    s = spread_tile(K, seed, spread)
    rng = np.random.default_rng(11)
    opac = rng.uniform(0.9, 0.99, (K, 1)).astype(np.float32)
    opac[rng.permutation(K)[:dead]] = DEAD_OPACITY
    return s._replace(opac=opac)


def two_tiles():
    return one_tile_scene(386, seed=SEED_129["two_tiles"], groups=[(129, SPREAD, SPREAD, None), (257, (19.0, 29.5), (19.0, 29.5), None)])


# name -> (builder, {tile: live entries})
SCENES = {f"live{L}": ((lambda L=L: spread_tile(L, SEED_129.get(f"live{L}", 5))), {0: L}) for L in LIVE_L}
SCENES.update({f"sparse{L}of{K}": ((lambda L=L, K=K: sparse(L, K, SEED_129.get(f"sparse{L}of{K}", 5))), {0: L}) for L, K in SPARSE})
SCENES["two_tiles"] = (two_tiles, {0: 129, 3: 257})
# (the dead counts are what leaves exactly 129 / 257 live: nearer opaque Gaussians hide some of the others from every pixel)
SCENES["opaque129of320"] = ((lambda: opaque(320, 191, (2.0, 12.0), SEED_129["opaque129of320"])), {0: 129})
SCENES["opaque257of400"] = ((lambda: opaque(400, 143, SPREAD)), {0: 257})
OPAQUE_NAMES = ("opaque129of320", "opaque257of400")
SPARSE_NAMES = tuple(f"sparse{L}of{K}" for L, K in SPARSE)
LIST_LENGTH = {**{f"live{L}": L for L in LIVE_L}, **{f"sparse{L}of{K}": K for L, K in SPARSE}, "two_tiles": 386, "opaque129of320": 320,
               "opaque257of400": 400}
TWO_TILES_RANGES = {0: (0, 129), 3: (129, 386)}   # (tiles 1 and 2 are empty)
DEG = 0


def key(name, *what):
    return ("light", name) + what


def scene(name):
    if key(name, "scene") not in _cache:
        _cache[key(name, "scene")] = SCENES[name][0]()
    return _cache[key(name, "scene")]


def case(name):
    """the scene as ref_parity's parties take it"""
    return SimpleNamespace(name=name, s=scene(name), deg=DEG, kw={})


def oracle_forward(O, name, cmath=False):
    """(state, party dict) of the oracle's light forward, once per build of the oracle"""
    k = key(name, "oracle", bool(cmath))
    if k not in _cache:
        O.use_cmath(cmath)
        try:
            _cache[k] = rp.module_forward(O, case(name))
        finally:
            O.use_cmath(False)
    return _cache[k]


def forward64(O, name, cmath=False):
    """(the float64 model's forward on the oracle's decisions, the alpha image every side's backward is handed)"""
    k = key(name, "f64", bool(cmath))
    if k not in _cache:
        f64 = rp.forward64(case(name), oracle_forward(O, name, cmath)[1])
        _cache[k] = (f64, rp.arbiter_alphas(f64))
    return _cache[k]


def live_positions(O, name):
    """{tile: the list positions some pixel of the tile blends, ascending} by the oracle's decisions (every tile of the frame),
    and `contributors`' tiles"""
    k = key(name, "live")
    if k not in _cache:
        s = scene(name)
        st, ref = oracle_forward(O, name)
        tiles = contributors(O, s, st)
        live = {t: np.zeros(0, np.int64) for t in range(len(st.get("ranges")) // 2)}
        for t in tiles:
            live[t.tile] = np.nonzero(t.valid.any((1, 2)))[0]
        _cache[k] = (live, tiles)
    return _cache[k]


class _Uncut:
    """an oracle state whose n_contrib is beyond every list: `contributors` then leaves the cut at the last contributor out"""

    def __init__(self, st):
        self.st = st

    def get(self, name):
        v = self.st.get(name)
        return np.full_like(v, 1 << 30) if name == "n_contrib" else v


def cut_pairs(O, name):
    """Per non-empty tile (cut [n_live, 16, 16] bool: the pixel passes the live entry's alpha test, but the entry lies at or behind
    the pixel's last contributor; by_index: those among them whose LIVE INDEX is smaller than the pixel's last contributor)."""
    s = scene(name)
    st, _ = oracle_forward(O, name)
    live, tiles = live_positions(O, name)
    assert s.H % 16 == 0 and s.W % 16 == 0   # (whole tiles)
    nc = st.get("n_contrib").reshape(s.H, s.W).astype(np.int64)
    out = []
    for t, u in zip(tiles, contributors(O, s, _Uncut(st))):
        cut = (u.valid & ~t.valid)[live[t.tile]]
        last = nc[t.y0:t.y0 + 16, t.x0:t.x0 + 16]
        out.append((cut, cut & (np.arange(cut.shape[0])[:, None, None] < last[None])))
    return out


def batch_size(total, split):
    """entries per backward batch of a tile with `total` live entries: `split` "equal" (paired lists), 128 or 64"""
    if split != "equal":
        return int(split)
    if total <= BWD_BATCH:
        return BWD_BATCH
    nbatch = -(-total // BWD_BATCH)
    return min(BWD_BATCH, int(np.float32(total) / np.float32(nbatch)) + 1)


def batch_of(live_index, total, per):
    """the batch (0: the one walked first, at the list's end) that holds a live entry"""
    return (total - 1 - np.asarray(live_index)) // per


def live_only(t, live):
    """a `contributors` tile reduced to its live entries: what the backward stages"""
    return SimpleNamespace(tile=t.tile, x0=t.x0, y0=t.y0, valid=t.valid[live])


def median_and_last(O, name):
    """Per non-empty tile, from the float64 model's weights on the oracle's decisions: namespace(tile, live [n]: the live list
    positions, any [npix]: the pixel blends something, last [npix]: the LIVE index of the pixel's last contributor, fire
    [npix]: that of the entry its median term fires at -- the first valid pair from the back whose transmittance before it,
    derived as the sides derive it from the alpha image they are handed, exceeds 0.5)."""
    import torch
    import fp64_model as M
    k = key(name, "median")
    if k in _cache:
        return _cache[k]
    c = case(name)
    s = c.s
    st, ref = oracle_forward(O, name)
    f64, alphas = forward64(O, name)
    factor = torch.tensor(rp.alpha_interface_factor(f64, alphas).reshape(s.H, s.W))
    vis = np.asarray(ref["radii"]) > 0
    idx = np.nonzero(vis)[0]
    pix = torch.tensor(f64["means2D"][idx])
    con = tuple(torch.tensor(f64["conic"][idx, i]) for i in range(3))
    opac = M.f64(s.opac)[torch.tensor(idx), 0]
    out = []
    for tl in M.tiles(s, vis, ref["point_list"], ref["ranges"], ref["n_contrib"]):
        power, a = M.alpha_of(tl, M.tile_xy(pix, tl), con, opac)
        valid = M.valid_pairs(tl, power, a)
        _, Texcl, _ = M.blend_weights(torch.where(valid, a, torch.zeros_like(a)))
        Texcl = Texcl * factor[tl.sel].reshape(-1)[None]
        live = np.nonzero(valid.any(1).numpy())[0]
        index = np.full(valid.shape[0], -1, np.int64)
        index[live] = np.arange(live.size)
        pos1 = (tl.pos + 1)
        last = (valid * pos1).max(0).values.numpy() - 1
        fire = ((valid & (Texcl > 0.5)) * pos1).max(0).values.numpy() - 1
        any_ = last >= 0
        assert np.all(fire[any_] >= 0)   # (the front-most contributor has T = 1 before it)
        out.append(SimpleNamespace(tile=tl.tile, live=live, any=any_, last=np.where(any_, index[last], -1), fire=np.where(any_, index[fire], -1)))
    _cache[k] = out
    return out


# ------------------------------------------------------------------------------------------ the backward's references
def pixel_grads(name, form="default"):
    """(gC, gD, gM, gV) float32, ref_parity.pixel_grads rounded once for every party; the images a form lacks are zero"""
    gC, gD, gM, gV = rp.pixel_grads(scene(name))
    if form in ("lean", "no_median"):
        gM = np.zeros_like(gM)
    if form in ("lean", "no_var"):
        gV = np.zeros_like(gV)
    return gC, gD, gM, gV


def references(O, name, mode=rp.MODES[0], form="default", cmath=False):
    """(pixel gradients, alphas, the oracle's gradients in `mode`, the float64 model's) of one scene, ref_parity.MODES entry and
    form; `cmath`: the C-math oracle and the model on ITS decisions.  `alphas` -- the model's alpha image rounded once -- is what
    every side's backward is handed.  The float64 gradients are the full backward's: a mode only switches outputs off."""
    _, track_off, map_off = mode
    c = case(name)
    st, ref = oracle_forward(O, name, cmath)
    f64, alphas = forward64(O, name, cmath)
    grads = pixel_grads(name, form)
    k64 = key(name, "g64", form, bool(cmath))
    if k64 not in _cache:
        _cache[k64] = rp.grads64(c, ref, grads, alphas, f64)[0]
    kor = key(name, "g_or", bool(track_off), bool(map_off), form, bool(cmath))
    if kor not in _cache:
        _cache[kor] = rp.module_backward(O, st, c, alphas, grads, track_off, map_off)
    return grads, alphas, _cache[kor], _cache[k64]
