"""Designed frames for the front end (csrc/segment_binning.hip, csrc/tile_sort.h, csrc/binning.hip): every frame places exact
numbers of Gaussians in chosen tiles, so that a tile list, a segment total or a rectangle sits ON an edge of the binning kernels.
tests/test_binning_frames.py verifies every design against the oracle's ranges on the CPU; tests/test_hip_binning_edges.py runs
the frames through the real forward and reads the path each segment took from dgr_debug_bin_tiles_trace.

`frame(W, H, blocks)` generalises util.one_tile_scene.  `blocks` lists the Gaussians IN INDEX ORDER (bin_segments deals index
ranges to its workgroups, so the order is part of a design):
  ("small", (tx, ty), n[, z])  n Gaussians inside tile (tx, ty): centres on pixels 5 .. 10 of the tile, radius 3 px at most,
                               opacity 0.02 .. 0.05 (nothing ends a tile's walk early); z: one depth for all of them, and one
                               centre, so that their depth bits are EQUAL and the ids alone order them;
  ("wide", cx, cy, r)          one isotropic Gaussian centred on pixel (cx, cy), also outside the frame, of radius exactly r px:
                               its tile rectangle is the square [cx - r, cx + r] x [cy - r, cy + r] cut to the frame (the
                               reference's getRect).  A rectangle that is not square is a square clipped by a frame edge;
  ("hidden", n)                n Gaussians behind the camera: culled, they only occupy indices.

The edges (segment_binning.hip unless named):
  REG_SORT_MAX 1024   a list up to here is sorted by one wave's register network of 1, 2, 4, 8 or 16 words per lane (n <= 64,
                      128, 256, 512, 1024); a segment with a longer list sorts 512-entry parts and merges them by rank;
  K2_CAP 6144         a segment with more instances is DENSE: its tiles are placed and sorted in groups whose keys fit LDS together
                      (`sum + tcnt[t1] <= K2_CAP`), a single list above K2_CAP in place in global memory (wg_sort_global), and under
                      8- and 16-tile segments helper workgroups take four tiles each;
  BIG_PAIRS 24        a rectangle of more (row, segment) pairs is walked by a wave from a queue of BIGQ = 512 entries per group of a
                      workgroup's Gaussians; an entry that finds the queue full is walked by its own lane;
  SORT_LDS_MAX 2048   (binning.hip, the "lds_count" = 0 path) longer lists are sorted in global memory.
Dense means gcount > K2_CAP and nothing else: `!in_regs` (more than 6144 PAIRS) implies it, because every pair carries at
least one instance -- no frame is dense "by pairs" alone, and none is looked for."""
import json
import os

import numpy as np

from dgr_amd.synth import camera, make_scene

K2_CAP, REG_SORT_MAX, BIG_PAIRS, BIGQ, SORT_LDS_MAX = 6144, 1024, 24, 512, 2048
K1_THREADS, SEG_MAX_WGS = 1024, 256


def per_wg(P):
    """Gaussians per bin_segments workgroup (segment_binning_per_wg)"""
    chunks = -(-P // K1_THREADS)
    return max(1, -(-chunks // SEG_MAX_WGS)) * K1_THREADS


def rect_of(W, H, cx, cy, r):
    """the reference's getRect: tiles [x0, x1) x [y0, y1)"""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    lo = lambda p, g: min(g, max(0, int((p - r) / 16)))           # noqa: E731  (C truncation, then the clamp)
    hi = lambda p, g: min(g, max(0, int((p + r + 15) / 16)))      # noqa: E731
    return lo(cx, gx), lo(cy, gy), hi(cx, gx), hi(cy, gy)


def frame(W, H, blocks, seed=5):
    """(scene, design): design = dict(lengths [gy, gx] designed tile list lengths, rects [(index, x0, y0, x1, y1)] of the wide
    Gaussians, visible [P] bool)"""
    base = make_scene(1, W, H, seed)
    tanfovx, tanfovy, Rm, t, *_ = camera(W, H, 0.05)
    rng = np.random.default_rng(2000 + seed)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    lengths = np.zeros((gy, gx), np.int64)
    px, py, z, sig, op, rects = [], [], [], [], [], []
    P = 0
    for b in blocks:
        if b[0] == "small":
            (tx, ty), n = b[1], b[2]
            assert 0 <= tx < gx and 0 <= ty < gy and 16 * tx + 13 < W and 16 * ty + 13 < H
            flat = len(b) > 3
            px.append(np.full(n, 16 * tx + 7.5) if flat else 16 * tx + rng.uniform(5.0, 10.0, n))
            py.append(np.full(n, 16 * ty + 7.5) if flat else 16 * ty + rng.uniform(5.0, 10.0, n))
            z.append(np.full(n, float(b[3])) if flat else rng.uniform(1.0, 6.0, n))
            sig.append(rng.uniform(0.3, 0.5, n))
            op.append(rng.uniform(0.02, 0.05, n))
            lengths[ty, tx] += n
        elif b[0] == "wide":
            _, cx, cy, r = b
            n = 1
            px.append(np.array([cx])); py.append(np.array([cy])); z.append(rng.uniform(1.0, 6.0, 1))
            # cov2D of an isotropic Gaussian of a px at the image centre, seen at (u, v) = (x / z, y / z): a^2 [[1 + u^2, u v],
            # [u v, 1 + v^2]] + 0.3 I (fx = fy here; the reference clamps u, v to 1.3 tan(fov / 2)), largest eigenvalue
            # a^2 (1 + u^2 + v^2) + 0.3; radius = ceil(3 sqrt of it) = r with half a pixel to spare
            u = np.clip(((2 * cx + 1) / W - 1) * tanfovx, -1.3 * tanfovx, 1.3 * tanfovx)
            v = np.clip(((2 * cy + 1) / H - 1) * tanfovy, -1.3 * tanfovy, 1.3 * tanfovy)
            sig.append(np.array([np.sqrt((((r - 0.5) / 3.0) ** 2 - 0.3) / (1 + u * u + v * v))]))
            op.append(rng.uniform(0.01, 0.03, 1))
            x0, y0, x1, y1 = rect_of(W, H, cx, cy, r)
            lengths[y0:y1, x0:x1] += 1
            rects.append((P, x0, y0, x1, y1))
        else:
            assert b[0] == "hidden"
            n = b[1]
            px.append(np.full(n, W / 2)); py.append(np.full(n, H / 2)); z.append(np.full(n, -1.0))
            sig.append(np.full(n, 0.4)); op.append(np.full(n, 0.03))
        P += n
    px, py, z, sig, op = (np.concatenate(a) for a in (px, py, z, sig, op))
    xc = ((2 * px + 1) / W - 1) * tanfovx * z
    yc = ((2 * py + 1) / H - 1) * tanfovy * z
    means = ((np.stack([xc, yc, z], 1) - t) @ Rm).astype(np.float32)
    scales = np.repeat((sig * (2 * tanfovx / W) * np.abs(z))[:, None], 3, 1).astype(np.float32)
    rots = np.zeros((P, 4), np.float32)
    rots[:, 0] = 1.0
    shs = np.zeros((P, 16, 3), np.float32)
    shs[:, 0, :] = rng.normal(size=(P, 3)).astype(np.float32) * 0.5
    s = base._replace(P=P, means=means, scales=scales, rots=rots, opac=op[:, None].astype(np.float32), shs=shs)
    return s, dict(lengths=lengths, rects=rects, visible=z > 0)


def table(rows):
    """[("small", (tx, ty), n)] of a list of rows of tile counts"""
    return [("small", (tx, ty), n) for ty, row in enumerate(rows) for tx, n in enumerate(row) if n]


# ------------------------------------------------------------------------------------------ the frames
RULE = ((1, 63, 64, 65), (128, 129, 256, 257), (512, 513, 1023, 1024))
PARTS = ((1025, 10, 0, 300), (1537, 1, 5, 7), (2048, 100, 100, 100), (2049, 1025, 3, 0))
GROUPS = ((3000, 3000, 3000, 144), (6144, 1, 0, 6144), (6145, 10, 0, 0), (8193, 0, 0, 100))
RAGGED = {5: (100, 200, 300, 3000, 3200), 7: (50,) + (0,) * 4 + (700, 1300), 9: (50,) + (0,) * 7 + (1300,),
          15: (50,) + (0,) * 12 + (700, 1300), 17: (50,) + (0,) * 15 + (1300,), 31: (50,) + (0,) * 28 + (700, 1300)}


def _rule(flat=False):
    if not flat:
        return 64, 48, table(RULE)
    return 64, 48, [b + (1.5 + 0.25 * i,) for i, b in enumerate(table(RULE))]


def _budget():
    return 512, 16, table([(384,) * 31 + (385,)])


def _spans():
    """512x32: 32 x 2 tiles.  Wide Gaussians whose squares cover a whole row of a segment (coverage byte: columns 0 .. 15 under 16-tile
    segments), start or end inside one and cross segment borders of every size; small ones among them."""
    rng = np.random.default_rng(11)
    blocks = table([(40, 0, 0, 7, 0, 0, 0, 0, 90, 0, 0, 0, 0, 0, 0, 33) * 2, (0, 0, 5, 0) * 8])
    for cx, cy, r, n in ((255.5, 15.5, 280, 40), (100.5, 8.5, 40, 30), (300.5, 20.5, 100, 30), (40.5, 8.5, 20, 20), (470.5, 24.5, 60, 20),
                         (200.5, 8.5, 8, 20)):
        blocks += [("wide", cx + float(rng.integers(-3, 4)), cy, r)] * n
    order = rng.permutation(len(blocks))
    return 512, 32, [blocks[i] for i in order]


def _runs():
    """P = 5000: bin_segments workgroups 0 .. 4 take 1024 indices each.  Tile A = (0, 0) gets pairs from workgroups 0, 2 and 4 only
    (empty runs in between), tile B = (0, 1) from workgroup 4 only (empty runs in front); tile C = (0, 2) from all five."""
    A, B, Ct = (0, 0), (0, 1), (0, 2)
    return 64, 48, [("small", A, 300), ("small", Ct, 724), ("small", Ct, 1024), ("small", A, 200), ("small", Ct, 824),
                    ("small", Ct, 1024), ("small", A, 100), ("small", B, 50), ("small", Ct, 754)]


def big_square(W, H, nsx, rows, S=4):
    """a wide Gaussian whose rectangle starts at the left frame edge, covers nsx segments of S tiles and `rows` rows from the top"""
    xr = 16 * (S * nsx - 2) + 8.5
    r = max(150, int(xr / 2) + 10)
    cy = {1: 8.5 - r, 2: 24.5 - r}.get(rows, H / 2 + 0.5)
    return ("wide", xr - r, cy, r)


RECT_NSX, RECT_ROWS = (3, 5, 6, 7, 11, 13), (1, 2, 16)


def _rectangles():
    """832x256: 52 x 16 tiles, 13 four-tile segments a row"""
    blocks = [("wide", 112.5, 64.5, 56),      # tiles 3 .. 10 x rows 0 .. 7: 3 segments x 8 rows = 24 pairs (its lane walks it)
              ("wide", 160.5, -47.5, 120)]    # tiles 2 .. 17 x rows 0 .. 4: 5 segments x 5 rows = 25 pairs (queued)
    blocks += [big_square(832, 256, nsx, rows) for nsx in RECT_NSX for rows in RECT_ROWS]
    blocks += [("wide", 800.5, 128.5, 100), ("wide", 400.5, 250.5, 60), ("wide", 880.5, 290.5, 120), ("wide", -30.5, 100.5, 50)]
    blocks += table([[0] * 52] * 3 + [[(7 * i) % 40 if i % 5 == 0 else 0 for i in range(52)]] + [[0] * 52] * 11 + [[3] * 52])
    return 832, 256, blocks


def _queue():
    """256x416: 16 x 26 tiles, so that a whole-frame rectangle has more than BIG_PAIRS pairs at every segment size (104, 52, 26).
    P = 8192, 1024 indices per bin_segments workgroup: 700 whole-frame Gaussians among indices 0 .. 1023 (workgroup 0: the queue
    of 512 is full, 188 are walked by their lanes), 10 among 4096 .. 5119 (workgroup 4: not full), 300 small ones, the rest hidden."""
    rng = np.random.default_rng(12)
    whole = ("wide", 127.5, 207.5, 300)
    first = [whole] * 700 + [("small", (int(rng.integers(0, 16)), int(rng.integers(0, 26))), 1) for _ in range(100)] + [("hidden", 1)] * 224
    first = [first[i] for i in rng.permutation(1024)]
    later = [whole] * 10 + [("small", (int(rng.integers(0, 16)), int(rng.integers(0, 26))), 1) for _ in range(200)] + [("hidden", 1)] * 814
    later = [later[i] for i in rng.permutation(1024)]
    return 256, 416, first + [("hidden", 3072)] + later + [("hidden", 3072)]


REREAD_P, REREAD_WG = 1049000, 200


def _reread():
    """P = 1 049 000: 5120 indices per bin_segments workgroup, more than the 4096 whose rectangles stay in registers between the two
    passes, so both passes load every group again.  Everything is hidden but workgroup 200's Gaussians: 2000 in its first group of
    4096 (20 of them whole-frame) and 1000 in its last, the 1024 behind (15 whole-frame).  256x112: 16 x 7 tiles, 28 pairs each."""
    rng = np.random.default_rng(13)
    assert per_wg(REREAD_P) == 5120
    whole = ("wide", 127.5, 55.5, 200)
    small = lambda n: [("small", (int(rng.integers(0, 16)), int(rng.integers(0, 7))), 1) for _ in range(n)]   # noqa: E731
    g_first = [whole] * 20 + small(1980) + [("hidden", 1)] * 2096
    g_last = [whole] * 15 + small(985) + [("hidden", 1)] * 24
    g0 = REREAD_WG * 5120
    mid = [g_first[i] for i in rng.permutation(4096)] + [g_last[i] for i in rng.permutation(1024)]
    return 256, 112, [("hidden", g0)] + mid + [("hidden", REREAD_P - g0 - 5120)]


def _wide41():
    """2688x32: 42 four-tile segments a row.  bin_segments' queue walk divides a pair number by the rectangle's segment count nsx in
    float, (p + 0.5) * (1 / nsx); without the half the quotient is wrong from nsx = 41 on (p = 41: 41 * fl(1 / 41) < 1), and not for
    any smaller nsx -- so the frame that needs the half is this wide.  One rectangle of 41 segments x 2 rows, one of all 42."""
    W, H = 2688, 32
    return W, H, [big_square(W, H, 41, 2), ("wide", 1343.5, 15.5, 1400)] + table([(9, 0, 0, 0) * 42, (0, 0, 4, 0) * 42])


FRAMES = {"wide41": _wide41, "rule": _rule, "rule_flat": lambda: _rule(True), "parts": lambda: (64, 64, table(PARTS)), "budget": _budget,
          "groups": lambda: (64, 64, table(GROUPS)), "spans": _spans, "runs": _runs, "rectangles": _rectangles, "queue": _queue,
          "reread": _reread}
FRAMES.update({f"ragged{gx}": (lambda gx=gx: (16 * gx, 16, table([RAGGED[gx]]))) for gx in RAGGED})

_cache = {}


def get(name):
    """(scene, design) of a frame, built once"""
    if name not in _cache:
        W, H, blocks = FRAMES[name]()
        blocks = _merge(blocks)
        _cache[name] = frame(W, H, blocks)
    return _cache[name]


def _merge(blocks):
    """runs of hidden singles as one block (the builder's cost is per block)"""
    out = []
    for b in blocks:
        if b[0] == "hidden" and out and out[-1][0] == "hidden":
            out[-1] = ("hidden", out[-1][1] + b[1])
        else:
            out.append(b)
    return out


# ------------------------------------------------------------------------------------------ what a design implies
def segments(design, S):
    """{segment index: (gcount, tmax, dense)} of the segments that own instances, at S tiles per segment"""
    n = design["lengths"]
    gy, gx = n.shape
    sgx = -(-gx // S)
    out = {}
    for ty in range(gy):
        for sx in range(sgx):
            part = n[ty, sx * S:(sx + 1) * S]
            if part.sum():
                out[ty * sgx + sx] = (int(part.sum()), int(part.max()), bool(part.sum() > K2_CAP))
    return out


def workgroups(design, S):
    """bin_tiles workgroups at S tiles per segment: one per segment and S / 4 - 1 helpers each"""
    gy, gx = design["lengths"].shape
    return gy * -(-gx // S) * (S // 4)


def small_pairs(design):
    """[gy, gx] lengths of the small Gaussians alone (each is one pair in its tile's segment)"""
    n = design["lengths"].copy()
    for _, x0, y0, x1, y1 in design["rects"]:
        n[y0:y1, x0:x1] -= 1
    return n


def pairs(design, S):
    """{segment index: (row, segment) pairs}: one per small Gaussian, one per row and segment a wide rectangle touches"""
    n = small_pairs(design)
    gy, gx = n.shape
    sgx = -(-gx // S)
    out = np.zeros((gy, sgx), np.int64)
    for sx in range(sgx):
        out[:, sx] = n[:, sx * S:(sx + 1) * S].sum(1)
    for _, x0, y0, x1, y1 in design["rects"]:
        if x1 > x0 and y1 > y0:
            out[y0:y1, x0 // S:(x1 - 1) // S + 1] += 1
    return {int(i): int(v) for i, v in enumerate(out.reshape(-1)) if v}


def pairs_of(rect, S):
    _, x0, y0, x1, y1 = rect
    return 0 if x1 <= x0 or y1 <= y0 else (y1 - y0) * ((x1 - 1) // S - x0 // S + 1)


def tile_lengths(s, ranges):
    gx, gy = (s.W + 15) // 16, (s.H + 15) // 16
    r = np.asarray(ranges).reshape(-1, 2).astype(np.int64)
    return (r[:, 1] - r[:, 0]).reshape(gy, gx)


_oracle = {}


def oracle_state(O, name):
    """(state, outputs) of the oracle's forward on a frame: computed once, changed by nobody"""
    if name not in _oracle:
        import hip_helpers as hh
        s, _ = get(name)
        _oracle[name] = hh.oracle_forward(O, s, 0)
    return _oracle[name]


# ------------------------------------------------------------------------------------------ the GPU side (test and child alike)
STATE = ("ranges", "point_list", "keys")
IMAGES = ("color", "depth", "depth_median", "depth_var", "opacity_map")


def read_trace(s, run):
    """run() under dgr_debug_bin_tiles_trace, decoded as profiles/r9/bin_tiles_trace.py does: (run's result, the number of workgroups
    that stamped word 0, [(workgroup, segment, gcount, n_pairs, tmax, dense)] of the workgroups that noted word 7 -- a segment's
    own workgroup when the segment owns instances, a helper only when it is dense)"""
    import torch
    from dgr_amd import _capi
    lib = _capi.load()
    gx, gy = (s.W + 15) // 16, (s.H + 15) // 16
    most = gy * -(-gx // 4) * 4 + 64           # more than any segment size launches
    buf = torch.zeros(most * 8, dtype=torch.int64, device="cuda")
    lib.dgr_debug_bin_tiles_trace(buf.data_ptr())
    try:
        result = run()
        torch.cuda.synchronize()
    finally:
        lib.dgr_debug_bin_tiles_trace(None)
    w = [[int(v) for v in row] for row in buf.cpu().numpy().view(np.uint64).reshape(-1, 8)]
    stamped = sum(1 for row in w if row[0])
    assert not any(any(row) for row in w[stamped:])   # the workgroups are 0 .. stamped - 1
    notes = [(i, (row[7] >> 32) & 0x7fffffff, row[6] & 0xffffffff, row[6] >> 32, row[7] & 0xffffffff, bool(row[7] >> 63))
             for i, row in enumerate(w[:stamped]) if row[7]]   # (tmax >= 1 wherever word 7 was written)
    return result, stamped, notes


def check_frame(name, O, S):
    """One frame through the forward in a process that bins at S tiles per segment.  Returns a list of failures (strings), empty when
    the state equals the oracle's bit for bit; the number of bin_tiles workgroups is that of S; every segment that owns instances
    noted the designed gcount, n_pairs, tmax and dense bit, and every helper of a dense segment (and no other) the same; and the
    global-counter binning ("lds_count" = 0) and the callback entry give the same state and the same five images."""
    import hip_helpers as hh
    from dgr_amd import _capi
    s, design = get(name)
    st, ref = oracle_state(O, name)
    bad = []

    def state_of(d):
        return {k: hh.hip_state(k, s, d) for k in STATE}

    hh.hip_forward(s, 0)    # (the shape's first forward sizes the binning buffer; the traced one is a settled call)
    (out, d), stamped, notes = read_trace(s, lambda: hh.hip_forward(s, 0))
    mine = state_of(d)
    if d["num_rendered"] != ref["num_rendered"]:
        bad.append(f"num_rendered {d['num_rendered']} != {ref['num_rendered']}")
    if not np.array_equal(d["radii"], ref["radii"]):
        bad.append("radii")
    bad += [f"{k} differs from the oracle's" for k in STATE if not np.array_equal(mine[k], st.get(k))]
    sizes = [c for c in (4, 8, 16) if workgroups(design, c) == stamped]
    if S not in sizes:
        bad.append(f"{stamped} bin_tiles workgroups: {sizes or 'no'} tiles per segment, not {S}")
    gy, gx = design["lengths"].shape
    nseg = gy * -(-gx // S)
    seg, pr = segments(design, S), pairs(design, S)
    want = {k: (g, pr[k], t, dense) for k, (g, t, dense) in seg.items()}
    own = {n[1]: n[2:] for n in notes if n[0] < nseg}
    if own != want or sum(1 for n in notes if n[0] < nseg) != len(own):
        diff = sorted((k, own.get(k), want.get(k)) for k in set(own) | set(want) if own.get(k) != want.get(k))
        bad.append(f"trace (gcount, n_pairs, tmax, dense) != design at {S} tiles per segment: {diff[:6]}")
    helpers = sorted(n[1:] for n in notes if n[0] >= nseg)
    if helpers != sorted((k,) + v for k, v in want.items() if v[3] for _ in range(S // 4 - 1)):
        bad.append(f"helper notes {helpers[:6]} for the dense segments {[k for k, v in want.items() if v[3]]} at {S} tiles per segment")
    res = {}
    old = os.environ.get("DGR_FORWARD_MODE")
    try:
        for mode, lds in (("presized", 0), ("callback", 1)):
            os.environ["DGR_FORWARD_MODE"] = mode
            _capi.set_option("lds_count", lds)
            try:
                _, d2 = hh.hip_forward(s, 0)
                res[mode, lds] = (d2, state_of(d2))
            finally:
                _capi.set_option("lds_count", 1)
    finally:
        if old is None:
            os.environ.pop("DGR_FORWARD_MODE", None)
        else:
            os.environ["DGR_FORWARD_MODE"] = old
    for path, (d2, st2) in res.items():
        if d2["num_rendered"] != d["num_rendered"] or not np.array_equal(d2["radii"], d["radii"]):
            bad.append(f"{path}: num_rendered / radii")
        bad += [f"{path}: {k}" for k in STATE if not np.array_equal(st2[k], mine[k])]
        bad += [f"{path}: {k}" for k in IMAGES if not np.array_equal(d2[k], d[k])]
    return bad


def child_main(argv):
    """tests/binning_frames_child.py: every frame (or the named ones) at the segment size DGR_SEG_SHIFT forces, one JSON line"""
    from oracle import oracle as O
    O.build()
    S = 1 << int(os.environ["DGR_SEG_SHIFT"])
    print(json.dumps({"tiles_per_segment": S, "failures": {n: check_frame(n, O, S) for n in (argv or list(FRAMES))}}))
    return 0
