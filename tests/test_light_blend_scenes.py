"""What tests/test_hip_light_blend_edges.py relies on, checked on the CPU from the oracle's decisions and the float64 model: the
scenes of tests/light_blend_scenes.py have the live counts their names claim, with the dead entries, the median's firing entries
and the last contributors where the light backward's live-entry batches have their edges; the float oracle and the C-math oracle
decide every pixel alike and no median decision is closer than 1e-5, so the GPU test leaves no pixel, row or element out.

A seed that fails one of these conditions is changed; the condition stays."""
import numpy as np
import pytest

import light_blend_scenes as S
from light_blend_scenes import BWD_BATCH, BWD_BATCH_DET
from ref_parity import GRADS, MODES, SANITY, alpha_interface_factor, scale_distance

ALL = list(S.SCENES)
MORE_THAN_ONE_BATCH = [n for n in ALL if max(S.SCENES[n][1].values()) > BWD_BATCH]


def splits_of(total):
    """the batch sizes the kernel walks a tile of `total` live entries with: (what, entries per batch)"""
    return [("equal", S.batch_size(total, "equal")), ("128", BWD_BATCH), ("64", BWD_BATCH_DET)]


@pytest.mark.parametrize("name", ALL)
def test_live_counts_are_the_names(oracle, name):
    s = S.scene(name)
    st, ref = S.oracle_forward(oracle, name)
    live, tiles = S.live_positions(oracle, name)
    want = S.SCENES[name][1]
    assert {t: v.size for t, v in live.items() if v.size} == want
    assert ref["num_rendered"] == S.LIST_LENGTH[name]
    nc = st.get("n_contrib").reshape(s.H, s.W).astype(np.int64)
    ranges = st.get("ranges").reshape(-1, 2).astype(np.int64)
    for t in tiles:   # the derivation reproduces the oracle's own last contributors: the deepest blended position + 1, per pixel
        deepest = np.where(t.valid.any(0), t.valid.shape[0] - np.argmax(t.valid[::-1], 0), 0)
        assert np.array_equal(deepest, nc[t.y0:t.y0 + 16, t.x0:t.x0 + 16]), name
    if name in S.OPAQUE_NAMES:   # pixels that finish: their last contributor is not their deepest entry that passes the alpha test
        assert S.LIST_LENGTH[name] - live[0].size > 0
    if name.startswith("live"):   # every list entry is live, and the list is walked to its end
        assert np.array_equal(live[0], np.arange(want[0])) and nc.max() == want[0]
    if name == "two_tiles":
        assert {t: tuple(r) for t, r in enumerate(ranges.tolist()) if r[1] > r[0]} == S.TWO_TILES_RANGES
        assert ranges[3, 0] % 2 == 1   # (the second tile's live list starts at an odd offset)


@pytest.mark.parametrize("name", S.SPARSE_NAMES + S.OPAQUE_NAMES)
def test_sparse_scenes_have_dead_entries_between_the_live_ones(oracle, name):
    live, _ = S.live_positions(oracle, name)
    pos = live[0]
    n = min(BWD_BATCH, pos.size)
    for i in range(pos.size - n + 1):   # a dead position within every 128 consecutive live entries (all 65, where there are no more)
        assert pos[i + n - 1] - pos[i] > n - 1, (name, i)
    for per in (BWD_BATCH_DET, S.batch_size(pos.size, "equal")):   # ... and within every batch of two entries or more that the kernel forms
        for hi in range(pos.size, 1, -per):
            lo = max(0, hi - per)
            assert hi - lo < 2 or pos[hi - 1] - pos[lo] > hi - 1 - lo, (name, per, hi)
    assert 2 * np.count_nonzero(pos != np.arange(pos.size)) > pos.size   # (live index and list position differ on most entries)


@pytest.mark.parametrize("name", ALL)
def test_the_cut_at_the_last_contributor_decides_on_the_opaque_scenes_only(oracle, name):
    """(pixel, live entry) pairs that pass the alpha test at or behind the pixel's last contributor -- kept out by the cut on the
    entry's list position alone: many on the opaque scenes, most of them with a live index in front of the last contributor (a
    cut taken on the index the loop counts would let them in); none anywhere else."""
    cut = sum(int(c.sum()) for c, _ in S.cut_pairs(oracle, name))
    by_index = sum(int(b.sum()) for _, b in S.cut_pairs(oracle, name))
    pixels = sum(int(b.any(0).sum()) for _, b in S.cut_pairs(oracle, name))
    print(f"{name:<16} pairs behind the last contributor that pass the alpha test {cut:>4}, with a live index in front of it {by_index:>4} "
          f"on {pixels} pixels")
    if name in S.OPAQUE_NAMES:
        assert cut >= 16 and by_index >= 16 and pixels >= 4
    else:
        assert cut == 0


@pytest.mark.parametrize("name", ALL)
def test_float_and_c_math_oracle_decide_alike(oracle, name):
    (st, ref), (st_c, ref_c) = S.oracle_forward(oracle, name), S.oracle_forward(oracle, name, cmath=True)
    assert ref["num_rendered"] == ref_c["num_rendered"] and np.array_equal(ref["radii"], ref_c["radii"])
    for k in ("point_list", "ranges", "n_contrib"):
        assert np.array_equal(st.get(k), st_c.get(k)), k
    s = S.scene(name)
    for a, b in zip(S.contributors(oracle, s, st), S.contributors(oracle, s, st_c)):
        assert a.tile == b.tile and np.array_equal(a.valid, b.valid), name
    assert np.array_equal(ref["gau_related_pixels"], ref_c["gau_related_pixels"])


@pytest.mark.parametrize("name", ALL)
def test_no_median_decision_is_close(oracle, name):
    """min_k |T_k - 0.5| of the transmittances the sides re-derive from the alpha image they are handed, less what that image's
    rounding moves them by against the float64 model's (ref_parity.compare_forward), is 1e-5 at least on every pixel with a
    contributor; nor does the model see an alpha within its window of the blend threshold."""
    s = S.scene(name)
    st, ref = S.oracle_forward(oracle, name)
    f64, alphas = S.forward64(oracle, name)
    margin = oracle.light_median_margin(st, alphas).reshape(s.H, s.W).astype(np.float64)
    margin -= np.abs(alpha_interface_factor(f64, alphas).reshape(s.H, s.W) - 1.0)
    has = st.get("n_contrib").reshape(s.H, s.W) > 0
    print(f"{name:<16} smallest median margin {margin[has].min():.2e}")
    assert has.any() and margin[has].min() >= 1e-5
    assert not f64["_ambiguous"].any()


@pytest.mark.parametrize("name", MORE_THAN_ONE_BATCH)
def test_median_and_last_contributor_cross_the_batch_edges(oracle, name):
    """Per tile of more than 128 live entries and per batch split the kernel walks it with: pixels whose median term fires in
    another batch than the one that holds their last contributor (the threshold is carried, unfired, across an edge), and pixels
    whose last contributor lies before the batch walked first (the cut `position < last_contributor` holds a whole batch back).
    A tile of 129 in batches of 128 -- the tracking instance's and every quadrant-list instance's split -- leaves ONE entry, the
    front-most, to its second batch: a pixel's median fires there when that entry alone takes T to 0.5 or below, its last
    contributor lies there when the pixel blends nothing else.  The seeds of the 129-live tiles are chosen for a pixel of each
    kind (light_blend_scenes.SEED_129)."""
    for tm in S.median_and_last(oracle, name):
        total = tm.live.size
        assert total > BWD_BATCH
        for what, per in splits_of(total):
            b_last, b_fire = S.batch_of(tm.last, total, per), S.batch_of(tm.fire, total, per)
            other = int(np.count_nonzero(tm.any & (b_last != b_fire)))
            before = int(np.count_nonzero(tm.any & (b_last > 0)))
            print(f"{name:<16} tile {tm.tile} live {total:>3} batches of {per:>3} ({what:<5}): median in another batch {other:>3}, "
                  f"last contributor before the first-walked batch {before:>3}")
            assert other > 0 and before > 0, (name, tm.tile, what)


@pytest.mark.parametrize("name", ALL)
def test_live_batches_have_neighbours_in_different_halves(oracle, name):
    """the paired steps (neighbouring entries of a quadrant's list that live in different halves) exist in the batches the paired
    kernel forms -- and in those of 128 and 64 entries, whose kernels must not pair them"""
    live, tiles = S.live_positions(oracle, name)
    for t in tiles:
        lv = S.live_only(t, live[t.tile])
        for what, per in splits_of(live[t.tile].size):
            n = S.split_neighbours(lv, per)
            print(f"{name:<16} tile {t.tile} batches of {per:>3} ({what:<5}): neighbours in different halves, the best quadrant list {n}")
            assert n > 0, (name, t.tile, what)


@pytest.mark.parametrize("name", ALL)
def test_the_oracle_is_close_to_float64_in_every_mode(oracle, name):
    for mode in MODES:
        _, track_off, map_off = mode
        _, _, g_or, g64 = S.references(oracle, name, mode)
        for k in GRADS:
            if k not in g64:
                continue
            if track_off if k == "dL_dview" else map_off:
                assert not np.asarray(g_or[k]).any(), (name, mode[0], k)
                continue
            e = scale_distance(g_or[k], g64[k])
            print(f"{name:<16} {mode[0]:<13} {k:<14} e_oracle {e:9.2e}")
            assert e <= SANITY, (name, mode[0], k)
