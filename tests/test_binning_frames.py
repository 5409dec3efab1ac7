"""What tests/test_hip_binning_edges.py relies on, checked on the CPU with the oracle alone: every frame of tests/binning_frames.py
has exactly the designed tile list lengths (hence segment totals, longest lists and dense bits at every segment size), its wide
Gaussians exactly the designed tile rectangles, and each design sits on the edge it is named for."""
import numpy as np
import pytest

import binning_frames as B
from binning_frames import BIG_PAIRS, BIGQ, K2_CAP, REG_SORT_MAX


@pytest.mark.parametrize("name", list(B.FRAMES))
def test_the_oracle_bins_every_frame_as_designed(oracle, name):
    s, design = B.get(name)
    st, ref = B.oracle_state(oracle, name)
    assert np.array_equal(B.tile_lengths(s, st.get("ranges")), design["lengths"])
    assert ref["num_rendered"] == design["lengths"].sum()
    assert np.array_equal(ref["radii"] > 0, design["visible"])
    xy = st.get("means2D").reshape(-1, 2)
    for i, x0, y0, x1, y1 in design["rects"][::7]:
        assert B.rect_of(s.W, s.H, float(xy[i, 0]), float(xy[i, 1]), int(ref["radii"][i])) == (x0, y0, x1, y1), i
    # a wrong segment size cannot pass for the right one: it launches another number of bin_tiles workgroups or has other segments
    assert len({(B.workgroups(design, S), tuple(sorted(B.segments(design, S).items()))) for S in (4, 8, 16)}) == 3


def test_rule_and_parts_sit_on_the_list_length_edges():
    for name in ("rule", "rule_flat"):
        _, design = B.get(name)
        assert sorted(design["lengths"].reshape(-1)) == [1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024]
        for S in (4, 8, 16):
            assert all(g <= K2_CAP and t <= REG_SORT_MAX and not d for g, t, d in B.segments(design, S).values())
    _, design = B.get("parts")
    for S in (4, 8, 16):
        seg = B.segments(design, S)
        assert sorted(t for _, t, _ in seg.values()) == [1025, 1537, 2048, 2049] and not any(d for _, _, d in seg.values())
    assert 2048 in design["lengths"] and 2049 in design["lengths"]   # SORT_LDS_MAX of the global-counter path


def test_rule_flat_has_one_depth_per_tile(oracle):
    s, design = B.get("rule_flat")
    st, _ = B.oracle_state(oracle, "rule_flat")
    keys, rg = st.get("keys"), st.get("ranges").reshape(-1, 2)
    for lo, hi in rg:
        assert hi <= lo or np.unique(keys[lo:hi] >> np.uint64(32)).size == 1
    assert np.unique(keys >> np.uint64(32)).size == 12


def test_budget_and_groups_sit_on_the_lds_budget():
    _, design = B.get("budget")
    assert B.segments(design, 16) == {0: (6144, 384, False), 1: (6145, 385, True)}
    assert not any(d for S in (4, 8) for _, _, d in B.segments(design, S).values())
    _, design = B.get("groups")
    for S in (4, 8, 16):
        assert B.segments(design, S) == {0: (9144, 3000, True), 1: (12289, 6144, True), 2: (6155, 6145, True), 3: (8293, 8193, True)}
    rows = design["lengths"]
    assert rows[0, 0] + rows[0, 1] <= K2_CAP < rows[0, 0] + rows[0, 1] + rows[0, 2]    # a group of two, then one of two
    assert rows[1, 0] == K2_CAP and rows[1, 2] == 0                                    # a group of exactly the budget; an empty tile
    assert rows[2, 0] == K2_CAP + 1 and rows[3, 0] > K2_CAP                            # single lists sorted in global memory


def test_ragged_loads_the_short_last_segment():
    for gx in B.RAGGED:
        _, design = B.get(f"ragged{gx}")
        for S in (4, 8, 16):
            if gx in (S + 1, 2 * S - 1):
                seg = B.segments(design, S)
                last = -(-gx // S) - 1
                assert gx % S and last in seg and seg[last][1] > REG_SORT_MAX, (gx, S)
    _, design = B.get("ragged5")
    assert B.segments(design, 16) == {0: (6800, 3200, True)} and B.segments(design, 8) == {0: (6800, 3200, True)}


def test_spans_cover_whole_segments_and_cross_their_borders():
    _, design = B.get("spans")
    for S in (4, 8, 16):
        seg, pr = B.segments(design, S), B.pairs(design, S)
        assert set(seg) == set(pr)
        assert sum(pr.values()) * 2 < sum(g for g, _, _ in seg.values())
        whole = [r for r in design["rects"] if any(r[1] <= a and a + S <= r[3] for a in range(0, 32, S))]   # columns 0 .. S - 1
        crossing = [r for r in design["rects"] if r[1] // S != (r[3] - 1) // S and (r[1] % S or r[3] % S)]
        assert len(whole) >= 30 and len(crossing) >= 20, S


def test_runs_leave_empty_runs_between_and_in_front(oracle):
    s, design = B.get("runs")
    assert s.P == 5000 and B.per_wg(s.P) == 1024
    st, _ = B.oracle_state(oracle, "runs")
    pl, rg = st.get("point_list"), st.get("ranges").reshape(-1, 2)
    from_wgs = lambda tile: sorted(set((pl[rg[tile, 0]:rg[tile, 1]] // 1024).tolist()))   # noqa: E731
    assert from_wgs(0) == [0, 2, 4] and from_wgs(4) == [4] and from_wgs(8) == [0, 1, 2, 3, 4]


def test_rectangles_sit_on_the_queue_threshold_and_have_every_width():
    s, design = B.get("rectangles")
    rects = design["rects"]
    assert B.pairs_of(rects[0], 4) == BIG_PAIRS and B.pairs_of(rects[1], 4) == BIG_PAIRS + 1
    shapes = {((x1 - 1) // 4 - x0 // 4 + 1, y1 - y0) for _, x0, y0, x1, y1 in rects}
    assert shapes >= {(nsx, rows) for nsx in B.RECT_NSX for rows in B.RECT_ROWS}
    gy, gx = design["lengths"].shape
    assert any(x0 == 0 and x1 < gx for _, x0, y0, x1, y1 in rects) and any(x1 == gx and x0 > 0 for _, x0, y0, x1, y1 in rects)
    assert any(y0 == 0 and y1 < gy for _, x0, y0, x1, y1 in rects) and any(y1 == gy and y0 > 0 for _, x0, y0, x1, y1 in rects)


def test_queue_is_full_in_one_workgroup_and_not_in_another():
    s, design = B.get("queue")
    assert s.P == 8192 and B.per_wg(s.P) == 1024
    for S in (4, 8, 16):
        big = [r[0] for r in design["rects"] if B.pairs_of(r, S) > BIG_PAIRS]
        assert sum(1 for i in big if i < 1024) == 700 > BIGQ
        assert sum(1 for i in big if 4096 <= i < 5120) == 10 and len(big) == 710
    assert 250 <= design["visible"].sum() - 710 <= 300


def test_reread_is_beyond_what_the_registers_hold():
    s, design = B.get("reread")
    assert s.P == B.REREAD_P > 256 * 4096 and B.per_wg(s.P) == 5120
    vis = np.nonzero(design["visible"])[0]
    g0 = B.REREAD_WG * 5120
    assert vis.min() >= g0 and vis.max() < g0 + 5120
    assert np.count_nonzero(vis < g0 + 4096) == 2000 and np.count_nonzero(vis >= g0 + 4096) == 1000
    big = np.array([r[0] for r in design["rects"] if B.pairs_of(r, 4) > BIG_PAIRS])
    assert big.size >= 30 and np.count_nonzero(big < g0 + 4096) == 20 and np.count_nonzero(big >= g0 + 4096) == 15


def test_wide41_is_the_frame_that_needs_the_half_in_the_float_division():
    """queued_pair's row = (int)((p + 0.5f) * (1.0f / nsx)), restated in float32: exact for every designed rectangle; without the
    half it is exact for the `rectangles` frame (nsx <= 13) and wrong for wide41's 41 segments -- the frame a kernel that lost the
    half would fail on."""
    f = np.float32

    def rows_ok(rect, half):
        _, x0, y0, x1, y1 = rect
        nsx = (x1 - 1) // 4 - x0 // 4 + 1
        p = np.arange((y1 - y0) * nsx)
        row = ((p.astype(f) + f(half)) * (f(1.0) / f(nsx))).astype(np.int64)
        return nsx, bool(np.array_equal(row, p // nsx))

    for name in ("rectangles", "queue", "reread", "spans", "wide41"):
        assert all(rows_ok(r, 0.5)[1] for r in B.get(name)[1]["rects"]), name
    assert all(rows_ok(r, 0.0)[1] for r in B.get("rectangles")[1]["rects"])
    got = [rows_ok(r, 0.0) for r in B.get("wide41")[1]["rects"]]
    assert got == [(41, False), (42, True)] and all(B.pairs_of(r, 4) > BIG_PAIRS for r in B.get("wide41")[1]["rects"])
