"""The light forward blend at the edges of its batch loop.

The forward stages a tile's list 256 entries at a time; behind each batch's pair loop it writes the batch's tag bytes, appends the
entries somebody blended to the tile's live list and takes the workgroup's vote "every pixel finished" (csrc/render_light.hip:
flush_slot).  What a staging thread needs for that -- its Gaussian's id -- stays in a register from staging to flush.  Here:

  * batch boundaries: ONE tile of a 32x32 frame with exactly K = 256, 257 and 512 entries (a full batch and nothing behind it, a
    second batch of one entry, two full batches);
  * a ragged 70x41 frame whose right and bottom edge tiles -- pixels outside the frame in every quadrant -- take several batches,
    with the backward against the oracle;
  * an opaque 48x48 frame whose tiles finish before their last batch: the unstaged tail's tag bytes are zero and the live count
    is what was flushed;

each on both lane mappings (option lane_lists = 0: half-wave lists, 1: quadrant lists).  Every case checks: the alpha image, the
median depth, n_contrib and the per-Gaussian pixel counts equal the oracle's bit for bit; colour, depth and gau_uncertainty meet the
bars of tests/test_hip_light_parity.py (assert_images_carry_the_references_bits: 1e-6 on every value); every list entry's tag byte
is written (it agrees with n_contrib, quadrant by quadrant); the live list is exactly the tagged entries in order, the live
count their number.
Colour and depth are NOT the oracle's bits, by the kernel's design (it sums them with fused multiply-adds, the oracle rounds
twice per term): on these scenes 58 .. 73 of 3072 colour values and 15 .. 20 of 1024 depth values differ in their last bits at
K = 256 .. 512, 2616 of 8610 / 768 of 2870 on the ragged frame, 1596 of 6912 / 421 of 2304 on the opaque one, max |d| below
1e-6 -- the same values, to the bit, before and after the forward's batch loop was reshaped, and on both lane mappings.
"""
import numpy as np
import pytest

from util import make_scene, one_tile_scene
import hip_helpers as hh
from hip_helpers import forced_lane_lists as lane_lists  # noqa: F401  (fixtures)
from test_hip_light_parity import assert_images_carry_the_references_bits, check_backward
from test_hip_live_lists import assert_live_list_is_the_tagged_entries, opaque_scene

pytestmark = pytest.mark.gpu

BATCH = 256  # entries the forward stages at a time (DGR_TILE_PIX)


def fold8(t):
    """a tag byte (bit 2 w + h: half h of quadrant wave w) -> four bits, one per quadrant"""
    t = (t | (t >> 1)) & 0x55
    return (t & 1) | ((t >> 1) & 2) | ((t >> 2) & 4) | ((t >> 3) & 8)


def assert_every_tag_byte_is_written(s, d, tags, ranges):
    """The bytes underneath the tags are the binning's (arrival ranks, column covers): an entry whose byte the forward did not
    write shows as a mark nobody's n_contrib accounts for.  Per tile and quadrant: a pixel's last contributor is marked, the
    deepest mark is the quadrant's deepest last contributor, and a quadrant nobody blended for has none."""
    nc = hh.hip_state("n_contrib", s, d).reshape(s.H, s.W)
    gx = (s.W + 15) // 16
    for tile, (lo, hi) in enumerate(ranges):
        tx, ty = tile % gx, tile // gx
        t = fold8(tags[lo:hi].astype(np.uint32))
        for q in range(4):
            x0, y0 = tx * 16 + (q & 1) * 8, ty * 16 + (q >> 1) * 8
            blk = nc[y0:y0 + 8, x0:x0 + 8]
            marked = np.nonzero((t >> q) & 1)[0]
            if blk.size == 0 or blk.max() == 0:
                assert marked.size == 0, (tile, q)
                continue
            assert marked.size and marked.max() == blk.max() - 1, (tile, q)
            assert np.all(((t[blk[blk > 0] - 1] >> q) & 1) == 1), (tile, q)


def check_forward(oracle, s, deg):
    """the checks every case shares; returns the forward's state and the exported tags, live counts and ranges"""
    _, d = hh.hip_forward(s, deg)
    st, ref = hh.oracle_forward(oracle, s, deg)
    assert d["num_rendered"] == ref["num_rendered"]
    assert np.array_equal(hh.hip_state("ranges", s, d), st.get("ranges"))
    assert_images_carry_the_references_bits(d, st, ref, s)  # (n_contrib, gau_related_pixels, gau_uncertainty among them)
    assert np.all(d["depth_var"] == 0)
    tags, counts, ranges = assert_live_list_is_the_tagged_entries(s, d)
    assert_every_tag_byte_is_written(s, d, tags, ranges)
    return d, tags, counts, ranges


@pytest.mark.parametrize("K", [256, 257, 512])
def test_batch_boundaries(oracle, lane_lists, K):
    s = one_tile_scene(K)
    d, tags, counts, ranges = check_forward(oracle, s, 0)
    assert ranges[0, 1] - ranges[0, 0] == K and d["num_rendered"] == K  # the tile's list has exactly K entries, the others none
    nc = hh.hip_state("n_contrib", s, d).reshape(s.H, s.W)
    assert nc.max() > K - 8         # the list is walked to its end: an entry of the last batch is somebody's last contributor
    assert counts[0] > 0 and not counts[1:].any()
    check_backward(oracle, s, 0, what=f"one tile, K={K}")


def test_ragged_frame(oracle, lane_lists):
    s = make_scene(6000, 70, 41, 6)
    d, tags, counts, ranges = check_forward(oracle, s, 3)
    gx, gy = (s.W + 15) // 16, (s.H + 15) // 16
    n = (ranges[:, 1] - ranges[:, 0]).reshape(gy, gx)
    assert n[:, gx - 1].max() > BATCH and n[gy - 1, :].max() > BATCH  # a right-edge and a bottom-edge tile of more than one batch
    check_backward(oracle, s, 3, what="ragged 70x41")


def test_early_finish(oracle, lane_lists):
    s = opaque_scene(3000, 48, 48, 3)
    d, tags, counts, ranges = check_forward(oracle, s, 3)
    nc = hh.hip_state("n_contrib", s, d).reshape(s.H, s.W)
    gx = (s.W + 15) // 16
    early = 0
    for tile, (lo, hi) in enumerate(ranges):
        tx, ty = tile % gx, tile // gx
        last = int(nc[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].max())
        walked = BATCH * -(-last // BATCH)  # the batches up to the one that holds the tile's last contributor
        if hi - lo > walked:
            early += 1
            assert not tags[lo + walked:hi].any(), tile                              # the tail: staged without effect or never staged
            assert counts[tile] == np.count_nonzero(tags[lo:lo + walked]), tile      # the live count is what was flushed
    assert early > 0
