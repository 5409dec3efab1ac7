"""What tests/test_hip_full_blend_edges.py relies on, checked on the CPU with the oracle's full forward and the float64 model: the
scenes of tests/full_blend_scenes.py put the lists, the first and the last contributors where the full blend kernels' batch loops
have their edges, and the float oracle and the C-math oracle decide every pixel alike, so the GPU tests need no flip mask."""
import numpy as np
import pytest

import fp64_model as M
import full_blend_scenes as S
from full_blend_scenes import BWD_BATCH, FWD_BATCH


def state(oracle, name):
    s, _ = S.scene(name)
    st, ref = S.oracle_full_forward(oracle, name)
    nc = st.get("n_contrib").reshape(s.H, s.W).astype(np.int64)
    return s, st, ref, nc


def derived(oracle, name):
    """(first_contrib, n_valid, contributors) from the oracle's state; the derivation reproduces the oracle's own counts"""
    s, st, ref, nc = state(oracle, name)
    tiles = S.contributors(oracle, s, st)
    first, count = S.first_and_count(s, tiles)
    assert np.array_equal(count, st.get("n_valid_contrib").reshape(s.H, s.W)), name
    assert np.array_equal(first > 0, nc > 0) and np.all(first <= nc), name
    return first, count, tiles


@pytest.mark.parametrize("K", S.EXACT_K)
def test_exact_is_one_list_of_K_entries_walked_to_its_end(oracle, K):
    s, st, ref, nc = state(oracle, f"exact{K}")
    n = S.tile_lengths(s, st).reshape(-1)
    assert n[0] == K and not n[1:].any() and ref["num_rendered"] == K
    assert nc.max() > K - 8


def test_shadowed_puts_first_and_last_contributors_in_other_batches(oracle):
    s, st, ref, nc = state(oracle, "shadowed")
    first, _, _ = derived(oracle, "shadowed")
    assert S.tile_lengths(s, st).reshape(-1)[0] == 384 and ref["num_rendered"] == 384
    assert np.count_nonzero(first > BWD_BATCH) >= 32
    # the equal halves cannot put 32 first contributors beyond the forward's first batch (full_blend_scenes.shadowed) ...
    assert np.count_nonzero((first > BWD_BATCH) & (first <= FWD_BATCH)) >= 32
    assert nc.max() > FWD_BATCH and np.count_nonzero((nc > 0) & (nc <= FWD_BATCH)) >= 32
    # ... its second variant does
    s2, st2, ref2, nc2 = state(oracle, "shadowed272")
    first2, _, _ = derived(oracle, "shadowed272")
    assert S.tile_lengths(s2, st2).reshape(-1)[0] == 384 and ref2["num_rendered"] == 384
    assert np.count_nonzero(first2 > FWD_BATCH) >= 32
    assert nc2.max() > FWD_BATCH and np.count_nonzero((nc2 > 0) & (nc2 <= FWD_BATCH)) >= 32


@pytest.mark.parametrize("name", S.ONE_TILE)
def test_one_tile_scenes_have_neighbours_in_different_halves(oracle, name):
    _, _, tiles = derived(oracle, name)
    assert max(S.split_neighbours(t) for t in tiles) >= 8


def test_ragged_has_edge_tiles_of_more_than_one_forward_batch(oracle):
    s, st, ref, nc = state(oracle, "ragged")
    n = S.tile_lengths(s, st)
    assert s.W % 16 and s.H % 16 and np.any(s.bg != 0)
    assert n[:, -1].max() > FWD_BATCH and n[-1, :].max() > FWD_BATCH
    derived(oracle, "ragged")


def test_opaque_finishes_early(oracle):
    s, st, ref, nc = state(oracle, "opaque")
    n, last = S.tile_lengths(s, st), S.tile_max(s, nc)
    walked = FWD_BATCH * -(-last // FWD_BATCH)   # the forward batches up to the one that holds the tile's last contributor
    assert np.any((last > 0) & (n > walked))     # an unstaged forward batch behind it
    assert np.any((last > 0) & (2 * last <= n))  # the backward walks min(range, max_last): half the list at most


@pytest.mark.parametrize("name", list(S.SCENES))
def test_float_and_c_math_oracle_decide_alike(oracle, name):
    st, ref = S.oracle_full_forward(oracle, name)
    st_c, ref_c = S.oracle_full_forward(oracle, name, cmath=True)
    assert ref["num_rendered"] == ref_c["num_rendered"] and np.array_equal(ref["radii"], ref_c["radii"])
    for k in ("point_list", "ranges", "n_contrib", "n_valid_contrib"):
        assert np.array_equal(st.get(k), st_c.get(k)), k
    assert ref["num_related"] == ref_c["num_related"]


def test_the_models_first_contrib_and_n_valid_are_the_oracles(oracle):
    name = "exact257"
    s, st, ref, nc = state(oracle, name)
    first, count, _ = derived(oracle, name)
    _, _, img = M.torch_full(s, 0, ref["radii"] > 0, st.get("point_list"), st.get("ranges"), st.get("n_contrib"), M.scaled_grads(s, "full"))
    assert img["first_contrib"].shape == (s.H, s.W) and img["n_valid"].shape == (s.H, s.W)
    assert np.array_equal(img["first_contrib"], first)
    assert np.array_equal(img["n_valid"], count)
    assert first.max() > BWD_BATCH  # (a first contributor beyond the backward's front batch is among what it found)
