"""The C-ABI library loads (no GPU needed) and exports every symbol include/dgr_hip.h declares."""
import ctypes
import os

import pytest

from dgr_amd import _capi

from abi_checks import declared_symbols


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_capi.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/dgr_hip.h but not exported"


def test_binding_covers_the_header():
    assert set(_capi.exported_symbols()) == set(declared_symbols())
    lib = _capi.load()
    assert lib.dgr_version().startswith(b"dgr_hip")


def test_state_sizes_scale_as_documented():
    lib = _capi.load()
    assert lib.dgr_geometry_bytes(0) == 0
    g1, g2 = lib.dgr_geometry_bytes(1000), lib.dgr_geometry_bytes(2000)
    # 64 (rec: 48 bytes of data in a 64-byte slot, one L2 line per gather) + 4 (depth) + 4 (radius) + 8 (rect) + 1 (clamped) +
    # 4 (goff) + 48 (SH direction derivatives) B per Gaussian, plus the per-256-Gaussian block totals and 256-byte alignment of each array
    assert 133 * 1000 <= g1 <= 133 * 1000 + 10 * 256 and g2 > g1
    # 24 B per instance (list, key scratch, ranks / pair columns, pair keys) + the segment binning's tables: per tile row
    # of a 64x64 frame (4 tiles: one 16-tile segment) one word per bin_segments workgroup (256) for the run starts (+ one
    # closing row) and one for the running instance counts
    b = lib.dgr_binning_bytes(1000, 64, 64)
    assert 24 * 1000 + 256 * (5 + 4) * 4 <= b <= 24 * 1000 + 256 * (5 + 4) * 4 + 8 * 256
    assert lib.dgr_binning_bytes(2000, 64, 64) > b and lib.dgr_binning_bytes(1000, 1920, 1080) - b >= 256 * (68 * 8 * 2 - 9) * 4
    assert lib.dgr_light_backward_scratch_bytes(1000, 64, 64) >= 64 * 1000


def test_options_round_trip_and_reject_unknown_names():
    lib = _capi.load()
    assert lib.dgr_get_option(b"tight_cull") == 0
    assert lib.dgr_set_option(b"tight_cull", 1) == 0 and lib.dgr_get_option(b"tight_cull") == 1
    assert lib.dgr_set_option(b"tight_cull", 0) == 0
    assert lib.dgr_set_option(b"profile_every", 8) == 0 and lib.dgr_get_option(b"profile_every") == 8
    assert lib.dgr_set_option(b"profile_every", 1) == 0
    assert lib.dgr_get_option(b"fast_alpha") == 0  # the default alpha path carries the host's bits
    assert lib.dgr_set_option(b"fast_alpha", 1) == 0 and lib.dgr_get_option(b"fast_alpha") == 1
    assert lib.dgr_set_option(b"fast_alpha", 0) == 0
    assert lib.dgr_get_option(b"lds_count") in (0, 1, 2)
    keep = lib.dgr_get_option(b"lds_count")
    assert lib.dgr_set_option(b"lds_count", 2) == 0 and lib.dgr_get_option(b"lds_count") == 2
    assert lib.dgr_set_option(b"lds_count", keep) == 0
    keep = lib.dgr_get_option(b"lane_lists")   # 2 (the frame picks the blend kernels' lane lists) unless DGR_FWD_HALVES forced one
    assert keep in (0, 1, 2)
    for v, want in ((0, 0), (1, 1), (2, 2), (7, 2), (-3, 0)):
        assert lib.dgr_set_option(b"lane_lists", v) == 0 and lib.dgr_get_option(b"lane_lists") == want
    assert lib.dgr_set_option(b"lane_lists", keep) == 0
    assert lib.dgr_set_option(b"no_such_option", 1) == _capi.DGR_ERR_BAD_ARGUMENT
    assert b"no_such_option" in lib.dgr_last_error()
    with pytest.raises(ValueError):
        _capi.set_option("no_such_option", 1)
    assert lib.dgr_profile_select(b"no_such_stage") == _capi.DGR_ERR_BAD_ARGUMENT


X = None  # dgr_set_option refuses the value (DGR_ERR_BAD_ARGUMENT) and the option keeps what it had
SET_VALUES = tuple(range(-2, 10))
NORMALISED = (1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1)
CLAMPED_0_2 = (0, 0, 0, 1, 2, 2, 2, 2, 2, 2, 2, 2)
ONLY_0_1 = (X, X, 0, 1, X, X, X, X, X, X, X, X)
# name: (default, dgr_get_option after dgr_set_option(name, v) for v = -2 .. 9) -- the option table of csrc/options.hip as a caller
# sees it (include/dgr_hip.h); "fast_alpha" is the alias of "alpha_mode" (set: value ? 1 : 0; get: mode == 1)
OPTION_TABLE = {
    "blend_wgs_per_cu": (0, (0, 0, 0, 0, 0, 3, 4, 5, 6, 7, 0, 0)),
    "tight_cull": (0, NORMALISED),
    "deterministic_grads": (0, NORMALISED),
    "batch_order": (0, NORMALISED),
    "fast_alpha": (0, NORMALISED),
    "tile_schedule": (2, CLAMPED_0_2),
    "lane_lists": (2, CLAMPED_0_2),
    "lds_count": (1, CLAMPED_0_2),
    "alpha_mode": (0, (X, X, 0, 1, 2, X, X, X, X, X, X, X)),
    "pose_grad": (0, ONLY_0_1),
    "silhouette_grad": (0, ONLY_0_1),
    "profile_every": (1, (1, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9)),
    "batch_streams": (2, (1, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 8)),
}
# name: largest value dgr_set_thread_option takes (None: any value >= 0 is normalised to 0 / 1); the field's shift in the options word
THREAD_OPTIONS = {"alpha_mode": (2, 0), "fast_alpha": (None, 0), "tight_cull": (None, 4), "deterministic_grads": (None, 8),
                  "pose_grad": (1, 12), "silhouette_grad": (1, 16)}
OPTION_ENV = ("DGR_TILE_SCHEDULE", "DGR_ALPHA_MODE", "DGR_FAST_ALPHA", "DGR_DETERMINISTIC_GRADS", "DGR_POSE_GRAD",
              "DGR_SILHOUETTE_GRAD", "DGR_FWD_HALVES", "DGR_LDS_COUNT", "DGR_BLEND_WGS_PER_CU")


def test_the_whole_option_table_process_and_thread():
    """Every option's default, what dgr_set_option makes of -2 .. 9 (clamp, normalise, window or refuse), the per-thread
    overrides, unknown names, the options word and its swap.  Host-side state only; every value touched is put back."""
    lib = _capi.load()
    BAD = _capi.DGR_ERR_BAD_ARGUMENT
    pristine = not any(v in os.environ for v in OPTION_ENV)  # (the environment sets initial values: defaults only without it)
    saved = {n: lib.dgr_get_option(n.encode()) for n in OPTION_TABLE if n != "fast_alpha"}
    saved_word = lib.dgr_thread_options_swap(-1)
    try:
        lib.dgr_thread_options_swap(0)  # no overrides while the process-wide values are walked
        if pristine:
            for name, (default, _) in OPTION_TABLE.items():
                assert lib.dgr_get_option(name.encode()) == default, name
            assert saved_word == 0
            assert lib.dgr_thread_options_effective() == 69905 == 0x11111
            assert lib.dgr_thread_options_swap(0) == 0
        # ---- process-wide
        for name, (_, after) in OPTION_TABLE.items():
            n = name.encode()
            for v, want in zip(SET_VALUES, after):
                before = lib.dgr_get_option(n)
                rc = lib.dgr_set_option(n, v)
                if want is X:
                    assert rc == BAD, (name, v)
                    assert lib.dgr_last_error().startswith(n + b": "), (name, v, lib.dgr_last_error())
                    assert lib.dgr_get_option(n) == before, (name, v)
                else:
                    assert rc == 0 and lib.dgr_get_option(n) == want, (name, v, lib.dgr_get_option(n))
            if name == "fast_alpha":  # the alias writes alpha_mode 0 / 1 and reads "alpha_mode == 1"
                for mode, fast in ((0, 0), (1, 1), (2, 0)):
                    assert lib.dgr_set_option(b"alpha_mode", mode) == 0 and lib.dgr_get_option(b"fast_alpha") == fast
                assert lib.dgr_set_option(b"fast_alpha", 5) == 0 and lib.dgr_get_option(b"alpha_mode") == 1
            lib.dgr_set_option(b"alpha_mode" if name == "fast_alpha" else n, saved["alpha_mode" if name == "fast_alpha" else name])
        # ---- unknown names: set says so, the getters return the error code and leave the last error alone
        assert lib.dgr_set_option(b"no_such_option", 1) == BAD and lib.dgr_last_error() == b"unknown option: no_such_option"
        assert lib.dgr_set_option(b"alpha_mode", 3) == BAD
        marker = lib.dgr_last_error()
        assert marker.startswith(b"alpha_mode: ")
        assert lib.dgr_get_option(b"no_such_option") == BAD and lib.dgr_get_thread_option(b"no_such_option") == BAD
        assert lib.dgr_get_thread_option(b"lds_count") == BAD  # (not a per-thread option: nothing to read either)
        assert lib.dgr_last_error() == marker
        # ---- per thread
        for name in list(OPTION_TABLE) + ["no_such_option"]:
            n = name.encode()
            if name not in THREAD_OPTIONS:
                for v in (-1, 0, 1):
                    assert lib.dgr_set_thread_option(n, v) == BAD, (name, v)
                    assert lib.dgr_last_error() == b"not a per-thread option: " + n
                continue
            top, shift = THREAD_OPTIONS[name]
            target = b"alpha_mode" if name == "fast_alpha" else n
            for process_value in (0, 1):
                assert lib.dgr_set_option(target, process_value) == 0
                for v in SET_VALUES:
                    before = lib.dgr_get_thread_option(n)
                    rc = lib.dgr_set_thread_option(n, v)
                    if top is not None and v > top:
                        assert rc == BAD, (name, v)
                        assert lib.dgr_last_error().startswith(n + b": ") and b"process-wide" in lib.dgr_last_error()
                        assert lib.dgr_get_thread_option(n) == before, (name, v)
                        continue
                    want = process_value if v < 0 else (v if top is not None else int(v != 0))
                    assert rc == 0 and lib.dgr_get_thread_option(n) == want, (name, v)
                    assert lib.dgr_get_option(target) == process_value, (name, v)  # the process-wide value is untouched
                    mode = lib.dgr_get_thread_option(target)
                    assert (lib.dgr_thread_options_effective() >> shift) & 15 == mode + 1, (name, v)
                    assert (lib.dgr_thread_options_swap(-1) >> shift) & 15 == (0 if v < 0 else mode + 1), (name, v)
                assert lib.dgr_set_thread_option(n, -1) == 0
            lib.dgr_set_option(target, saved[target.decode()])
        # ---- the options word: every field value + 1, swap installs overrides (field 0 = inherit) and returns the previous word
        for n in saved:
            lib.dgr_set_option(n.encode(), 0 if n in ("alpha_mode", "tight_cull", "deterministic_grads", "pose_grad", "silhouette_grad") else saved[n])
        assert lib.dgr_thread_options_swap(0) == 0 and lib.dgr_thread_options_effective() == 0x11111
        word = (2 + 1) | (1 + 1) << 4 | (0 + 1) << 8 | (1 + 1) << 12 | (1 + 1) << 16
        assert lib.dgr_thread_options_swap(word) == 0
        assert lib.dgr_thread_options_effective() == word and lib.dgr_thread_options_swap(-1) == word
        got = [lib.dgr_get_thread_option(n) for n in (b"alpha_mode", b"fast_alpha", b"tight_cull", b"deterministic_grads", b"pose_grad", b"silhouette_grad")]
        assert got == [2, 0, 1, 0, 1, 1]
        assert all(lib.dgr_get_option(n.encode()) == 0 for n in ("alpha_mode", "tight_cull", "deterministic_grads", "pose_grad", "silhouette_grad"))
        partial = (1 + 1) << 4  # only tight_cull overridden: the other four inherit
        assert lib.dgr_thread_options_swap(partial) == word
        assert lib.dgr_thread_options_effective() == 0x11111 + (1 << 4) and lib.dgr_thread_options_swap(-1) == partial
        assert lib.dgr_thread_options_swap(0) == partial and lib.dgr_thread_options_effective() == 0x11111
    finally:
        for n, v in saved.items():
            lib.dgr_set_option(n.encode(), v)
        lib.dgr_thread_options_swap(saved_word)
    assert {n: lib.dgr_get_option(n.encode()) for n in saved} == saved and lib.dgr_thread_options_swap(-1) == saved_word


def test_early_status_without_a_forward_reports_nothing_posted():
    import ctypes
    lib = _capi.load()
    buf = (ctypes.c_int * 4)(7, 7, 7, 7)
    assert lib.dgr_early_status_arm() == 0
    assert lib.dgr_early_status_wait(buf) == 1 and list(buf) == [0, 0, 0, 0]


def test_batch_entry_points_reject_bad_view_counts_before_touching_the_gpu():
    lib = _capi.load()
    views = (_capi.LightView * 1)()
    args = (0, 3, 16, None, 64, 48, None, None, None, None, None, 1.0, None, None, 0.6, 0.45, 0)
    assert lib.dgr_light_forward_batch(None, 0, views, *args) == _capi.DGR_ERR_BAD_ARGUMENT
    assert lib.dgr_light_forward_batch(None, _capi.MAX_BATCH_VIEWS + 1, views, *args) == _capi.DGR_ERR_BAD_ARGUMENT
    assert b"views per batch" in lib.dgr_last_error()
    grads = (_capi.LightViewGrad * 1)()
    assert lib.dgr_light_backward_batch(None, 0, grads, 0, 3, 16, None, 64, 48, None, None, None, None, 1.0, None, None, 0.6,
                                        0.45, None, None, None, None, None, None, None, 0, 0) == _capi.DGR_ERR_BAD_ARGUMENT
    # the ctypes structs mirror the C layout: 17 / 19 eight-byte slots (an int is padded to pointer alignment; round 9 added
    # dgr_light_view_grad.num_rendered behind scratch_bytes)
    assert ctypes.sizeof(_capi.LightView) == 17 * 8 and ctypes.sizeof(_capi.LightViewGrad) == 19 * 8
    assert lib.dgr_get_option(b"batch_streams") == 2
    assert lib.dgr_set_option(b"batch_streams", 1) == 0 and lib.dgr_get_option(b"batch_streams") == 1
    assert lib.dgr_set_option(b"batch_streams", 2) == 0
    assert lib.dgr_get_option(b"batch_order") == 0
    assert lib.dgr_set_option(b"batch_order", 1) == 0 and lib.dgr_get_option(b"batch_order") == 1
    assert lib.dgr_set_option(b"batch_order", 0) == 0


def test_thread_options_override_the_process_wide_ones_per_thread():
    """include/dgr_hip.h: dgr_set_thread_option / dgr_thread_options_swap -- host-side state only, no GPU needed."""
    import threading
    lib = _capi.load()
    assert lib.dgr_get_option(b"alpha_mode") == 0 and lib.dgr_get_thread_option(b"alpha_mode") == 0
    seen = {}

    def other():
        seen["before"] = lib.dgr_get_thread_option(b"alpha_mode")
        with _capi.thread_options(alpha_mode=2, deterministic_grads=1):
            seen["inside"] = (lib.dgr_get_thread_option(b"alpha_mode"), lib.dgr_get_thread_option(b"deterministic_grads"))
        seen["after"] = lib.dgr_get_thread_option(b"alpha_mode")

    with _capi.thread_options(alpha_mode=1, tight_cull=1):
        assert lib.dgr_get_thread_option(b"alpha_mode") == 1 and lib.dgr_get_thread_option(b"tight_cull") == 1
        assert lib.dgr_get_thread_option(b"fast_alpha") == 1
        assert lib.dgr_get_option(b"alpha_mode") == 0 and lib.dgr_get_option(b"tight_cull") == 0   # process-wide: untouched
        t = threading.Thread(target=other)
        t.start()
        t.join()
        word = lib.dgr_thread_options_effective()
        assert (word & 15) - 1 == 1 and ((word >> 4) & 15) - 1 == 1 and ((word >> 8) & 15) - 1 == 0
        with _capi.thread_options(alpha_mode=0):                      # nests
            assert lib.dgr_get_thread_option(b"alpha_mode") == 0 and lib.dgr_get_thread_option(b"tight_cull") == 1
        assert lib.dgr_get_thread_option(b"alpha_mode") == 1
    assert seen == {"before": 0, "inside": (2, 1), "after": 0}         # the other thread never saw this thread's values
    assert lib.dgr_get_thread_option(b"alpha_mode") == 0 and lib.dgr_get_thread_option(b"tight_cull") == 0
    # a forward's snapshot installed around a backward on another thread, then removed
    prev = lib.dgr_thread_options_swap(word)
    assert lib.dgr_get_thread_option(b"alpha_mode") == 1 and lib.dgr_get_thread_option(b"tight_cull") == 1
    lib.dgr_thread_options_swap(prev)
    assert lib.dgr_get_thread_option(b"alpha_mode") == 0
    assert lib.dgr_set_thread_option(b"lds_count", 1) != 0            # not a per-call option
    with pytest.raises(ValueError):
        with _capi.thread_options(alpha_mode=7):
            pass
    assert lib.dgr_get_thread_option(b"alpha_mode") == 0


def test_tile_sort_self_test_refuses_lengths_its_routines_are_not_called_with():
    """dgr_debug_tile_sort checks mode, pointers and every list's length on the host before anything touches the GPU: the ids form
    of the wave sort is only valid in the ranges sort_tile_in_wave gives it, and the LDS array holds 6144 keys."""
    import ctypes as C
    from abi_checks import FAKE, refused
    lib = _capi.load()
    off = lambda *v: (C.c_int * len(v))(*v)   # noqa: E731
    who = "dgr_debug_tile_sort"
    assert lib.dgr_debug_tile_sort(None, 0, 0, None, None, None, None) == 0
    refused(lib.dgr_debug_tile_sort(None, 5, 1, FAKE, off(0, 1), FAKE, FAKE), who, "bad argument")
    refused(lib.dgr_debug_tile_sort(None, -1, 1, FAKE, off(0, 1), FAKE, FAKE), who, "bad argument")
    refused(lib.dgr_debug_tile_sort(None, 0, 1, FAKE, off(0, 1), None, FAKE), who, "bad argument")    # WAVE writes ids
    refused(lib.dgr_debug_tile_sort(None, 1, 1, FAKE, off(0, 1), FAKE, None), who, "bad argument")    # PART writes keys
    refused(lib.dgr_debug_tile_sort(None, 0, 1, None, off(0, 1), FAKE, FAKE), who, "bad argument")
    for mode, n in ((0, 1025), (0, 0), (1, 513), (2, 1024), (2, 6145), (3, 0), (4, -1)):
        refused(lib.dgr_debug_tile_sort(None, mode, 2, FAKE, off(0, 1 if mode != 2 else 1025, (1 if mode != 2 else 1025) + n), FAKE, FAKE),
                who, "list 1 has")
