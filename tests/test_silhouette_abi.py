"""The exact silhouette gradient (option "silhouette_grad", include/dgr_hip.h: dgr_*_backward*_silhouette) without a GPU: the
four entry points are exported and bound, the option's process / thread values and its field in the options word, and the
closed form the blend backwards use -- dA/dalpha_k = T_final / (1 - alpha_k) for A = sum_k alpha_k T_k -- in float64."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dgr_amd import _capi

from abi_checks import assert_entry_points

NEW = ("dgr_light_backward_silhouette", "dgr_full_backward_silhouette", "dgr_light_backward_batch_silhouette",
       "dgr_full_backward_batch_silhouette")


def test_silhouette_symbols_are_exported_and_bound():
    assert_entry_points(NEW)
    lib = _capi.load()
    for name in NEW:
        fn = getattr(lib, name)
        namesake = name.replace("_silhouette", "_absgrad")
        # the namesake's arguments, then one more: a device image (one view) or a host array of device pointers (batch)
        assert fn.argtypes[:-1] == getattr(lib, namesake).argtypes, name
        want = C.POINTER(C.c_void_p) if "batch" in name else C.c_void_p
        assert fn.argtypes[-1] == want and fn.restype == C.c_int, name


@pytest.fixture
def restore_silhouette():
    lib = _capi.load()
    prev = lib.dgr_get_option(b"silhouette_grad")
    word = lib.dgr_thread_options_swap(-1)
    yield lib
    lib.dgr_set_option(b"silhouette_grad", prev)
    lib.dgr_thread_options_swap(word)


def field(word, shift):
    return (word >> shift) & 15


def test_silhouette_option_process_and_thread(restore_silhouette):
    lib = restore_silhouette
    assert lib.dgr_get_option(b"silhouette_grad") in (0, 1)
    assert lib.dgr_set_option(b"silhouette_grad", 0) == 0 and lib.dgr_get_option(b"silhouette_grad") == 0
    assert lib.dgr_get_thread_option(b"silhouette_grad") == 0
    assert lib.dgr_set_option(b"silhouette_grad", 1) == 0 and lib.dgr_get_option(b"silhouette_grad") == 1
    assert lib.dgr_get_thread_option(b"silhouette_grad") == 1  # (inherited)
    assert lib.dgr_set_thread_option(b"silhouette_grad", 0) == 0
    assert lib.dgr_get_thread_option(b"silhouette_grad") == 0 and lib.dgr_get_option(b"silhouette_grad") == 1
    assert lib.dgr_set_thread_option(b"silhouette_grad", -1) == 0
    assert lib.dgr_get_thread_option(b"silhouette_grad") == 1
    with _capi.thread_options(silhouette_grad=0):
        assert lib.dgr_get_thread_option(b"silhouette_grad") == 0
    assert lib.dgr_get_thread_option(b"silhouette_grad") == 1


def test_silhouette_option_refuses_bad_values(restore_silhouette):
    lib = restore_silhouette
    lib.dgr_set_option(b"silhouette_grad", 0)
    for v in (-1, 2, 7):
        assert lib.dgr_set_option(b"silhouette_grad", v) != 0
        assert "silhouette_grad" in _capi.last_error()
    assert lib.dgr_get_option(b"silhouette_grad") == 0
    for v in (2, 15):
        assert lib.dgr_set_thread_option(b"silhouette_grad", v) != 0
    assert lib.dgr_get_thread_option(b"silhouette_grad") == 0
    with pytest.raises(ValueError):
        with _capi.thread_options(silhouette_grad=3):
            pass


def test_silhouette_field_in_the_options_word(restore_silhouette):
    lib = restore_silhouette
    lib.dgr_set_option(b"silhouette_grad", 0)
    base = lib.dgr_thread_options_effective()
    assert field(base, 16) == 1
    with _capi.thread_options(silhouette_grad=1):
        on = lib.dgr_thread_options_effective()
        assert field(on, 16) == 2 and _capi.silhouette_on(on)
    assert not _capi.silhouette_on(base)
    # the other fields (alpha_mode, tight_cull, deterministic_grads, pose_grad) are unaffected
    for shift in (0, 4, 8, 12):
        assert field(on, shift) == field(base, shift)
    assert on & ~(15 << 16) == base & ~(15 << 16)
    # ... and the field does not follow theirs
    with _capi.thread_options(pose_grad=1, deterministic_grads=1):
        w = lib.dgr_thread_options_effective()
        assert field(w, 16) == 1 and field(w, 12) == 2 and field(w, 8) == 2
    # a swapped-in word sets the thread's override, field 0 inherits
    prev = lib.dgr_thread_options_swap(2 << 16)
    assert lib.dgr_get_thread_option(b"silhouette_grad") == 1
    assert field(lib.dgr_thread_options_effective(), 0) == field(base, 0)
    lib.dgr_thread_options_swap(0)
    assert lib.dgr_get_thread_option(b"silhouette_grad") == 0
    lib.dgr_thread_options_swap(prev)
    # the process-wide value shows in the word of a thread without an override
    lib.dgr_set_option(b"silhouette_grad", 1)
    assert field(lib.dgr_thread_options_effective(), 16) == 2


OPTION_VARS = ("DGR_TILE_SCHEDULE", "DGR_ALPHA_MODE", "DGR_FAST_ALPHA", "DGR_DETERMINISTIC_GRADS", "DGR_POSE_GRAD",
               "DGR_SILHOUETTE_GRAD", "DGR_FWD_HALVES", "DGR_LDS_COUNT", "DGR_BLEND_WGS_PER_CU")


def env_case(variable, option, string, want, also=None, id=None):
    return pytest.param(variable, option, string, want, also or {}, id=id or f"{variable}-{string}")


# (variable, option, string, expected initial value[, other variables set beside it]): the eight variables of the option table
# (csrc/options.hip) with the strings INTEGRATION.md and include/dgr_hip.h offer, DGR_FAST_ALPHA behind DGR_ALPHA_MODE, and per
# variable one malformed string: the whole string must be one accepted digit, anything else leaves the default.
ENV_CASES = [
    env_case("DGR_SILHOUETTE_GRAD", "silhouette_grad", "1", 1, id="1-1"),
    env_case("DGR_SILHOUETTE_GRAD", "silhouette_grad", "0", 0, id="0-0"),
    env_case("DGR_SILHOUETTE_GRAD", "silhouette_grad", "2", 0, id="2-0"),
    env_case("DGR_SILHOUETTE_GRAD", "silhouette_grad", "11", 0, id="11-0"),
    env_case("DGR_TILE_SCHEDULE", "tile_schedule", "0", 0),
    env_case("DGR_TILE_SCHEDULE", "tile_schedule", "1", 1),
    env_case("DGR_TILE_SCHEDULE", "tile_schedule", "2", 2),
    env_case("DGR_TILE_SCHEDULE", "tile_schedule", "12", 2),
    env_case("DGR_ALPHA_MODE", "alpha_mode", "0", 0),
    env_case("DGR_ALPHA_MODE", "alpha_mode", "1", 1),
    env_case("DGR_ALPHA_MODE", "alpha_mode", "2", 2),
    env_case("DGR_ALPHA_MODE", "alpha_mode", "11", 0),
    env_case("DGR_ALPHA_MODE", "alpha_mode", "0", 0, {"DGR_FAST_ALPHA": "1"}, id="DGR_ALPHA_MODE-0-before-DGR_FAST_ALPHA"),
    env_case("DGR_ALPHA_MODE", "alpha_mode", "2", 2, {"DGR_FAST_ALPHA": "1"}, id="DGR_ALPHA_MODE-2-before-DGR_FAST_ALPHA"),
    env_case("DGR_ALPHA_MODE", "alpha_mode", "7", 1, {"DGR_FAST_ALPHA": "1"}, id="DGR_ALPHA_MODE-refused-then-DGR_FAST_ALPHA"),
    env_case("DGR_FAST_ALPHA", "alpha_mode", "1", 1),
    env_case("DGR_FAST_ALPHA", "fast_alpha", "1", 1, id="DGR_FAST_ALPHA-1-by-its-own-name"),
    env_case("DGR_FAST_ALPHA", "alpha_mode", "0", 0),
    env_case("DGR_FAST_ALPHA", "alpha_mode", "11", 0),
    env_case("DGR_DETERMINISTIC_GRADS", "deterministic_grads", "1", 1),
    env_case("DGR_DETERMINISTIC_GRADS", "deterministic_grads", "0", 0),
    env_case("DGR_DETERMINISTIC_GRADS", "deterministic_grads", "10", 0),
    env_case("DGR_POSE_GRAD", "pose_grad", "1", 1),
    env_case("DGR_POSE_GRAD", "pose_grad", "0", 0),
    env_case("DGR_POSE_GRAD", "pose_grad", "11", 0),
    env_case("DGR_FWD_HALVES", "lane_lists", "0", 0),
    env_case("DGR_FWD_HALVES", "lane_lists", "1", 1),
    env_case("DGR_FWD_HALVES", "lane_lists", "2", 2),
    env_case("DGR_FWD_HALVES", "lane_lists", "10", 2),
    env_case("DGR_LDS_COUNT", "lds_count", "0", 0),
    env_case("DGR_LDS_COUNT", "lds_count", "1", 1),
    env_case("DGR_LDS_COUNT", "lds_count", "2", 2),
    env_case("DGR_LDS_COUNT", "lds_count", "05", 1),
    env_case("DGR_BLEND_WGS_PER_CU", "blend_wgs_per_cu", "3", 3),
    env_case("DGR_BLEND_WGS_PER_CU", "blend_wgs_per_cu", "7", 7),
    env_case("DGR_BLEND_WGS_PER_CU", "blend_wgs_per_cu", "2", 0),
    env_case("DGR_BLEND_WGS_PER_CU", "blend_wgs_per_cu", "8", 0),
    env_case("DGR_BLEND_WGS_PER_CU", "blend_wgs_per_cu", "35", 0),
]


@pytest.mark.parametrize("variable,option,value,want,also", ENV_CASES)
def test_silhouette_env_in_a_fresh_process(variable, option, value, want, also):
    code = f"from dgr_amd import _capi; print(_capi.get_option('{option}'))"
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__)))  # (the child imports the package from the tree)
    env = {k: v for k, v in os.environ.items() if k not in OPTION_VARS}         # (only the case's own variables)
    env.update(also)
    env[variable] = value
    env["PYTHONPATH"] = os.pathsep.join([pkg, os.environ.get("PYTHONPATH", "")])
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) == want


def composite(alpha, clamp=True):
    """One pixel's front-to-back blend of K Gaussians in float64: A = sum_k alpha_k T_k, T_final = prod (1 - alpha_k), with the
    kernels' straight-through 0.99 clamp (its value, the unclamped derivative)."""
    a = alpha + (torch.clamp(alpha, max=0.99) - alpha).detach() if clamp else alpha
    T_incl = torch.cumprod(1.0 - a, 0)
    T_excl = torch.cat([torch.ones(1, dtype=torch.float64), T_incl[:-1]])
    return (a * T_excl).sum(), T_incl[-1], a


@pytest.mark.parametrize("seed", range(6))
def test_silhouette_closed_form_fp64(seed):
    rng = np.random.default_rng(seed)
    K = int(rng.integers(1, 24))
    alpha = torch.tensor(rng.uniform(15.0 / 255.0, 0.999, K), dtype=torch.float64, requires_grad=True)
    g_A = float(rng.normal())
    A, T_final, a = composite(alpha)
    (g_A * A).backward()
    want = (T_final / (1.0 - a) * g_A).detach()
    assert torch.allclose(alpha.grad, want, rtol=1e-12, atol=1e-15)
    # A = 1 - T_final: the silhouette term has the shape of the background term, -T_final <bg, g_C> / (1 - alpha)
    assert abs(float(A + T_final) - 1.0) < 1e-12
    bg, g_C = rng.normal(size=3), rng.normal(size=3)
    alpha.grad = None
    A, T_final, a = composite(alpha)
    (float(bg @ g_C) * T_final + g_A * A).backward()
    want = (T_final * (g_A - float(bg @ g_C)) / (1.0 - a)).detach()
    assert torch.allclose(alpha.grad, want, rtol=1e-10, atol=1e-14)
