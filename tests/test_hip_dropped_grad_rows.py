"""The one-view autograd surfaces ask the library for dL_dcolors and dL_dcov3D only when the caller has a leaf for them.

A caller that passes SH coefficients and scale / rotation has no `colors_precomp` or `cov3Ds_precomp` input for autograd to hand a
gradient to: the compiled node (csrc/torch_ext.cpp: Node::backward) then carves no arena segment for the two and passes NULL, and
the per-Gaussian backward -- every dense output of which may be NULL -- does not write their 36 bytes per Gaussian; the Python
Functions (dgr_amd/_frontend.py: _run_backward; the ctypes binding) hand autograd None for the two.  With such a leaf its gradient
is delivered as before.  The mirrors of the reference binding (`_C.rasterize_gaussians_backward`) return all eight tensors as before, and the six
segments `dgr_amd.multiview.GradientArena` reduces in one collective stay one contiguous span.

Both variants, both bindings, 1000 Gaussians at 64 x 64; gradients against the oracle with the bars of __graft_entry__.smoke
(light) and tests/test_hip_full_parity.py (full)."""
import functools

import numpy as np
import pytest
import torch

import hip_helpers as hh
from dgr_amd import full as F
from dgr_amd import light as L
from dgr_amd.multiview import GradientArena, make_settings
from hip_helpers import binding  # noqa: F401  (fixture)
from util import assert_grad_close, make_scene

pytestmark = pytest.mark.gpu

P, W, H, SEED, DEG = 1000, 64, 64, 5, 3
VARIANTS = ("light", "full")
BARS = {"light": dict(rel_to_max=1e-5, elem_rtol=1e-3, elem_frac=1e-3), "full": dict(rel_to_max=1e-5, elem_rtol=2e-3, elem_frac=2e-3)}
VIEW_BARS = {"light": dict(rel_to_max=1e-5, elem_rtol=1e-3, elem_frac=0.0), "full": dict(rel_to_max=5e-5, elem_rtol=5e-3, elem_frac=0.1)}
# node inputs: means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix
COLORS_SLOT, COV3D_SLOT = 3, 7


@functools.lru_cache(maxsize=None)
def the_scene():
    return make_scene(P, W, H, SEED)


def pixel_grads(s, variant):
    g = (s.gC, s.gD, s.gM, s.gV) if variant == "light" else (s.gC, s.gD, s.gV)
    return tuple(x * (W * H) ** 0.5 for x in g)


@pytest.fixture(scope="module")
def precomputed(oracle):
    """the colours and 3D covariances the oracle's own forward forms from the scene's SH rows, scales and rotations"""
    s = the_scene()
    st, _ = hh.oracle_forward(oracle, s, DEG)
    return st.get("rgb").reshape(-1, 3).copy(), st.get("cov3D").reshape(-1, 6).copy()


def oracle_grads(oracle, variant, colors=None, cov3D=None):
    s = the_scene()
    grads = pixel_grads(s, variant)
    if variant == "full":
        return hh.oracle_full(oracle, s, DEG, colors_precomp=colors, cov3D_precomp=cov3D, grads=grads)[2]
    st, ref = hh.oracle_forward(oracle, s, DEG, colors_precomp=colors, cov3D_precomp=cov3D)
    return hh.oracle_backward(oracle, st, s, DEG, ref["opacity_map"], colors_precomp=colors, cov3D_precomp=cov3D, grads=grads)


def render_and_backward(variant, colors=None, cov3D=None, watch=True):
    """One view through the variant's GaussianRasterizer and a backward of all its gradient images.  Returns the leaves by the
    oracle's gradient name and, per node input, whether the node handed autograd no gradient for it (`watch`: a hook on the
    node; it keeps no tensor, so `.grad` still aliases the arena)."""
    s, T, dev = the_scene(), hh.T, hh.dev()
    leaf = lambda a: T(a).requires_grad_()  # noqa: E731
    leaves = dict(dL_dmeans3D=leaf(s.means), dL_dopacity=leaf(s.opac), dL_dview=leaf(s.view),
                  dL_dmeans2D=torch.zeros((P, 3), device=dev, requires_grad=True))
    kw = {}
    if colors is None:
        leaves["dL_dsh"] = kw["shs"] = leaf(s.shs)
    else:
        leaves["dL_dcolors"] = kw["colors_precomp"] = leaf(colors)
    if cov3D is None:
        leaves["dL_dscales"], leaves["dL_drotations"] = kw["scales"], kw["rotations"] = leaf(s.scales), leaf(s.rots)
    else:
        leaves["dL_dcov3D"] = kw["cov3D_precomp"] = leaf(cov3D)
    if variant == "light":
        rast = L.GaussianRasterizer(make_settings(s, DEG, dev))
    else:
        rast = F.GaussianRasterizer(F.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=T(s.bg), scale_modifier=1.0, viewmatrix=T(s.view),
            projmatrix=T(s.proj), sh_degree=DEG, campos=T(s.campos), prefiltered=False, perspec_matrix=T(s.persp)))
    outs = rast(means3D=leaves["dL_dmeans3D"], means2D=leaves["dL_dmeans2D"], opacities=leaves["dL_dopacity"],
                viewmatrix=leaves["dL_dview"], gt_depth=T(s.gt), **kw)
    none_slots = []
    if watch:
        outs[0].grad_fn.register_hook(lambda grad_inputs, grad_outputs: none_slots.extend(g is None for g in grad_inputs))
    gC, gD, *rest = (T(g if g.ndim == 3 else g[None]) for g in pixel_grads(s, variant))
    if variant == "light":
        color, radii, depth, median, var = outs[:5]
        torch.autograd.backward([color, depth, median, var], [gC, gD, *rest])
    else:
        color, radii, depth, unc = outs
        torch.autograd.backward([color, depth, unc], [gC, gD, *rest])
    torch.cuda.synchronize()
    return leaves, none_slots


def assert_leaves_match(leaves, want, variant):
    for name, x in leaves.items():
        assert x.grad is not None, name
        got, ref = x.grad.detach().cpu().numpy(), np.asarray(want[name])
        assert got.size == ref.size, name
        assert_grad_close(got, ref.reshape(got.shape), name, **(VIEW_BARS if name == "dL_dview" else BARS)[variant])


@pytest.mark.parametrize("variant", VARIANTS)
def test_without_precomputed_leaves_the_two_rows_are_not_asked_for(oracle, binding, variant):
    leaves, none_slots = render_and_backward(variant)
    assert len(none_slots) > COV3D_SLOT
    assert none_slots[COLORS_SLOT] and none_slots[COV3D_SLOT]
    assert not any(none_slots[i] for i in (0, 1, 2, 4, 5, 6, 8))  # means3D, means2D, sh, opacities, scales, rotations, viewmatrix
    assert_leaves_match(leaves, oracle_grads(oracle, variant), variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_colors_precomp_leaf_gets_its_gradient(oracle, precomputed, binding, variant):
    colors, _ = precomputed
    leaves, none_slots = render_and_backward(variant, colors=colors)
    assert not none_slots[COLORS_SLOT] and none_slots[COV3D_SLOT]
    assert float(leaves["dL_dcolors"].grad.abs().max()) > 0
    assert_leaves_match(leaves, oracle_grads(oracle, variant, colors=colors), variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_cov3D_precomp_leaf_gets_its_gradient(oracle, precomputed, binding, variant):
    _, cov3D = precomputed
    leaves, none_slots = render_and_backward(variant, cov3D=cov3D)
    assert none_slots[COLORS_SLOT] and not none_slots[COV3D_SLOT]
    assert float(leaves["dL_dcov3D"].grad.abs().max()) > 0
    assert_leaves_match(leaves, oracle_grads(oracle, variant, cov3D=cov3D), variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_reference_bindings_mirror_still_returns_eight_tensors(binding, variant):
    s = the_scene()
    if variant == "light":
        out, _ = hh.hip_forward(s, DEG)
        g = hh.hip_backward_raw(s, DEG, out)
    else:
        out, _ = hh.hip_full_forward(s, DEG)
        g = hh.hip_full_backward_raw(s, DEG, out)
    shapes = [(P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, 16, 3), (P, 3), (P, 4)]
    assert len(g) == 9
    for x, shape in zip(g[:8], shapes):
        assert isinstance(x, torch.Tensor) and tuple(x.shape) == shape and bool(torch.isfinite(x).all())
    assert float(g[1].abs().max()) > 0 and float(g[4].abs().max()) > 0  # dL_dcolors and dL_dcov3D are written


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_all_reduce_span_stays_one_piece(binding, variant):
    leaves, _ = render_and_backward(variant, watch=False)
    params = [leaves[k] for k in ("dL_dmeans3D", "dL_dmeans2D", "dL_dsh", "dL_dopacity", "dL_dscales", "dL_drotations")]
    span = GradientArena(params).fused_span()
    assert span is not None
    assert span.data_ptr() == leaves["dL_dmeans3D"].grad.data_ptr()  # the arena's first segment
    pad = lambda n: (n + 63) // 64 * 64  # noqa: E731  (segments are 256-byte aligned)
    assert span.numel() == sum(pad(p.numel()) for p in params[:-1]) + params[-1].numel()
