"""`slam.masked_l1_loss` (csrc/masked_loss.hip) on the GPU against the CPU model of tests/masked_loss_model.py.

The definition is made of single fp32 operations, so masks, counts and the BITS of the medians must equal the model's, with no
tolerance and no excluded pixel.  The loss is compared with the model's float64 sum: exactly on the dyadic family (every sum is
exact there in any order), otherwise within (n + 2) 2^-24 loss64 -- the bound for adding n non-negative fp32 terms in any order
(each of the n - 1 additions and the final scaling and rounding contributes at most one relative 2^-24)."""
import pytest
import torch

from dgr_amd import slam

import masked_loss_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(x, grad=True):
    y = {k: (v.to(DEV) if v is not None else None) for k, v in x.items()}
    if grad:
        y["color"].requires_grad_()
        y["depth"].requires_grad_()
    return y


def _run(x, **kw):
    """(loss, stats, dcolor, ddepth) of one forward + backward on fresh GPU copies of the inputs x (a model-style dict)."""
    g = _gpu(x)
    loss, stats = slam.masked_l1_loss(g["color"], g["depth"], g["color_obs"], g["depth_obs"], g.get("opacity_map"), g.get("mask"),
                                      return_stats=True, **kw)
    loss.backward()
    return loss.detach(), stats, g["color"].grad, g["depth"].grad


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_stats(stats, m, what):
    assert stats.mask.dtype == torch.bool and stats.median.dtype == torch.float32 and stats.base.dtype == torch.int32
    assert stats.mask.shape == m["mask"].shape and stats.median.shape == m["median"].shape
    assert torch.equal(stats.base.cpu(), m["base"]), (what, stats.base.tolist(), m["base"].tolist())
    assert torch.equal(_bits(stats.median), _bits(m["median"])), (what, stats.median.tolist(), m["median"].tolist())
    assert torch.equal(stats.kept.cpu(), m["kept"]), (what, stats.kept.tolist(), m["kept"].tolist())
    assert torch.equal(stats.mask.cpu(), m["mask"]), (what, int((stats.mask.cpu() != m["mask"]).sum()))


def _same_loss_and_grads(loss, dc, dd, m, what, exact=False):
    loss64 = float(m["loss"])
    if exact:
        assert float(loss) == loss64, (what, float(loss), loss64)
        assert torch.equal(dc.cpu().double(), m["dcolor"]) and torch.equal(dd.cpu().double(), m["ddepth"]), what
    else:
        bound = (m["n_terms"] + 2) * 2.0 ** -24 * abs(loss64)
        print(f"{what}: loss {float(loss)!r} model {loss64!r} error {abs(float(loss) - loss64):.3e} bound {bound:.3e}")
        assert abs(float(loss) - loss64) <= bound, (what, float(loss), loss64, bound)
        for got, want in ((dc, m["dcolor"]), (dd, m["ddepth"])):
            got = got.cpu().double()
            assert torch.equal(got == 0, want == 0), what  # zero outside the set, exactly
            assert torch.allclose(got, want, rtol=1e-6, atol=0), what


@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", M.FAMILIES)
def test_stats_equal_the_model_and_the_loss_follows(family, shape):
    x = M.inputs(family, shape)
    x = {k: x[k] for k in ("color", "depth", "color_obs", "depth_obs", "opacity_map")}
    # "sum" with both weights 1: on the dyadic family the loss is exact in fp32 whatever the order of summation
    kw = dict(w_color=1.0, w_depth=1.0)
    m = M.model(**x, **kw)
    loss, stats, dc, dd = _run(x, **kw)
    _same_stats(stats, m, (family, shape))
    _same_loss_and_grads(loss, dc, dd, m, (family, shape, "sum"), exact=family == "dyadic")
    if family == "dyadic":
        assert set(dd.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(dc.unique().tolist()) <= {-1.0, 0.0, 1.0}
    if shape == (3, 3, 33, 65):
        assert m["base"].tolist()[1] == 0 and stats.median.tolist()[1] == 0.0 and not bool(stats.mask[1].any())
    kw = dict(w_color=0.7, w_depth=1.3, reduction="mean")
    m = M.model(**x, **kw)
    loss, stats, dc, dd = _run(x, **kw)
    _same_stats(stats, m, (family, shape, "mean"))
    _same_loss_and_grads(loss, dc, dd, m, (family, shape, "mean"))


VARIANTS = {
    "no-rejection": dict(outlier_factor=None),
    "mapping-form": dict(mask_color=False),
    "mapping-form-mean": dict(mask_color=False, reduction="mean", outlier_factor=None),
    "no-opacity_map": dict(opacity_map=None),
    "user-mask": dict(mask=True),
    "user-mask-bool-no-opacity": dict(mask="bool", opacity_map=None),
    "depth-range": dict(depth_range=(1.0, 3.0)),
    "threshold": dict(silhouette_threshold=0.5, outlier_factor=1.0),
}


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("family", M.FAMILIES)
def test_variants_match_the_model_run_with_the_same_arguments(family, name):
    kw = dict(VARIANTS[name])
    x = dict(M.inputs(family, (1, 3, 37, 53)))
    want_mask = kw.pop("mask", None)
    if "opacity_map" in kw:
        x["opacity_map"] = kw.pop("opacity_map")
    if want_mask is None:
        x["mask"] = None
    elif want_mask == "bool":
        x["mask"] = x["mask"].bool()
    m = M.model(**x, **kw)
    loss, stats, dc, dd = _run(x, **kw)
    _same_stats(stats, m, (family, name))
    _same_loss_and_grads(loss, dc, dd, m, (family, name))
    if kw.get("outlier_factor", 10.0) is None:
        assert torch.equal(stats.base, stats.kept)


def test_a_perfect_fit_keeps_its_base_set_at_factor_zero():
    x = dict(M.inputs("random", (1, 3, 37, 53)))
    x["depth"] = x["depth_obs"].clone()
    x["mask"] = None
    m = M.model(**x, outlier_factor=0.0)
    loss, stats, dc, dd = _run(x, outlier_factor=0.0)
    _same_stats(stats, m, "perfect fit")
    assert stats.median.tolist() == [0.0] and torch.equal(stats.kept, stats.base) and int(stats.base[0]) > 0
    assert not bool(dd.any())
    _same_loss_and_grads(loss, dc, dd, m, "perfect fit")


def test_shapes_without_a_view_dimension():
    x = M.inputs("random", (1, 3, 37, 53))
    ref = _run({k: x[k] for k in ("color", "depth", "color_obs", "depth_obs", "opacity_map", "mask")})
    for dshape in ((1, 37, 53), (37, 53)):
        y = dict(color=x["color"][0], color_obs=x["color_obs"][0], depth=x["depth"].view(dshape), depth_obs=x["depth_obs"].view(dshape),
                 opacity_map=x["opacity_map"].view(dshape), mask=x["mask"].view(dshape))
        loss, stats, dc, dd = _run(y)
        assert dc.shape == (3, 37, 53) and dd.shape == dshape and stats.mask.shape == (1, 37, 53)
        assert torch.equal(loss, ref[0]) and torch.equal(stats.mask, ref[1].mask) and torch.equal(dc, ref[2][0])
        assert torch.equal(dd.view(-1), ref[3].view(-1))


def test_two_runs_give_identical_bits():
    for family, shape in (("random", (3, 3, 33, 65)), ("random", (1, 3, 480, 640))):
        x = M.inputs(family, shape)
        a, b = _run(x, reduction="mean"), _run(x, reduction="mean")
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[2]), _bits(b[2])) and torch.equal(_bits(a[3]), _bits(b[3]))
        for s, t in zip(a[1], b[1]):
            assert torch.equal(s, t) if s.dtype != torch.float32 else torch.equal(_bits(s), _bits(t))


def test_no_grad_gives_the_same_stats():
    x = M.inputs("random", (3, 3, 33, 65))
    loss, stats, _, _ = _run(x)
    g = _gpu(x)
    with torch.no_grad():
        loss0, stats0 = slam.masked_l1_loss(g["color"], g["depth"], g["color_obs"], g["depth_obs"], g["opacity_map"], g["mask"],
                                            return_stats=True)
    assert not loss0.requires_grad and torch.equal(loss0, loss)
    for s, t in zip(stats, stats0):
        assert torch.equal(_bits(s), _bits(t)) if s.dtype == torch.float32 else torch.equal(s, t)
    plain = slam.masked_l1_loss(g["color"], g["depth"], g["color_obs"], g["depth_obs"], g["opacity_map"], g["mask"])
    assert plain.requires_grad and torch.equal(plain.detach(), loss)


def test_replayed_from_a_hipgraph():
    shape = (3, 3, 33, 65)
    old, new = _gpu(M.inputs("dyadic", shape)), M.inputs("random", shape)

    def step():
        old["color"].grad = old["depth"].grad = None
        loss, stats = slam.masked_l1_loss(old["color"], old["depth"], old["color_obs"], old["depth_obs"], old["opacity_map"], old["mask"],
                                          reduction="mean", return_stats=True)
        loss.backward()
        return (loss.detach(), old["color"].grad, old["depth"].grad) + tuple(stats)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    with torch.no_grad():
        for k, v in new.items():
            old[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    loss, stats, dc, dd = _run(new, reduction="mean")
    for a, b in zip(replayed, (loss, dc, dd) + tuple(stats)):
        assert torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)


def test_gradient_through_the_rasterizer_matches_the_torch_composition():
    """64 x 48 synthetic scene: one masked_l1_loss backward through slam.render against the same loss built from torch ops (the
    mask and the median by torch.median on the GPU).  rtol 1e-5 of the gradient's maximum: both backwards feed the rasterizer the
    same images up to the loss scale's rounding, and the reduction order into the Gaussians is the rasterizer's."""
    import numpy as np
    from dgr_amd.synth import camera, make_scene
    from test_slam_render import Model

    dev = torch.device(DEV)
    W, H = 64, 48
    s = make_scene(3000, W, H, 5)
    tanfovx, tanfovy, Rm, t_true, *_ = camera(W, H, 0.05)
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, :3], w2c[:3, 3] = Rm, t_true
    vm = torch.from_numpy(np.ascontiguousarray(w2c.T)).to(dev)
    bg, gt_depth = torch.from_numpy(s.bg).to(dev), torch.from_numpy(s.gt).to(dev)
    kw = dict(viewmatrix=vm, fov=(tanfovx, tanfovy), HW=(H, W), gt_depth=gt_depth)

    def fresh():
        pc = Model(s, dev)
        pc.get_xyz.requires_grad_()
        return pc

    with torch.no_grad():
        obs = slam.render(None, fresh(), None, bg, **kw)
    g = torch.Generator().manual_seed(7)
    obs_c = (obs["render"] + 0.05 * torch.randn(obs["render"].shape, generator=g).to(dev)).contiguous()
    obs_d = obs["depth"] + 0.02 * torch.randn(obs["depth"].shape, generator=g).to(dev)
    obs_d = torch.where((torch.rand(obs_d.shape, generator=g) < 0.2).to(dev), torch.zeros((), device=dev), obs_d)
    obs_d = torch.where((torch.rand(obs_d.shape, generator=g) < 0.02).to(dev), obs_d + 5.0, obs_d).contiguous()

    pc = fresh()
    out = slam.render(None, pc, None, bg, **kw)
    loss, stats = slam.masked_l1_loss(out["render"], out["depth"], obs_c, obs_d, out["opacity_map"], silhouette_threshold=0.5,
                                      reduction="mean", return_stats=True)
    loss.backward()

    pc2 = fresh()
    out = slam.render(None, pc2, None, bg, **kw)
    with torch.no_grad():
        e = (out["depth"] - obs_d).abs()
        B = (obs_d > 0) & torch.isfinite(e) & (out["opacity_map"] > 0.5)
        K = B & (e <= 10.0 * torch.median(e[B]))
    assert torch.equal(K.view(1, H, W), stats.mask) and 0 < int(stats.kept[0]) < int(stats.base[0]) < H * W
    n = K.sum()
    loss2 = 0.5 * ((out["depth"] - obs_d).abs() * K).sum() / n + ((out["render"] - obs_c).abs() * K).sum() / (3 * n)
    loss2.backward()
    a, b = pc.get_xyz.grad, pc2.get_xyz.grad
    scale = float(b.abs().max())
    assert scale > 0 and abs(float(loss.detach()) - float(loss2.detach())) <= 1e-5 * float(loss2.detach())
    assert float((a - b).abs().max()) <= 1e-5 * scale, (float((a - b).abs().max()), scale)
