"""dgr_set_option("deterministic_grads", 1): the light backward without order-dependent float atomics (csrc/render_light.hip: DET).

The default backward -- like the reference's (L/cuda_rasterizer/backward.cu:593-596, 666-680) -- sums a Gaussian's per-tile totals
with float atomics in arrival order: two runs differ in the last bits (~1e-7 of a row, which computeCov2DCUDA's backward amplifies
to 4e-3 on single ill-conditioned rows), and a parity bar near that noise is set by luck.  With the option on
  * two runs of the same backward give the same BITS in every gradient tensor, including the pose gradient;
  * the sums are taken in a fixed order (waves of a tile, tiles of a Gaussian ascending, blocks ascending), so the distance to the
    oracle -- which sums in double and rounds once -- is arithmetic, not arrival order: the 1e-5-of-scale bars of the default path
    tighten to 2e-6 at configs 1-3;
  * round 9: the full variant's backward and the batched light backward take the option too (they refused it before): the same
    scheme per view, the batch's per-Gaussian sums over the views formed in view order in registers."""
import numpy as np
import pytest
import torch

from util import make_scene
import hip_helpers as hh
from hip_helpers import deterministic  # noqa: F401  (fixtures)
from test_hip_light_parity import GRAD_NAMES, check_backward

pytestmark = pytest.mark.gpu

CONFIGS = [(10000, 256, 256, 0, 0), (100000, 640, 480, 3, 0), (500000, 1920, 1080, 3, 0)]  # BASELINE configs 1-3 (sizes)


def backward_twice(s, deg, **kw):
    grads = tuple(g * (s.W * s.H) ** 0.5 for g in (s.gC, s.gD, s.gM, s.gV))
    out, d = hh.hip_forward(s, deg)
    a = hh.hip_backward(s, deg, out, grads=grads, **kw)
    torch.cuda.synchronize()
    b = hh.hip_backward(s, deg, out, grads=grads, **kw)
    return a, b


@pytest.mark.parametrize("case", CONFIGS + [(3835, 16, 5, 3, 5)])
@pytest.mark.parametrize("mode", [dict(), dict(map_off=True), dict(track_off=True)])
def test_two_runs_give_the_same_bits(deterministic, case, mode):
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    a, b = backward_twice(s, deg, **mode)
    for k in list(GRAD_NAMES) + ["dL_dview"]:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (k, int((a[k] != b[k]).sum()))
    if not mode.get("map_off"):
        assert np.abs(a["dL_dmeans3D"]).max() > 0
    if not mode.get("track_off"):
        assert np.abs(a["dL_dview"]).max() > 0


def test_the_default_backward_is_not_bit_reproducible_which_is_what_the_option_is_for():
    """Informational (never fails on equality): how far two default runs are apart at config 2's size."""
    s = make_scene(100000, 640, 480, 0)
    a, b = backward_twice(s, 3)
    worst = {k: float(np.abs(a[k].astype(np.float64) - b[k]).max() / max(np.abs(a[k]).max(), 1e-30)) for k in list(GRAD_NAMES) + ["dL_dview"]}
    print("\n[default backward, two runs, max |difference| / max |value|]", {k: "%.1e" % v for k, v in worst.items()})
    assert max(worst.values()) < 1e-4


@pytest.mark.parametrize("case", CONFIGS)
def test_the_oracle_bar_tightens(deterministic, oracle, case):
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    check_backward(oracle, s, deg, rel_to_max=2e-6, view_rel_to_max=2e-6, what=f"deterministic P={P}")


def test_one_tile_frame_at_the_tight_bar(deterministic, oracle):
    """3 835 Gaussians on 16 x 5 pixels -- one tile, every Gaussian's total a single row: the frame whose default-path error
    (1.02e-5, arrival order of one row's float atomics) moved tests/test_hip_random_sweep.py's bar to 2e-5.  Deterministic: 2.1e-6
    (float sums of up to 80 pixels in the butterfly's order against the oracle's double sums), the same on every run."""
    s = make_scene(3835, 16, 5, 5)
    check_backward(oracle, s, 3, rel_to_max=4e-6, view_rel_to_max=4e-6, what="deterministic one-tile frame")


def test_heavy_tailed_scene(deterministic, oracle):
    """Splats of hundreds to thousands of tiles: their rows in the instance-major buffer are summed by one 16-lane group each."""
    from dgr_amd.synth import heavy_tail_scene
    s = heavy_tail_scene(make_scene(100000, 1920, 1080, 0))
    a, b = backward_twice(s, 3)
    for k in list(GRAD_NAMES) + ["dL_dview"]:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    check_backward(oracle, s, 3, what="deterministic heavy tail")


@pytest.mark.parametrize("sync_mode", ["strict", "lazy"])
def test_through_the_autograd_surface(deterministic, monkeypatch, sync_mode):
    """GaussianRasterizer -> loss.backward(), twice: the same bits in every leaf's .grad.  In lazy mode the backward is handed the
    binning CAPACITY as R (the host never learnt num_rendered): the row buffer is sized by it.  (Here with a constant count;
    tests/test_hip_lazy_safety.py grows the count under a lazy forward on every call path.)"""
    from dgr_amd import light
    from dgr_amd.multiview import make_settings
    monkeypatch.setenv("DGR_SYNC_MODE", sync_mode)
    dev = hh.dev()
    s = make_scene(20000, 320, 200, 3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rast = light.GaussianRasterizer(make_settings(s, 3, dev))
    gC, gD, gM = (t(g) * (s.W * s.H) ** 0.5 for g in (s.gC, s.gD[None], s.gM[None]))
    res = []
    for _ in range(3):
        L = dict(means3D=t(s.means), shs=t(s.shs), opac=t(s.opac), scales=t(s.scales), rots=t(s.rots), view=t(s.view))
        for v in L.values():
            v.requires_grad_(True)
        m2 = torch.zeros((s.P, 3), device=dev, requires_grad=True)
        color, radii, depth, median, var, alpha, unc, px = rast(means3D=L["means3D"], means2D=m2, opacities=L["opac"], shs=L["shs"],
                                                                scales=L["scales"], rotations=L["rots"], viewmatrix=L["view"], gt_depth=t(s.gt))
        torch.autograd.backward([color, depth, median], [gC, gD, gM])
        torch.cuda.synchronize()
        res.append({k: v.grad.cpu().numpy() for k, v in L.items()} | {"means2D": m2.grad.cpu().numpy()})
    light.check_async_errors()
    for k in res[0]:
        assert np.abs(res[0][k]).max() > 0, k
        assert np.array_equal(res[1][k].view(np.uint32), res[2][k].view(np.uint32)), k  # (run 0 sized the lazy capacity)


@pytest.mark.parametrize("case", [(2000, 64, 48, 0, 1), (10000, 256, 256, 3, 0), (100000, 640, 480, 3, 0)])
def test_full_variant_two_runs_give_the_same_bits_and_agree_with_the_oracle(deterministic, oracle, case):
    """BASELINE config 2 is this variant: F/cuda_rasterizer/backward.cu:540-836 sums with float atomics like the light one."""
    P, W, H, deg, seed = case
    s = make_scene(P, W, H, seed)
    grads = tuple(g * (W * H) ** 0.5 for g in (s.gC, s.gD, s.gV))
    out, d = hh.hip_full_forward(s, deg)
    a = hh.hip_full_backward(s, deg, out, grads=grads)
    torch.cuda.synchronize()
    b = hh.hip_full_backward(s, deg, out, grads=grads)
    names = ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dview")
    for k in names:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (k, int((a[k] != b[k]).sum()))
    assert np.abs(a["dL_dmeans3D"]).max() > 0 and np.abs(a["dL_dview"]).max() > 0
    from util import assert_grad_close
    _, _, gr = hh.oracle_full(oracle, s, deg, grads=grads)
    for k in names[:-1]:
        assert_grad_close(a[k], gr[k], k, rel_to_max=4e-6, elem_rtol=2e-3, elem_frac=1e-3)


@pytest.mark.parametrize("case", [(2000, 70, 45, 3, 1, 3), (20000, 320, 200, 3, 0, 4)])
@pytest.mark.parametrize("mode", [dict(), dict(map_off=True)])
def test_batched_backward_two_runs_give_the_same_bits_and_match_the_one_view_calls(deterministic, case, mode):
    import test_hip_batch as tb
    P, W, H, deg, seed, V = case
    ss = tb.scenes(P, W, H, V, seed)
    outb, cams = tb.batch_forward(ss, deg)
    grads = [tuple(g * (W * H) ** 0.5 for g in (x.gC, x.gD, x.gM, x.gV)) for x in ss]
    a = tb.batch_backward(ss, deg, outb, cams, grads, **mode)
    torch.cuda.synchronize()
    b = tb.batch_backward(ss, deg, outb, cams, grads, **mode)
    for k, v in a.items():
        if v is not None:
            assert np.array_equal(v.view(np.uint32), b[k].view(np.uint32)), (k, int((v != b[k]).sum()))
    assert np.abs(a["dL_dview"]).max() > 0
    # every view's pose gradient and screen-space gradients are those of a deterministic one-view backward of that view, bit for bit
    for v in range(V):
        one = hh.hip_backward(ss[v], deg, tb.one_view_dict(outb, v), grads=grads[v], **mode)
        assert np.array_equal(one["dL_dview"].view(np.uint32), a["dL_dview"][v].view(np.uint32)), v
        if not mode.get("map_off"):
            assert np.array_equal(one["dL_dmeans2D"].view(np.uint32), a["dL_dmeans2D"][v].view(np.uint32)), v
