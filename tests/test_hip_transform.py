"""dgr_amd.optim.transform_map / pose_corrections (csrc/transform.hip) against the float64 model of tests/transform_model.py, inside
the bars derived there: every kind and order, every SH layout, anchors in runs and shuffled, rows and transforms that must stay;
composition; a recorded graph that follows rewritten transforms; the render of a moved map from the moved camera; and the anchor
leaf through the steps that copy it."""
import numpy as np
import pytest
import torch

import hip_helpers as hh
import transform_model as tm
from dgr_amd.optim import (SparseAdam, densify_and_prune, pose_corrections, relocate_dead, seed_from_frame, transform_map)
from dgr_amd.synth import make_scene
from hip_helpers import dev
from map_step_cases import assert_in_place, bits_equal, on_device

pytestmark = pytest.mark.gpu

NAN = float("nan")
KIND = {"xyz": "xyz", "rotation": "quat", "scaling": "log_scale", "f_rest": "sh", "shs": "sh"}


def make_case(P, K, seed, sh="f_rest15", runs=True, weird=True, bad_transforms=True):
    """CPU inputs (numpy): leaves with a pair of moments each, [K, 4, 4] transforms with s cycling over 1, 0.5, 3, the anchors.
    `sh`: "f_rest<M>" (M = 0, 3, 8, 15) or "shs<M + 1>".  `runs`: anchors in runs of 64 or more rows (whole waves share one), else
    shuffled per lane.  `weird`: some rows anchored to -1, K, 2.5 and NaN.  `bad_transforms` (K >= 3): transform 1 is a reflection,
    transform K - 1 has a NaN entry."""
    rng = np.random.RandomState(seed)
    L = {"xyz": 3 * rng.standard_normal((P, 3)), "scaling": 0.7 * rng.standard_normal((P, 3)) - 2, "rotation": rng.standard_normal((P, 4)),
         "opacity": rng.standard_normal((P, 1)), "f_dc": rng.standard_normal((P, 1, 3))}
    name, width = ("shs", int(sh[3:])) if sh.startswith("shs") else ("f_rest", int(sh[6:]))
    L[name] = 0.3 * rng.standard_normal((P, width, 3))
    L["label"] = rng.standard_normal(P)
    if runs:
        anchor = np.repeat(rng.randint(0, K, P // 64 + 1), 64)[:P].astype(np.float64)
    else:
        anchor = rng.randint(0, K, P).astype(np.float64)
    if weird and P > 8:
        rows = rng.choice(P, 8, replace=False) if not runs else np.arange(P - 8, P)
        anchor[rows] = [-1, K, 2.5, NAN, -1, K + 3, 0.5, NAN]
    L["anchor"] = anchor
    L = {n: t.astype(np.float32) for n, t in L.items()}
    M = {n: (rng.standard_normal(t.shape).astype(np.float32), (rng.rand(*t.shape) + 0.5).astype(np.float32)) for n, t in L.items()
         if n != "label"}
    transforms = np.stack([tm.random_sim3(rng, (1.0, 0.5, 3.0)[k % 3]) for k in range(K)])
    if bad_transforms and K >= 3:
        transforms[1, :3, 2] *= -1
        transforms[K - 1, 2, 3] = NAN
    return L, M, transforms


def run_hip(L, M, transforms, optimizer=True, anchor="anchor", **kw):
    params, opt, moments, before = on_device(L, M, optimizer, frozen=("label", "anchor"), grouped=M)
    counts = transform_map(params, opt, torch.from_numpy(transforms).to(dev()), anchor=anchor, **kw)
    torch.cuda.synchronize()
    assert_in_place(before, params, opt)
    out = {n: p.detach().cpu().numpy() for n, p in params.items()}
    mom = {n: tuple(t.cpu().numpy() for t in pair) for n, pair in moments.items()}
    return out, mom, counts.cpu().numpy()


def check_tensor(got, before, kind, order, idx, plans, skip, what, factor=1.0):
    want, bar = tm.transform_model(before, kind, order, idx, plans, skip)
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bar > 0, err / bar, 0.0)
    assert (err <= factor * bar).all(), (what, float(ratio.max()))
    assert bits_equal(got[idx < 0], before[idx < 0]), what  # an untouched row keeps its bits
    return float(ratio.max()) if ratio.size else 0.0


def check_against_model(L, M, transforms, optimizer=True, anchor="anchor", moments="rotate"):
    P = L["xyz"].shape[0]
    plans = [tm.plan_model(T) for T in transforms]
    idx, counts = tm.classify(L["anchor"] if anchor == "anchor" else None, plans, P)
    out, mom, got_counts = run_hip(L, M, transforms, optimizer, anchor, moments=moments)
    assert got_counts.dtype == np.int32 and tuple(got_counts) == counts, (got_counts, counts)
    worst = {}
    for name, t in L.items():
        kind = KIND.get(name)
        skip = 3 if name == "shs" else 0
        if kind == "sh" and t.shape[1] * 3 - skip == 0:
            kind = None
        if kind is None:  # outside the table: every bit stays, the moments' too
            assert bits_equal(out[name], t), name
            if name in mom:
                assert bits_equal(mom[name][0], M[name][0]) and bits_equal(mom[name][1], M[name][1]), name
            continue
        worst[name] = check_tensor(out[name], t, kind, tm.VALUE, idx, plans, skip, name)
        if name in mom:
            if kind == "log_scale" or moments == "keep":
                assert bits_equal(mom[name][0], M[name][0]) and bits_equal(mom[name][1], M[name][1]), name
            else:
                worst[name + ".m1"] = check_tensor(mom[name][0], M[name][0], kind, tm.MOMENT1, idx, plans, skip, name + " exp_avg")
                worst[name + ".m2"] = check_tensor(mom[name][1], M[name][1], kind, tm.MOMENT2, idx, plans, skip, name + " exp_avg_sq")
                assert (mom[name][1] >= 0).all(), name
    print(f"P = {P}, K = {len(plans)}: counts {counts}; worst error / bar: " + ", ".join(f"{n} {v:.2f}" for n, v in worst.items()))
    return idx, counts, out


CASES = [  # P, K, sh layout, anchors in runs, with an optimiser
    (1, 1, "f_rest15", True, True), (1, 3, "shs16", False, False), (255, 1, "f_rest3", True, True), (255, 3, "f_rest8", False, True),
    (255, 70, "f_rest15", False, False), (257, 1, "shs16", True, True), (257, 3, "f_rest0", False, True), (257, 70, "f_rest3", True, False),
    (1000, 1, "f_rest8", False, False), (1000, 3, "f_rest15", True, True), (1000, 70, "shs16", False, True), (1000, 70, "f_rest15", True, True),
    (1000, 3, "shs4", False, True), (257, 3, "shs9", True, True), (255, 3, "shs1", False, True),
]


@pytest.mark.parametrize("P, K, sh, runs, optimizer", CASES, ids=[f"P{c[0]}-K{c[1]}-{c[2]}-{'runs' if c[3] else 'mixed'}" for c in CASES])
def test_matches_the_model(P, K, sh, runs, optimizer):
    L, M, transforms = make_case(P, K, 1000 * K + P, sh, runs)
    idx, counts, _ = check_against_model(L, M, transforms, optimizer)
    if P >= 255:
        assert counts[0] > 0 and counts[1] == 8
        assert counts[2] == (2 if K >= 3 else 0) and (counts[3] > 0) == (K == 3 or (K > 3 and counts[3] > 0))


def test_one_global_transform_and_kept_moments():
    L, M, transforms = make_case(300, 2, 5, weird=False)
    idx, counts, _ = check_against_model(L, M, transforms, anchor=None)
    assert counts == (300, 0, 0, 0) and (idx == 0).all()
    check_against_model(L, M, transforms, moments="keep")


def test_rows_and_transforms_that_must_stay():
    """every row anchored to -1, K, 2.5, NaN, a reflection or a transform with a NaN entry keeps its bits in every tensor; the counts
    are exact"""
    P, K = 320, 4
    L, M, transforms = make_case(P, K, 6, weird=False, bad_transforms=False)
    transforms[1, :3, 0] *= -1
    transforms[3, 0, 1] = NAN
    L["anchor"] = np.tile(np.array([0, 1, 2, 3, -1, K, 2.5, NAN], np.float32), P // 8)
    idx, counts, out = check_against_model(L, M, transforms)
    assert counts == (P // 4, P // 2, 2, P // 4) and sorted(set(idx.tolist())) == [-1, 0, 2]
    # all transforms invalid: nothing moves at all
    transforms[0, 3, 3] = np.inf
    transforms[2] = 0
    idx, counts, out = check_against_model(L, M, transforms)
    assert counts == (0, P // 2, 4, P // 2) and all(bits_equal(out[n], L[n]) for n in L)


def test_two_calls_compose_to_the_call_with_the_product():
    """T_1 then T_2 against the one call with T_2 T_1 (formed in float64, rounded to fp32), within twice the bars.  The bars are the
    model's recipe -- the kind's count of roundings x 2^-24 x the magnitude of the terms summed -- on the terms the two calls sum,
    |W_2| (|W_1| |x| + |t_1|) + |t_2| (tests/transform_model.py: path_bar); those of the one call, on |W_2 W_1| |x| + |t|, are never
    larger, and the two-call result was measured at 2.10 of them (xyz, first moment), which no triangle inequality forbids.
    The quaternion of a product is that of the two up to its sign, which the step does not canonicalise: a rotation row and its
    first moment are compared up to one sign per row.  The second moments do NOT compose value by value -- the diagonal of a rotated
    second moment without its cross terms is (W o W) v, and (W_2 o W_2)(W_1 o W_1) is not (W_2 W_1) o (W_2 W_1) -- but their sum
    over a row's components (a band's, per channel) does, W being orthogonal: that is what is compared for them."""
    P, K = 600, 3
    L, M, T1 = make_case(P, K, 7, weird=False, bad_transforms=False)
    _, _, T2 = make_case(P, K, 8, weird=False, bad_transforms=False)
    product = (T2.astype(np.float64) @ T1.astype(np.float64)).astype(np.float32)
    once, once_m, _ = run_hip(L, M, product)
    half, half_m, _ = run_hip(L, M, T1)
    twice, twice_m, counts = run_hip(half, half_m, T2)
    assert tuple(counts) == (P, 0, 0, 0)
    plans, plans_1, plans_2 = ([tm.plan_model(T) for T in stack] for stack in (product, T1, T2))
    idx, _ = tm.classify(L["anchor"], plans, P)
    sign = np.sign((once["rotation"] * twice["rotation"]).sum(axis=1, keepdims=True)).astype(np.float32)
    assert (np.abs(sign) == 1).all()
    twice["rotation"], twice_m["rotation"] = twice["rotation"] * sign, (twice_m["rotation"][0] * sign, twice_m["rotation"][1])
    for name, kind in KIND.items():
        if name not in L:
            continue
        for order, a, b, before in ((tm.VALUE, twice[name], once[name], L[name]), (tm.MOMENT1, twice_m[name][0], once_m[name][0], M[name][0]),
                                    (tm.MOMENT2, twice_m[name][1], once_m[name][1], M[name][1])):
            if kind == "log_scale" and order != tm.VALUE:
                assert bits_equal(a, before) and bits_equal(b, before)
                continue
            bar = tm.path_bar(before, kind, order, idx, plans_1, plans_2)
            if order == tm.MOMENT2:  # the traces: per row for xyz and the quaternion, per band and channel for the SH rows
                groups = [(slice(0, a.shape[1]), 1)] if kind != "sh" else [(slice(sl.start + ch, sl.stop, 3), 1) for sl, *_ in
                                                                           tm.linear_parts(kind, order, plans[0], 0, 45) for ch in range(3)]
                a, b, bar = (np.stack([t.reshape(P, -1)[:, g].astype(np.float64).sum(axis=1) for g, _ in groups], axis=1) for t in (a, b, bar))
            else:
                assert (bar >= tm.transform_model(before, kind, order, idx, plans)[1] * (1 - 1e-6)).all()
            err = np.abs(a.astype(np.float64) - b.astype(np.float64))
            print(f"composition, {name} order {order}: worst difference / bar = {float((err / bar).max()):.2f} (bound 2)")
            assert (err <= 2.0 * bar).all(), (name, order)


def test_recorded_into_a_graph_it_follows_rewritten_transforms():
    d, P, K = dev(), 700, 5
    L, M, T_a = make_case(P, K, 9)
    _, _, T_b = make_case(P, K, 10)
    static = {n: torch.from_numpy(t).to(d) for n, t in L.items()}
    transforms = torch.from_numpy(T_a).to(d)
    opt = SparseAdam([{"params": [p], "lr": 1e-3} for n, p in static.items() if n in M])
    for n, (m, v) in M.items():
        opt.state[static[n]] = (torch.from_numpy(m).to(d), torch.from_numpy(v).to(d))
    transform_map(static, opt, transforms)  # (the library is loaded before the capture)

    def reset():
        for n, t in L.items():
            static[n].copy_(torch.from_numpy(t))
        for n, (m, v) in M.items():
            opt.state[static[n]][0].copy_(torch.from_numpy(m))
            opt.state[static[n]][1].copy_(torch.from_numpy(v))

    reset()
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=d)
    side.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            counts = transform_map(static, opt, transforms)
    torch.cuda.current_stream(d).wait_stream(side)
    for T in (T_a, T_b):
        reset()
        transforms.copy_(torch.from_numpy(T))
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_m, eager_counts = run_hip(L, M, T)
        assert np.array_equal(counts.cpu().numpy(), eager_counts)
        for n in L:
            assert bits_equal(static[n].cpu().numpy(), eager[n]), n
        for n in M:
            assert all(bits_equal(opt.state[static[n]][i].cpu().numpy(), eager_m[n][i]) for i in (0, 1)), n


def test_a_second_apply_call_with_the_same_scratch_leaves_the_same_counts():
    """the C ABI directly: one plan, the xyz tensor in one apply call and the rotation in a second one"""
    from dgr_amd import _capi
    d, P, K = dev(), 300, 3
    L, _, transforms = make_case(P, K, 14)
    plans = [tm.plan_model(T) for T in transforms]
    idx, want = tm.classify(L["anchor"], plans, P)
    xyz, rot, anchor, T = (torch.from_numpy(a).to(d) for a in (L["xyz"], L["rotation"], L["anchor"], transforms))
    scratch = torch.empty(_capi.load().dgr_transform_scratch_bytes(K), dtype=torch.uint8, device=d)
    counts = torch.full((4,), -7, dtype=torch.int32, device=d)
    seen = []
    with _capi.StepCalls(d) as abi:
        abi.call("dgr_transform_plan", K, T.data_ptr(), scratch.data_ptr(), counts.data_ptr())
        seen.append(counts.tolist())
        for t, k, mode in ((xyz, 3, _capi.TRANSFORM_XYZ), (rot, 4, _capi.TRANSFORM_QUAT)):
            desc = (_capi.TransformTensor * 1)()
            desc[0].data, desc[0].k, desc[0].mode, desc[0].skip = t.data_ptr(), k, mode, 0
            abi.call("dgr_transform_apply", P, K, scratch.data_ptr(), anchor.data_ptr(), 1, desc, counts.data_ptr())
            seen.append(counts.tolist())
    assert seen == [[0, 0, want[2], 0], list(want), list(want)]
    check_tensor(xyz.cpu().numpy(), L["xyz"], "xyz", tm.VALUE, idx, plans, 0, "xyz")
    check_tensor(rot.cpu().numpy(), L["rotation"], "quat", tm.VALUE, idx, plans, 0, "rotation")


def test_refusals():
    L, M, transforms = make_case(64, 2, 11)
    d = dev()
    params = {n: torch.from_numpy(t).to(d) for n, t in L.items()}
    T = torch.from_numpy(transforms).to(d)
    with pytest.raises(RuntimeError, match="transforms"):
        transform_map(params, None, T.reshape(2, 16))
    with pytest.raises(KeyError, match="anchor"):
        transform_map(params, None, T, anchor="keyframe")
    with pytest.raises(RuntimeError, match="anchor"):
        transform_map(params, None, T, anchor=torch.zeros(63, device=d))
    with pytest.raises(ValueError, match="moments"):
        transform_map(params, None, T, moments="zero")
    with pytest.raises(RuntimeError, match="complete bands"):
        transform_map(dict(params, f_rest=torch.zeros((64, 5, 3), device=d)), None, T)
    with pytest.raises(RuntimeError, match="contiguous"):
        transform_map(dict(params, xyz=torch.zeros((3, 64), device=d).t()), None, T)
    for n, t in L.items():
        assert bits_equal(params[n].cpu().numpy(), t), n


def test_pose_corrections_keep_a_point_fixed_in_its_keyframe():
    rng = np.random.RandomState(12)
    W2C_old = np.stack([np.linalg.inv(tm.random_sim3(rng).astype(np.float64)) for _ in range(5)])
    W2C_new = np.stack([np.linalg.inv(tm.random_sim3(rng).astype(np.float64)) for _ in range(5)])
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1)).astype(np.float32)).to(dev())  # noqa: E731
    T = pose_corrections(to_dev(W2C_old), to_dev(W2C_new))
    assert T.shape == (5, 4, 4) and T.dtype == torch.float32 and T.is_contiguous()
    want = np.linalg.inv(W2C_new.astype(np.float32).astype(np.float64)) @ W2C_old.astype(np.float32).astype(np.float64)
    assert np.abs(T.cpu().numpy() - want).max() < 1e-5
    assert all(tm.plan_model(t) is not None for t in T.cpu().numpy())
    assert torch.equal(pose_corrections(to_dev(W2C_old).reshape(5, 16), to_dev(W2C_new)), T)


# ------------------------------------------------------------------------------------------ the render of a moved map
def render(variant, s, leaves, view, proj, campos):
    """colour, depth, silhouette and n_contrib of the leaves (xyz, log scale, rotation, shs [P, 16, 3]) from the camera"""
    s = s._replace(means=leaves["xyz"], scales=torch.exp(leaves["scaling"]), rots=leaves["rotation"], shs=leaves["shs"],
                   view=view, proj=proj, campos=campos)
    if variant == "light":
        out, d = hh.hip_forward(s, 3)
        images = {"color": d["color"], "depth": d["depth"], "silhouette": d["opacity_map"]}
    else:
        out, d = hh.hip_full_forward(s, 3)
        images = {"color": d["color"], "depth": d["depth"], "silhouette": d["uncertainty"]}
    return images, hh.hip_state("n_contrib", s, d).reshape(s.H, s.W)


def distance(a, b):
    """per image the largest difference over the pixels whose n_contrib agrees, and the fraction of pixels left out"""
    (ia, na), (ib, nb) = a, b
    same = na == nb
    return {k: float(np.abs(ia[k].astype(np.float64) - ib[k].astype(np.float64)).reshape(-1, *same.shape)[:, same].max()) for k in ia}, \
        1.0 - float(same.mean())


@pytest.mark.parametrize("variant", ["light", "full"])
@pytest.mark.parametrize("k", [0, 1], ids=["s=1", "s=0.7"])
def test_the_moved_map_renders_the_same_from_the_moved_camera(variant, k):
    """2000 Gaussians at 64 x 48, degree 3; two anchors with different Sim(3) (s = 1 and s = 0.7), every row on anchor k.  The render
    of the transformed map from the camera viewmatrix T^-1 against the original render: e_inv.  The control e_ctl: the same
    statistic between the transformed render and that of the transformed leaves moved one ulp each in a seeded direction.  The bar
    is B e_ctl with B the largest count of roundings of the model's bars; with the SH coefficients left unrotated the same
    comparison misses it by more than 10 x."""
    d = dev()
    s = make_scene(2000, 64, 48, 31)
    rng = np.random.RandomState(32)
    transforms = np.stack([tm.random_sim3(rng, 1.0, 0.5), tm.random_sim3(rng, 0.7, 0.5)])
    T = transforms[k].astype(np.float64)
    leaves = {"xyz": torch.from_numpy(s.means).to(d), "scaling": torch.log(torch.from_numpy(s.scales).to(d)),
              "rotation": torch.from_numpy(s.rots).to(d), "opacity": torch.from_numpy(s.opac).to(d),
              "shs": torch.from_numpy(s.shs).to(d), "anchor": torch.full((s.P,), float(k), device=d)}
    original = render(variant, s, leaves, s.view, s.proj, s.campos)
    moved = {n: t.clone() for n, t in leaves.items()}
    counts = transform_map(moved, None, torch.from_numpy(transforms).to(d))
    assert counts.tolist() == [s.P, 0, 0, 0]
    T_inv = np.linalg.inv(T)
    view = (T_inv.T @ s.view.astype(np.float64)).astype(np.float32)  # (W2C T^-1)^T
    proj = (T_inv.T @ s.proj.astype(np.float64)).astype(np.float32)
    campos = (T[:3, :3] @ s.campos.astype(np.float64) + T[:3, 3]).astype(np.float32)
    after = render(variant, s, moved, view, proj, campos)
    nudged = {}
    for n in ("xyz", "scaling", "rotation", "shs"):
        t = moved[n].cpu().numpy()
        nudged[n] = torch.from_numpy(np.nextafter(t, np.where(rng.rand(*t.shape) < 0.5, -np.inf, np.inf).astype(np.float32))).to(d)
    control = render(variant, s, dict(moved, **nudged), view, proj, campos)
    unrotated = render(variant, s, dict(moved, shs=leaves["shs"]), view, proj, campos)
    e_inv, out_inv = distance(after, original)
    e_ctl, out_ctl = distance(after, control)
    e_bad, _ = distance(unrotated, original)
    B = tm.WORST_ROUNDINGS
    print(f"{variant} s = {(1.0, 0.7)[k]}: left out {out_inv:.4f} (control {out_ctl:.4f}); B = {B}; " +
          "; ".join(f"{n}: e_inv {e_inv[n]:.3e} e_ctl {e_ctl[n]:.3e} unrotated {e_bad[n]:.3e}" for n in e_inv))
    assert out_inv <= 0.005 and out_ctl <= 0.005
    for n in e_inv:
        assert e_inv[n] <= B * e_ctl[n], (n, e_inv[n], e_ctl[n])
    assert e_bad["color"] >= 10 * B * e_ctl["color"]


# ------------------------------------------------------------------------------------------ the anchor leaf through the other steps
def small_map(P, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = {"xyz": torch.randn((P, 3), generator=g), "scaling": 0.3 * torch.randn((P, 3), generator=g) - 2.0,
         "rotation": torch.randn((P, 4), generator=g), "opacity": torch.randn((P, 1), generator=g), "f_dc": torch.randn((P, 1, 3), generator=g),
         "anchor": torch.randint(0, 5, (P,), generator=g).float(), "row": torch.arange(P).float()}
    return {n: t.to(dev()) for n, t in L.items()}


def test_the_existing_steps_carry_the_anchor():
    d, P = dev(), 400
    params = small_map(P, 13)
    before = params["anchor"].clone()
    # seeding: the new rows carry the keyframe's index, the old rows keep theirs
    H, W = 16, 24
    view = torch.eye(4, device=d).reshape(16)
    out, _, _, _, counts = seed_from_frame(params, None, torch.full((3, H, W), 0.5, device=d), torch.full((H, W), 2.0, device=d), view,
                                           20.0, 20.0, 12.0, 8.0, fill={"anchor": 7.0, "row": -1.0})
    assert counts.new == H * W and torch.equal(out["anchor"][:P], before) and (out["anchor"][P:] == 7.0).all()
    # densify-and-prune: clones and children carry their parent's anchor ("row" names the parent)
    P2 = out["xyz"].shape[0]
    out["row"] = torch.arange(P2, device=d).float()
    anchors = out["anchor"].clone()
    grad = torch.rand((P2, 1), device=d)
    out2, _, _, _, c = densify_and_prune(out, None, grad, torch.ones((P2, 1), device=d), None, grad_threshold=0.5, extent=10.0)
    assert c.clones + c.children > 0 and c.rows != P2
    assert torch.equal(out2["anchor"], anchors[out2["row"].long()])
    # relocation: a relocated row carries its source's anchor
    out2["opacity"][::3] = -8.0
    anchors = out2["anchor"].clone()
    res = relocate_dead(out2, None, seed=3)
    src = res.source.long()
    moved = src >= 0
    assert int(moved.sum()) > 50 and torch.equal(out2["anchor"][moved], anchors[src[moved]])
    assert torch.equal(out2["anchor"][~moved], anchors[~moved])
