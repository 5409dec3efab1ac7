"""The step code by concern: `dgr_amd.pose`, `dgr_amd.losses`, `dgr_amd.keyframes` behind the public names of `dgr_amd.slam`,
`dgr_amd.map_steps` behind those of `dgr_amd.optim`, and the one path by which all 21 step calls enter the C ABI
(`_capi.StepCalls`, of which `_capi.call` is one use): the tensors' device made current, ITS current stream as the first argument,
the library's message raised on a non-zero result.  No device work: the library is a recording stub."""
import ctypes

import numpy as np
import pytest
import torch

from dgr_amd import _capi, keyframes, losses, map_steps, multiview, optim, pose, slam

MOVED = {pose: ("projection_matrix", "quat_to_rotmat", "w2c_from_quat_trans", "camera_tensors", "pose_to_camera"),
         losses: ("l1_loss", "ssim", "l1_ssim_loss", "MaskedLossStats", "masked_l1_loss"),
         keyframes: ("KeyframeOverlap", "keyframe_overlap", "select_keyframes")}
KEPT = ("render", "render_views", "render_batch_fused", "render_batch")


def test_slam_keeps_its_seventeen_public_names():
    assert sum(len(names) for names in MOVED.values()) == 13
    for module, names in MOVED.items():
        for n in names:
            assert getattr(slam, n) is getattr(module, n), n
    for n in KEPT:
        assert callable(getattr(slam, n)) and getattr(slam, n).__module__ == "dgr_amd.slam", n


MOVED_MAP_STEPS = ("add_densification_stats", "DensifyCounts", "DEFAULT_ROLES", "densify_thresholds", "densify_and_prune",
                   "SeedCounts", "SEED_ROLES", "seed_constants", "seed_from_frame", "RelocateResult", "relocate_dead",
                   "inject_position_noise")


def test_optim_keeps_its_thirteen_public_names():
    assert len(MOVED_MAP_STEPS) == 12
    for n in MOVED_MAP_STEPS:
        assert getattr(optim, n) is getattr(map_steps, n), n
    assert isinstance(optim.SparseAdam, type) and optim.SparseAdam.__module__ == "dgr_amd.optim"


class StubLibrary:
    """Every dgr_* entry point: records (name, arguments) and returns `rc_of[name]`, else `rc` (the scratch-size queries: a size
    that fits; no stream is being captured).  The plan entries write `COUNTS` through their last argument, counts8_device, which
    is host memory here."""
    SIZES = {"dgr_l1_loss_scratch_floats": 128, "dgr_masked_loss_scratch_bytes": 4096, "dgr_keyframe_overlap_scratch_bytes": 64,
             "dgr_densify_plan_bytes": 256, "dgr_seed_plan_bytes": 256, "dgr_relocate_scratch_bytes": 1024}
    COUNTS = {"dgr_densify_plan": (7, 4, 1, 2, 1), "dgr_seed_plan": (7, 2, 6, 2, 0)}  # (P = 5: DensifyCounts, SeedCounts)

    def __init__(self):
        self.rc, self.rc_of, self.calls = 0, {}, []

    def dgr_last_error(self):
        return b"the stub's message"

    def dgr_stream_is_capturing(self, stream):
        return 0

    def dgr_ssim_scratch_floats(self, V, C, H, W):
        return 64 + 3 * V * C * H * W

    def __getattr__(self, name):
        if name in self.SIZES:
            return lambda *a: self.SIZES[name]

        def entry(*args):
            self.calls.append((name, args))
            if name in self.COUNTS:
                (ctypes.c_int * 8).from_address(args[-1])[:] = self.COUNTS[name] + (0, 0, 0)
            return self.rc_of.get(name, self.rc)
        return entry


@pytest.fixture
def stub(monkeypatch):
    lib = StubLibrary()
    lib.devices, lib.streams = [], []  # (the guards entered, the stream lookups)

    class Guard:
        def __init__(self, dev):
            lib.devices.append(dev)

        def __enter__(self):
            return None

        def __exit__(self, *a):
            return False

    monkeypatch.setattr(_capi, "load", lambda: lib)
    monkeypatch.setattr(_capi, "stream_handle", lambda index=None: (lib.streams.append(index), ("current stream of device", index))[1])
    monkeypatch.setattr(_capi, "on_device", Guard)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)  # (SparseAdam's question before its first step)
    return lib


DEV1 = torch.device("cuda", 1)  # (a device object only: nothing is allocated on it)


def test_call_uses_the_given_devices_stream_and_raises_the_librarys_message(stub):
    _capi.call("dgr_pose_backward", DEV1, 11, 12)
    _capi.call(stub.dgr_anything, DEV1, 13)
    assert stub.calls == [("dgr_pose_backward", (("current stream of device", 1), 11, 12)),
                          ("dgr_anything", (("current stream of device", 1), 13))]
    assert stub.devices == [DEV1, DEV1]
    stub.rc = -4
    with pytest.raises(RuntimeError, match="the stub's message"):
        _capi.call("dgr_pose_forward", DEV1, 1)


class _OnDevice1(torch.Tensor):
    """A host tensor that says it lives on cuda:1: a step that asks for the CURRENT device's stream (a bare `stream_handle()`)
    instead of its tensors' is told apart from one that follows them."""
    device = property(lambda self: DEV1)
    is_cuda = property(lambda self: True)


def _step_calls():
    """name of the C entry point -> (a function that prepares the step call and returns the call itself): the four forwards, the
    four backwards (prepared by their forward) and keyframe_overlap, on fake cuda:1 tensors (which the public wrappers of the
    losses and the pose refuse: their autograd Functions are entered directly)"""
    g = torch.Generator().manual_seed(5)
    rand = lambda *shape: torch.rand(shape, generator=g).as_subclass(_OnDevice1).requires_grad_()  # noqa: E731
    c, d, c_obs, d_obs = rand(3, 5, 7), rand(1, 5, 7), rand(3, 5, 7).detach(), rand(1, 5, 7).detach()
    q, t, perspec = rand(4), rand(3), torch.eye(4)
    params = _capi.MaskedLossParams(0.0, 10.0, 0.99, 10.0, 1, 1, _capi.MASKED_LOSS_SUM, 1.0, 0.5)
    forwards = {
        "dgr_pose": lambda: pose._PoseToCamera.apply(q, t, perspec)[0].sum(),
        "dgr_l1_loss": lambda: losses._L1Loss.apply(c, d, c_obs, d_obs, 1.0, 0.5),
        "dgr_ssim_loss": lambda: losses._SsimLoss.apply(c, d, c_obs, d_obs, (1, 3, 5, 7), 0.8, 0.2, 0.5, True, False),
        "dgr_masked_loss": lambda: losses._MaskedL1Loss.apply(c, d, c_obs, d_obs, None, None, (1, 3, 5, 7), params)[0],
        "dgr_keyframe_overlap": lambda: keyframes.keyframe_overlap(d_obs, torch.eye(4), torch.eye(4).repeat(2, 1, 1), 5.0, 5.0,
                                                                   3.0, 2.0, stride=2),
    }
    calls = {"dgr_keyframe_overlap": lambda: forwards["dgr_keyframe_overlap"]}
    for name, fwd in list(forwards.items())[:4]:
        calls[name + "_forward"] = lambda fwd=fwd: fwd
        calls[name + "_backward"] = lambda fwd=fwd: fwd().backward  # (the forward runs here, and succeeds)
    return calls


def _fake(*shape, dtype=torch.float32, seed=9):
    g = torch.Generator().manual_seed(seed + len(shape))
    t = torch.rand(shape, generator=g) if dtype == torch.float32 else torch.randint(0, 3, shape, generator=g, dtype=dtype)
    return t.as_subclass(_OnDevice1)


def _model(P=5):
    return {"xyz": _fake(P, 3), "scaling": _fake(P, 3, seed=1), "rotation": _fake(P, 4), "opacity": _fake(P, 1), "f_dc": _fake(P, 3, seed=2)}


def _adam(capturable):
    def run():
        params = [_fake(5, 3).requires_grad_(), _fake(5, 1).requires_grad_()]
        for p in params:
            p.grad = _fake(*p.shape, seed=3)
        optim.SparseAdam(params, lr=0.01, capturable=capturable).step(visible=_fake(5, dtype=torch.int32))
    return run


def _map_step_calls():
    """name of the C entry point -> (a function that prepares the step and returns the call that reaches the entry point), for the
    twelve map-step, Adam and cov3d entry points: P = 5 rows, a 4 x 6 frame at stride 2, every tensor a fake cuda:1 one.  The
    apply entry points are reached through their plan call, which succeeds."""
    P = 5
    acc = lambda: (_fake(P, 1), _fake(P, 1), _fake(P))  # noqa: E731
    densify = lambda: map_steps.densify_and_prune(_model(), None, *acc(), grad_threshold=0.1, extent=2.0)  # noqa: E731
    seed = lambda: map_steps.seed_from_frame(_model(), None, _fake(3, 4, 6), _fake(4, 6), _fake(16), 5.0, 5.0, 3.0, 2.0,  # noqa: E731
                                             stride=2, xyz_gradient_accum=_fake(P, 1))

    def relocate():
        params = _model()
        adam = optim.SparseAdam(list(params.values()))
        adam.state = {p: (_fake(*p.shape, seed=4), _fake(*p.shape, seed=5)) for p in params.values()}
        map_steps.relocate_dead(params, adam, xyz_gradient_accum=_fake(P, 1), denom=_fake(P, 1))

    cov = lambda: multiview._SharedCov3D.apply(_fake(P, 3).requires_grad_(), _fake(P, 4).requires_grad_(), 1.0).sum()  # noqa: E731
    direct = {
        "dgr_densification_stats": lambda: map_steps.add_densification_stats(_fake(P, 3), _fake(P, dtype=torch.int32), *acc()),
        "dgr_densify_plan": densify, "dgr_densify_apply": densify, "dgr_seed_plan": seed, "dgr_seed_apply": seed,
        "dgr_relocate_plan": relocate, "dgr_relocate_apply": relocate,
        "dgr_position_noise": lambda: map_steps.inject_position_noise(_model(), 1e-4),
        "dgr_sparse_adam": _adam(False), "dgr_sparse_adam_capturable": _adam(True), "dgr_cov3d_forward": cov,
    }
    calls = {name: (lambda run=run: run) for name, run in direct.items()}
    calls["dgr_cov3d_backward"] = lambda: cov().backward  # (the forward runs here, and succeeds)
    return calls


# the calls a step makes before (and with) the one named, all under ONE guard and ONE stream lookup
SEQUENCE = {"dgr_densify_apply": ["dgr_densify_plan", "dgr_densify_apply"], "dgr_seed_apply": ["dgr_seed_plan", "dgr_seed_apply"],
            "dgr_relocate_apply": ["dgr_relocate_plan", "dgr_relocate_apply"], "dgr_sparse_adam": ["dgr_sparse_adam"] * 2,
            "dgr_sparse_adam_capturable": ["dgr_sparse_adam_capturable"] * 2}


def test_the_21_step_calls_go_through_the_one_call_path(stub, monkeypatch):
    monkeypatch.setattr(keyframes, "_check_gpu", lambda *a: None)  # (keyframe_overlap is no autograd Function: let host tensors in)
    real_empty, real_full = torch.empty, torch.full
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real_empty(*a, **kw))  # (the steps' buffers "on cuda:1")
    monkeypatch.setattr(torch, "full", lambda *a, device=None, **kw: real_full(*a, **kw))
    calls = dict(_step_calls(), **_map_step_calls())
    assert len(calls) == 21
    through = []
    real_call = _capi.StepCalls.call
    monkeypatch.setattr(_capi.StepCalls, "call", lambda self, name, *args: (through.append((name, self.device)), real_call(self, name, *args))[1])
    for name, prepare in calls.items():
        for rc in (0, -1):
            del stub.calls[:], stub.devices[:], stub.streams[:], through[:]
            stub.rc_of = {}
            step = prepare()
            stub.rc_of = {name: rc}
            if rc == 0:
                step()
            else:  # the library's refusal, forwards and backwards alike
                with pytest.raises(RuntimeError, match="the stub's message"):
                    step()
            if rc:  # (a refused call is the step's last; a plan call that succeeds is followed by its apply call)
                assert through[-1][0] == stub.calls[-1][0] == name
            assert (name, DEV1) in through, (name, rc)                    # entered through the one path, with the tensors' device
            assert stub.devices[-1] == DEV1, (name, rc)                   # ... which was made current for the call
            args = [a for c, a in stub.calls if c == name][-1]
            assert args[0] == ("current stream of device", 1), (name, rc)  # ... and whose stream went in first
            assert [c for c, _ in through] == [c for c, _ in stub.calls]  # (no call reached the library by another way)
            if name.endswith("_backward"):
                assert [n for n, _ in stub.calls] == [name[:-len("backward")] + "forward", name]
            if name in SEQUENCE:  # a group of calls: every one on that path, one guard and one stream lookup for all of them
                n = len(SEQUENCE[name]) if rc == 0 or name.endswith("_apply") else 1  # (a refused Adam call is the first tensor's)
                assert [c for c, _ in stub.calls] == SEQUENCE[name][:n] and through == [(c, DEV1) for c in SEQUENCE[name][:n]]
                assert all(a[0] == ("current stream of device", 1) for _, a in stub.calls)
                asked = 1 if "adam" in name else 0  # (an optimiser's first step asks its device whether a hipGraph is recorded)
                assert stub.devices == [DEV1] * (asked + 1) and stub.streams == [1], (name, rc)


def test_a_refused_adam_step_leaves_the_optimiser_as_it_was(stub, monkeypatch):
    """SparseAdam.step's promise: a call refused by the host checks leaves `steps`, the device step count and `state` untouched.
    A failure of the library itself (rc = -1 on the first tensor) is no such refusal and is raised with the library's message
    after that one call: the step had begun, as it always has (`steps` counts it, the first tensor has its moments, no other)."""
    real_full = torch.full
    monkeypatch.setattr(torch, "full", lambda *a, device=None, **kw: real_full(*a, **kw))
    for capturable in (False, True):
        params = [_fake(5, 3).requires_grad_(), _fake(5, 1).requires_grad_()]
        for p in params:
            p.grad = _fake(*p.shape, seed=3)
        adam = optim.SparseAdam(params, capturable=capturable)
        for bad in (_fake(5), _fake(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int32)):  # float; 4 rows; another device
            with pytest.raises(RuntimeError, match="SparseAdam: `visible`"):
                adam.step(visible=bad)
            assert adam.steps == 0 and adam._step_dev is None and adam.state == {} and stub.calls == [] and stub.devices == []
        stub.rc = -1
        with pytest.raises(RuntimeError, match="the stub's message"):
            adam.step()
        stub.rc = 0
        assert len(stub.calls) == 1 and adam.steps == 1 and list(adam.state) == [params[0]]
        assert (adam._step_dev is None) == (not capturable)
        del stub.calls[:], stub.devices[:]


def test_relocate_dead_refuses_a_strided_leaf_before_it_copies_any(stub, monkeypatch):
    copies = []
    real_contiguous = torch.Tensor.contiguous
    monkeypatch.setattr(torch.Tensor, "contiguous", lambda self, *a, **kw: (copies.append(self.shape), real_contiguous(self, *a, **kw))[1])
    params = _model()
    params["f_dc"] = _fake(5, 6)[:, ::2]
    assert not params["f_dc"].is_contiguous() and params["f_dc"].is_cuda
    with pytest.raises(RuntimeError, match=r"relocate_dead: params\['f_dc'\] is rewritten in place and must be contiguous"):
        map_steps.relocate_dead(params, None)
    assert copies == [] and stub.calls == []


def _descriptors(stub, entry):
    """every descriptor that reached `entry` (a dgr_*_apply), as tuples of its fields, with the count handed over beside the array"""
    rows = []
    for name, args in stub.calls:
        if name != entry:
            continue
        (i, descs), = [(i, a) for i, a in enumerate(args) if isinstance(a, ctypes.Array)]
        assert args[i - 1] == len(descs)
        rows += [tuple(getattr(d, f) for f, _ in d._fields_) for d in descs]
    return rows


def test_a_zero_width_leaf_reaches_no_kernel(stub, monkeypatch):
    """A degree-0 model as 3DGS builds it: f_dc [P, 1, 3] and f_rest [P, 0, 3].  The C ABI refuses a descriptor with k < 1 or a NULL
    tensor, so none may leave Python: the descriptors of densify_and_prune, seed_from_frame and relocate_dead, and the calls of
    SparseAdam.step (eager and capturable), are those of the same call on the model without f_rest; f_rest and its moments come
    back empty, with the new number of rows, `requires_grad` kept, and the optimiser pointed at them."""
    real_empty, real_full = torch.empty, torch.full
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real_empty(*a, **kw))
    monkeypatch.setattr(torch, "full", lambda *a, device=None, **kw: real_full(*a, **kw))
    P = 5
    base = {"xyz": _fake(P, 3), "f_dc": _fake(P, 1, 3, seed=2), "opacity": _fake(P, 1), "scaling": _fake(P, 3, seed=1),
            "rotation": _fake(P, 4)}
    for t in base.values():
        t.requires_grad_()
    f_rest = _fake(P, 0, 3).requires_grad_()
    assert f_rest.shape == (P, 0, 3) and f_rest.is_cuda
    with_rest = dict(list(base.items())[:2] + [("f_rest", f_rest)] + list(base.items())[2:])
    moments = {name: (_fake(*t.shape, seed=4), _fake(*t.shape, seed=5)) for name, t in with_rest.items()}
    acc = (_fake(P, 1), _fake(P, 1), _fake(P))

    def adam_over(params):
        adam = optim.SparseAdam(list(params.values()))
        adam.state = {t: moments[name] for name, t in params.items()}
        return adam

    steps = {
        "dgr_densify_apply": lambda params, adam: map_steps.densify_and_prune(params, adam, *acc, grad_threshold=0.1, extent=2.0)[0],
        "dgr_seed_apply": lambda params, adam: map_steps.seed_from_frame(params, adam, _fake(3, 4, 6), _fake(4, 6), _fake(16), 5.0, 5.0,
                                                                         3.0, 2.0, stride=2, xyz_gradient_accum=acc[0])[0],
        "dgr_relocate_apply": lambda params, adam: (map_steps.relocate_dead(params, adam, xyz_gradient_accum=acc[0], denom=acc[1]), params)[1],
    }
    for entry, run in steps.items():
        seen = {}
        for label, params in (("without", base), ("with", with_rest)):
            del stub.calls[:]
            adam = adam_over(params)
            out = run(dict(params), adam)
            seen[label] = rows = _descriptors(stub, entry)
            n_leaves = len(base)
            assert len(rows) >= 3 * n_leaves, entry  # every leaf with its two moments, then the accumulators
            for row in rows:
                fields = dict(zip([f for f, _ in {"dgr_densify_apply": _capi.DensifyTensor, "dgr_seed_apply": _capi.SeedTensor,
                                                 "dgr_relocate_apply": _capi.RelocateTensor}[entry]._fields_], row))
                assert fields["k"] >= 1, (entry, label, fields)
                assert fields.get("dst", 1) and fields.get("data", 1), (entry, label, fields)  # (a NULL src is a mode's: zeros, constants)
            if label == "with":
                rows_new = P if entry == "dgr_relocate_apply" else 7  # (the stub's plan: 7 rows after either resize)
                got = out["f_rest"]
                assert got.shape == (rows_new, 0, 3) and got.requires_grad and got.dtype == torch.float32
                assert got in adam.state and [tuple(m.shape) for m in adam.state[got]] == [(rows_new, 0, 3)] * 2
                assert any(p is got for g in adam.param_groups for p in g["params"])
                assert all(out[name].shape[0] == rows_new for name in base)
        # the same descriptors, in the same order (a resize writes into tensors of its own: `dst` differs from call to call)
        strip = (lambda row: row[:1] + row[2:]) if entry != "dgr_relocate_apply" else (lambda row: row)
        assert [strip(r) for r in seen["with"]] == [strip(r) for r in seen["without"]], entry

    for t in with_rest.values():
        t.grad = _fake(*t.shape, seed=3)
    for capturable in (False, True):
        entry = "dgr_sparse_adam_capturable" if capturable else "dgr_sparse_adam"
        seen = {}
        for label, params in (("without", base), ("with", with_rest)):
            del stub.calls[:]
            adam = optim.SparseAdam(list(params.values()), lr=0.01, capturable=capturable)
            adam.step()
            adam.step(visible=_fake(P, dtype=torch.int32))
            calls = [a for name, a in stub.calls if name == entry]
            assert len(calls) == len(stub.calls) == 2 * len(base)
            for a in calls:  # (stream, rows, k, parameter, gradient, exp_avg, exp_avg_sq, ...)
                assert a[1] == P and a[2] >= 1 and all(a[3:7]), (entry, label, a[:7])
            seen[label] = [a[1:5] for a in calls]
            if label == "with":
                assert [tuple(m.shape) for m in adam.state[f_rest]] == [(P, 0, 3)] * 2 and adam.steps == 2
        assert seen["with"] == seen["without"], entry


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason=f"needs two GPUs, this machine has {torch.cuda.device_count()}")
def test_steps_follow_their_tensors_device_not_the_current_one():
    """Inputs on device 1 while device 0 is current: the pose and L1 steps, SparseAdam.step and add_densification_stats used to
    take the CURRENT device's stream.  The results must be the bits of the same calls made with device 1 current.  [3,5,7] +
    [1,5,7]: 105 elements, past one wave; [3,13,40]: a second SSIM tile in x; P = 300 rows: a second 256-row block."""
    dev = torch.device("cuda", 1)
    rng = np.random.default_rng(7)
    on = lambda *shape: torch.from_numpy(rng.random(shape, dtype=np.float32)).to(dev)  # noqa: E731
    q, t = on(4) + 0.5, on(3)
    c, d, c_obs, d_obs = on(3, 5, 7), on(1, 5, 7), on(3, 5, 7), on(1, 5, 7)
    img, ref = on(3, 13, 40), on(3, 13, 40)
    P = 300
    leaves, grads, dmeans2D = (on(P, 3), on(P, 1)), (on(P, 3) - 0.5, on(P, 1) - 0.5), on(P, 3) - 0.5
    radii = torch.from_numpy(rng.integers(-1, 4, P).astype(np.int32)).to(dev)

    def run():
        out = []
        qq, tt = q.clone().requires_grad_(), t.clone().requires_grad_()
        view, proj, perspec, campos = slam.pose_to_camera(qq, tt, 1.0, 0.75)
        (view * torch.arange(16.0, device=dev).view(4, 4)).sum().backward()
        out += [view, proj, perspec, campos, qq.grad, tt.grad]
        for loss_fn, a, b in ((lambda x, y: slam.l1_loss(x, y, c_obs, d_obs), c, d),
                              (lambda x, y: slam.l1_ssim_loss(x, None, ref, None), img, None)):
            a = a.clone().requires_grad_()
            b = b.clone().requires_grad_() if b is not None else None
            loss = loss_fn(a, b)
            loss.backward()
            out += [loss, a.grad] + ([b.grad] if b is not None else [])
        for capturable in (False, True):
            params = [x.clone().requires_grad_() for x in leaves]
            for p, g in zip(params, grads):
                p.grad = g.clone()
            adam = optim.SparseAdam(params, lr=0.01, capturable=capturable)
            adam.step()
            adam.step(visible=radii)
            out += params + [m for p in params for m in adam.state[p]]
        acc = [torch.zeros(P, 1, device=dev), torch.zeros(P, 1, device=dev), torch.zeros(P, device=dev)]
        optim.add_densification_stats(dmeans2D, radii, *acc)
        out += acc
        torch.cuda.synchronize(dev)
        return [o.detach().cpu() for o in out]

    with torch.cuda.device(0):
        away = run()
    with torch.cuda.device(1):
        home = run()
    assert len(away) == len(home) == 11 + 2 * 6 + 3
    for k, (x, y) in enumerate(zip(away, home)):
        assert torch.equal(x, y), k
