"""The step code by concern: `dgr_amd.pose`, `dgr_amd.losses`, `dgr_amd.keyframes` behind the public names of `dgr_amd.slam`, and
the one path by which their nine step calls enter the C ABI (`_capi.call`): the tensors' device made current, ITS current stream
as the first argument, the library's message raised on a non-zero result.  No device work: the library is a recording stub."""
import numpy as np
import pytest
import torch

from dgr_amd import _capi, keyframes, losses, pose, slam

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


class StubLibrary:
    """Every dgr_* entry point: records (name, arguments) and returns `rc` (the scratch-size queries: a size that fits)."""
    SIZES = {"dgr_l1_loss_scratch_floats": 128, "dgr_masked_loss_scratch_bytes": 4096, "dgr_keyframe_overlap_scratch_bytes": 64}

    def __init__(self):
        self.rc, self.calls = 0, []

    def dgr_last_error(self):
        return b"the stub's message"

    def dgr_ssim_scratch_floats(self, V, C, H, W):
        return 64 + 3 * V * C * H * W

    def __getattr__(self, name):
        if name in self.SIZES:
            return lambda *a: self.SIZES[name]

        def entry(*args):
            self.calls.append((name, args))
            return self.rc
        return entry


@pytest.fixture
def stub(monkeypatch):
    lib = StubLibrary()
    lib.devices = []

    class Guard:
        def __init__(self, dev):
            lib.devices.append(dev)

        def __enter__(self):
            return None

        def __exit__(self, *a):
            return False

    monkeypatch.setattr(_capi, "load", lambda: lib)
    monkeypatch.setattr(_capi, "stream_handle", lambda index=None: ("current stream of device", index))
    monkeypatch.setattr(_capi, "on_device", Guard)
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


def test_the_nine_step_calls_go_through_the_one_call_path(stub, monkeypatch):
    monkeypatch.setattr(keyframes, "_check_gpu", lambda *a: None)  # (keyframe_overlap is no autograd Function: let host tensors in)
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real_empty(*a, **kw))  # (the steps' buffers "on cuda:1")
    calls = _step_calls()
    assert len(calls) == 9
    through = []
    real_call = _capi.call
    monkeypatch.setattr(_capi, "call", lambda name, device, *args: (through.append((name, device)), real_call(name, device, *args))[1])
    for name, prepare in calls.items():
        for rc in (0, -1):
            del stub.calls[:], stub.devices[:], through[:]
            stub.rc = 0
            step = prepare()
            stub.rc = rc
            if rc == 0:
                step()
            else:  # the library's refusal, forwards and backwards alike
                with pytest.raises(RuntimeError, match="the stub's message"):
                    step()
            assert through[-1] == (name, DEV1), (name, rc)                # entered through _capi.call, with the tensors' device
            assert stub.devices[-1] == DEV1, (name, rc)                   # ... which was made current for the call
            last, args = stub.calls[-1]
            assert last == name and args[0] == ("current stream of device", 1), (name, rc)  # ... and whose stream went in first
            if name.endswith("_backward"):
                assert [n for n, _ in stub.calls] == [name[:-len("backward")] + "forward", name]


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason=f"needs two GPUs, this machine has {torch.cuda.device_count()}")
def test_steps_follow_their_tensors_device_not_the_current_one():
    """Inputs on device 1 while device 0 is current: the pose and L1 steps used to take the CURRENT device's stream.  The results
    must be the bits of the same calls made with device 1 current.  [3,5,7] + [1,5,7]: 105 elements, past one wave; [3,13,40]:
    a second SSIM tile in x."""
    dev = torch.device("cuda", 1)
    rng = np.random.default_rng(7)
    on = lambda *shape: torch.from_numpy(rng.random(shape, dtype=np.float32)).to(dev)  # noqa: E731
    q, t = on(4) + 0.5, on(3)
    c, d, c_obs, d_obs = on(3, 5, 7), on(1, 5, 7), on(3, 5, 7), on(1, 5, 7)
    img, ref = on(3, 13, 40), on(3, 13, 40)

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
        torch.cuda.synchronize(dev)
        return [o.detach().cpu() for o in out]

    with torch.cuda.device(0):
        away = run()
    with torch.cuda.device(1):
        home = run()
    assert len(away) == len(home) == 11
    for k, (x, y) in enumerate(zip(away, home)):
        assert torch.equal(x, y), k
