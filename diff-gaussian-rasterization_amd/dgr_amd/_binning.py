"""The binning capacity and status policy of every forward, one-view and batch, of both variants and both bindings.

A forward runs in one of three modes (`_binning_policy`): 0 = the reference's resize callbacks and blocking read
(DGR_FORWARD_MODE=callback), 1 = strict (presized, one host wait for the exact count, an overflow retried inside the call),
2 = lazy (presized, no host wait: the device status word {num_rendered, overflow, prefiltered violation, num_related} is read
by a later call).  After it, `record` notes what the forward left to be learnt; `strict_retry` and `run_batch` drive the
strict attempts and the batches.  The state below is shared by all of them, so the variants cannot diverge.
"""
import ctypes as C
import os
import weakref

import torch

from . import _capi

# binning capacity learned per (device, P, H, W): largest num_rendered seen for that shape
_capacity_cache = {}

# DGR_SYNC_MODE=lazy: once a shape's num_rendered is known, forward performs NO host synchronisation.  The binning
# buffer is over-provisioned (1.5x the largest count seen); the device status word {num_rendered, overflow,
# prefiltered violation, -} is copied asynchronously to pinned host memory behind an event, and inspected when a
# later call starts (or by check_async_errors()), by which time the event has long fired.  An overflow or a
# `prefiltered` violation therefore raises one or two calls late.  Default ("strict"): one status read at the end of
# every forward, like the reference's blocking copy of num_rendered (L/cuda_rasterizer/rasterizer_impl.cu:287).
_pending_status = []   # [(ticket of dgr_status_post, key)]
# Status words left unread when a forward is issued.  1: view i is issued once view i-2's forward has reported -- with several
# views in flight on several streams (dgr_amd.multiview.ViewStreams) that starves a stream whose previous view has finished
# while the view whose report the host waits for is still in its blend kernels; ViewStreams raises it to its number of streams
# (three views in flight, config 3: 0.483 -> 0.473 ms per step over 20 steps, 0.434 -> 0.428 over 100: profiles/r6/lazy_depth.txt).
# The price: an overflow or a `prefiltered` violation is reported up to depth + 1 calls late instead of two.
_LAZY_DEPTH = max(1, int(os.environ.get("DGR_LAZY_DEPTH", "1")))


def lazy_depth():
    return _LAZY_DEPTH


def set_lazy_depth(n):
    """See _LAZY_DEPTH above; returns the previous value."""
    global _LAZY_DEPTH
    prev, _LAZY_DEPTH = _LAZY_DEPTH, max(1, int(n))
    return prev
_last_status = {}      # key -> the most recent status word read back for that shape
_NO_STATUS = (0, 0, 0, 0)


def _sync_mode():
    return os.environ.get("DGR_SYNC_MODE", "strict")


# Status words of forwards recorded into a hipGraph (torch.cuda.graph): nothing can be read back while capturing, so the
# device tensors are kept and inspected on request after a replay (check_captured_status()).
_captured_status = []     # weak references: a status word lives as long as the capture that owns it
_capture_keepalive = []   # strong references collected during ONE capture; CapturedStep takes them over


def raise_prefiltered():
    raise RuntimeError("Point is filtered although prefiltered is set. This shouldn't happen!")


def _check(rc):
    """A C-ABI return code: returned when >= 0, else raised with the library's message."""
    if rc >= 0:
        return rc
    msg = _capi.last_error()
    if rc == _capi.DGR_ERR_PREFILTERED:
        raise_prefiltered()
    if rc == _capi.DGR_ERR_BAD_ARGUMENT:
        raise RuntimeError(f"dgr_hip: bad argument: {msg}")
    raise RuntimeError(f"dgr_hip: error {rc}: {msg}")


# Lazy mode is only as safe as its capacity guess (1.5 x the largest count seen for the shape): a count that GROWS -- the camera
# closing in, splats being scaled up, a map that densifies without changing P -- reaches it within a few frames, and frames rendered
# past it have empty tile lists.  Three guards (round 9):
#   * the blend kernels write NaN images for an overflowed forward (csrc/render_light.hip), never a plausible empty frame, and its
#     backward (empty lists) yields zero gradients: nothing wrong reaches an optimiser unnoticed;
#   * a shape whose count grew by more than 25 % between two status reads, came within 20 % of the capacity it was rendered with,
#     or overflowed, is UNSETTLED: its next forwards run strict (exact count, overflow retried inside the call) until three
#     reads in a row show less than 10 % growth;
#   * check_async_errors() before optimizer.step() reads every outstanding word (the forwards' words arrive while their backward
#     kernels are still queued: the wait costs the GPU nothing) and raises -- dgr_amd.slam's loops and examples/mapping.py do.
_unsettled = {}        # key -> strict forwards still to run
_GROWTH_STRICT, _SETTLED_READS = 1.25, 3


def _note_growth(key, prev, s, capacity_used=None):
    grew = prev > 0 and s[0] > _GROWTH_STRICT * prev
    near = capacity_used is not None and s[0] > 0.8 * capacity_used
    if s[1] or grew or near:
        _unsettled[key] = _SETTLED_READS
    elif key in _unsettled and prev > 0 and s[0] <= 1.1 * prev:
        _unsettled[key] -= 1
        if _unsettled[key] <= 0:
            del _unsettled[key]


def _strict_read(key, cap, rendered, related=None):
    """A strict forward returned its exact count (and retried an overflow inside the call).  `related`: the full variant's
    num_related (the status word's [3], which its lazy forwards report), kept in every sync mode; < 0 when the forward did not
    wait for it, and then the last one read stays."""
    last = _last_status.get(key)  # (the previous count, read before it is overwritten)
    lazy = _sync_mode() == "lazy"
    if lazy:
        _note_growth(key, last[0] if last else 0, (rendered, 0, 0, 0))
    if lazy or related is not None:
        if related is None or related < 0:
            related = last[3] if last else 0
        _last_status[key] = [rendered, 0, 0, related]
    _capacity_cache[key] = max(cap, rendered)


def _check_oldest():
    ticket, key = _pending_status.pop(0)
    buf = (C.c_int * 4)()
    _check(_capi.load().dgr_status_poll(ticket, 1, buf))  # waits for that forward only
    s = list(buf)
    prev = _last_status.get(key, _NO_STATUS)[0]
    _note_growth(key, prev, s, capacity_used=int(_capacity_cache.get(key, 0) * 1.5) + 4096)
    _capacity_cache[key] = max(_capacity_cache.get(key, 0), s[0])
    _last_status[key] = s
    if s[2]:
        raise_prefiltered()
    if s[1]:
        raise RuntimeError(f"dgr_hip: binning buffer overflow in an earlier lazily-checked forward (needed {s[0]} "
                           f"instances); its outputs were invalid -- rerun that step")


def check_captured_status():
    """After replaying a graph that contains forwards: raises if one of them overflowed its binning buffer (the graph
    was captured with a smaller scene than it is replayed on) or hit the prefiltered trap.  Blocks on the device.
    Status words whose graph no longer exists (the tensor's storage was freed with the graph's pool) are dropped."""
    _captured_status[:] = [r for r in _captured_status if r() is not None]
    for ref in _captured_status:
        st = ref()
        if st is None:
            continue
        for s in st.reshape(-1, 4).tolist():  # (a batched forward keeps the [V,4] status words of its views in one tensor)
            if s[2]:
                raise_prefiltered()
            if s[1]:
                raise RuntimeError(f"dgr_hip: binning buffer overflow in a graph-captured forward (needed {s[0]} instances): "
                                   f"re-capture after an eager warm-up on the larger scene")


def check_async_errors():
    """Raises if an earlier lazily-checked forward overflowed its binning buffer or hit the prefiltered trap."""
    while _pending_status:
        _check_oldest()


def _binning_policy(key, P, views=None):
    """(mode, capacity, cached count) of the next forward of shape `key` = (device, P, H, W); see csrc/torch_ext.cpp:
    forward_core.  `views`: a batch of that many views, which leaves one status word per view unread (the depth,
    lazy_depth() otherwise) and has no resize-callback form: it runs strict where a one-view forward takes mode 0."""
    cap = _capacity_cache.get(key, 0)
    if os.environ.get("DGR_FORWARD_MODE", "presized") == "callback" or P == 0:
        if views is None:
            return 0, 0, cap
    elif _sync_mode() == "lazy" and cap > 0:
        while len(_pending_status) > (_LAZY_DEPTH if views is None else views) and not torch.cuda.is_current_stream_capturing():
            _check_oldest()  # status words of earlier calls have long completed: no stall
        if key not in _unsettled or torch.cuda.is_current_stream_capturing():
            return 2, int(cap * 1.5) + 4096, cap
        # an unsettled shape (above): strict forwards, which also keep the count history going
        return 1, int(cap * 1.5) + 4096, cap
    return 1, (int(cap * 1.25) + 4096 if cap else 4 * P + 4096), cap


def _post(key, status, tickets=None):
    """A forward that was not waited for (lazy, or recorded into a hipGraph) leaves its status words -- `status` [4], or [V,4] for
    a batch -- to be read later: by a later call or check_async_errors() when posted (dgr_status_post: a copy to pinned host memory
    behind an event), after a replay (check_captured_status) when captured.  `tickets`: the extension's, none while capturing;
    None: the ctypes binding's forward, posted here."""
    if tickets is None and not torch.cuda.is_current_stream_capturing():
        post, st, p = _capi.load().dgr_status_post, _capi.stream_handle(status.device.index), status.data_ptr()
        tickets = [_check(post(st, p + 16 * v)) for v in range(status.numel() // 4)]
    if tickets:
        _pending_status.extend((t, key) for t in tickets)
    else:  # recorded into a hipGraph: nothing can be read back now
        _captured_status.append(weakref.ref(status))  # kept alive by the captured step's results (CapturedStep.keep)
        _capture_keepalive.append(status)


def record(key, mode, cap, use, rendered, status, ticket=None, related=None):
    """After a one-view forward that ran in `mode` with capacity `use` (_binning_policy): returns the num_rendered and num_related
    (the full variant's; None for the light one) to report, and R for its backward.  A lazy or captured forward's status word is
    left to be read later (_post); it reports the values last read for the shape and hands its backward the capacity its binning
    buffer was carved with -- at least the frame's count, which the deterministic backward's row buffer needs
    (csrc/render_light.hip: det_gather_kernel writes NaN past R).  A strict forward reports its exact count (_strict_read); a
    callback one records nothing.  `ticket`: the extension's (< 0 while capturing), None for the ctypes binding."""
    if mode == 2:
        if ticket is not None and ticket >= 0:
            _pending_status.append((ticket, key))
        else:
            _post(key, status, None if ticket is None else ())
        return _capacity_cache[key], (None if related is None else _last_status.get(key, _NO_STATUS)[3]), use
    if mode == 1:
        _strict_read(key, cap, rendered, related)
    return rendered, related, rendered


def compiled_forward(fn, args, device_index, P, H, W, full):
    """A one-view forward of the compiled extension, `fn` = its light_forward / full_forward / light_apply / full_apply: the policy's
    capacity and mode go in behind `args`, the forward's report (csrc/torch_ext.cpp: FwdReport) comes back in front of its tensors
    and is recorded.  `full`: the report's num_related is the variant's (the light one records none).  Returns (R for the backward,
    num_rendered and num_related to report, the tensors)."""
    key = (device_index, P, H, W)
    mode, use, cap = _binning_policy(key, P)
    (rendered, related, ticket, used, status), tensors = fn(*args, use, mode)
    rendered, related, R = record(key, mode, cap, used, rendered, status, ticket, related if full else None)
    return R, rendered, related, tensors


def strict_retry(key, cap, use, attempt, related=None):
    """Strict forwards: runs attempt(capacity) -> (its views' status words [[num_rendered, -, prefiltered violation, -], ...], a
    result) until every count fits the capacity, and records the largest count.  `related()`: the full variant's num_related,
    read once the last attempt has fit.  Returns (the views' counts, num_related or None, the last attempt's result)."""
    while True:
        words, result = attempt(use)
        if any(w[2] for w in words):
            raise_prefiltered()
        rendered = max(w[0] for w in words)
        if rendered <= use:
            break
        use = int(rendered * 1.1) + 4096  # overflow: every tile list was left empty; run again
    if related is not None:
        related = related()
    _strict_read(key, cap, rendered, related)
    return [w[0] for w in words], related, result


def run_batch(key, P, V, attempt):
    """The forward of a batch of V views of shape `key`: attempt(capacity, lazy) -> (outputs, the [V,4] status words first; the
    extension's tickets, or None).  Returns (per-view R for the backward, the outputs): a lazy or captured batch hands its backward
    the capacity its binning buffers were carved with (the views' counts are read later), a strict one the views' exact counts."""
    mode, use, cap = _binning_policy(key, P, V)
    if P == 0 or mode == 2 or torch.cuda.is_current_stream_capturing():
        out, tickets = attempt(use, mode == 2)
        if P == 0:
            return [0] * V, out
        _post(key, out[0], tickets)
        return [use] * V, out  # an upper bound of every view's count

    def strict(capacity):
        out = attempt(capacity, False)[0]
        return out[0].tolist(), out  # the one host wait of a strict batch
    R, _, out = strict_retry(key, cap, use, strict)
    return R, out
