// status.hip -- how a forward's status word reaches the host: the early status (a copy behind the binning kernels), the pooled
// status slots (posted: a copy behind an event; armed: written by the forward blend into mapped pinned memory, a tag last), the
// tile-schedule hints that ride on an armed slot's report, and the resident-scratch arm flag.  status.h is what api.hip sees.
#include "status.h"

#include <chrono>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <vector>

#include "host_util.h"
#include "options.h"

namespace dgr {
namespace {

// ---- early status (dgr_early_status_arm / _wait): num_rendered and the prefiltered flag are final after scan_blocks,
// a tenth of the way into the forward; a caller that needs them on the host (the reference's blocking copy of
// num_rendered) waits for a copy issued at that point instead of for the whole forward.
struct EarlyStatus {
    bool armed = false, pending = false;
    hipEvent_t ev = nullptr;   // an event belongs to the device that was current when it was created:
    int ev_device = -1;        // re-created when this thread moves to another device
    int* pinned = nullptr;
};
thread_local EarlyStatus g_early;
}  // namespace

int early_status_post(const int* device_status, hipStream_t st) {
    if (!g_early.armed) return DGR_OK;
    g_early.armed = false;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (!g_early.ev || g_early.ev_device != dev) {
        if (g_early.ev) HIP_TRY(hipEventDestroy(g_early.ev));
        g_early.ev = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&g_early.ev, hipEventDisableTiming));
        g_early.ev_device = dev;
    }
    if (!g_early.pinned) HIP_TRY(hipHostMalloc((void**)&g_early.pinned, 4 * sizeof(int), hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(g_early.pinned, device_status, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(g_early.ev, st));
    g_early.pending = true;
    return DGR_OK;
}

namespace {
// Waiting for a status copy that is tens of microseconds away: hipEventSynchronize parks the thread and pays a wake-up
// of the order of 100 us when the event has not fired yet (measured: a 640x480 tracking iteration went from 0.46 to
// 0.55 ms when the status moved 20 us later in the forward), so poll for a while first.
hipError_t wait_event_spinning(hipEvent_t ev) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(400)) return hipEventSynchronize(ev);
    }
}

// ---- resident backward scratch (dgr_backward_scratch_clean_arm): the next backward of this thread finds its scratch all zero and
// leaves it all zero -- no clearing launch in front of the blend backward.
thread_local bool g_scratch_clean_armed = false;
}  // namespace
bool take_scratch_clean_arm() {
    const bool armed = g_scratch_clean_armed;
    g_scratch_clean_armed = false;
    return armed;
}

namespace {

// ---- asynchronous status read-back (dgr_status_post / _poll): the lazy mode of the bindings copies a forward's status
// word to pinned host memory behind an event and looks at it one or two calls later.  Slots are pooled per device.
// Two ways to fill a slot: dgr_status_post copies a device word behind an event (any status word, after the fact);
// dgr_status_arm hands the slot to the NEXT presized forward, whose forward blend (workgroup 0, first thing) writes the word
// straight into the slot's pinned memory (mapped into the device's address space) with a tag last -- no copy, no event, nothing
// to wait for on the stream.  One device word owned by the slot (zero between forwards) gathers the frame's longest tile list.
struct StatusSlot {
    hipEvent_t ev = nullptr;
    int* pinned = nullptr;       // host int[8]: {num_rendered, overflow, prefiltered violation, num_related | tag, longest list, -, -}
    int* pinned_dev = nullptr;   // the same memory as the device sees it
    uint32_t* ws = nullptr;      // device uint32[16], zero between forwards
    int device = -1;
    bool busy = false;
    bool mapped = false;         // this use of the slot: armed (written by the kernels) rather than posted (copied)
    uint32_t tag = 0;
    int W = 0, H = 0, P = 0;     // the forward that took the arm (key of the schedule hint below)
    hipStream_t stream = nullptr;  // ... and the stream its kernels were enqueued on (dgr_status_poll watches it while it waits)
    bool enqueued = false;         // the forward's blend kernel -- which delivers the word -- has been enqueued
    bool quarantined = false;      // a poll gave this slot up (timeout, stream error) while its forward may still be queued: the
                                   // blend kernel can still write words 0-5 and its tag here, so the slot is not handed out again
                                   // before that stream has drained (status_slot_acquire)
};
std::mutex g_status_mu;
std::vector<StatusSlot> g_status_slots;
uint32_t g_status_tag = 0;
thread_local long g_armed_slot = -1;

// ---- tile schedule policy (option "tile_schedule", options.h): 1 = every forward runs tile_schedule_kernel (the blend kernels
// take their tiles classes of long lists first), 0 = never (static XCD band map), 2 (default) = by the frame: a forward whose
// status word came back through an armed slot also reports its longest tile list, and the NEXT forward of that shape
// (device, P, W, H) skips the schedule when the longest list was within 2x the mean + 32 -- on such a frame the schedule buys
// nothing (uniform synth-v1 scene: 1 % of the blend time) and costs a launch, a 1024-thread workgroup in front of the blend
// (11 us at 1080p) and some of the blend's L2 locality; a clustered frame (longest list 5x the mean) gets it back one
// forward later.  Forwards without a report (callback path, batched entry points, hipGraph capture, direct C-ABI callers that
// never arm) keep the schedule.  Results do not depend on it: only the order in which tiles are worked on.
struct SchedHint { int device, W, H, P, on, longest; };
std::vector<SchedHint> g_sched_hints;  // (under g_status_mu)
}  // namespace
bool want_schedule(int W, int H, int P) {
    const int mode = option(OPT_TILE_SCHEDULE);
    if (mode != 2) return mode != 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return true;
    std::lock_guard<std::mutex> lk(g_status_mu);
    for (const auto& h : g_sched_hints)
        if (h.device == dev && h.W == W && h.H == H && h.P == P) return h.on != 0;
    return true;
}
// The same report also sizes the binning's row segments (segment_binning.hip: segment_shift): the longest tile list of this shape's
// last reported frame, or -1 without one.  On a clustered frame the capacity alone says "16 tiles per segment" (the AVERAGE
// segment fits bin_tiles' LDS) while every segment of the cluster overflows it and takes the dense path.
int hinted_longest_list(int W, int H, int P) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    std::lock_guard<std::mutex> lk(g_status_mu);
    for (const auto& h : g_sched_hints)
        if (h.device == dev && h.W == W && h.H == H && h.P == P) return h.longest;
    return -1;
}
namespace {
void note_schedule_hint(const StatusSlot& sl, const int* word) {  // (g_status_mu held)
    const long tiles = (long)dgr::tiles_x(sl.W) * dgr::tiles_y(sl.H);
    if (tiles <= 0 || word[1] /* overflow: the lists were left empty */) return;
    const long longest = word[5];
    const int on = (longest >= 0x7fffffff || longest * tiles > 2L * word[0] + 32L * tiles) ? 1 : 0;
    const int lg = longest >= 0x7fffffff ? -1 : (int)longest;
    for (auto& h : g_sched_hints)
        if (h.device == sl.device && h.W == sl.W && h.H == sl.H && h.P == sl.P) { h.on = on; h.longest = lg; return; }
    if (g_sched_hints.size() >= 64) g_sched_hints.erase(g_sched_hints.begin());
    g_sched_hints.push_back(SchedHint{sl.device, sl.W, sl.H, sl.P, on, lg});
}

// a free slot of the current device (g_status_mu held); creates one when all are busy
long status_slot_acquire() {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    for (size_t i = 0; i < g_status_slots.size(); i++) {
        StatusSlot& c = g_status_slots[i];
        if (c.busy || c.device != dev) continue;
        if (c.quarantined) {  // (given up by a poll: reusable once the stream its forward was queued on has drained)
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(c.stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) continue;  // a query would invalidate the capture
            if (hipStreamQuery(c.stream) != hipSuccess) { (void)hipGetLastError(); continue; }
            c.quarantined = false;
        }
        return (long)i;
    }
    StatusSlot sl;
    HIP_TRY(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    HIP_TRY(hipHostMalloc((void**)&sl.pinned, 8 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
    HIP_TRY(hipHostGetDevicePointer((void**)&sl.pinned_dev, sl.pinned, 0));
    HIP_TRY(hipMalloc((void**)&sl.ws, 16 * sizeof(uint32_t)));
    HIP_TRY(hipMemset(sl.ws, 0, 16 * sizeof(uint32_t)));  // (once per slot; the kernels keep the words zero between forwards)
    for (int i = 0; i < 8; i++) sl.pinned[i] = 0;
    sl.device = dev;
    g_status_slots.push_back(sl);
    return (long)g_status_slots.size() - 1;
}

// What dgr_status_poll needs of a slot, copied out under the lock
struct SlotUse {
    hipEvent_t ev;
    int* pinned;
    bool mapped, enqueued;
    uint32_t tag;
    hipStream_t stream;
};

// A poll gives a slot up: free again, and quarantined where its forward may still be queued and write the slot later
int status_slot_give_up(long ticket, const char* why, bool quarantine) {
    std::lock_guard<std::mutex> lk(g_status_mu);
    g_status_slots[(size_t)ticket].busy = false;
    g_status_slots[(size_t)ticket].quarantined = quarantine;
    set_last_error(why);
    return DGR_ERR_HIP;
}

// The wait for the tag of an armed slot: 1 = the word is there, 0 = not yet (and `wait` == 0), < 0 = given up (the slot released).
// Poll for a while, then stop burning the core (as wait_event_spinning).  The tag comes from ONE workgroup of ONE kernel:
// if an earlier kernel of that forward faults, the device hangs or the stream was being captured when the forward was
// issued, it never arrives -- so every millisecond the stream itself is asked: an error ends the wait with that error, a
// stream that has finished all its work without the tag having been written ends it too, and so does a hard limit
// (DGR_STATUS_TIMEOUT_MS, default 30 000).
// (DGR_STATUS_TIMEOUT_MS = 0: no limit -- profiler replays and collectives' stragglers can legitimately hold a queue
//  for longer than any default)
int wait_mapped_tag(long ticket, const SlotUse& u, int wait) {
    const auto tag_here = [&] { return __atomic_load_n(u.pinned + 4, __ATOMIC_ACQUIRE) == (int)u.tag; };
    if (tag_here()) return 1;
    if (!wait) return 0;
    static const long limit_ms = [] { const char* e = getenv("DGR_STATUS_TIMEOUT_MS"); return e ? (atol(e) > 0 ? atol(e) : 0L) : 30000L; }();
    const auto t0 = std::chrono::steady_clock::now();
    auto next_query = t0 + std::chrono::milliseconds(1);
    while (!tag_here()) {
        const auto now = std::chrono::steady_clock::now();
        if (now - t0 > std::chrono::microseconds(400)) std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (now < next_query) continue;
        next_query = now + std::chrono::milliseconds(1);
        if (u.enqueued) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            const bool capturing = hipStreamIsCapturing(u.stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
            if (!capturing) {  // (a query on a capturing stream invalidates the capture)
                const hipError_t e = hipStreamQuery(u.stream);
                if (e == hipSuccess) {  // everything enqueued on the stream has completed: the tag is there, or it never will be
                    if (tag_here()) break;
                    return status_slot_give_up(ticket, "dgr_status_poll: the forward's stream is idle and its status word never arrived (was the forward "
                                                       "issued while the stream was being captured?)", false);
                }
                if (e != hipErrorNotReady) {
                    (void)status_slot_give_up(ticket, "", true);
                    return hip_fail(e, "dgr_status_poll: hipStreamQuery on the forward's stream");
                }
            }
        }
        if (limit_ms > 0 && now - t0 > std::chrono::milliseconds(limit_ms))
            return status_slot_give_up(ticket, "dgr_status_poll: timed out waiting for the forward's status word (DGR_STATUS_TIMEOUT_MS; 0 = no limit)", true);
    }
    return 1;
}
}  // namespace

// ---- the armed slot of this thread, taken by a presized forward (status.h)
ArmedReport::ArmedReport(int W, int H, int P, hipStream_t st) {
    id = g_armed_slot;
    g_armed_slot = -1;
    if (id < 0) return;
    std::lock_guard<std::mutex> lk(g_status_mu);
    StatusSlot& sl = g_status_slots[(size_t)id];
    sl.W = W; sl.H = H; sl.P = P; sl.stream = st; sl.enqueued = false;
    rep.host = sl.pinned_dev; rep.tag = sl.tag; rep.ws = sl.ws;
}
ArmedReport::~ArmedReport() {
    if (id < 0) return;
    std::lock_guard<std::mutex> lk(g_status_mu);
    StatusSlot& sl = g_status_slots[(size_t)id];
    if (handed_over) { sl.enqueued = true; return; }
    volatile int* w = sl.pinned;
    w[0] = w[1] = w[2] = w[3] = 0; w[5] = 0x7fffffff;
    w[4] = (int)sl.tag;
}

}  // namespace dgr

using namespace dgr;

extern "C" {

long dgr_status_post(void* stream, const int* device_status) {
    if (!device_status) { set_last_error("dgr_status_post: NULL"); return DGR_ERR_BAD_ARGUMENT; }
    std::lock_guard<std::mutex> lk(g_status_mu);
    const long id = status_slot_acquire();
    if (id < 0) return id;
    StatusSlot& sl = g_status_slots[(size_t)id];
    HIP_TRY(hipMemcpyAsync(sl.pinned, device_status, 4 * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipEventRecord(sl.ev, (hipStream_t)stream));
    sl.busy = true;
    sl.mapped = false;
    return id;
}

long dgr_status_arm(void) {
    std::lock_guard<std::mutex> lk(g_status_mu);
    if (g_armed_slot >= 0) {  // armed twice without a forward in between: the first arm is withdrawn
        g_status_slots[(size_t)g_armed_slot].busy = false;
        g_armed_slot = -1;
    }
    const long id = status_slot_acquire();
    if (id < 0) return id;
    StatusSlot& sl = g_status_slots[(size_t)id];
    if (++g_status_tag == 0u) ++g_status_tag;
    sl.tag = g_status_tag;
    sl.busy = true;
    sl.mapped = true;
    ((volatile int*)sl.pinned)[4] = 0;
    g_armed_slot = id;
    return id;
}

int dgr_status_poll(long ticket, int wait, int* host_status4) {
    SlotUse u;
    {
        std::lock_guard<std::mutex> lk(g_status_mu);
        if (ticket < 0 || (size_t)ticket >= g_status_slots.size() || !g_status_slots[(size_t)ticket].busy || !host_status4) {
            set_last_error("dgr_status_poll: bad ticket");
            return DGR_ERR_BAD_ARGUMENT;
        }
        if (ticket == g_armed_slot) { set_last_error("dgr_status_poll: the slot is armed and no forward has taken it"); return DGR_ERR_BAD_ARGUMENT; }
        const StatusSlot& sl = g_status_slots[(size_t)ticket];
        u = SlotUse{sl.ev, sl.pinned, sl.mapped, sl.enqueued, sl.tag, sl.stream};
    }
    if (u.mapped) {  // written by the forward blend's first workgroup, the tag last: nothing to wait for on a stream
        const int there = wait_mapped_tag(ticket, u, wait);
        if (there <= 0) return there;
        const volatile int* w = u.pinned;
        int word[8];
        for (int i = 0; i < 8; i++) word[i] = w[i];
        for (int i = 0; i < 4; i++) host_status4[i] = word[i];
        std::lock_guard<std::mutex> lk(g_status_mu);
        note_schedule_hint(g_status_slots[(size_t)ticket], word);
        g_status_slots[(size_t)ticket].busy = false;
        return 1;
    }
    if (wait) {
        HIP_TRY(wait_event_spinning(u.ev));
    } else {
        const hipError_t e = hipEventQuery(u.ev);
        if (e == hipErrorNotReady) return 0;
        if (e != hipSuccess) return hip_fail(e, "hipEventQuery");
    }
    for (int i = 0; i < 4; i++) host_status4[i] = u.pinned[i];
    std::lock_guard<std::mutex> lk(g_status_mu);
    g_status_slots[(size_t)ticket].busy = false;
    return 1;
}

int dgr_stream_is_capturing(void* stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return st == hipStreamCaptureStatusActive ? 1 : 0;
}

int dgr_backward_scratch_clean_arm(void) {
    g_scratch_clean_armed = true;
    return DGR_OK;
}

int dgr_early_status_arm(void) {
    g_early.armed = true;
    g_early.pending = false;
    return DGR_OK;
}
int dgr_early_status_wait(int* host_status4) {
    if (!host_status4) { set_last_error("dgr_early_status_wait: NULL"); return DGR_ERR_BAD_ARGUMENT; }
    if (!g_early.pending) {  // nothing was posted (P == 0, or no presized forward since arming)
        g_early.armed = false;
        host_status4[0] = host_status4[1] = host_status4[2] = host_status4[3] = 0;
        return 1;
    }
    HIP_TRY(wait_event_spinning(g_early.ev));
    for (int i = 0; i < 4; i++) host_status4[i] = g_early.pinned[i];
    g_early.pending = false;
    return DGR_OK;
}

}  // extern "C"
