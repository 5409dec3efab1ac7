// torch_support.h -- what csrc/torch_ext.cpp stands on and no variant or call path shapes: the host profile of the binding, several
// tensors over one allocation (the raw tensor windows and their guard) and the resident backward scratch.  Header-only; torch_ext.cpp
// is its one includer.
#pragma once
#include <torch/extension.h>
#include <c10/util/accumulate.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "dgr_hip.h"

namespace dgr_ext {

using at::Tensor;

[[noreturn]] inline void fail(int rc) {
    const std::string msg = dgr_last_error();
    if (rc == DGR_ERR_PREFILTERED) throw std::runtime_error("Point is filtered although prefiltered is set. This shouldn't happen!");
    if (rc == DGR_ERR_BAD_ARGUMENT) throw std::runtime_error("dgr_hip: bad argument: " + msg);
    throw std::runtime_error("dgr_hip: error " + std::to_string(rc) + ": " + msg);
}
inline void check(long rc) {
    if (rc < 0) fail((int)rc);
}

// ---- host-side profile of the binding (DGR_HOST_PROF=1; profiles/host_breakdown.py prints it): where a forward's and a
// backward's microseconds on the issuing thread go.  Off: one predictable branch per probe.
inline const bool g_host_prof = [] { const char* e = getenv("DGR_HOST_PROF"); return e && e[0] == '1'; }();
struct HostProf {
    const char* name;
    double us = 0;
    long n = 0;
};
inline HostProf g_hp[] = {{"fwd: apply() total"}, {"fwd: node forward()"}, {"fwd: core: guard + f32c"}, {"fwd: core: output allocations"},
                          {"fwd: core: status arm"}, {"fwd: core: state allocation"}, {"fwd: core: C ABI (launches)"},
                          {"fwd: save_for_backward + saved_data"}, {"bwd: node backward()"}, {"bwd: arena + scratch + dview"},
                          {"bwd: C ABI (launches)"}, {"bwd: unpack saved"}};
enum { HP_APPLY, HP_FWD, HP_PRELUDE, HP_OUT_ALLOC, HP_ARM, HP_STATE_ALLOC, HP_FWD_C, HP_SAVE, HP_BWD, HP_BWD_ALLOC, HP_BWD_C, HP_UNPACK };
struct Probe {
    int id;
    std::chrono::steady_clock::time_point t0;
    explicit Probe(int i) : id(g_host_prof ? i : -1) { if (id >= 0) t0 = std::chrono::steady_clock::now(); }
    void stop() {
        if (id < 0) return;
        g_hp[id].us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        g_hp[id].n++;
        id = -1;
    }
    ~Probe() { stop(); }
};
inline std::string host_prof_dump(bool reset) {
    std::string out;
    for (auto& h : g_hp) {
        if (h.n) out += std::string(h.name) + ": " + std::to_string(h.us / (double)h.n) + " us x " + std::to_string(h.n) + "\n";
        if (reset) { h.us = 0; h.n = 0; }
    }
    return out;
}

// ---- several tensors over ONE allocation.  A forward used to make twelve at::empty calls and a backward three plus
// sixteen narrow / view calls for the gradient arena's segments -- each a trip through the dispatcher and, for the
// allocations, the caching allocator's lock.  view_of builds the TensorImpl of a contiguous window into `base`'s storage
// directly (what as_strided does underneath, without the dispatch); byte offsets are multiples of 256.
inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
// The raw construction below was validated on PyTorch 2.10 (TensorImpl::VIEW constructor, set_sizes_contiguous, set_storage_offset,
// wrap_tensor_impl; the autograd engine's saved-tensor version check on such outputs: tests/test_hip_binding_guard.py).  Built
// against another PyTorch it is NOT used unless DGR_RAW_VIEWS=1 asks for it; DGR_RAW_VIEWS=0 switches it off anywhere; and the
// first view made in a process is checked against the dispatcher's own view of the same window (pointer, sizes, strides, dtype,
// aliasing, a fresh version counter) -- a mismatch falls back for good, with one warning.  The fall-back is at::from_blob over the
// window, its deleter holding `base`: a tensor of its own (own storage object, own version counter, not a view in autograd's
// books), like the raw one.  NOT narrow / view / as_strided: a custom Function that returns several views of one base may not have
// them edited in place at all, and views of one base share a version counter -- editing `color` would then invalidate the saved
// `opacity_map`; neither happens with the reference's separately allocated outputs.
inline Tensor dispatcher_view(const Tensor& base, size_t byte_off, c10::IntArrayRef sizes, at::ScalarType dt) {
    Tensor keep = base;
    return at::from_blob(static_cast<char*>(base.data_ptr()) + byte_off, sizes, [keep](void*) mutable { keep = Tensor(); },
                         at::TensorOptions().dtype(dt).device(base.device()));
}
inline Tensor raw_view(const Tensor& base, size_t byte_off, c10::IntArrayRef sizes, at::ScalarType dt) {
    auto impl = c10::make_intrusive<c10::TensorImpl>(c10::TensorImpl::VIEW, c10::Storage(base.storage()), base.key_set(),
                                                     c10::scalarTypeToTypeMeta(dt));
    impl->set_sizes_contiguous(sizes);
    impl->set_storage_offset((int64_t)(byte_off / c10::elementSize(dt)));
    return Tensor::wrap_tensor_impl(std::move(impl));
}
inline std::atomic<int> g_raw_views{-1};  // -1: not decided yet, 0: dispatcher views, 1: raw views
inline bool decide_raw_views(const Tensor& base, size_t byte_off, c10::IntArrayRef sizes, at::ScalarType dt) {
    const char* e = getenv("DGR_RAW_VIEWS");
    if (e && e[0] == '0') return false;
    // validated on PyTorch 2.10; later releases take the self-check below (which the first view of every process runs anyway),
    // earlier ones the dispatcher's windows unless DGR_RAW_VIEWS=1 asks for the check
#if !(defined(TORCH_VERSION_MAJOR) && (TORCH_VERSION_MAJOR > 2 || (TORCH_VERSION_MAJOR == 2 && TORCH_VERSION_MINOR >= 10)))
    if (!(e && e[0] == '1')) return false;
#endif
    bool ok = false;
    try {
        const Tensor a = raw_view(base, byte_off, sizes, dt), b = dispatcher_view(base, byte_off, sizes, dt);
        ok = a.data_ptr() == b.data_ptr() && a.sizes() == b.sizes() && a.strides() == b.strides() && a.scalar_type() == b.scalar_type() &&
             a.device() == b.device() && a.is_alias_of(base) && a._version() == 0 && a.is_contiguous() && !a.requires_grad() &&
             !a.is_view() && a.numel() == b.numel() && a.key_set() == b.key_set();
    } catch (...) {
        ok = false;
    }
    if (!ok) TORCH_WARN_ONCE("dgr_hip: the raw tensor views of csrc/torch_support.h do not behave as on the PyTorch they were validated on; "
                             "using at::from_blob windows instead");
    return ok;
}
inline Tensor view_of(const Tensor& base, size_t byte_off, c10::IntArrayRef sizes, at::ScalarType dt) {
    int mode = g_raw_views.load(std::memory_order_relaxed);
    if (mode < 0) {
        mode = decide_raw_views(base, byte_off, sizes, dt) ? 1 : 0;
        g_raw_views.store(mode, std::memory_order_relaxed);
    }
    return mode ? raw_view(base, byte_off, sizes, dt) : dispatcher_view(base, byte_off, sizes, dt);
}
inline Tensor bytes_on(const c10::Device& dev, size_t n) {
    return at::empty({(long long)std::max<size_t>(n, 1)}, at::TensorOptions().dtype(at::kByte).device(dev));
}
// One allocation carved into the given windows, in their order, each padded to a multiple of 256 bytes
struct Window {
    Tensor* t;
    c10::IntArrayRef sizes;
    at::ScalarType dt;
    size_t bytes() const { return up256(c10::elementSize(dt) * (size_t)c10::multiply_integers(sizes)); }
};
inline void carve(const c10::Device& dev, std::initializer_list<Window> windows) {
    size_t total = 0, off = 0;
    for (const Window& w : windows) total += w.bytes();
    const Tensor base = bytes_on(dev, total);
    for (const Window& w : windows) {
        *w.t = view_of(base, off, w.sizes, w.dt);
        off += w.bytes();
    }
}

// The three opaque state buffers of a presized forward as windows of one allocation (they are saved and released together).
struct StateArena {
    Tensor geom, binning, img;
    StateArena(const c10::Device& dev, int P, int W, int H, long cap) {
        const long long ng = up256(dgr_geometry_bytes(P)), ni = up256(dgr_image_bytes(W, H)), nb = up256(dgr_binning_bytes((int)cap, W, H));
        carve(dev, {{&geom, {ng}, at::kByte}, {&img, {ni}, at::kByte}, {&binning, {nb}, at::kByte}});
    }
};

// ---- resident backward scratch.  The backward's accumulator rows (64 bytes per Gaussian) must be zero when the blend
// backward starts; a fresh allocation per call needs a clearing launch in front of it.  Instead one buffer per (device,
// stream, size) is kept across calls: zero-filled when created, and every backward leaves it zero again (include/dgr_hip.h:
// dgr_backward_scratch_clean_arm -- the per-Gaussian kernel clears the rows it reads).  Calls that share a buffer run on one
// stream, i.e. in order.  Not while a hipGraph is being recorded (a replay may run on any stream, next to anything): a
// capture gets a fresh buffer and the clearing launch.  DGR_RESIDENT_SCRATCH=0 switches the cache off.
struct ScratchEntry {
    int device;
    void* stream;
    size_t bytes;
    Tensor buf;
    uint64_t stamp;
};
inline std::mutex g_scr_mu;
inline std::vector<ScratchEntry>& scratch_cache() {
    static auto* v = new std::vector<ScratchEntry>();  // never destroyed: tensors must not outlive the allocator at exit
    return *v;
}
inline uint64_t g_scr_clock = 0;
inline const bool g_resident_scratch = [] { const char* e = getenv("DGR_RESIDENT_SCRATCH"); return !(e && e[0] == '0'); }();
inline Tensor backward_scratch(const c10::Device& dev, void* stream, size_t nbytes, bool* resident) {
    *resident = false;
    if (!g_resident_scratch || dgr_stream_is_capturing(stream)) return bytes_on(dev, nbytes);
    std::lock_guard<std::mutex> lk(g_scr_mu);
    auto& c = scratch_cache();
    for (auto& e : c)
        if (e.device == dev.index() && e.stream == stream && e.bytes == nbytes) {
            e.stamp = ++g_scr_clock;
            *resident = true;
            return e.buf;
        }
    if (c.size() >= 32) {  // drop the entry used longest ago (its memory goes back to the caching allocator)
        size_t old = 0;
        for (size_t i = 1; i < c.size(); i++)
            if (c[i].stamp < c[old].stamp) old = i;
        c.erase(c.begin() + (long)old);
    }
    Tensor buf = at::zeros({(long long)std::max<size_t>(nbytes, 1)}, at::TensorOptions().dtype(at::kByte).device(dev));
    c.push_back(ScratchEntry{dev.index(), stream, nbytes, buf, ++g_scr_clock});
    *resident = true;
    return buf;
}
inline void drop_scratch(const c10::Device& dev, void* stream) {  // after a failed call the buffer's contents are unknown
    std::lock_guard<std::mutex> lk(g_scr_mu);
    auto& c = scratch_cache();
    for (size_t i = 0; i < c.size();)
        if (c[i].device == dev.index() && c[i].stream == stream) c.erase(c.begin() + (long)i); else i++;
}
// A one-view backward's C ABI call `call(scratch)` on the scratch above: armed clean when the buffer is resident, dropped when the
// call fails
template <typename Call>
void on_backward_scratch(const c10::Device& dev, void* st, size_t nscr, Call call) {
    bool resident = false;
    const Tensor scratch = backward_scratch(dev, st, nscr, &resident);
    if (resident) dgr_backward_scratch_clean_arm();
    const int rc = call((char*)scratch.data_ptr());
    if (rc < 0 && resident) drop_scratch(dev, st);
    check(rc);
}

}  // namespace dgr_ext
