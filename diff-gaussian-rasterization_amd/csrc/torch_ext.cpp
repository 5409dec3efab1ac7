// torch_ext.cpp -- compiled `_C` and compiled autograd nodes of both variants: the counterpart of the reference's pybind11 torch
// extensions (L/ext.cpp:15-19, L/rasterize_points.cu:35-256; F/ext.cpp:15-19, F/rasterize_points.cu:35-239) over the gfx950 C ABI
// (include/dgr_hip.h).
//
// torch supplies device memory, the current HIP stream and the device guard; every compute call goes through the C
// ABI in lib/libdgr_hip.so.  The Python side (dgr_amd/light.py, full.py, batch.py, batch_full.py) keeps only the policy that is
// cheap there -- the binning capacity learned per shape and the list of lazily checked status tickets (dgr_amd/_binning.py) -- and
// hands it in / gets it back as plain integers, so that a forward costs one pybind call instead of ~40 Python-level tensor
// operations and a 40-argument ctypes call (profiles/host_breakdown.py: 137 + 162 us per view in the ctypes binding).
//
// What differs between the variants is in two descriptions, `Light` and `Full`: the output set and its layout, the entry points
// and their trailing arguments, the gradient images, what a node saves beyond the common set.  Everything else is one template
// over them: forward_core, backward, Node / apply, forward_batch, backward_batch.  The host profile, the tensor windows and the
// resident backward scratch are in csrc/torch_support.h.
#include <torch/extension.h>

// (a ROCm build of torch calls its devices "cuda": the guard and stream accessors that accept them are the
// "masquerading" ones)
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPCachingAllocatorMasqueradingAsCUDA.h>

#include <array>
#include <tuple>

#include "torch_support.h"

namespace {

using namespace dgr_ext;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

// contiguous fp32 tensor on `dev` (L/rasterize_points.cu:101-125 calls .contiguous() on every input)
inline Tensor f32c(const Tensor& t, const c10::Device& dev) {
    // (an empty tensor stands for "None" and is passed on as nullptr: converting the caller's empty CPU tensor to the
    //  device would cost two dispatcher calls and an allocation per argument per call)
    if (t.numel() == 0 || (t.scalar_type() == at::kFloat && t.is_contiguous() && t.device() == dev)) return t;
    return t.to(dev, at::kFloat).contiguous();
}
// perspec_matrix: the default pose gradient reads entries 0 and 5 only (L/cr/backward.cu:725-739) -- the diagonal, which a
// transposed 4x4 (how callers usually hold Proj^T: `projection.transpose(0, 1)`) keeps in place: no copy kernel per backward
// for it.  The complete one (option "pose_grad" = 1, in effect for the calling thread) reads entries 3, 8, 9 and 11 as well,
// which the transposed storage does not hold where the kernels look: it gets the contiguous copy.
inline Tensor f32c_diag4(const Tensor& t, const c10::Device& dev) {
    if (t.scalar_type() == at::kFloat && t.device() == dev && t.dim() == 2 && t.size(0) == 4 && t.size(1) == 4 && t.stride(0) == 1 &&
        t.stride(1) == 4 && ((dgr_thread_options_effective() >> DGR_OPT_SHIFT_POSE_GRAD) & 15) != 2)
        return t;
    return f32c(t, dev);
}
// the reference's nullptr convention: an empty tensor stands for "None"
template <typename T>
inline T* ptr(const Tensor& t) {
    return t.numel() == 0 ? nullptr : t.data_ptr<T>();
}
inline char* bytes(const Tensor& t) { return t.numel() == 0 ? nullptr : reinterpret_cast<char*>(t.data_ptr()); }
inline void* stream_of(const c10::Device& dev) { return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream(); }
// row v of a [V, ...] tensor (NULL for an empty one)
inline char* row_bytes(const Tensor& t, long v) { return t.numel() == 0 ? nullptr : reinterpret_cast<char*>(t.data_ptr()) + v * t.stride(0) * t.element_size(); }
template <typename T>
inline T* row(const Tensor& t, long v) { return reinterpret_cast<T*>(row_bytes(t, v)); }
// a batch's perspec_matrix: one [4,4] for every view, or [V,4,4] (a projection per view)
inline float* perspec_row(const Tensor& t, long v) { return t.dim() == 3 ? row<float>(t, v) : ptr<float>(t); }

// PyTorch's rule for a tensor read on another stream than the one it was allocated on: tell the caching allocator, or
// the block is handed out again while that stream's kernels still read it.  A forward issued on a side stream (views in
// flight, dgr_amd.multiview.ViewStreams) does it for its inputs -- a per-view viewmatrix or gt_depth made on the
// caller's stream and dropped right after the call is the case that bites; the saved inputs are read by the backward
// on the same stream, so the one record covers both.  The ORIGINAL arguments are recorded: where f32c converts one (a
// transposed perspec_matrix is the usual case) the conversion reads it on this stream and its result is a temporary of
// this stream.  On the default stream: one comparison.
const bool g_record_inputs = [] { const char* e = getenv("DGR_RECORD_INPUT_STREAMS"); return !(e && e[0] == '0'); }();
inline void keep_until_read(const c10::Device& dev, const Tensor* const* inputs, size_t n) {
    if (!g_record_inputs) return;  // (DGR_RECORD_INPUT_STREAMS=0: the caller keeps its inputs alive until the streams are joined)
    const auto s = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index());
    if (s == c10::hip::getDefaultHIPStreamMasqueradingAsCUDA(dev.index())) return;
    for (size_t i = 0; i < n; i++)
        if (inputs[i]->defined() && inputs[i]->numel() != 0 && inputs[i]->is_cuda())
            c10::hip::HIPCachingAllocatorMasqueradingAsCUDA::recordStreamMasqueradingAsCUDA(inputs[i]->storage().data_ptr(), s);
}

struct Alloc {
    Tensor* t;
    c10::Device dev;
};
char* resize_cb(size_t n, void* user) {  // the reference's resizeFunctional (L/rasterize_points.cu:27-33)
    auto* a = static_cast<Alloc*>(user);
    *a->t = at::empty({(long long)std::max<size_t>(n, 1)}, at::TensorOptions().dtype(at::kByte).device(a->dev));
    return reinterpret_cast<char*>(a->t->data_ptr());
}
// the callback entry points take ONE user pointer for their three callbacks: three trampolines route to three tensors
struct Alloc3 {
    Alloc geom, binning, img;
};
char* cb_geom(size_t n, void* u) { return resize_cb(n, &static_cast<Alloc3*>(u)->geom); }
char* cb_binning(size_t n, void* u) { return resize_cb(n, &static_cast<Alloc3*>(u)->binning); }
char* cb_img(size_t n, void* u) { return resize_cb(n, &static_cast<Alloc3*>(u)->img); }

// ------------------------------------------------------------------------------------------------ forward
// A forward's inputs as contiguous fp32 tensors on the Gaussians' device, under its device guard (one-view forwards: one camera;
// batches: [V, ...] per camera)
inline c10::Device forward_device(const Tensor& means3D) {
    if (means3D.dim() != 2 || means3D.size(1) != 3) throw std::runtime_error("means3D must have dimensions (num_points, 3)");
    const c10::Device dev = means3D.device();
    if (!dev.is_cuda()) throw std::runtime_error("dgr_hip runs on the GPU only (no CPU path exists, as in the reference)");
    return dev;
}
struct FwdInputs {
    c10::Device dev;
    c10::hip::HIPGuardMasqueradingAsCUDA guard;
    int P, M;
    Tensor means3D, bg, colors, opacity, scales, rotations, cov3D, view, proj, campos, gt, sh;
    FwdInputs(const c10::Device& d, const Tensor& background, const Tensor& means3D_, const Tensor& colors_, const Tensor& opacity_,
              const Tensor& scales_, const Tensor& rotations_, const Tensor& cov3D_, const Tensor& view_, const Tensor& gt_,
              const Tensor& proj_, const Tensor& sh_, const Tensor& campos_)
        : dev(d), guard(d), P((int)means3D_.size(0)), means3D(f32c(means3D_, d)), bg(f32c(background, d)), colors(f32c(colors_, d)),
          opacity(f32c(opacity_, d)), scales(f32c(scales_, d)), rotations(f32c(rotations_, d)), cov3D(f32c(cov3D_, d)),
          view(f32c(view_, d)), proj(f32c(proj_, d)), campos(f32c(campos_, d)), gt(f32c(gt_, d)), sh(f32c(sh_, d)) {
        M = sh.numel() != 0 ? (int)sh.size(1) : 0;
    }
};
// The scene prefix of the forward entry points' arguments (include/dgr_hip.h), as a tuple that a call is applied to between its own
// head and tail.  `camera`: the one-view entry points' (viewmatrix, projmatrix, campos); none for the batched ones, whose cameras are
// in their per-view structs
template <typename... Camera>
inline auto scene_args(const FwdInputs& in, long degree, long W, long H, double scale_modifier, double tan_fovx, double tan_fovy,
                       bool prefiltered, Camera... camera) {
    return std::make_tuple(in.P, (int)degree, in.M, ptr<float>(in.bg), (int)W, (int)H, ptr<float>(in.means3D), ptr<float>(in.sh),
                           ptr<float>(in.colors), ptr<float>(in.opacity), ptr<float>(in.scales), (float)scale_modifier,
                           ptr<float>(in.rotations), ptr<float>(in.cov3D), camera..., (float)tan_fovx, (float)tan_fovy,
                           prefiltered ? 1 : 0);
}

// What a forward reports beside its tensors: num_rendered or -1, num_related (full) or -1, status ticket or -1, the capacity used
// and the device status word.  Python gets it first in every one-view result (dgr_amd/_binning.py: compiled_forward).
struct FwdReport {
    long rendered = -1, related = -1, ticket = -1, cap = 0;
    Tensor status;
    std::tuple<long, long, long, long, Tensor> py() const { return {rendered, related, ticket, cap, status}; }
};
using PyForward = std::tuple<std::tuple<long, long, long, long, Tensor>, std::vector<Tensor>>;
// ... and its tensors; a variant leaves those it does not have undefined (`unc`: the light variant's gau_uncertainty [P,1], the
// full one's uncertainty image)
struct Fwd : FwdReport {
    Tensor color, depth, median, var, alpha, unc, radii, px, geom, binning, img;
};

// mode: 0 = callback entry point (the strict mirror: allocation callbacks + the reference's blocking read),
//       1 = presized, strict: one host wait until num_rendered is known; retries a too-small capacity itself,
//       2 = presized, lazy: no host synchronisation; returns a status ticket (dgr_status_post) or -1 while capturing.
// Modes 1 and 2 around `run(cap)`: the state allocation and the variant's presized entry point.  The forward reports through an
// armed status slot (pinned host memory written by the forward blend's first workgroup, include/dgr_hip.h: dgr_status_arm): no
// copy, no event.  Strict mode's one host wait polls that memory -- the reference's blocking copy of num_rendered
// (L/cuda_rasterizer/rasterizer_impl.cu:287) without the copy and the wake-up, and with the longest-list report that lets the next
// forward of the shape skip the tile schedule.  While a hipGraph is recorded nothing can be read back: no slot is armed, and
// strict mode, whose wait would never end, cannot be captured.
template <typename Run>
void presized_forward(Run& run, long capacity, long mode, void* st, FwdReport& o) {
    const bool capturing = dgr_stream_is_capturing(st);
    if (capturing && mode != 2)
        throw std::runtime_error("strict status mode (one host wait per forward) cannot run while its stream is being captured into a "
                                 "hipGraph: use the lazy mode (DGR_SYNC_MODE=lazy), after a few eager forwards of the same shape");
    for (long cap = capacity;;) {
        long ticket = -1;
        {
            Probe p_arm(HP_ARM);
            if (!capturing) check(ticket = dgr_status_arm());
        }
        try {
            run(cap);
        } catch (...) {
            int unused[4];
            if (ticket >= 0) (void)dgr_status_poll(ticket, 1, unused);  // (completed by the library: releases the slot)
            throw;
        }
        o.cap = cap;
        if (mode == 2) {
            o.ticket = ticket;
            return;
        }
        int s[4] = {0, 0, 0, 0};
        check(dgr_status_poll(ticket, 1, s));  // the one host wait of this forward: until num_rendered is known
        if (s[2]) throw std::runtime_error("Point is filtered although prefiltered is set. This shouldn't happen!");
        o.rendered = s[0];
        if (o.rendered <= cap) return;
        cap = (long)(o.rendered * 1.1) + 4096;  // overflow: every tile list was left empty; run again
    }
}

// ------------------------------------------------------------------------------------------------ backward, what the variants share
// absgrad: a backward's tenth result, the absolute screen-space gradient [P,3] -- or, for a batch of V views, every view's
// [V,P,3] (every row written) -- and the per-view output pointers; neither when `on` is false.
struct AbsGrad {
    Tensor t;
    float* view[DGR_MAX_BATCH_VIEWS] = {};
    AbsGrad(bool on, const Tensor& means3D, long V) {
        if (!on) return;
        const long P = means3D.size(0);
        const auto f32 = at::TensorOptions().dtype(at::kFloat).device(means3D.device());
        t = V ? at::empty({V, P, 3}, f32) : at::empty({P, 3}, f32);
        for (long v = 0; v < std::max(V, 1L) && v < DGR_MAX_BATCH_VIEWS && P > 0; v++) view[v] = row<float>(t, v);
    }
    float* const* views() const { return t.defined() ? view : nullptr; }
};

// The flat arena of the eight per-Gaussian gradients (dgr_amd.light._grad_arena): segments in the order means3D, means2D,
// sh, opacity, scales, rotations | cov3D, colors, 256-byte aligned; the first six are one contiguous span = the multi-GPU
// all-reduce payload.  g[] receives them in the return order of the reference binding: means2D, colors, opacity, means3D,
// cov3D, sh, scales, rotations.  Every row is written by the kernels (zeros for invisible Gaussians; M > 16: api.hip clears dL_dsh
// first): no zero-fill.  The two trailing segments are carved only on demand (want_cov3D, want_colors): a caller without a
// cov3D_precomp / colors_precomp leaf has no use for them, g[4] / g[1] then stay undefined and gp[4] / gp[1] NULL, and the
// per-Gaussian backward -- every dense output of which may be NULL -- does not write the 24 + 12 bytes per Gaussian.
inline void grad_arena(const c10::Device& dev, int P, int M, Tensor* g, float** gp, bool want_colors = true, bool want_cov3D = true) {
    const int64_t s3[] = {P, 3}, ssh[] = {P, M, 3}, s1[] = {P, 1}, s4[] = {P, 4}, s6[] = {P, 6};  // (a Window refers to its sizes)
    const Window w[8] = {{&g[3], s3, at::kFloat}, {&g[0], s3, at::kFloat}, {&g[5], ssh, at::kFloat}, {&g[2], s1, at::kFloat},
                         {&g[6], s3, at::kFloat}, {&g[7], s4, at::kFloat}, {&g[4], s6, at::kFloat}, {&g[1], s3, at::kFloat}};
    if (want_colors && want_cov3D) carve(dev, {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]});
    else if (want_cov3D) carve(dev, {w[0], w[1], w[2], w[3], w[4], w[5], w[6]});
    else if (want_colors) carve(dev, {w[0], w[1], w[2], w[3], w[4], w[5], w[7]});
    else carve(dev, {w[0], w[1], w[2], w[3], w[4], w[5]});
    for (int i = 0; i < 8; i++) gp[i] = g[i].defined() ? ptr<float>(g[i]) : nullptr;
}

// What a backward reads of its forward, FwdInputs' counterpart: the saved inputs as contiguous fp32 tensors on the Gaussians' device,
// under its device guard, and the forward's own tensors as they are (one view: one camera; batches: [V, ...] per camera)
struct BwdScene {
    c10::Device dev;
    c10::hip::HIPGuardMasqueradingAsCUDA guard;
    int P, M, degree;
    float scale_modifier, tan_fovx, tan_fovy;
    Tensor means3D, bg, colors, scales, rotations, cov3D, view, proj, campos, gt, sh, perspec;
    const Tensor &radii, &geom, &binning, &img, &perspec_arg;
    BwdScene(const Tensor& background, const Tensor& means3D_, const Tensor& radii_, const Tensor& colors_, const Tensor& scales_,
             const Tensor& rotations_, double scale_modifier_, const Tensor& cov3D_, const Tensor& view_, const Tensor& proj_,
             double tan_fovx_, double tan_fovy_, const Tensor& gt_, const Tensor& sh_, long degree_, const Tensor& campos_,
             const Tensor& geom_, const Tensor& binning_, const Tensor& img_, const Tensor& perspec_)
        : dev(means3D_.device()), guard(dev), P((int)means3D_.size(0)), degree((int)degree_), scale_modifier((float)scale_modifier_),
          tan_fovx((float)tan_fovx_), tan_fovy((float)tan_fovy_), means3D(f32c(means3D_, dev)), bg(f32c(background, dev)),
          colors(f32c(colors_, dev)), scales(f32c(scales_, dev)), rotations(f32c(rotations_, dev)), cov3D(f32c(cov3D_, dev)),
          view(f32c(view_, dev)), proj(f32c(proj_, dev)), campos(f32c(campos_, dev)), gt(f32c(gt_, dev)), sh(f32c(sh_, dev)),
          perspec(f32c_diag4(perspec_, dev)), radii(radii_), geom(geom_), binning(binning_), img(img_), perspec_arg(perspec_) {
        M = sh.numel() != 0 ? (int)sh.size(1) : 0;
    }
};
// the light variant's switches of a backward (the full one has none)
struct BwdFlags {
    bool debug = false, track_off = false, map_off = false;
};

// A batch backward's results: g[1..7] the arena's seven sums (gp[1..7]: their pointers; none without need_gaussian_grads), g[0]
// every view's dL_dmeans2D [V,P,3] (need_means2D) or None, g[8] dL_dview [V,4,4]; and V scratch rows of nscr bytes
struct BatchBwdOut {
    std::vector<Tensor> g = std::vector<Tensor>(9);
    float* gp[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    Tensor scratch;
    size_t nscr;
    BatchBwdOut(const c10::Device& dev, int P, int M, long V, long W, long H, bool need_gaussian_grads, bool need_means2D,
                const std::vector<long>& num_rendered) {
        const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
        if (need_gaussian_grads) {
            grad_arena(dev, P, M, g.data(), gp);
            g[0].zero_();  // the arena's one-view means2D slot: a batch returns those gradients per view, beside the arena
            g[0] = need_means2D ? at::empty({V, P, 3}, f32) : Tensor();
        }
        g[8] = at::empty({V, 4, 4}, f32);
        // (deterministic_grads: + 64 bytes per tile instance of the view with the most of them; the views' rows are equally long)
        long rmax = 0;
        for (long r : num_rendered) rmax = std::max(rmax, r);
        nscr = std::max<size_t>(up256(dgr_light_backward_scratch_bytes_r(P, (int)W, (int)H, (int)rmax)), 256);
        scratch = at::empty({V, (long long)nscr}, at::TensorOptions().dtype(at::kByte).device(dev));
    }
    float* dmean2D(long v) const { return g[0].defined() ? row<float>(g[0], v) : nullptr; }
};
inline int rendered_of(const std::vector<long>& num_rendered, long v) { return (size_t)v < num_rendered.size() ? (int)num_rendered[v] : 0; }

// The tensors a node saves, by name: the common set (L/__init__.py:101-102, F/__init__.py:89-90, + the settings' tensors, which the
// Python Functions read from ctx.raster_settings), then a variant's own from S_COMMON on
enum Saved { S_COLORS, S_MEANS3D, S_SCALES, S_ROTATIONS, S_COV3D, S_VIEW, S_RADII, S_SH, S_GEOM, S_BINNING, S_IMG, S_GT, S_BG, S_PROJ,
             S_CAMPOS, S_PERSPEC, S_COMMON };

// ------------------------------------------------------------------------------------------------ the two variants
// Each description holds what differs and nothing else.  Gradient images go to a backward as an array of N_IMAGES tensors indexed by
// the variant's enum: GC, GD (colour, depth) and SIL (the exact silhouette gradient image, option "silhouette_grad"; empty: none) in
// both.  gp[] of a backward: [0] means2D [1] colors [2] opacity [3] means3D [4] cov3D [5] sh [6] scales [7] rotations.
struct Light {
    enum { GC, GD, GM, GV, SIL, ALPHAS, N_IMAGES };  // + the median depth's and the depth variance's; the forward's alpha image rides along
    using Images = std::array<Tensor, N_IMAGES>;
    using View = dgr_light_view;
    using ViewGrad = dgr_light_view_grad;
    enum { S_ALPHA = S_COMMON, N_SAVED };
    static constexpr bool tracking_flags = true;  // the settings carry track_off / map_off
    // dL_dview is [1,4,4]: the reference binding returns a per-pixel [H*W,4,4] buffer that L/__init__.py:160-161 sums over dim 0;
    // one already-reduced "pixel" keeps that code working
    static constexpr bool dview_leading_one = true;

    // allocation 1: the five images (every pixel is written by the blend kernel); allocation 2: radii (written for every
    // Gaussian), the two median statistics (cleared by the kernels) and the status word
    static void outputs(Fwd& o, const c10::Device& dev, int P, long H, long W) {
        carve(dev, {{&o.color, {3, H, W}, at::kFloat}, {&o.depth, {1, H, W}, at::kFloat}, {&o.median, {1, H, W}, at::kFloat},
                    {&o.var, {1, H, W}, at::kFloat}, {&o.alpha, {1, H, W}, at::kFloat}});
        carve(dev, {{&o.radii, {P}, at::kInt}, {&o.unc, {P, 1}, at::kFloat}, {&o.px, {P, 1}, at::kInt}, {&o.status, {4}, at::kInt}});
    }
    static auto output_args(const Fwd& o, const Tensor& gt) {
        return std::make_tuple(ptr<float>(o.color), ptr<float>(o.depth), ptr<float>(o.median), ptr<float>(o.alpha), ptr<float>(gt),
                               ptr<float>(o.var), ptr<float>(o.unc), ptr<int>(o.px), ptr<int>(o.radii));
    }
    template <typename Args>
    static int forward(const Args& args, bool debug, long&) {
        return std::apply([&](auto... a) { return dgr_light_forward(a..., debug ? 1 : 0); }, args);
    }
    template <typename Args>
    static int forward_presized(const Args& args) {
        return std::apply([](auto... a) { return dgr_light_forward_presized(a...); }, args);
    }
    static void after_strict(Fwd&, void* st, bool debug, bool) {
        if (debug) check(hipStreamSynchronize((hipStream_t)st) == hipSuccess ? 0 : DGR_ERR_HIP);
    }
    // the `_C.rasterize_gaussians` tuple (L/rasterize_points.cu:35-129) behind num_rendered
    static std::vector<Tensor> forward_tensors(const Fwd& o) {
        return {o.color, o.depth, o.median, o.var, o.alpha, o.radii, o.geom, o.binning, o.img, o.unc, o.px};
    }

    // L/rasterize_points.cu:131-236.  Median and variance gradients that are absent stay NULL: the lean blend backward
    static int backward(void* st, const BwdScene& s, const Images& im, long W, long H, long R, float* const* gp, float* dview,
                        BwdFlags f, bool need_gaussian_grads, char* scratch, size_t nscr, float* abs) {
        // (without per-Gaussian gradients nobody reads the per-Gaussian sums: the blend kernel forms the three pose sums only)
        const bool map_off = f.map_off || !need_gaussian_grads;
        return dgr_light_backward_silhouette(
            st, s.P, s.degree, s.M, (int)R, ptr<float>(s.bg), (int)W, (int)H, ptr<float>(s.means3D), ptr<float>(s.sh),
            ptr<float>(s.colors), ptr<float>(im[ALPHAS]), ptr<float>(s.scales), s.scale_modifier, ptr<float>(s.rotations),
            ptr<float>(s.cov3D), ptr<float>(s.view), ptr<float>(s.proj), ptr<float>(s.campos), s.tan_fovx, s.tan_fovy, ptr<int>(s.radii),
            bytes(s.geom), bytes(s.binning), bytes(s.img), ptr<float>(im[GC]), ptr<float>(im[GD]), ptr<float>(im[GM]), ptr<float>(im[GV]),
            gp[0], nullptr, gp[2], gp[1], nullptr, gp[3], gp[4], gp[5], gp[6], gp[7], f.debug ? 1 : 0, nullptr, ptr<float>(s.perspec),
            dview, nullptr, ptr<float>(s.gt), f.track_off ? 1 : 0, map_off ? 1 : 0, scratch, nscr, abs, ptr<float>(im[SIL]));
    }

    // the node (L/__init__.py:46-176): outputs, the extra saved tensor, the gradient images of its backward
    static variable_list node_outputs(const Fwd& o) { return {o.color, o.radii, o.depth, o.median, o.var, o.alpha, o.unc, o.px}; }
    // four of the eight outputs (radii, opacity_map, gau_uncertainty, gau_related_pixels) have no gradient input in the
    // backward -- opacity_map has one with the option "silhouette_grad"
    static variable_list non_differentiable(const Fwd& o) { return {o.radii, o.px}; }
    static void save_extra(variable_list& sv, const Fwd& o) { sv[S_ALPHA] = o.alpha; }
    // (no gradient image for the median depth / the depth variance: undefined, NULL at the C ABI -- no zero images are made, filled
    //  and read.  The opacity_map gradient is the silhouette image when the option was on at the forward; unused, or the option off: none)
    static std::array<const Tensor*, N_IMAGES> node_images(const Tensor& gC, const Tensor& gD, const variable_list& grad,
                                                          const variable_list& sv, bool silhouette, const Tensor& none) {
        return {&gC, &gD, &grad[3], &grad[4], silhouette ? &grad[5] : &none, &sv[S_ALPHA]};
    }

    // dgr_amd.batch: [V,...] outputs, one struct of pointers per view
    static void batch_outputs(Fwd& o, long V, int P, long H, long W, const at::TensorOptions& f32, const at::TensorOptions& i32) {
        o.color = at::empty({V, 3, H, W}, f32); o.depth = at::empty({V, 1, H, W}, f32); o.median = at::empty({V, 1, H, W}, f32);
        o.var = at::empty({V, 1, H, W}, f32); o.alpha = at::empty({V, 1, H, W}, f32);
        o.radii = P ? at::empty({V, P}, i32) : at::zeros({V, P}, i32);
        o.unc = P ? at::empty({V, P, 1}, f32) : at::zeros({V, P, 1}, f32);
        o.px = P ? at::empty({V, P, 1}, i32) : at::zeros({V, P, 1}, i32);
    }
    static View view(long v, int capacity, const Fwd& o, const FwdInputs& in) {
        return View{row_bytes(o.geom, v), row_bytes(o.binning, v), capacity, row_bytes(o.img, v), row<int>(o.status, v),
                    row<float>(in.view, v), row<float>(in.proj, v), row<float>(in.campos, v), row<float>(o.color, v),
                    row<float>(o.depth, v), row<float>(o.median, v), row<float>(o.alpha, v), row<float>(in.gt, v),
                    row<float>(o.var, v), row<float>(o.unc, v), row<int>(o.px, v), row<int>(o.radii, v)};
    }
    template <typename... A>
    static int forward_batch(A... a) { return dgr_light_forward_batch(a...); }
    static std::vector<Tensor> batch_tensors(const Fwd& o) {
        return {o.status, o.color, o.depth, o.median, o.var, o.alpha, o.radii, o.geom, o.binning, o.img, o.unc, o.px};
    }
    static ViewGrad view_grad(long v, const BwdScene& s, const Images& im, const BatchBwdOut& o, int rendered) {
        return ViewGrad{row_bytes(s.geom, v), row_bytes(s.binning, v), row_bytes(s.img, v), row<float>(s.view, v), row<float>(s.proj, v),
                        row<float>(s.campos, v), perspec_row(s.perspec, v), row<float>(im[ALPHAS], v), row<float>(s.gt, v),
                        row<int>(s.radii, v), row<float>(im[GC], v), row<float>(im[GD], v), row<float>(im[GM], v), row<float>(im[GV], v),
                        o.dmean2D(v), row<float>(o.g[8], v), row_bytes(o.scratch, v), o.nscr, rendered};
    }
    static int backward_batch(void* st, int V, const ViewGrad* w, const BwdScene& s, long W, long H, float* const* gp, BwdFlags f,
                              bool need_gaussian_grads, float* const* abs, const float* const* sil) {
        const bool map_off = f.map_off || !need_gaussian_grads;  // (as Light::backward)
        return dgr_light_backward_batch_silhouette(st, V, w, s.P, s.degree, s.M, ptr<float>(s.bg), (int)W, (int)H, ptr<float>(s.means3D),
                                                   ptr<float>(s.sh), ptr<float>(s.colors), ptr<float>(s.scales), s.scale_modifier,
                                                   ptr<float>(s.rotations), ptr<float>(s.cov3D), s.tan_fovx, s.tan_fovy, gp[2], gp[1],
                                                   gp[3], gp[4], gp[5], gp[6], gp[7], f.track_off ? 1 : 0, map_off ? 1 : 0, abs, sil);
    }
};

struct Full {
    enum { GC, GD, GU, SIL, N_IMAGES };  // + the uncertainty image's, in the reference's variance form
    using Images = std::array<Tensor, N_IMAGES>;
    using View = dgr_full_view;
    using ViewGrad = dgr_full_view_grad;
    enum { N_SAVED = S_COMMON };
    static constexpr bool tracking_flags = false;
    static constexpr bool dview_leading_one = false;  // dL_dview is [4,4]

    static void outputs(Fwd& o, const c10::Device& dev, int P, long H, long W) {
        carve(dev, {{&o.color, {3, H, W}, at::kFloat}, {&o.depth, {1, H, W}, at::kFloat}, {&o.unc, {1, H, W}, at::kFloat}});
        carve(dev, {{&o.radii, {P}, at::kInt}, {&o.status, {4}, at::kInt}});  // (radii: written for every Gaussian by preprocess_fwd)
    }
    static auto output_args(const Fwd& o, const Tensor& gt) {
        return std::make_tuple(ptr<float>(o.color), ptr<float>(o.depth), ptr<float>(gt), ptr<float>(o.unc), ptr<int>(o.radii));
    }
    template <typename Args>
    static int forward(const Args& args, bool, long& related) {
        int ng = 0;
        const int rc = std::apply([&](auto... a) { return dgr_full_forward(a..., &ng); }, args);
        related = ng;
        return rc;
    }
    template <typename Args>
    static int forward_presized(const Args& args) {
        return std::apply([](auto... a) { return dgr_full_forward_presized(a...); }, args);
    }
    // num_related (the reference's NG) is produced by the forward blend: the reference's second blocking read
    // (F/cuda_rasterizer/rasterizer_impl.cu:498) -- a wait for the whole forward.  The `_C.rasterize_gaussians` mirror returns the
    // number, as the reference's does; the autograd node does not wait for it: NG only sizes the reference's pair lists in ITS
    // backward (F/__init__.py:91,100,130), which this backward does not have (csrc/render_full.hip), and no caller of
    // GaussianRasterizer.forward ever sees it.  The strict forward then returns as soon as num_rendered is known, the blend
    // still running (config 2, one view at a time in the default mode: 0.205 -> 0.17 ms).
    static void after_strict(Fwd& o, void*, bool, bool want_related) {
        if (want_related) o.related = o.status.to(at::kCPU).data_ptr<int>()[3];
    }
    // the `_C.rasterize_gaussians` tuple (F/rasterize_points.cu:35-120) behind num_rendered and num_related
    static std::vector<Tensor> forward_tensors(const Fwd& o) { return {o.color, o.depth, o.unc, o.radii, o.geom, o.binning, o.img}; }

    // F/rasterize_points.cu:122-239.  im[GU] keeps the reference's variance form (the bindings pass none there when the option
    // "silhouette_grad" is on)
    static int backward(void* st, const BwdScene& s, const Images& im, long W, long H, long R, float* const* gp, float* dview, BwdFlags,
                        bool, char* scratch, size_t nscr, float* abs) {
        return dgr_full_backward_silhouette(
            st, s.P, s.degree, s.M, (int)R, ptr<float>(s.bg), (int)W, (int)H, ptr<float>(s.means3D), ptr<float>(s.sh),
            ptr<float>(s.colors), ptr<float>(s.scales), s.scale_modifier, ptr<float>(s.rotations), ptr<float>(s.cov3D), ptr<float>(s.view),
            ptr<float>(s.proj), ptr<float>(s.campos), s.tan_fovx, s.tan_fovy, ptr<int>(s.radii), bytes(s.geom), bytes(s.binning),
            bytes(s.img), ptr<float>(im[GC]), ptr<float>(im[GD]), gp[0], nullptr, gp[2], gp[1], gp[3], gp[4], gp[5], gp[6], gp[7], nullptr,
            nullptr, nullptr, nullptr, nullptr, ptr<float>(s.perspec), nullptr, nullptr, nullptr, dview, nullptr, nullptr, nullptr,
            ptr<float>(s.gt), ptr<float>(im[GU]), scratch, nscr, abs, ptr<float>(im[SIL]));
    }

    // the node (F/__init__.py:46-151)
    static variable_list node_outputs(const Fwd& o) { return {o.color, o.radii, o.depth, o.unc}; }
    static variable_list non_differentiable(const Fwd& o) { return {o.radii}; }
    static void save_extra(variable_list&, const Fwd&) {}
    // (no gradient image for the uncertainty output: undefined, NULL at the C ABI, which then runs the lean blend backward.  Option
    //  "silhouette_grad" at the forward: that gradient is the exact silhouette image, and dL_duncertainties NULL -- the lean kernel)
    static std::array<const Tensor*, N_IMAGES> node_images(const Tensor& gC, const Tensor& gD, const variable_list& grad,
                                                          const variable_list&, bool silhouette, const Tensor& none) {
        return {&gC, &gD, silhouette ? &none : &grad[3], silhouette ? &grad[3] : &none};
    }

    // dgr_amd.batch_full
    static void batch_outputs(Fwd& o, long V, int P, long H, long W, const at::TensorOptions& f32, const at::TensorOptions& i32) {
        o.color = at::empty({V, 3, H, W}, f32); o.depth = at::empty({V, 1, H, W}, f32); o.unc = at::empty({V, 1, H, W}, f32);
        o.radii = P ? at::empty({V, P}, i32) : at::zeros({V, P}, i32);
    }
    static View view(long v, int capacity, const Fwd& o, const FwdInputs& in) {
        return View{row_bytes(o.geom, v), row_bytes(o.binning, v), capacity, row_bytes(o.img, v), row<int>(o.status, v),
                    row<float>(in.view, v), row<float>(in.proj, v), row<float>(in.campos, v), row<float>(o.color, v),
                    row<float>(o.depth, v), row<float>(in.gt, v), row<float>(o.unc, v), row<int>(o.radii, v)};
    }
    template <typename... A>
    static int forward_batch(A... a) { return dgr_full_forward_batch(a...); }
    static std::vector<Tensor> batch_tensors(const Fwd& o) { return {o.status, o.color, o.depth, o.unc, o.radii, o.geom, o.binning, o.img}; }
    static ViewGrad view_grad(long v, const BwdScene& s, const Images& im, const BatchBwdOut& o, int rendered) {
        // an undefined or empty dL_dout_unc: no view's loss used the uncertainty image (the lean blend backward)
        const bool lean = !im[GU].defined() || im[GU].numel() == 0;
        return ViewGrad{row_bytes(s.geom, v), row_bytes(s.binning, v), row_bytes(s.img, v), row<float>(s.view, v), row<float>(s.proj, v),
                        row<float>(s.campos, v), perspec_row(s.perspec, v), row<float>(s.gt, v), row<int>(s.radii, v), row<float>(im[GC], v),
                        row<float>(im[GD], v), lean ? nullptr : row<float>(im[GU], v), o.dmean2D(v), row<float>(o.g[8], v),
                        row_bytes(o.scratch, v), o.nscr, rendered};
    }
    static int backward_batch(void* st, int V, const ViewGrad* w, const BwdScene& s, long W, long H, float* const* gp, BwdFlags, bool,
                              float* const* abs, const float* const* sil) {
        return dgr_full_backward_batch_silhouette(st, V, w, s.P, s.degree, s.M, ptr<float>(s.bg), (int)W, (int)H, ptr<float>(s.means3D),
                                                  ptr<float>(s.sh), ptr<float>(s.colors), ptr<float>(s.scales), s.scale_modifier,
                                                  ptr<float>(s.rotations), ptr<float>(s.cov3D), s.tan_fovx, s.tan_fovy, gp[2], gp[1], gp[3],
                                                  gp[4], gp[5], gp[6], gp[7], abs, sil);
    }
};

// ------------------------------------------------------------------------------------------------ one view
// `debug` (light): passed to the callback entry point, and a strict forward ends with a stream synchronise; `want_related` (full):
// a strict forward reads num_related back (Full::after_strict).
template <class V>
Fwd forward_core(const Tensor& background, const Tensor& means3D_, const Tensor& colors_, const Tensor& opacity_, const Tensor& scales_,
                 const Tensor& rotations_, double scale_modifier, const Tensor& cov3D_, const Tensor& viewmatrix_, const Tensor& gt_depth_,
                 const Tensor& projmatrix_, double tan_fovx, double tan_fovy, long H, long W, const Tensor& sh_, long degree,
                 const Tensor& campos_, bool prefiltered, bool debug, long capacity, long mode, bool want_related) {
    Probe p_pre(HP_PRELUDE);
    const FwdInputs in(forward_device(means3D_), background, means3D_, colors_, opacity_, scales_, rotations_, cov3D_, viewmatrix_,
                       gt_depth_, projmatrix_, sh_, campos_);
    const c10::Device dev = in.dev;
    const int P = in.P;
    const Tensor* const inputs[] = {&means3D_, &background, &colors_, &opacity_, &scales_, &rotations_, &cov3D_, &viewmatrix_, &projmatrix_,
                                    &campos_, &gt_depth_, &sh_};
    keep_until_read(dev, inputs, std::size(inputs));
    const auto u8 = at::TensorOptions().dtype(at::kByte).device(dev);
    p_pre.stop();
    Probe p_out(HP_OUT_ALLOC);
    Fwd o;
    V::outputs(o, dev, P, H, W);  // allocations 1 and 2
    void* st = stream_of(dev);
    const auto args = std::tuple_cat(scene_args(in, degree, W, H, scale_modifier, tan_fovx, tan_fovy, prefiltered, ptr<float>(in.view),
                                                ptr<float>(in.proj), ptr<float>(in.campos)), V::output_args(o, in.gt));
    p_out.stop();

    if (mode == 0 || P == 0) {
        o.geom = at::empty({0}, u8); o.binning = at::empty({0}, u8); o.img = at::empty({0}, u8);
        Alloc3 al{{&o.geom, dev}, {&o.binning, dev}, {&o.img, dev}};
        const int rc = V::forward(std::tuple_cat(std::make_tuple(st, cb_geom, cb_binning, cb_img, &al), args), debug, o.related);
        check(rc);
        o.rendered = o.cap = rc;
        return o;
    }
    auto run = [&](long cap) {
        Probe p_st(HP_STATE_ALLOC);
        const StateArena sa(dev, P, (int)W, (int)H, cap);  // allocation 3
        o.geom = sa.geom; o.binning = sa.binning; o.img = sa.img;
        p_st.stop();
        Probe p_c(HP_FWD_C);
        check(V::forward_presized(std::tuple_cat(std::make_tuple(st, (char*)o.geom.data_ptr(), (char*)o.binning.data_ptr(), (int)cap,
                                                                 (char*)o.img.data_ptr(), o.status.data_ptr<int>()), args)));
    };
    presized_forward(run, capacity, mode, st, o);
    if (mode != 2) V::after_strict(o, st, debug, want_related);
    return o;
}

// The `_C.rasterize_gaussians` of a variant plus the policy values the Python side keeps: (the report, V::forward_tensors)
template <class V>
PyForward forward(const Tensor& background, const Tensor& means3D, const Tensor& colors, const Tensor& opacity, const Tensor& scales,
                  const Tensor& rotations, double scale_modifier, const Tensor& cov3D, const Tensor& viewmatrix, const Tensor& gt_depth,
                  const Tensor& projmatrix, double tan_fovx, double tan_fovy, long H, long W, const Tensor& sh, long degree,
                  const Tensor& campos, bool prefiltered, bool debug, long capacity, long mode) {
    const Fwd o = forward_core<V>(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D, viewmatrix, gt_depth,
                                  projmatrix, tan_fovx, tan_fovy, H, W, sh, degree, campos, prefiltered, debug, capacity, mode,
                                  /*want_related=*/true);
    return {o.py(), V::forward_tensors(o)};
}

// Returns (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dL_dview -- light
// [1,4,4], full [4,4]); the first eight are windows of one flat arena (grad_arena above), or undefined tensors (None) when
// need_gaussian_grads is false (tracking: the library then skips every dense per-Gaussian row).  `images`: the variant's gradient
// images as the caller holds them.  absgrad (dgr_*_backward_absgrad): a tenth result, the [P,3] absolute screen-space gradient.
// R: the forward's num_rendered, or a lazy forward's capacity.  want_colors / want_cov3D: false leaves dL_dcolors / dL_dcov3D out
// (undefined, NULL to the library: grad_arena) -- the autograd nodes' rule for a caller without that leaf; the mirrors of the
// reference binding below always return all eight.
template <class V>
std::vector<Tensor> backward(const BwdScene& s, const std::array<const Tensor*, V::N_IMAGES>& images, long R, BwdFlags flags,
                             bool need_gaussian_grads, bool absgrad, bool want_colors = true, bool want_cov3D = true) {
    AbsGrad abs(absgrad, s.means3D, 0);
    const c10::Device dev = s.dev;
    const long H = images[V::GC]->size(1), W = images[V::GC]->size(2);
    typename V::Images im;
    for (size_t i = 0; i < im.size(); i++) im[i] = f32c(*images[i], dev);
    // (the forward recorded the saved inputs; the gradient images of a graph root are whatever the caller passed in)
    const Tensor* recorded[V::N_IMAGES + 1];
    *std::copy(images.begin(), images.end(), recorded) = &s.perspec_arg;
    keep_until_read(dev, recorded, std::size(recorded));
    Probe p_al(HP_BWD_ALLOC);
    std::vector<Tensor> g(9);
    float* gp[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (need_gaussian_grads) grad_arena(dev, s.P, s.M, g.data(), gp, want_colors, want_cov3D);
    // scratch: accumulator rows, cleared by the backward's first launch
    // (with the option "deterministic_grads" the scratch also holds 64 bytes per tile instance)
    const size_t nscr = up256(dgr_light_backward_scratch_bytes_r(s.P, (int)W, (int)H, (int)R));
    void* st = stream_of(dev);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    g[8] = V::dview_leading_one ? at::empty({1, 4, 4}, f32) : at::empty({4, 4}, f32);
    on_backward_scratch(dev, st, nscr, [&](char* scratch) {
        p_al.stop();
        Probe p_bc(HP_BWD_C);
        return V::backward(st, s, im, W, H, R, gp, g[8].data_ptr<float>(), flags, need_gaussian_grads, scratch, nscr, abs.view[0]);
    });
    if (absgrad) g.push_back(std::move(abs.t));
    return g;
}

// The reference's `_C.rasterize_gaussians_backward` signatures.  dL_dout_alpha / dL_dout_sil: the silhouette image [1,H,W], or
// undefined / empty (NULL)
std::vector<Tensor> light_backward(const Tensor& background, const Tensor& means3D, const Tensor& radii, const Tensor& colors,
                                   const Tensor& scales, const Tensor& rotations, double scale_modifier, const Tensor& cov3D,
                                   const Tensor& viewmatrix, const Tensor& projmatrix, double tan_fovx, double tan_fovy,
                                   const Tensor& dL_dout_color, const Tensor& dL_dout_depth, const Tensor& dL_dout_median,
                                   const Tensor& dL_dout_var, const Tensor& gt_depth, const Tensor& sh, long degree, const Tensor& campos,
                                   const Tensor& geomBuffer, long R, const Tensor& binningBuffer, const Tensor& imageBuffer,
                                   const Tensor& alphas, bool debug, const Tensor& perspec, bool track_off, bool map_off,
                                   bool need_gaussian_grads, const Tensor& dL_dout_alpha, bool absgrad) {
    const BwdScene s(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D, viewmatrix, projmatrix, tan_fovx,
                     tan_fovy, gt_depth, sh, degree, campos, geomBuffer, binningBuffer, imageBuffer, perspec);
    return backward<Light>(s, {&dL_dout_color, &dL_dout_depth, &dL_dout_median, &dL_dout_var, &dL_dout_alpha, &alphas}, R,
                           {debug, track_off, map_off}, need_gaussian_grads, absgrad);
}
std::vector<Tensor> full_backward(const Tensor& background, const Tensor& means3D, const Tensor& radii, const Tensor& colors,
                                  const Tensor& scales, const Tensor& rotations, double scale_modifier, const Tensor& cov3D,
                                  const Tensor& viewmatrix, const Tensor& gt_depth, const Tensor& projmatrix, double tan_fovx,
                                  double tan_fovy, const Tensor& dL_dout_color, const Tensor& dL_dout_depth, const Tensor& dL_dout_unc,
                                  const Tensor& sh, long degree, const Tensor& campos, const Tensor& geomBuffer, long R,
                                  const Tensor& binningBuffer, const Tensor& imageBuffer, long NG, const Tensor& perspec,
                                  bool need_gaussian_grads, const Tensor& dL_dout_sil, bool absgrad) {
    (void)NG;  // (sizes the reference's pair lists, which this backward does not have)
    const BwdScene s(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D, viewmatrix, projmatrix, tan_fovx,
                     tan_fovy, gt_depth, sh, degree, campos, geomBuffer, binningBuffer, imageBuffer, perspec);
    return backward<Full>(s, {&dL_dout_color, &dL_dout_depth, &dL_dout_unc, &dL_dout_sil}, R, {}, need_gaussian_grads, absgrad);
}

// ------------------------------------------------------------------------------------------------ autograd nodes
// The reference's surface is an eager autograd.Function written in Python over `_C` (L/__init__.py:46-176,
// F/__init__.py:46-151).  Kept as that (dgr_amd.light / full._RasterizeGaussians: the debug path, the ctypes binding), it
// costs a Python frame, a tuple of forty arguments and a context object per forward, and in the backward a hand-off from the
// autograd engine's thread into the interpreter -- together more than the GPU needs for a 640x480 / 100 k view (BASELINE
// config 2).  Node<V> below is the same Function in C++: ONE Python -> C++ crossing per forward, and a backward that runs
// inside the engine without the interpreter.  Same inputs in the same order, same saved state, same outputs, same None
// gradients for gt_depth and the settings.
//
// dgr_amd.multiview.ViewStreams.before_backward(): an event the backward THAT RUNS ON A GIVEN STREAM makes that stream wait
// for once its kernels are issued -- before autograd goes on to the accumulation into shared `.grad`.  Keyed by the raw
// stream handle; the Python side keeps the torch objects alive until it drops the entry.
std::mutex g_wait_mu;
std::vector<std::pair<void*, void*>> g_post_backward_waits;  // (stream, event)
void set_post_backward_wait(long stream, long event) {
    std::lock_guard<std::mutex> lk(g_wait_mu);
    for (auto& e : g_post_backward_waits)
        if (e.first == (void*)stream) { e.second = (void*)event; return; }
    g_post_backward_waits.emplace_back((void*)stream, (void*)event);
}
void drop_post_backward_wait(long stream) {
    std::lock_guard<std::mutex> lk(g_wait_mu);
    for (size_t i = 0; i < g_post_backward_waits.size(); i++)
        if (g_post_backward_waits[i].first == (void*)stream) { g_post_backward_waits.erase(g_post_backward_waits.begin() + (long)i); return; }
}
void consume_post_backward_wait(void* stream) {
    void* ev = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_wait_mu);
        for (size_t i = 0; i < g_post_backward_waits.size(); i++)
            if (g_post_backward_waits[i].first == stream) {
                ev = g_post_backward_waits[i].second;
                g_post_backward_waits.erase(g_post_backward_waits.begin() + (long)i);
                break;
            }
    }
    if (ev) check(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0) == hipSuccess ? 0 : DGR_ERR_HIP);
}

// a forward's report on its way out of Function::apply (read by apply<V> right after it)
thread_local FwdReport g_report;

// A node's scalars in ctx->saved_data: each() names every key once, for the forward's write and the backward's read
struct SavedScalars {
    double scale_modifier, tanfovx, tanfovy;
    int64_t degree, R, H, W, options;  // R: num_rendered, or a lazy forward's capacity; options: the forward's per-call option word
    bool track_off = false, map_off = false;
    template <typename Op>
    void each(Op op, bool tracking_flags) {
        op("scale_modifier", scale_modifier); op("tanfovx", tanfovx); op("tanfovy", tanfovy); op("degree", degree); op("R", R);
        op("H", H); op("W", W); op("options", options);
        if (tracking_flags) { op("track_off", track_off); op("map_off", map_off); }
    }
    template <typename Map>
    void write(Map& d, bool tracking_flags) { each([&](const char* key, auto& v) { d[key] = v; }, tracking_flags); }
    template <typename Map>
    void read(Map& d, bool tracking_flags) {
        each([&](const char* key, auto& v) { v = d[key].template to<std::decay_t<decltype(v)>>(); }, tracking_flags);
    }
};

// an output that did not take part in the loss arrives undefined: zeros, as the reference's autograd would have passed
inline Tensor grad_or_zeros(const Tensor& g, long c, long H, long W, const c10::Device& dev) {
    return g.defined() ? g : at::zeros({c, H, W}, at::TensorOptions().dtype(at::kFloat).device(dev));
}
// (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp): tracking needs none
inline bool needs_gaussian_grads(AutogradContext* ctx) {
    bool need = false;
    for (int i = 0; i < 8; i++) need = need || ctx->needs_input_grad(i);
    return need;
}

// the "silhouette_grad" field (DGR_OPT_SHIFT_SILHOUETTE_GRAD) of such a word: the exact silhouette gradient was on at the forward
inline bool silhouette_on(int word) { return ((word >> DGR_OPT_SHIFT_SILHOUETTE_GRAD) & 15) == 2; }
// a block under a word of dgr_thread_options_effective() (include/dgr_hip.h): a backward under its forward's options
struct UnderOptions {
    int prev;
    explicit UnderOptions(int word) : prev(dgr_thread_options_swap(word)) {}
    ~UnderOptions() { dgr_thread_options_swap(prev); }
};

// A backward's gradients (means2D, colors, opacity, means3D, cov3D, sh, scales, rotations, dL_dview [4,4]) in the order of the
// nodes' inputs (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix); None for the rest
constexpr size_t kNodeInputs = 25;
variable_list node_grads(std::vector<Tensor>& g) {
    variable_list out(kNodeInputs);
    out[0] = std::move(g[3]); out[1] = std::move(g[0]); out[2] = std::move(g[5]); out[3] = std::move(g[1]);
    out[4] = std::move(g[2]); out[5] = std::move(g[6]); out[6] = std::move(g[7]); out[7] = std::move(g[4]);
    out[8] = std::move(g[8]);
    return out;
}

template <class V>
struct Node : public torch::autograd::Function<Node<V>> {
    // inputs 0..9 as L/__init__.py:46-60; then the settings' tensors and scalars (L/__init__.py:180-195; track_off and map_off are the
    // light variant's, false for the full one) and the binning policy
    static variable_list forward(AutogradContext* ctx, const Tensor& means3D, const Tensor& means2D, const Tensor& sh,
                                 const Tensor& colors_precomp, const Tensor& opacities, const Tensor& scales, const Tensor& rotations,
                                 const Tensor& cov3Ds_precomp, const Tensor& viewmatrix, const Tensor& gt_depth, const Tensor& bg,
                                 const Tensor& projmatrix, const Tensor& campos, const Tensor& perspec, double scale_modifier,
                                 double tanfovx, double tanfovy, int64_t H, int64_t W, int64_t degree, bool prefiltered,
                                 bool track_off, bool map_off, int64_t capacity, int64_t mode) {
        (void)means2D;  // never read (L/__init__.py:66-87): it exists so that autograd hands dL_dmeans2D back
        Probe p_f(HP_FWD);
        const Fwd o = forward_core<V>(bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3Ds_precomp, viewmatrix,
                                      gt_depth, projmatrix, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered, /*debug=*/false,
                                      capacity, mode, /*want_related=*/false);
        g_report = o;
        Probe p_s(HP_SAVE);
        variable_list sv(V::N_SAVED);
        sv[S_COLORS] = colors_precomp; sv[S_MEANS3D] = means3D; sv[S_SCALES] = scales; sv[S_ROTATIONS] = rotations;
        sv[S_COV3D] = cov3Ds_precomp; sv[S_VIEW] = viewmatrix; sv[S_RADII] = o.radii; sv[S_SH] = sh; sv[S_GEOM] = o.geom;
        sv[S_BINNING] = o.binning; sv[S_IMG] = o.img; sv[S_GT] = gt_depth; sv[S_BG] = bg; sv[S_PROJ] = projmatrix;
        sv[S_CAMPOS] = campos; sv[S_PERSPEC] = perspec;
        V::save_extra(sv, o);
        ctx->save_for_backward(std::move(sv));
        // (the backward runs under the forward's per-call options)
        SavedScalars{scale_modifier, tanfovx, tanfovy, degree, (int64_t)(o.rendered >= 0 ? o.rendered : o.cap), H, W,
                     (int64_t)dgr_thread_options_effective(), track_off, map_off}
            .write(ctx->saved_data, V::tracking_flags);
        // no zero-filled gradient tensors for the outputs that have no gradient input in the backward
        ctx->set_materialize_grads(false);
        ctx->mark_non_differentiable(V::non_differentiable(o));
        return V::node_outputs(o);
    }

    static variable_list backward(AutogradContext* ctx, variable_list grad) {
        Probe p_b(HP_BWD);
        Probe p_u(HP_UNPACK);
        const auto sv = ctx->get_saved_variables();
        SavedScalars c;
        c.read(ctx->saved_data, V::tracking_flags);
        const Tensor& means3D = sv[S_MEANS3D];
        const c10::Device dev = means3D.device();
        p_u.stop();
        const Tensor gC = grad_or_zeros(grad[0], 3, c.H, c.W, dev), gD = grad_or_zeros(grad[2], 1, c.H, c.W, dev), none;
        const auto images = V::node_images(gC, gD, grad, sv, silhouette_on((int)c.options), none);
        const UnderOptions under((int)c.options);  // (the engine may run this node on a thread of its own)
        const BwdScene s(sv[S_BG], means3D, sv[S_RADII], sv[S_COLORS], sv[S_SCALES], sv[S_ROTATIONS], c.scale_modifier, sv[S_COV3D],
                         sv[S_VIEW], sv[S_PROJ], c.tanfovx, c.tanfovy, sv[S_GT], sv[S_SH], c.degree, sv[S_CAMPOS], sv[S_GEOM],
                         sv[S_BINNING], sv[S_IMG], sv[S_PERSPEC]);
        // (dL_dcolors / dL_dcov3D only for a colors_precomp / cov3Ds_precomp leaf: inputs 3 and 7.  Without one autograd would
        //  drop the tensor, and the per-Gaussian backward would have written its 36 bytes per Gaussian for nobody.)
        const bool want_colors = ctx->needs_input_grad(3) && sv[S_COLORS].numel() != 0;
        const bool want_cov3D = ctx->needs_input_grad(7) && sv[S_COV3D].numel() != 0;
        std::vector<Tensor> g = ::backward<V>(s, images, c.R, {false, c.track_off, c.map_off}, needs_gaussian_grads(ctx), /*absgrad=*/false,
                                              want_colors, want_cov3D);
        consume_post_backward_wait(stream_of(dev));
        // (the reference sums light's [H*W,4,4] buffer over dim 0, L/__init__.py:160-161; here it is [1,4,4], already reduced)
        if (V::dview_leading_one) g[8] = view_of(g[8], 0, {4, 4}, at::kFloat);
        return node_grads(g);
    }
};

// `_RasterizeGaussians.apply` of a variant: (the report, V::node_outputs)
template <class V>
PyForward apply(const Tensor& means3D, const Tensor& means2D, const Tensor& sh, const Tensor& colors_precomp, const Tensor& opacities,
                const Tensor& scales, const Tensor& rotations, const Tensor& cov3Ds_precomp, const Tensor& viewmatrix,
                const Tensor& gt_depth, const Tensor& bg, const Tensor& projmatrix, const Tensor& campos, const Tensor& perspec,
                double scale_modifier, double tanfovx, double tanfovy, long H, long W, long degree, bool prefiltered, bool track_off,
                bool map_off, long capacity, long mode) {
    Probe p_a(HP_APPLY);
    variable_list out = Node<V>::apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix,
                                       gt_depth, bg, projmatrix, campos, perspec, scale_modifier, tanfovx, tanfovy, (int64_t)H,
                                       (int64_t)W, (int64_t)degree, prefiltered, track_off, map_off, (int64_t)capacity, (int64_t)mode);
    p_a.stop();
    PyForward result{g_report.py(), std::move(out)};
    g_report.status = Tensor();
    return result;
}

// ------------------------------------------------------------------------------------------------ batched views
// dgr_amd.batch / batch_full over the C ABI's batched entry points (include/dgr_hip.h: dgr_*_forward_batch / _backward_batch): V
// cameras over one set of Gaussians per call.  ONE attempt with the given binning capacity per view and no host
// synchronisation; the capacity policy, the strict mode's status read and its retry stay in Python (dgr_amd/_binning.py).
inline long batch_size(long V) {
    if (V < 1 || V > DGR_MAX_BATCH_VIEWS) throw std::runtime_error("1 .. " + std::to_string(DGR_MAX_BATCH_VIEWS) + " views per batch");
    return V;
}
// lazy mode: every view's status word copied to pinned memory behind an event; returns the tickets
std::vector<long> post_batch_status(bool post_status, int P, void* st, const Tensor& status, long V) {
    std::vector<long> tickets;
    if (post_status && P > 0 && !dgr_stream_is_capturing(st)) {
        for (long v = 0; v < V; v++) {
            const long t = dgr_status_post(st, row<int>(status, v));
            check(t);
            tickets.push_back(t);
        }
    }
    return tickets;
}

// post_status: copy every view's status word to pinned memory behind an event (lazy mode) and return the tickets.
// Returns (V::batch_tensors: the [V,4] status first, then the outputs [V,...] and the state buffers) and the tickets.
template <class V>
std::tuple<std::vector<Tensor>, std::vector<long>>
forward_batch(const Tensor& background, const Tensor& means3D_, const Tensor& colors_, const Tensor& opacity_, const Tensor& scales_,
              const Tensor& rotations_, double scale_modifier, const Tensor& cov3D_, const Tensor& viewmatrices_, const Tensor& gt_depths_,
              const Tensor& projmatrices_, double tan_fovx, double tan_fovy, long H, long W, const Tensor& sh_, long degree,
              const Tensor& campos_, bool prefiltered, long capacity, bool post_status) {
    const c10::Device dev = forward_device(means3D_);
    const long nv = batch_size(viewmatrices_.dim() == 3 ? viewmatrices_.size(0) : 0);
    const FwdInputs in(dev, background, means3D_, colors_, opacity_, scales_, rotations_, cov3D_, viewmatrices_, gt_depths_,
                       projmatrices_, sh_, campos_);
    const int P = in.P;
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    const auto i32 = at::TensorOptions().dtype(at::kInt).device(dev);
    const auto u8 = at::TensorOptions().dtype(at::kByte).device(dev);
    Fwd o;
    V::batch_outputs(o, nv, P, H, W, f32, i32);
    o.geom = at::empty({nv, (long long)std::max<size_t>(dgr_geometry_bytes(P), 1)}, u8);
    o.img = at::empty({nv, (long long)std::max<size_t>(dgr_image_bytes((int)W, (int)H), 1)}, u8);
    o.binning = at::empty({nv, (long long)std::max<size_t>(dgr_binning_bytes((int)capacity, (int)W, (int)H), 1)}, u8);
    o.status = at::zeros({nv, 4}, i32);
    typename V::View w[DGR_MAX_BATCH_VIEWS];
    for (long v = 0; v < nv; v++) w[v] = V::view(v, (int)capacity, o, in);
    void* st = stream_of(dev);
    check(std::apply([&](auto... scene) { return V::forward_batch(st, (int)nv, w, scene...); },
                     scene_args(in, degree, W, H, scale_modifier, tan_fovx, tan_fovy, prefiltered)));
    return {V::batch_tensors(o), post_batch_status(post_status, P, st, o.status, nv)};
}

// Returns (dL_dmeans2D [V,P,3] or None, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations --
// the SUMS over the views, views of one flat arena laid out as a one-view backward's -- and dL_dview [V,4,4]).  `images`: every
// view's gradient images [V,...]; absgrad (dgr_*_backward_batch_absgrad): a tenth result, every view's absolute screen-space
// gradient [V,P,3]
template <class V>
std::vector<Tensor> backward_batch(const BwdScene& s, const std::array<const Tensor*, V::N_IMAGES>& images, BwdFlags flags,
                                   bool need_gaussian_grads, bool need_means2D, const std::vector<long>& num_rendered, bool absgrad) {
    const long nv = s.view.size(0), H = images[V::GC]->size(2), W = images[V::GC]->size(3);
    AbsGrad abs(absgrad, s.means3D, nv);
    batch_size(nv);
    typename V::Images im;
    for (size_t i = 0; i < im.size(); i++) im[i] = f32c(*images[i], s.dev);
    BatchBwdOut o(s.dev, s.P, s.M, nv, W, H, need_gaussian_grads, need_means2D, num_rendered);
    typename V::ViewGrad w[DGR_MAX_BATCH_VIEWS];
    const float* sil[DGR_MAX_BATCH_VIEWS] = {};
    for (long v = 0; v < nv; v++) {
        sil[v] = row<float>(im[V::SIL], v);
        w[v] = V::view_grad(v, s, im, o, rendered_of(num_rendered, v));
    }
    check(V::backward_batch(stream_of(s.dev), (int)nv, w, s, W, H, o.gp, flags, need_gaussian_grads, abs.views(),
                            im[V::SIL].numel() ? sil : nullptr));
    if (absgrad) o.g.push_back(std::move(abs.t));
    return o.g;
}

// sil: every view's opacity_map gradient (light) / exact silhouette gradient (full) [V,1,H,W], or undefined / empty
std::vector<Tensor> light_backward_batch(const Tensor& background, const Tensor& means3D, const Tensor& radii, const Tensor& colors,
                                         const Tensor& scales, const Tensor& rotations, double scale_modifier, const Tensor& cov3D,
                                         const Tensor& viewmatrices, const Tensor& projmatrices, double tan_fovx, double tan_fovy,
                                         const Tensor& dL_dout_color, const Tensor& dL_dout_depth, const Tensor& dL_dout_median,
                                         const Tensor& dL_dout_var, const Tensor& gt_depths, const Tensor& sh, long degree,
                                         const Tensor& campos, const Tensor& geom, const Tensor& binning, const Tensor& img,
                                         const Tensor& alphas, const Tensor& perspec, bool track_off, bool map_off,
                                         bool need_gaussian_grads, bool need_means2D, const std::vector<long>& num_rendered,
                                         const Tensor& sil, bool absgrad) {
    const BwdScene s(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D, viewmatrices, projmatrices, tan_fovx,
                     tan_fovy, gt_depths, sh, degree, campos, geom, binning, img, perspec);
    return backward_batch<Light>(s, {&dL_dout_color, &dL_dout_depth, &dL_dout_median, &dL_dout_var, &sil, &alphas},
                                 {false, track_off, map_off}, need_gaussian_grads, need_means2D, num_rendered, absgrad);
}
std::vector<Tensor> full_backward_batch(const Tensor& background, const Tensor& means3D, const Tensor& radii, const Tensor& colors,
                                        const Tensor& scales, const Tensor& rotations, double scale_modifier, const Tensor& cov3D,
                                        const Tensor& viewmatrices, const Tensor& projmatrices, double tan_fovx, double tan_fovy,
                                        const Tensor& dL_dout_color, const Tensor& dL_dout_depth, const Tensor& dL_dout_unc,
                                        const Tensor& gt_depths, const Tensor& sh, long degree, const Tensor& campos, const Tensor& geom,
                                        const Tensor& binning, const Tensor& img, const Tensor& perspec, bool need_gaussian_grads,
                                        bool need_means2D, const std::vector<long>& num_rendered, const Tensor& sil, bool absgrad) {
    const BwdScene s(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D, viewmatrices, projmatrices, tan_fovx,
                     tan_fovy, gt_depths, sh, degree, campos, geom, binning, img, perspec);
    return backward_batch<Full>(s, {&dL_dout_color, &dL_dout_depth, &dL_dout_unc, &sil}, {}, need_gaussian_grads, need_means2D,
                                num_rendered, absgrad);
}

Tensor mark_visible(const Tensor& means3D_, const Tensor& viewmatrix_, const Tensor& projmatrix_) {  // L/rasterize_points.cu:238-256
    const c10::Device dev = means3D_.device();
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const int P = (int)means3D_.size(0);
    Tensor present = at::zeros({P}, at::TensorOptions().dtype(at::kBool).device(dev));
    if (P != 0) {
        const Tensor m = f32c(means3D_, dev), v = f32c(viewmatrix_, dev), pj = f32c(projmatrix_, dev);
        check(dgr_mark_visible(stream_of(dev), P, ptr<float>(m), ptr<float>(v), ptr<float>(pj),
                               reinterpret_cast<uint8_t*>(present.data_ptr<bool>())));
    }
    return present;
}

// status ticket of a lazy forward: None while the copy has not landed (wait = false), else [num_rendered, overflow,
// prefiltered violation, num_related]
py::object status_poll(long ticket, bool wait) {
    int s[4];
    const int rc = dgr_status_poll(ticket, wait ? 1 : 0, s);
    check(rc);
    if (rc == 0) return py::none();
    return py::make_tuple(s[0], s[1], s[2], s[3]);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("light_forward", &forward<Light>);
    m.def("light_backward", &light_backward);
    m.def("full_forward", &forward<Full>);
    m.def("full_backward", &full_backward);
    m.def("light_forward_batch", &forward_batch<Light>);
    m.def("light_backward_batch", &light_backward_batch);
    m.def("full_forward_batch", &forward_batch<Full>);
    m.def("full_backward_batch", &full_backward_batch);
    m.def("host_prof_dump", &host_prof_dump);
    m.def("light_apply", &apply<Light>);
    m.def("full_apply", &apply<Full>);
    m.def("set_post_backward_wait", &set_post_backward_wait);
    m.def("drop_post_backward_wait", &drop_post_backward_wait);
    m.def("mark_visible", &mark_visible);
    m.def("status_poll", &status_poll);
    // which kind of views the outputs are: 1 = raw TensorImpl windows, 0 = dispatcher views, -1 = not decided yet (no view made)
    m.def("raw_views", [] { return g_raw_views.load(); });
    // TEST-ONLY (tests/test_hip_binding_guard.py): not synchronised with forwards in flight on other threads
    m.def("set_raw_views", [](long v) { g_raw_views.store(v < 0 ? -1 : v ? 1 : 0); });
}
