// api.hip -- C-ABI entry points (include/dgr_hip.h) and host orchestration.
//
// Replaces CudaRasterizer::Rasterizer::{forward, backward, markVisible}
// (L/cuda_rasterizer/rasterizer_impl.cu:141-153, 197-350, 354-495).  Stage order per view:
//   forward : zero histogram -> preprocess (+ per-tile histogram) -> scan tiles -> emit keys ->
//             per-tile sort -> blend
//   backward: zero accumulator rows -> blend backward -> fused per-Gaussian backward -> pose reduce
// Nothing here touches the CPU oracle; a missing GPU or a failed launch is reported, never papered over.
// The library options are in options.hip, the status read-back in status.hip, the stage profiler in profile.hip,
// dgr_state_export in state_export.hip and the entry points of the steps around the rasteriser (optimiser, map resize, pose,
// losses, keyframe overlap) in api_steps.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/dgr_hip.h"
#include "dgr_common.h"
#include "host_util.h"
#include "kernels.h"
#include "options.h"
#include "profile.h"
#include "status.h"

namespace dgr {
namespace {
thread_local std::string g_last_error = "";
}
void set_last_error(const std::string& text) { g_last_error = text; }
}  // namespace dgr

using namespace dgr;

namespace {

struct FwdCommon {
    int P, D, M, W, H;
    const float *background, *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
    float scale_modifier;
    const float *viewmatrix, *projmatrix, *cam_pos;
    float tan_fovx, tan_fovy;
    int prefiltered;
    float *out_color, *out_depth, *out_median_depth, *out_alpha;
    const float* gt_depth;
    float *out_depth_var, *gau_uncertainty;
    int *gau_related_pixels, *radii;
};

// One view's forward arguments as the entry points of a variant take them, in the C ABI's order
FwdCommon light_common(int P, int D, int M, const float* background, int width, int height, const float* means3D, const float* shs,
                       const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                       const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                       const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color, float* out_depth,
                       float* out_median_depth, float* out_alpha, const float* gt_depth, float* out_depth_var, float* gau_uncertainty,
                       int* gau_related_pixels, int* radii) {
    return FwdCommon{P, D, M, width, height, background, means3D, shs, colors_precomp, opacities, scales, rotations,
                     cov3D_precomp, scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered,
                     out_color, out_depth, out_median_depth, out_alpha, gt_depth, out_depth_var, gau_uncertainty,
                     gau_related_pixels, radii};
}
// ... the full variant: the uncertainty image in the alpha slot, no light-only outputs
FwdCommon full_common(int P, int D, int M, const float* background, int width, int height, const float* means3D, const float* shs,
                      const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                      const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                      const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color, float* out_depth,
                      const float* gt_depth, float* out_uncertainty, int* radii) {
    return light_common(P, D, M, background, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
                        cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, out_color, out_depth, nullptr,
                        out_uncertainty, gt_depth, nullptr, nullptr, nullptr, radii);
}

// P == 0: the reference launches nothing and returns zero-filled outputs (L/rasterize_points.cu:88).
int zero_outputs(const FwdCommon& c, hipStream_t st) {
    const size_t N = (size_t)c.W * c.H;
    HIP_TRY(hipMemsetAsync(c.out_color, 0, 3 * N * 4, st));
    HIP_TRY(hipMemsetAsync(c.out_depth, 0, N * 4, st));
    if (c.out_median_depth) HIP_TRY(hipMemsetAsync(c.out_median_depth, 0, N * 4, st));
    if (c.out_alpha) HIP_TRY(hipMemsetAsync(c.out_alpha, 0, N * 4, st));
    if (c.out_depth_var) HIP_TRY(hipMemsetAsync(c.out_depth_var, 0, N * 4, st));
    return DGR_OK;
}

// preprocess.  Callback path (path.callback): afterwards geom.block_tiles holds the instance totals per 256-Gaussian
// block and scan_blocks turns them into offsets and num_rendered.  Presized path (the binning buffer exists already):
// the kernel also takes the tile-counter atomics and stores the ranks (count_rank.h), behind one small clear of the
// counters; scan_blocks and count_rank disappear.
// Which binning follows (dgr::BinPath, kernels.h): the segment binning wherever "lds_count" allows it and the frame's segment
// tables fit LDS, the global tile counters otherwise.
dgr::BinPath bin_path(int W, int H, bool callback) {
    return {option(OPT_LDS_COUNT) != 0 && dgr::segment_binning_fits(W, H), callback};
}
dgr::StatusReport report_of(const ArmedReport* armed) { return armed ? armed->rep : dgr::StatusReport{nullptr, 0u, nullptr}; }
// The scene half of the preprocess arguments: what the views of a batch share
void preprocess_scene(dgr::PreprocessFwdArgs& a, const FwdCommon& c) {
    a.P = c.P; a.D = c.D; a.M = c.M; a.W = c.W; a.H = c.H; a.grid_x = dgr::tiles_x(c.W); a.grid_y = dgr::tiles_y(c.H);
    a.means3D = c.means3D; a.scales = c.scales; a.scale_modifier = c.scale_modifier; a.rotations = c.rotations;
    a.opacities = c.opacities; a.shs = c.shs; a.cov3D_precomp = c.cov3D_precomp; a.colors_precomp = c.colors_precomp;
    a.tan_fovx = c.tan_fovx; a.tan_fovy = c.tan_fovy;
    a.focal_y = c.H / (2.0f * c.tan_fovy);  // rasterizer_impl.cu:228-229
    a.focal_x = c.W / (2.0f * c.tan_fovx);
    a.prefiltered = c.prefiltered;
    a.tight_cull = opt_tight_cull();
    a.sh_vec_ok = aligned16(c.shs);
}
// (presized path: `bin`, `capacity` and `image_base` are the view's binning view, its capacity and its image buffer)
int forward_front(const FwdCommon& c, dgr::GeometryView geom, dgr::ImageView img, hipStream_t st, dgr::BinPath path,
                  const dgr::BinningView* bin, int capacity, char* image_base) {
    // No memsets: preprocess clears the per-Gaussian median statistics (and, on the callback path, the tile counters);
    // scan_blocks / scan_tiles initialise the status word.
    dgr::PreprocessFwdArgs a{};
    preprocess_scene(a, c);
    a.view = c.viewmatrix; a.proj = c.projmatrix; a.campos = c.cam_pos;
    a.geom = geom; a.radii_out = c.radii;
    a.gau_uncertainty = c.gau_uncertainty; a.gau_related_pixels = c.gau_related_pixels;
    if (!path.callback && path.segments) {
        // nothing to clear: the kernel leaves its per-block instance totals (and the `prefiltered` flag) in
        // geom.block_tiles, bin_segments / bin_tiles take it from there
        { ScopedStage t(ST_PRE_FWD, st); HIP_TRY(dgr::launch_preprocess_fwd(a, st)); }
        return DGR_OK;
    }
    if (!path.callback) {
        // cursor + padded tile counters: everything between the start of the image buffer and the range table
        { ScopedStage t(ST_ZERO_FWD, st); HIP_TRY(dgr::launch_zero_fill(image_base, (size_t)((char*)img.ranges - image_base), st)); }
        a.fused_count = 1; a.tile_count = img.tile_count; a.cursor = img.cursor; a.ranks = bin->ranks; a.capacity = capacity;
        { ScopedStage t(ST_PRE_FWD, st); HIP_TRY(dgr::launch_preprocess_fwd(a, st)); }
        return DGR_OK;
    }
    a.zero_words = img.tile_count; a.n_zero_words = (int)(((char*)img.ranges - (char*)img.tile_count) / 4);
    { ScopedStage t(ST_PRE_FWD, st); HIP_TRY(dgr::launch_preprocess_fwd(a, st)); }
    // per-block instance totals -> exclusive prefix; status[0] = num_rendered
    { ScopedStage t(ST_SCAN_BLOCKS, st); HIP_TRY(dgr::launch_scan_blocks(c.P, geom, img, st)); }
    return DGR_OK;
}

// histogram + ranks, range table (status[0] = num_rendered, status[1] = overflow), key scatter, per-tile sort
// (presized path: the status word is complete after bin_tiles / scan_tiles, which is where a caller that armed the early status
// gets its copy; callback path: the caller has read it already)
int binning_stages(const FwdCommon& c, dgr::GeometryView geom, dgr::ImageView img, dgr::BinningView bin, int capacity,
                   hipStream_t st, dgr::BinPath path, char* binning_base, ArmedReport* armed) {
    const int gx = dgr::tiles_x(c.W), gy = dgr::tiles_y(c.H), tiles = gx * gy;
    // the tile schedule: always, unless this shape's last reported frame had even lists (want_schedule above)
    const bool sched_on = !(armed && armed->id >= 0) ? (option(OPT_TILE_SCHEDULE) != 0) : want_schedule(c.W, c.H, c.P);
    const int lists = option(OPT_LANE_LISTS);
    const int blend_flags = (sched_on ? dgr::BLEND_SCHEDULE : 0) | (lists == 0 ? dgr::BLEND_LISTS_QUADRANT : lists == 2 ? dgr::BLEND_LISTS_AUTO : 0);
    const dgr::StatusReport rep = report_of(armed);
    if (path.segments) {
        const dgr::SegmentTables tb = dgr::carve_segment_tables(binning_base + bin.bytes, c.W, c.H);
        const int longest = (armed && armed->id >= 0) ? hinted_longest_list(c.W, c.H, c.P) : -1;
        const int ss = dgr::segment_shift(c.W, c.H, capacity, longest);
        { ScopedStage t(ST_BIN_SEGMENTS, st); HIP_TRY(dgr::launch_bin_segments(c.P, geom, bin, tb, gx, gy, ss, capacity, path, st)); }
        { ScopedStage t(ST_BIN_TILES, st); HIP_TRY(dgr::launch_bin_tiles(c.P, geom, img, bin, tb, gx, gy, ss, capacity, path, blend_flags, rep, st)); }
        if (!path.callback) { const int rc = early_status_post(img.status, st); if (rc) return rc; }  // (bin_tiles writes the status word)
        if (sched_on) { ScopedStage t(ST_TILE_SCHED, st); HIP_TRY(dgr::launch_tile_schedule(img, tiles, st)); }
        return DGR_OK;
    }
    // (presized: preprocess_fwd counted already)
    if (path.callback) { ScopedStage t(ST_COUNT_RANK, st); HIP_TRY(dgr::launch_count_rank(c.P, geom, img, bin, gx, capacity, st)); }
    { ScopedStage t(ST_SCAN, st); HIP_TRY(dgr::launch_scan_tiles(img, tiles, gx, capacity, path, blend_flags, rep, st)); }
    if (!path.callback) { const int rc = early_status_post(img.status, st); if (rc) return rc; }
    { ScopedStage t(ST_EMIT, st); HIP_TRY(dgr::launch_emit_instances(c.P, geom, img, bin, gx, st)); }
    { ScopedStage t(ST_SORT, st); HIP_TRY(dgr::launch_sort_tiles(img, bin, tiles, st)); }
    if (sched_on) { ScopedStage t(ST_TILE_SCHED, st); HIP_TRY(dgr::launch_tile_schedule(img, tiles, st)); }
    return DGR_OK;
}

// The forward blend, light or full (the full variant's uncertainty image in c.out_alpha)
template <class A>
void blend_fwd_common(A& r, const FwdCommon& c, dgr::GeometryView geom, dgr::ImageView img, dgr::BinningView bin, ArmedReport* armed) {
    r.W = c.W; r.H = c.H; r.grid_x = dgr::tiles_x(c.W); r.grid_y = dgr::tiles_y(c.H);
    r.sched = img.tile_sched; r.ranges = img.ranges; r.sched_flag = img.cursor + 3; r.point_list = bin.point_list; r.rec = geom.rec; r.bg = c.background;
    r.out_color = c.out_color; r.out_depth = c.out_depth; r.n_contrib = img.n_contrib; r.status = img.status;
    r.rep = report_of(armed);
}
int forward_blend(const FwdCommon& c, dgr::GeometryView geom, dgr::ImageView img, dgr::BinningView bin, hipStream_t st, bool full,
                  ArmedReport* armed = nullptr) {
    ScopedStage t(ST_RENDER_FWD, st);
    if (full) {
        dgr::RenderFwdFullArgs r{};
        blend_fwd_common(r, c, geom, img, bin, armed);
        r.out_uncertainty = c.out_alpha; r.n_valid = img.n_valid; r.first_contrib = img.first_contrib; r.final_T = img.final_T;
        HIP_TRY(dgr::launch_render_fwd_full(r, opt_alpha_mode(), st));
    } else {
        dgr::RenderFwdLightArgs r{};
        blend_fwd_common(r, c, geom, img, bin, armed);
        r.gt_depth = c.gt_depth; r.out_median = c.out_median_depth; r.out_alpha = c.out_alpha; r.out_depth_var = c.out_depth_var;
        r.gau_uncertainty = c.gau_uncertainty; r.gau_related_pixels = c.gau_related_pixels;
        r.live_counts = img.tile_count;  // (dead since the binning: the blend's live counts, render_common.h)
        HIP_TRY(dgr::launch_render_fwd_light(r, opt_alpha_mode(), st));
    }
    if (armed) armed->handed_over = true;  // (workgroup 0 of the blend delivers the word)
    return DGR_OK;
}

// (the SH basis is written out for degrees 0 .. 3: a larger one would be read as 3 by some kernels and as itself by others)
const char* const BAD_DEGREE = "the SH degree must be 0 .. 3";
int check_common(const FwdCommon& c) {
    if (c.P < 0 || c.W <= 0 || c.H <= 0) { set_last_error("bad sizes"); return DGR_ERR_BAD_ARGUMENT; }
    if (c.D < 0 || c.D > 3) { set_last_error(BAD_DEGREE); return DGR_ERR_BAD_ARGUMENT; }
    if ((unsigned)c.P > DGR_ID_MASK) { set_last_error("more than 2^28 Gaussians"); return DGR_ERR_BAD_ARGUMENT; }
    if (c.P > 0 && !c.shs && !c.colors_precomp) { set_last_error("need SHs or precomputed colours"); return DGR_ERR_BAD_ARGUMENT; }
    if (c.P > 0 && !c.cov3D_precomp && (!c.scales || !c.rotations)) { set_last_error("need scale/rotation or cov3D"); return DGR_ERR_BAD_ARGUMENT; }
    // (2^30 pixels: the blend kernels index pixels, and the three colour planes, with 32-bit words)
    if (dgr::tiles_x(c.W) > 65535 || dgr::tiles_y(c.H) > 65535 || (long long)c.W * c.H > (1ll << 30)) { set_last_error("image too large"); return DGR_ERR_BAD_ARGUMENT; }
    return DGR_OK;
}

// ---- batched views (dgr_light_forward_batch / dgr_light_backward_batch) ----
// The per-Gaussian kernels of a batch run ONCE for all views on the caller's stream; the per-view stages in between
// (binning + blend, blend backward) are independent and mix kernels that leave the chip idle (count, scan, emit, sort) with
// kernels bound by VALU issue (blend), so view v runs them on stream v mod K -- the caller's stream and K - 1 helper
// streams of this thread -- forked and joined with events: what DESIGN.md s7 measured for "views in flight", inside one call
// and capturable into one hipGraph.  dgr_set_option("batch_streams", K), K = 1..8: at most K streams; the views are dealt
// out in rounds, and a batch uses the fewest streams that keep the number of rounds minimal, since the join waits for the
// longest stream.  Default 2, measured (profiles/batch_streams.sh, config 3, ms per view for K = 1 / 2 / 3 / 4 / 8):
// 3 views 0.459 / 0.434 / 0.436 / 0.438 / 0.444, 4 views 0.450 / 0.415 / 0.419 / 0.446 / 0.437, 8 views 0.425 / 0.377 /
// 0.380 / 0.391 / 0.407 -- one view's binning under another view's blend is the whole gain; more blend kernels at once
// only take each other's L2 and wave slots.
// dgr_set_option("batch_order", o): how the per-view stages of a batch are spread over the streams.
//   0 (default) = round robin: view v's whole chain on stream v mod K ("batch_streams");
//   1 = pipeline: the views' BINNING stages (count, scan, emit, sort -- kernels that leave most of the chip idle) one after the
//       other on a helper stream, the views' BLEND stages one after the other on the caller's stream, view v's blend waiting
//       for view v's binning with an event (the backward likewise: the next view's scratch cleared under the current blend).
//       On paper binning v + 1 always runs under blend v and two VALU-bound blend kernels never share the chip; measured
//       (profiles/batch_order.sh) it LOSES to the round robin at every size -- config 3, ms per view, pipeline / round robin:
//       2 views 0.509 / 0.461, 4 views 0.468 / 0.417, 8 views 0.431 / 0.383; config 2: 0.193 / 0.156, 0.172 / 0.130,
//       0.156 / 0.116 -- slower even than one stream (0.450 at 4 views): one cross-stream event wait per view each way costs more
//       than the overlap it arranges (the same finding as round 1's high-priority companion stream).  Kept as the
//       measured alternative.
inline int batch_stream_count(int n_views) {
    const int kmax = std::max(1, std::min(option(OPT_BATCH_STREAMS), DGR_BATCH_MAX_STREAMS));
    const int rounds = (n_views + kmax - 1) / kmax;
    return (n_views + rounds - 1) / rounds;
}
struct BatchStreams {
    int device = -1;
    hipStream_t helper[DGR_BATCH_MAX_STREAMS - 1] = {};
    hipEvent_t fork = nullptr;
    hipEvent_t join[DGR_BATCH_MAX_STREAMS - 1] = {};
    hipEvent_t stage[DGR_MAX_BATCH_VIEWS] = {};  // pipelined order: view v's binning (forward) / cleared scratch (backward) is ready
};
// One set per device and thread: streams and events belong to the device that was current when they were created, and a
// single-process loop that alternates between GPUs (dgr_amd._capi.on_device) must neither re-create them on every call
// nor lose the old ones.
constexpr int DGR_BATCH_MAX_DEVICES = 32;
thread_local BatchStreams g_batch_pool[DGR_BATCH_MAX_DEVICES];
thread_local BatchStreams* g_batch_p = nullptr;
int batch_streams_ready() {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= DGR_BATCH_MAX_DEVICES) { set_last_error("device index above DGR_BATCH_MAX_DEVICES"); return DGR_ERR_BAD_ARGUMENT; }
    g_batch_p = &g_batch_pool[dev];
    if (g_batch_p->device == dev) return DGR_OK;
    for (int i = 0; i < DGR_BATCH_MAX_STREAMS - 1; i++) {
        HIP_TRY(hipStreamCreateWithFlags(&g_batch_p->helper[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&g_batch_p->join[i], hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&g_batch_p->fork, hipEventDisableTiming));
    for (int v = 0; v < DGR_MAX_BATCH_VIEWS; v++) HIP_TRY(hipEventCreateWithFlags(&g_batch_p->stage[v], hipEventDisableTiming));
    g_batch_p->device = dev;
    return DGR_OK;
}
// stream of view v among K; fork: the helpers wait for what the caller's stream has enqueued so far
inline hipStream_t batch_stream(hipStream_t main, int v, int K) { return (v % K == 0) ? main : g_batch_p->helper[v % K - 1]; }
int batch_fork(hipStream_t main, int K) {
    if (K <= 1) return DGR_OK;
    HIP_TRY(hipEventRecord(g_batch_p->fork, main));
    for (int i = 0; i < K - 1; i++) HIP_TRY(hipStreamWaitEvent(g_batch_p->helper[i], g_batch_p->fork, 0));
    return DGR_OK;
}
int batch_join(hipStream_t main, int K) {
    for (int i = 0; i < K - 1; i++) {
        HIP_TRY(hipEventRecord(g_batch_p->join[i], g_batch_p->helper[i]));
        HIP_TRY(hipStreamWaitEvent(main, g_batch_p->join[i], 0));
    }
    return DGR_OK;
}
// After batch_fork the helper streams may hold kernels that touch the caller's buffers: whatever way the call leaves --
// an error in the middle of the view loop included -- the caller's stream must wait for them (and a stream capture must
// see the forked streams rejoined).  done() performs the join once and reports its status.
struct BatchJoinGuard {
    hipStream_t main;
    int K;
    bool armed;
    BatchJoinGuard(hipStream_t m, int k) : main(m), K(k), armed(true) {}
    int done() { armed = false; return batch_join(main, K); }
    ~BatchJoinGuard() { if (armed) batch_join(main, K); }
};
// Which stream the per-view stages of view v start on, and how they hand over to the caller's stream ("batch_order", above):
// round robin = view v's whole chain on stream v mod K; pipeline = every view's first stage on one helper stream and the rest on
// the caller's stream, behind an event.
struct BatchPlan {
    hipStream_t main;
    bool pipeline;
    int K;
    BatchPlan(hipStream_t st, int n_views)
        : main(st), pipeline(option(OPT_BATCH_ORDER) == 1 && n_views > 1 && option(OPT_BATCH_STREAMS) > 1),
          K(pipeline ? 2 : batch_stream_count(n_views)) {}
    hipStream_t first_stream(int v) const { return pipeline ? g_batch_p->helper[0] : batch_stream(main, v, K); }
    // sv = the stream of view v's remaining stages, ordered behind what its first stage enqueued on sv
    int hand_over(int v, hipStream_t& sv) const {
        if (!pipeline) return DGR_OK;
        HIP_TRY(hipEventRecord(g_batch_p->stage[v], sv));
        HIP_TRY(hipStreamWaitEvent(main, g_batch_p->stage[v], 0));
        sv = main;
        return DGR_OK;
    }
};

// The body of dgr_light_forward_batch / dgr_full_forward_batch: cv[v] = view v's arguments as the one-view presized call takes
// them (full: the uncertainty image in the out_alpha slot, as dgr_full_forward_presized passes it), bs[v] its state buffers.
struct BatchViewState {
    char* geometry_buffer;
    char* binning_buffer;
    int binning_capacity;
    char* image_buffer;
    int* status;
};
int forward_batch(hipStream_t st, int n_views, const FwdCommon* cv, const BatchViewState* bs, bool full) {
    const int P = cv[0].P, width = cv[0].W, height = cv[0].H;
    for (int v = 0; v < n_views; v++) {
        const FwdCommon& w = cv[v];
        if (!w.viewmatrix || !w.projmatrix || !w.cam_pos || !w.out_color || !w.out_depth || (full && !w.out_alpha)) {
            set_last_error("view without camera or outputs");
            return DGR_ERR_BAD_ARGUMENT;
        }
        if (P > 0 && (!bs[v].geometry_buffer || !bs[v].image_buffer || !bs[v].binning_buffer || bs[v].binning_capacity < 0)) {
            set_last_error("view without state buffers");
            return DGR_ERR_BAD_ARGUMENT;
        }
    }
    int rc = check_common(cv[0]);
    if (rc) return rc;
    if (P == 0) {
        for (int v = 0; v < n_views; v++) {
            if (bs[v].status) HIP_TRY(hipMemsetAsync(bs[v].status, 0, 16, st));
            if ((rc = zero_outputs(cv[v], st))) return rc;
        }
        return DGR_OK;
    }
    if ((rc = batch_streams_ready())) return rc;
    dgr::GeometryView geom[DGR_MAX_BATCH_VIEWS];
    dgr::ImageView img[DGR_MAX_BATCH_VIEWS];
    dgr::BinningView bin[DGR_MAX_BATCH_VIEWS];
    for (int v = 0; v < n_views; v++) {
        geom[v] = dgr::carve_geometry(bs[v].geometry_buffer, P);
        img[v] = dgr::carve_image(bs[v].image_buffer, width, height);
        if (bs[v].status) img[v].status = bs[v].status;
        bin[v] = dgr::carve_binning(bs[v].binning_buffer, (size_t)bs[v].binning_capacity);
    }
    // One preprocess launch for all views needs the segment binning behind it (its epilogue leaves per-block instance
    // totals); frames whose segment tables do not fit LDS, or "lds_count" = 0, take the one-view front end per view.
    const dgr::BinPath path = bin_path(width, height, /*callback=*/false);
    if (path.segments) {
        dgr::PreprocessFwdBatchArgs b{};
        preprocess_scene(b.base, cv[0]);
        b.V = n_views;
        for (int v = 0; v < n_views; v++) {
            b.v[v].view = cv[v].viewmatrix; b.v[v].proj = cv[v].projmatrix; b.v[v].campos = cv[v].cam_pos;
            b.v[v].geom = geom[v]; b.v[v].radii_out = cv[v].radii; b.v[v].gau_uncertainty = cv[v].gau_uncertainty;
            b.v[v].gau_related_pixels = cv[v].gau_related_pixels;
        }
        { ScopedStage t(ST_PRE_FWD, st); HIP_TRY(dgr::launch_preprocess_fwd_batch(b, st)); }
    }
    const BatchPlan plan(st, n_views);
    if ((rc = batch_fork(st, plan.K))) return rc;
    BatchJoinGuard joined(st, plan.K);  // (an early return below still rejoins the helper streams)
    for (int v = 0; v < n_views; v++) {
        hipStream_t sv = plan.first_stream(v);
        const int cap = bs[v].binning_capacity;
        if (!path.segments && (rc = forward_front(cv[v], geom[v], img[v], sv, path, &bin[v], cap, bs[v].image_buffer))) return rc;
        if ((rc = binning_stages(cv[v], geom[v], img[v], bin[v], cap, sv, path, bs[v].binning_buffer, nullptr))) return rc;
        if ((rc = plan.hand_over(v, sv))) return rc;  // (pipeline: the blend on the caller's stream, behind the view's binning)
        if ((rc = forward_blend(cv[v], geom[v], img[v], bin[v], sv, full))) return rc;
    }
    return joined.done();
}

// absgrad (dgr_*_backward*_absgrad, dgr_hip.h): what is refused, before any device call
int absgrad_refused(bool wanted, int map_off) {
    if (!wanted) return DGR_OK;
    if (map_off) { set_last_error("absgrad: not with map_off (tracking forms no per-Gaussian gradients)"); return DGR_ERR_BAD_ARGUMENT; }
    if (opt_det_grads()) { set_last_error("absgrad: no deterministic form (deterministic_grads is set)"); return DGR_ERR_BAD_ARGUMENT; }
    if (opt_alpha_mode() == 2) { set_last_error("absgrad: needs alpha_mode 0 or 1 (not the glibc A/B form)"); return DGR_ERR_BAD_ARGUMENT; }
    return DGR_OK;
}
// deterministic gradients: behind the standard scratch, {per-block instance sums u32[blocks] | per-block pose partials
// double[blocks][12] | instance-major rows float[R][16]}
struct DetScratch {
    uint32_t* blk;
    double* pose;
    float* rows;
    size_t bytes;
};
DetScratch carve_det_scratch(char* base, int P, int R) {
    const size_t nb = ((size_t)(P > 0 ? P : 0) + 255) / 256;
    DetScratch d;
    size_t o = dgr::carve_backward_scratch(nullptr, P).bytes;
    d.blk = (uint32_t*)(base + o);  o = dgr::align_up(o + 4 * nb, 256);
    d.pose = (double*)(base + o);   o = dgr::align_up(o + 8 * 12 * nb, 256);
    d.rows = (float*)(base + o);    o = dgr::align_up(o + sizeof(float) * DGR_ACC_STRIDE * (size_t)(R > 0 ? R : 0), 256);
    d.bytes = o;
    return d;
}

// The body of dgr_light_forward_presized / dgr_full_forward_presized (full: the uncertainty image in c.out_alpha)
int forward_presized(hipStream_t st, const FwdCommon& c, char* geometry_buffer, char* binning_buffer, int binning_capacity,
                     char* image_buffer, int* status, bool full) {
    ArmedReport armed(c.W, c.H, c.P, st);  // (dgr_status_arm: completed from the host on every path that enqueues no binning kernel)
    int rc = check_common(c);
    if (rc) return rc;
    if (c.P == 0) {
        if (status) HIP_TRY(hipMemsetAsync(status, 0, 16, st));
        return zero_outputs(c, st);
    }
    // (the binning buffer also holds the segment binning's tables behind its per-instance arrays: dgr_binning_bytes() is
    //  non-zero for a capacity of 0, and a NULL buffer is never valid for P > 0)
    if (!geometry_buffer || !image_buffer || !binning_buffer || binning_capacity < 0) {
        set_last_error("presized forward: geometry, binning and image buffers are required (sizes: dgr_*_bytes)");
        return DGR_ERR_BAD_ARGUMENT;
    }
    dgr::GeometryView geom = dgr::carve_geometry(geometry_buffer, c.P);
    dgr::ImageView img = dgr::carve_image(image_buffer, c.W, c.H);
    if (status) img.status = status;  // the kernels write the caller's status word directly
    dgr::BinningView bin = dgr::carve_binning(binning_buffer, (size_t)binning_capacity);
    const dgr::BinPath path = bin_path(c.W, c.H, /*callback=*/false);
    if ((rc = forward_front(c, geom, img, st, path, &bin, binning_capacity, image_buffer))) return rc;
    if ((rc = binning_stages(c, geom, img, bin, binning_capacity, st, path, binning_buffer, &armed))) return rc;
    return forward_blend(c, geom, img, bin, st, full, &armed);
}

// The body of dgr_light_forward / dgr_full_forward.  num_related (full): the reference's second blocking read, or NULL.
int forward_callback(hipStream_t st, const FwdCommon& c, dgr_alloc_fn geometryBuffer, dgr_alloc_fn binningBuffer,
                     dgr_alloc_fn imageBuffer, void* alloc_user, bool full, int* num_related, int debug) {
    if (num_related) *num_related = 0;
    int rc = check_common(c);
    if (rc) return rc;
    // The callback entry points block the host to size the binning buffer, as the reference does (rasterizer_impl.cu:287): on a
    // capturing stream that synchronisation would fail AND invalidate the capture -- refuse before anything touches the stream.
    if (dgr_stream_is_capturing(st)) {
        set_last_error("the resize-callback forward blocks the host (it sizes the binning buffer): it cannot be captured into a graph -- use the presized entry point");
        return DGR_ERR_BAD_ARGUMENT;
    }
    if (c.P == 0) return zero_outputs(c, st);
    char* gptr = geometryBuffer(dgr_geometry_bytes(c.P), alloc_user);
    char* iptr = imageBuffer(dgr_image_bytes(c.W, c.H), alloc_user);
    if (!gptr || !iptr) { set_last_error("allocation callback returned NULL"); return DGR_ERR_ALLOC; }
    dgr::GeometryView geom = dgr::carve_geometry(gptr, c.P);
    dgr::ImageView img = dgr::carve_image(iptr, c.W, c.H);
    dgr::BinPath path = bin_path(c.W, c.H, /*callback=*/true);
    if ((rc = forward_front(c, geom, img, st, path, nullptr, 0, nullptr))) return rc;
    // the one blocking read the reference also has (rasterizer_impl.cu:287, F/...:435): num_rendered sizes the binning buffer
    int status[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(status, img.status, sizeof(status), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (status[2]) { set_last_error("Point is filtered although prefiltered is set. This shouldn't happen!"); return DGR_ERR_PREFILTERED; }
    const int R = status[0];
    char* bptr = nullptr;
    if (R > 0) {
        bptr = binningBuffer(dgr_binning_bytes(R, c.W, c.H), alloc_user);
        if (!bptr) { set_last_error("allocation callback returned NULL"); return DGR_ERR_ALLOC; }
    } else {
        binningBuffer(0, alloc_user);
    }
    dgr::BinningView bin = dgr::carve_binning(bptr, (size_t)R);
    // (also with R == 0: nothing to bin, and no buffer for the segment tables -- count_rank and scan_tiles write the empty range table)
    if (R <= 0) path.segments = false;
    if ((rc = binning_stages(c, geom, img, bin, R, st, path, bptr, nullptr))) return rc;
    if ((rc = forward_blend(c, geom, img, bin, st, full))) return rc;
    if (num_related) {  // second blocking read of the reference (F/cuda_rasterizer/rasterizer_impl.cu:498)
        HIP_TRY(hipMemcpyAsync(status, img.status, sizeof(status), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *num_related = status[3];
    }
    if (debug) HIP_TRY(hipStreamSynchronize(st));  // CHECK_CUDA(..., debug): L/cuda_rasterizer/auxiliary.h:166-173
    return R;
}

// ---- backward (one view, or a batch).  The scene's side -- the Gaussians, their gradients, the variant -- is a PreprocessBwdArgs
// whose per-view members are filled per view; the full variant is the light path with track_off = map_off = 0, full_variant = 1.
// One view's side, as the one-view entry points and the batches' view structs give it:
struct BwdView {
    char *geometry_buffer, *binning_buffer, *image_buffer;
    const float *viewmatrix, *projmatrix, *cam_pos, *perspec_matrix, *gt_depth;
    const int* radii;
    const float *alphas, *dL_dpix, *dL_dpix_depth, *dL_dpix_median_depth, *dL_dpix_depth_var;  // (light; full: dL_dpix only)
    const float *dL_depths, *dL_duncertainties;                                                 // (full)
    float *dL_dmean2D, *dL_dview, *dL_dmean2D_abs;
    const float* dL_dpix_silhouette;  // dL/d(opacity_map) (light) or the exact dL/d(uncertainty) (full), or NULL
    char* scratch;
    size_t scratch_bytes;
    int R;  // >= the view's num_rendered: sizes the deterministic row buffer
};
BwdView bwd_view(const dgr_light_view_grad& w, float* abs, const float* sil) {
    return BwdView{w.geometry_buffer, w.binning_buffer, w.image_buffer, w.viewmatrix, w.projmatrix, w.cam_pos, w.perspec_matrix,
                   w.gt_depth, w.radii, w.alphas, w.dL_dpix, w.dL_dpix_depth, w.dL_dpix_median_depth, w.dL_dpix_depth_var, nullptr,
                   nullptr, w.dL_dmean2D, w.dL_dview, abs, sil, w.scratch, w.scratch_bytes, w.num_rendered};
}
BwdView bwd_view(const dgr_full_view_grad& w, float* abs, const float* sil) {
    return BwdView{w.geometry_buffer, w.binning_buffer, w.image_buffer, w.viewmatrix, w.projmatrix, w.cam_pos, w.perspec_matrix,
                   w.gt_depth, w.radii, nullptr, w.dL_dpix, nullptr, nullptr, nullptr, w.dL_depths, w.dL_duncertainties,
                   w.dL_dmean2D, w.dL_dview, abs, sil, w.scratch, w.scratch_bytes, w.num_rendered};
}
dgr::PreprocessBwdArgs bwd_scene(int P, int D, int M, int W, int H, const float* means3D, const float* shs, const float* scales,
                                 float scale_modifier, const float* rotations, const float* cov3D_precomp, float tan_fovx,
                                 float tan_fovy, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D,
                                 float* dL_dsh, float* dL_dscale, float* dL_drot, int track_off, int map_off, int full) {
    dgr::PreprocessBwdArgs b{};
    b.P = P; b.D = D; b.M = M; b.W = W; b.H = H; b.means3D = means3D; b.shs = shs; b.scales = scales;
    b.rotations = rotations; b.scale_modifier = scale_modifier; b.cov3D_precomp = cov3D_precomp;
    b.tan_fovx = tan_fovx; b.tan_fovy = tan_fovy;
    b.focal_y = H / (2.0f * tan_fovy);
    b.focal_x = W / (2.0f * tan_fovx);
    b.sh_vec_ok = aligned16(shs) && aligned16(dL_dsh);
    b.track_off = track_off; b.map_off = map_off; b.full_variant = full;
    b.dL_dopacity = dL_dopacity; b.dL_dcolor = dL_dcolor; b.dL_dmean3D = dL_dmean3D; b.dL_dcov3D = dL_dcov3D; b.dL_dsh = dL_dsh;
    b.dL_dscale = dL_dscale; b.dL_drot = dL_drot;
    return b;
}

// M > 16: the per-Gaussian backward writes the 16 coefficients the SH basis has; the rest of every dL_dsh row is zero, as in the
// reference (which zero-fills the tensor), cleared here ahead of the kernel.  M <= 16 rows are written whole by the kernel.
int zero_wide_sh_rows(const dgr::PreprocessBwdArgs& b, hipStream_t st) {
    if (b.M > 16 && b.dL_dsh) { ScopedStage t(ST_ZERO, st); HIP_TRY(dgr::launch_zero_floats(b.dL_dsh, 3 * (size_t)b.P * (size_t)b.M, st)); }
    return DGR_OK;
}

// A view's state and scratch, carved
struct BwdBufs {
    dgr::GeometryView geom;
    dgr::ImageView img;
    dgr::BackwardScratch sc;
    DetScratch ds;
};
// Carves a view's buffers and clears what its blend backward adds into: the accumulator rows (unless the resident scratch is
// known to be clean), the absgrad output and, with deterministic_grads, the row buffer; then the Gaussians' first-instance offsets.
int bwd_view_prepare(const BwdView& w, int P, int W, int H, bool det, bool scratch_clean, BwdBufs& s, hipStream_t st) {
    s.geom = dgr::carve_geometry(w.geometry_buffer, P);
    s.img = dgr::carve_image(w.image_buffer, W, H);
    s.sc = dgr::carve_backward_scratch(w.scratch, P);
    s.ds = DetScratch{nullptr, nullptr, nullptr, 0};
    if (!scratch_clean) { ScopedStage t(ST_ZERO, st); HIP_TRY(dgr::launch_zero_fill(s.sc.acc, s.sc.zero_bytes, st)); }
    if (w.dL_dmean2D_abs) { ScopedStage t(ST_ZERO, st); HIP_TRY(dgr::launch_zero_floats(w.dL_dmean2D_abs, 3 * (size_t)P, st)); }
    if (det) {
        // (the Gaussians' first-instance offsets go into the geometry state's goff array, which only the global-counter binning
        //  of the FORWARD uses: free by now)
        s.ds = carve_det_scratch(w.scratch, P, w.R);
        { ScopedStage t(ST_ZERO, st); HIP_TRY(dgr::launch_zero_fill(s.ds.rows, sizeof(float) * DGR_ACC_STRIDE * (size_t)w.R, st)); }
        HIP_TRY(dgr::launch_det_offsets(P, s.geom.rect, s.ds.blk, s.geom.goff, st));
    }
    return DGR_OK;
}

// The blend backward of one view: what both variants' arguments share, then one function per variant that fills the rest and
// launches it (absgrad: the _abs instance)
template <class A>
void blend_bwd_common(A& r, const BwdView& w, const float* bg, int W, int H, const BwdBufs& s, bool det) {
    r.W = W; r.H = H; r.grid_x = dgr::tiles_x(W); r.grid_y = dgr::tiles_y(H);
    r.sched = s.img.tile_sched; r.ranges = s.img.ranges; r.sched_flag = s.img.cursor + 3; r.point_list = (const uint32_t*)w.binning_buffer;
    r.rec = s.geom.rec; r.bg = bg; r.gt_depth = w.gt_depth; r.n_contrib = s.img.n_contrib; r.acc = s.sc.acc;
    if (det) { r.det_rows = s.ds.rows; r.det_rect = s.geom.rect; r.det_goff = s.geom.goff; r.det_R = (uint32_t)w.R; }
}
int blend_bwd_light(const BwdView& w, const dgr::PreprocessBwdArgs& b, const float* bg, const BwdBufs& s, bool det, bool complete,
                    hipStream_t st) {
    dgr::RenderBwdLightArgs r{};
    blend_bwd_common(r, w, bg, b.W, b.H, s, det);
    r.alphas = w.alphas; r.dL_dpix = w.dL_dpix; r.dL_dpix_depth = w.dL_dpix_depth; r.dL_dpix_median = w.dL_dpix_median_depth;
    r.dL_dpix_var = w.dL_dpix_depth_var; r.dL_dpix_silhouette = w.dL_dpix_silhouette; r.live_counts = s.img.tile_count;
    // (complete pose gradient: the tracking blend's three sums are not enough -- the mapping blend backward forms all of them)
    r.means3D = b.means3D; r.view = w.viewmatrix; r.track_off = b.track_off; r.map_off = complete ? 0 : b.map_off;
    ScopedStage t(ST_RENDER_BWD, st);
    if (w.dL_dmean2D_abs) HIP_TRY(dgr::launch_render_bwd_light_abs(r, w.dL_dmean2D_abs, opt_alpha_mode(), st));
    else HIP_TRY(dgr::launch_render_bwd_light(r, opt_alpha_mode(), st));
    return DGR_OK;
}
int blend_bwd_full(const BwdView& w, const dgr::PreprocessBwdArgs& b, const float* bg, const BwdBufs& s, bool det, hipStream_t st) {
    dgr::RenderBwdFullArgs r{};
    blend_bwd_common(r, w, bg, b.W, b.H, s, det);
    r.final_T = s.img.final_T; r.first_contrib = s.img.first_contrib;
    r.dL_dpix = w.dL_dpix; r.dL_depths = w.dL_depths; r.dL_duncertainties = w.dL_duncertainties;
    r.dL_dpix_silhouette = w.dL_dpix_silhouette;
    ScopedStage t(ST_RENDER_BWD, st);
    if (w.dL_dmean2D_abs) HIP_TRY(dgr::launch_render_bwd_full_abs(r, w.dL_dmean2D_abs, opt_alpha_mode(), st));
    else HIP_TRY(dgr::launch_render_bwd_full(r, opt_alpha_mode(), st, det));
    return DGR_OK;
}
// ... and the gather of the deterministic rows into the accumulators behind it
int bwd_view_blend(const BwdView& w, const dgr::PreprocessBwdArgs& b, const float* bg, const BwdBufs& s, bool det, bool complete,
                   hipStream_t st) {
    const int rc = b.full_variant ? blend_bwd_full(w, b, bg, s, det, st) : blend_bwd_light(w, b, bg, s, det, complete, st);
    if (rc) return rc;
    if (det) HIP_TRY(dgr::launch_det_gather(b.P, s.geom.rect, s.geom.goff, s.ds.rows, (uint32_t)w.R, s.sc.acc, st));
    return DGR_OK;
}

// The per-view members of the per-Gaussian backward: PreprocessBwdArgs (one view) or a batch's BwdViewPart
template <class Q>
void bwd_view_part(Q& q, const BwdView& w, const BwdBufs& s, bool det) {
    q.det_pose = det ? s.ds.pose : nullptr;
    q.view = w.viewmatrix; q.proj = w.projmatrix; q.campos = w.cam_pos; q.perspec = w.perspec_matrix;
    q.radii = w.radii ? w.radii : s.geom.radii; q.geom = s.geom; q.acc = s.sc.acc; q.dL_dmean2D = w.dL_dmean2D;
    q.pose_part = s.sc.pose_part; q.ticket = s.sc.ticket; q.dL_dview = w.dL_dview;
}

// The body of dgr_{light,full}_backward[_absgrad|_silhouette]
int backward_one(hipStream_t st, dgr::PreprocessBwdArgs b, const float* background, const BwdView& w, int debug) {
    const bool scratch_clean = take_scratch_clean_arm();  // (consumed by every call, a refused one included)
    const int P = b.P, width = b.W, height = b.H, R = w.R;
    if (int rc = absgrad_refused(w.dL_dmean2D_abs != nullptr, b.map_off)) return rc;
    if (P < 0 || width <= 0 || height <= 0 || (long long)width * height > (1ll << 30)) { set_last_error("bad sizes"); return DGR_ERR_BAD_ARGUMENT; }
    if (b.D < 0 || b.D > 3) { set_last_error(BAD_DEGREE); return DGR_ERR_BAD_ARGUMENT; }
    if (P == 0) {  // L/rasterize_points.cu:188: nothing runs, gradients stay zero
        HIP_TRY(hipMemsetAsync(w.dL_dview, 0, 16 * 4, st));
        return DGR_OK;
    }
    const bool det = opt_det_grads() != 0 && !(b.track_off && b.map_off);
    const bool complete = opt_pose_grad() != 0 && !b.track_off;  // (track_off: no pose gradient, nothing to complete)
    if (det && opt_alpha_mode() != 0) { set_last_error("deterministic_grads needs alpha_mode 0"); return DGR_ERR_BAD_ARGUMENT; }
    if (det && R <= 0) { set_last_error("deterministic_grads: the backward needs R >= num_rendered (it sizes the instance-major row buffer)"); return DGR_ERR_BAD_ARGUMENT; }
    if (w.scratch_bytes < dgr_light_backward_scratch_bytes_r(P, width, height, R) || !w.scratch) {
        set_last_error(det ? "backward scratch too small (deterministic_grads: dgr_light_backward_scratch_bytes_r)" : "backward scratch too small");
        return DGR_ERR_BAD_ARGUMENT;
    }
    // (the 3D covariance is not kept by the forward: the backward re-forms it from scale and rotation -- the SAME tensors the
    //  forward saw, or the bits differ -- unless the caller precomputed it)
    if (!b.cov3D_precomp && (!b.scales || !b.rotations)) { set_last_error("backward: need scale/rotation or cov3D"); return DGR_ERR_BAD_ARGUMENT; }
    if (!w.geometry_buffer || !w.binning_buffer || !w.image_buffer) { set_last_error("backward: the forward's three state buffers are required"); return DGR_ERR_BAD_ARGUMENT; }
    BwdBufs s;
    if (int rc = bwd_view_prepare(w, P, width, height, det, scratch_clean, s, st)) return rc;
    if (int rc = bwd_view_blend(w, b, background, s, det, complete, st)) return rc;
    if (int rc = zero_wide_sh_rows(b, st)) return rc;
    bwd_view_part(b, w, s, det);
    b.clear_scratch = scratch_clean ? 1 : 0;
    { ScopedStage t(ST_PRE_BWD, st); HIP_TRY(dgr::launch_preprocess_bwd(b, st, complete)); }
    if (debug && !dgr_stream_is_capturing(st)) HIP_TRY(hipStreamSynchronize(st));  // (CHECK_CUDA(..., debug); a capturing stream cannot be waited for -- and the attempt would invalidate the capture)
    return DGR_OK;
}

// The inputs a view of a batch backward must have (the full blend backward reads gt_depth on every path, the lean one included)
bool bwd_view_complete(const BwdView& w, bool full) {
    if (!w.geometry_buffer || !w.binning_buffer || !w.image_buffer || !w.viewmatrix || !w.projmatrix || !w.cam_pos || !w.perspec_matrix)
        return false;
    if (full) return w.gt_depth && w.dL_dpix && w.dL_depths;
    return w.alphas && w.dL_dpix && w.dL_dpix_depth && w.dL_dpix_median_depth && w.dL_dpix_depth_var;
}

// The body of dgr_{light,full}_backward_batch[_absgrad|_silhouette]: per view the scheme of the one-view backward (without the resident
// scratch), the per-Gaussian backward once for all views
int backward_batch(hipStream_t st, dgr::PreprocessBwdArgs b, const float* background, int n_views, const BwdView* views) {
    const int P = b.P, width = b.W, height = b.H;
    const bool det = opt_det_grads() != 0 && !(b.track_off && b.map_off);
    const bool complete = opt_pose_grad() != 0 && !b.track_off;
    if (det && opt_alpha_mode() != 0) { set_last_error("deterministic_grads needs alpha_mode 0"); return DGR_ERR_BAD_ARGUMENT; }
    if (n_views < 1 || n_views > DGR_MAX_BATCH_VIEWS || !views) { set_last_error("1 .. DGR_MAX_BATCH_VIEWS views per batch"); return DGR_ERR_BAD_ARGUMENT; }
    bool any_abs = false;  // (absgrad: a NULL array or NULL entries -- those views as without it)
    for (int v = 0; v < n_views; v++) any_abs |= views[v].dL_dmean2D_abs != nullptr;
    if (int rc = absgrad_refused(any_abs, b.map_off)) return rc;
    if (P < 0 || width <= 0 || height <= 0 || (long long)width * height > (1ll << 30)) { set_last_error("bad sizes"); return DGR_ERR_BAD_ARGUMENT; }
    if (b.D < 0 || b.D > 3) { set_last_error(BAD_DEGREE); return DGR_ERR_BAD_ARGUMENT; }
    for (int v = 0; v < n_views; v++)
        if (!views[v].dL_dview) { set_last_error("view without dL_dview"); return DGR_ERR_BAD_ARGUMENT; }
    if (P > 0 && !b.cov3D_precomp && (!b.scales || !b.rotations)) { set_last_error("backward: need scale/rotation or cov3D"); return DGR_ERR_BAD_ARGUMENT; }
    if (P == 0) {  // L/rasterize_points.cu:188: nothing runs, gradients stay zero
        for (int v = 0; v < n_views; v++) HIP_TRY(hipMemsetAsync(views[v].dL_dview, 0, 16 * 4, st));
        return DGR_OK;
    }
    for (int v = 0; v < n_views; v++) {
        const BwdView& w = views[v];
        if (det && w.R <= 0) { set_last_error("deterministic_grads: every view needs num_rendered (it sizes the view's row buffer)"); return DGR_ERR_BAD_ARGUMENT; }
        const size_t need = dgr_light_backward_scratch_bytes_r(P, width, height, w.R);
        if (!w.scratch || w.scratch_bytes < need) { set_last_error("backward scratch too small"); return DGR_ERR_BAD_ARGUMENT; }
        if (!bwd_view_complete(w, b.full_variant != 0)) {
            set_last_error("view with a missing state buffer, camera or gradient image");
            return DGR_ERR_BAD_ARGUMENT;
        }
    }
    int rc;
    if ((rc = batch_streams_ready())) return rc;
    const BatchPlan plan(st, n_views);
    dgr::PreprocessBwdBatchArgs bb{};
    bb.base = b;
    if ((rc = batch_fork(st, plan.K))) return rc;
    BatchJoinGuard joined(st, plan.K);  // (an early return below still rejoins the helper streams)
    for (int v = 0; v < n_views; v++) {
        const BwdView& w = views[v];
        hipStream_t sv = plan.first_stream(v);
        BwdBufs s;
        if ((rc = bwd_view_prepare(w, P, width, height, det, false, s, sv))) return rc;
        if ((rc = plan.hand_over(v, sv))) return rc;  // (pipeline: the blend backward on the caller's stream, behind the cleared scratch)
        if ((rc = bwd_view_blend(w, b, background, s, det, complete, sv))) return rc;
        bwd_view_part(bb.v[v], w, s, det);
    }
    if ((rc = joined.done())) return rc;
    bb.V = n_views;
    if ((rc = zero_wide_sh_rows(b, st))) return rc;
    { ScopedStage t(ST_PRE_BWD, st); HIP_TRY(dgr::launch_preprocess_bwd_batch(bb, st, complete)); }
    return DGR_OK;
}
// the batch's view structs as BwdView (as many as the batch may hold: backward_batch checks n_views)
template <class G>
int backward_batch_views(hipStream_t st, const dgr::PreprocessBwdArgs& b, const float* background, int n_views, const G* views,
                         float* const* dL_dmean2D_abs, const float* const* dL_dpix_silhouette) {
    BwdView bv[DGR_MAX_BATCH_VIEWS];
    for (int v = 0; views && v < n_views && v < DGR_MAX_BATCH_VIEWS; v++)
        bv[v] = bwd_view(views[v], dL_dmean2D_abs ? dL_dmean2D_abs[v] : nullptr, dL_dpix_silhouette ? dL_dpix_silhouette[v] : nullptr);
    return backward_batch(st, b, background, n_views, views ? bv : nullptr);
}
}  // namespace

extern "C" {

const char* dgr_last_error(void) { return g_last_error.c_str(); }
const char* dgr_version(void) { return "dgr_hip 0.1 gfx950"; }

size_t dgr_geometry_bytes(int P) { return dgr::carve_geometry(nullptr, P).bytes; }
size_t dgr_image_bytes(int width, int height) { return dgr::carve_image(nullptr, width, height).bytes; }
size_t dgr_binning_bytes(int cap, int width, int height) {
    // the sorted list, key scratch, ranks / pair columns and pair keys of `cap` instances, then the forward-only tables of
    // the segment binning
    return dgr::carve_binning(nullptr, (size_t)(cap > 0 ? cap : 0)).bytes + dgr::carve_segment_tables(nullptr, width, height).bytes;
}
size_t dgr_light_backward_scratch_bytes(int P, int, int) { return dgr::carve_backward_scratch(nullptr, P).bytes; }
size_t dgr_light_backward_scratch_bytes_r(int P, int W, int H, int R) {
    if (!opt_det_grads()) return dgr_light_backward_scratch_bytes(P, W, H);
    return carve_det_scratch(nullptr, P, R).bytes;
}

int dgr_mark_visible(void* stream, int P, const float* means3D, const float* viewmatrix, const float*, uint8_t* present) {
    HIP_TRY(dgr::launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream));
    return DGR_OK;
}


int dgr_light_forward_presized(void* stream, char* geometry_buffer, char* binning_buffer, int binning_capacity,
                               char* image_buffer, int* status, int P, int D, int M, const float* background,
                               int width, int height, const float* means3D, const float* shs,
                               const float* colors_precomp, const float* opacities, const float* scales,
                               float scale_modifier, const float* rotations, const float* cov3D_precomp,
                               const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                               float tan_fovx, float tan_fovy, int prefiltered, float* out_color, float* out_depth,
                               float* out_median_depth, float* out_alpha, const float* gt_depth,
                               float* out_depth_var, float* gau_uncertainty, int* gau_related_pixels, int* radii) {
    const FwdCommon c = light_common(P, D, M, background, width, height, means3D, shs, colors_precomp, opacities, scales,
                                     scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
                                     prefiltered, out_color, out_depth, out_median_depth, out_alpha, gt_depth, out_depth_var,
                                     gau_uncertainty, gau_related_pixels, radii);
    return forward_presized((hipStream_t)stream, c, geometry_buffer, binning_buffer, binning_capacity, image_buffer, status, false);
}

int dgr_light_forward(void* stream, dgr_alloc_fn geometryBuffer, dgr_alloc_fn binningBuffer, dgr_alloc_fn imageBuffer,
                      void* alloc_user, int P, int D, int M, const float* background, int width, int height,
                      const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                      const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                      const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                      float tan_fovy, int prefiltered, float* out_color, float* out_depth, float* out_median_depth,
                      float* out_alpha, const float* gt_depth, float* out_depth_var, float* gau_uncertainty,
                      int* gau_related_pixels, int* radii, int debug) {
    const FwdCommon c = light_common(P, D, M, background, width, height, means3D, shs, colors_precomp, opacities, scales,
                                     scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
                                     prefiltered, out_color, out_depth, out_median_depth, out_alpha, gt_depth, out_depth_var,
                                     gau_uncertainty, gau_related_pixels, radii);
    return forward_callback((hipStream_t)stream, c, geometryBuffer, binningBuffer, imageBuffer, alloc_user, false, nullptr, debug);
}

int dgr_light_backward(void* stream, int P, int D, int M, int R, const float* background, int width, int height,
                       const float* means3D, const float* shs, const float* colors_precomp, const float* alphas,
                       const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                       float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                       const float* dL_dpix, const float* dL_dpix_depth, const float* dL_dpix_median_depth,
                       const float* dL_dpix_depth_var, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                       float* dL_dcolor, float* dL_ddepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                       float* dL_dscale, float* dL_drot, int debug, float* dgndcs_dviewmatrix,
                       const float* perspec_matrix, float* dL_dview, float* dg_camd_dviewmatrix,
                       const float* gt_depth, int track_off, int map_off, char* scratch, size_t scratch_bytes) {
    return dgr_light_backward_absgrad(stream, P, D, M, R, background, width, height, means3D, shs, colors_precomp, alphas, scales,
                                      scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy,
                                      radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dpix_depth,
                                      dL_dpix_median_depth, dL_dpix_depth_var, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor,
                                      dL_ddepth, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, debug, dgndcs_dviewmatrix,
                                      perspec_matrix, dL_dview, dg_camd_dviewmatrix, gt_depth, track_off, map_off, scratch,
                                      scratch_bytes, nullptr);
}
int dgr_light_backward_absgrad(void* stream, int P, int D, int M, int R, const float* background, int width, int height,
                               const float* means3D, const float* shs, const float* colors_precomp, const float* alphas,
                               const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                               const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                               float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                               const float* dL_dpix, const float* dL_dpix_depth, const float* dL_dpix_median_depth,
                               const float* dL_dpix_depth_var, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                               float* dL_dcolor, float* dL_ddepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                               float* dL_dscale, float* dL_drot, int debug, float* dgndcs_dviewmatrix,
                               const float* perspec_matrix, float* dL_dview, float* dg_camd_dviewmatrix,
                               const float* gt_depth, int track_off, int map_off, char* scratch, size_t scratch_bytes, float* dL_dmean2D_abs) {
    return dgr_light_backward_silhouette(stream, P, D, M, R, background, width, height, means3D, shs, colors_precomp, alphas, scales,
                                         scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy,
                                         radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dpix_depth,
                                         dL_dpix_median_depth, dL_dpix_depth_var, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor,
                                         dL_ddepth, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, debug, dgndcs_dviewmatrix,
                                         perspec_matrix, dL_dview, dg_camd_dviewmatrix, gt_depth, track_off, map_off, scratch,
                                         scratch_bytes, dL_dmean2D_abs, nullptr);
}
int dgr_light_backward_silhouette(void* stream, int P, int D, int M, int R, const float* background, int width, int height,
                               const float* means3D, const float* shs, const float* colors_precomp, const float* alphas,
                               const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                               const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                               float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                               const float* dL_dpix, const float* dL_dpix_depth, const float* dL_dpix_median_depth,
                               const float* dL_dpix_depth_var, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                               float* dL_dcolor, float* dL_ddepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                               float* dL_dscale, float* dL_drot, int debug, float* dgndcs_dviewmatrix,
                               const float* perspec_matrix, float* dL_dview, float* dg_camd_dviewmatrix,
                               const float* gt_depth, int track_off, int map_off, char* scratch, size_t scratch_bytes, float* dL_dmean2D_abs,
                               const float* dL_dpix_silhouette) {
    (void)dgndcs_dviewmatrix; (void)dg_camd_dviewmatrix; (void)colors_precomp;
    dgr::PreprocessBwdArgs b = bwd_scene(P, D, M, width, height, means3D, shs, scales, scale_modifier, rotations, cov3D_precomp,
                                         tan_fovx, tan_fovy, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale,
                                         dL_drot, track_off, map_off, 0);
    b.dL_dconic = dL_dconic; b.dL_ddepth = dL_ddepth;
    const BwdView w{geom_buffer, binning_buffer, image_buffer, viewmatrix, projmatrix, campos, perspec_matrix, gt_depth, radii,
                    alphas, dL_dpix, dL_dpix_depth, dL_dpix_median_depth, dL_dpix_depth_var, nullptr, nullptr, dL_dmean2D, dL_dview,
                    dL_dmean2D_abs, dL_dpix_silhouette, scratch, scratch_bytes, R};
    return backward_one((hipStream_t)stream, b, background, w, debug);
}

// ------------------------------------------------------------------------------------------------ full variant
int dgr_full_forward_presized(void* stream, char* geometry_buffer, char* binning_buffer, int binning_capacity,
                              char* image_buffer, int* status, int P, int D, int M, const float* background, int width,
                              int height, const float* means3D, const float* shs, const float* colors_precomp,
                              const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                              const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                              const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                              float* out_depth, const float* gt_depth, float* out_uncertainty, int* radii) {
    const FwdCommon c = full_common(P, D, M, background, width, height, means3D, shs, colors_precomp, opacities, scales,
                                    scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
                                    prefiltered, out_color, out_depth, gt_depth, out_uncertainty, radii);
    return forward_presized((hipStream_t)stream, c, geometry_buffer, binning_buffer, binning_capacity, image_buffer, status, true);
}

int dgr_full_forward(void* stream, dgr_alloc_fn geometryBuffer, dgr_alloc_fn binningBuffer, dgr_alloc_fn imageBuffer,
                     void* alloc_user, int P, int D, int M, const float* background, int width, int height,
                     const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                     const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                     const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                     float tan_fovy, int prefiltered, float* out_color, float* out_depth, const float* gt_depth,
                     float* out_uncertainty, int* radii, int* num_related_primitives) {
    const FwdCommon c = full_common(P, D, M, background, width, height, means3D, shs, colors_precomp, opacities, scales,
                                    scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
                                    prefiltered, out_color, out_depth, gt_depth, out_uncertainty, radii);
    return forward_callback((hipStream_t)stream, c, geometryBuffer, binningBuffer, imageBuffer, alloc_user, true,
                            num_related_primitives, 0);
}

int dgr_full_backward(void* stream, int P, int D, int M, int R, const float* background, int width, int height,
                      const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                      float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                      const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                      char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix,
                      const float* dL_depths, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                      float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                      float* dpixel_dgc, int* gau_id_list, int* pix_id_list, float* dgc_dCam_position, float* dpixel_dndcs,
                      const float* perspec_matrix, float* dgndcs_dviewmatrix, float* dpixel_dinvcovs,
                      float* dgc_invcovs_dT, float* dL_dview, float* dL_dgau_depth, float* ddepth_dndcs,
                      float* ddepth_dinvcovs, const float* gt_depth, const float* dL_duncertainties, char* scratch,
                      size_t scratch_bytes) {
    return dgr_full_backward_absgrad(stream, P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales,
                                     scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy,
                                     radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_depths, dL_dmean2D, dL_dconic,
                                     dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, dpixel_dgc,
                                     gau_id_list, pix_id_list, dgc_dCam_position, dpixel_dndcs, perspec_matrix, dgndcs_dviewmatrix,
                                     dpixel_dinvcovs, dgc_invcovs_dT, dL_dview, dL_dgau_depth, ddepth_dndcs, ddepth_dinvcovs,
                                     gt_depth, dL_duncertainties, scratch, scratch_bytes, nullptr);
}
int dgr_full_backward_absgrad(void* stream, int P, int D, int M, int R, const float* background, int width, int height,
                              const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                              float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                              char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix,
                              const float* dL_depths, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                              float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                              float* dpixel_dgc, int* gau_id_list, int* pix_id_list, float* dgc_dCam_position, float* dpixel_dndcs,
                              const float* perspec_matrix, float* dgndcs_dviewmatrix, float* dpixel_dinvcovs,
                              float* dgc_invcovs_dT, float* dL_dview, float* dL_dgau_depth, float* ddepth_dndcs,
                              float* ddepth_dinvcovs, const float* gt_depth, const float* dL_duncertainties, char* scratch,
                              size_t scratch_bytes, float* dL_dmean2D_abs) {
    return dgr_full_backward_silhouette(stream, P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales,
                                        scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy,
                                        radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_depths, dL_dmean2D, dL_dconic,
                                        dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, dpixel_dgc,
                                        gau_id_list, pix_id_list, dgc_dCam_position, dpixel_dndcs, perspec_matrix, dgndcs_dviewmatrix,
                                        dpixel_dinvcovs, dgc_invcovs_dT, dL_dview, dL_dgau_depth, ddepth_dndcs, ddepth_dinvcovs,
                                        gt_depth, dL_duncertainties, scratch, scratch_bytes, dL_dmean2D_abs, nullptr);
}
int dgr_full_backward_silhouette(void* stream, int P, int D, int M, int R, const float* background, int width, int height,
                              const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                              float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                              char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix,
                              const float* dL_depths, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                              float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                              float* dpixel_dgc, int* gau_id_list, int* pix_id_list, float* dgc_dCam_position, float* dpixel_dndcs,
                              const float* perspec_matrix, float* dgndcs_dviewmatrix, float* dpixel_dinvcovs,
                              float* dgc_invcovs_dT, float* dL_dview, float* dL_dgau_depth, float* ddepth_dndcs,
                              float* ddepth_dinvcovs, const float* gt_depth, const float* dL_duncertainties, char* scratch,
                              size_t scratch_bytes, float* dL_dmean2D_abs, const float* dL_dpix_silhouette) {
    (void)colors_precomp; (void)dpixel_dgc; (void)gau_id_list; (void)pix_id_list; (void)dgc_dCam_position;
    (void)dpixel_dndcs; (void)dgndcs_dviewmatrix; (void)dpixel_dinvcovs; (void)dgc_invcovs_dT; (void)ddepth_dndcs;
    (void)ddepth_dinvcovs;
    dgr::PreprocessBwdArgs b = bwd_scene(P, D, M, width, height, means3D, shs, scales, scale_modifier, rotations, cov3D_precomp,
                                         tan_fovx, tan_fovy, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale,
                                         dL_drot, 0, 0, 1);
    b.dL_dconic = dL_dconic; b.dL_ddepth = dL_dgau_depth;
    const BwdView w{geom_buffer, binning_buffer, image_buffer, viewmatrix, projmatrix, campos, perspec_matrix, gt_depth, radii,
                    nullptr, dL_dpix, nullptr, nullptr, nullptr, dL_depths, dL_duncertainties, dL_dmean2D, dL_dview,
                    dL_dmean2D_abs, dL_dpix_silhouette, scratch, scratch_bytes, R};
    return backward_one((hipStream_t)stream, b, background, w, 0);
}

int dgr_light_forward_batch(void* stream, int n_views, const dgr_light_view* views, int P, int D, int M,
                            const float* background, int width, int height, const float* means3D, const float* shs,
                            const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                            const float* rotations, const float* cov3D_precomp, float tan_fovx, float tan_fovy, int prefiltered) {
    if (n_views < 1 || n_views > DGR_MAX_BATCH_VIEWS || !views) { set_last_error("1 .. DGR_MAX_BATCH_VIEWS views per batch"); return DGR_ERR_BAD_ARGUMENT; }
    FwdCommon cv[DGR_MAX_BATCH_VIEWS];
    BatchViewState bs[DGR_MAX_BATCH_VIEWS];
    for (int v = 0; v < n_views; v++) {
        const dgr_light_view& w = views[v];
        cv[v] = light_common(P, D, M, background, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier,
                             rotations, cov3D_precomp, w.viewmatrix, w.projmatrix, w.cam_pos, tan_fovx, tan_fovy, prefiltered,
                             w.out_color, w.out_depth, w.out_median_depth, w.out_alpha, w.gt_depth, w.out_depth_var,
                             w.gau_uncertainty, w.gau_related_pixels, w.radii);
        bs[v] = BatchViewState{w.geometry_buffer, w.binning_buffer, w.binning_capacity, w.image_buffer, w.status};
    }
    return forward_batch((hipStream_t)stream, n_views, cv, bs, false);
}

int dgr_full_forward_batch(void* stream, int n_views, const dgr_full_view* views, int P, int D, int M,
                           const float* background, int width, int height, const float* means3D, const float* shs,
                           const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                           const float* rotations, const float* cov3D_precomp, float tan_fovx, float tan_fovy, int prefiltered) {
    if (n_views < 1 || n_views > DGR_MAX_BATCH_VIEWS || !views) { set_last_error("1 .. DGR_MAX_BATCH_VIEWS views per batch"); return DGR_ERR_BAD_ARGUMENT; }
    FwdCommon cv[DGR_MAX_BATCH_VIEWS];
    BatchViewState bs[DGR_MAX_BATCH_VIEWS];
    for (int v = 0; v < n_views; v++) {
        const dgr_full_view& w = views[v];
        cv[v] = full_common(P, D, M, background, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier,
                            rotations, cov3D_precomp, w.viewmatrix, w.projmatrix, w.cam_pos, tan_fovx, tan_fovy, prefiltered,
                            w.out_color, w.out_depth, w.gt_depth, w.out_uncertainty, w.radii);
        bs[v] = BatchViewState{w.geometry_buffer, w.binning_buffer, w.binning_capacity, w.image_buffer, w.status};
    }
    return forward_batch((hipStream_t)stream, n_views, cv, bs, true);
}

int dgr_light_backward_batch(void* stream, int n_views, const dgr_light_view_grad* views, int P, int D, int M,
                             const float* background, int width, int height, const float* means3D, const float* shs,
                             const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                             const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity, float* dL_dcolor,
                             float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                             int track_off, int map_off) {
    return dgr_light_backward_batch_absgrad(stream, n_views, views, P, D, M, background, width, height, means3D, shs,
                                            colors_precomp, scales, scale_modifier, rotations, cov3D_precomp, tan_fovx, tan_fovy,
                                            dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, track_off,
                                            map_off, nullptr);
}
int dgr_light_backward_batch_absgrad(void* stream, int n_views, const dgr_light_view_grad* views, int P, int D, int M,
                                     const float* background, int width, int height, const float* means3D, const float* shs,
                                     const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                                     const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity, float* dL_dcolor,
                                     float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                     int track_off, int map_off, float* const* dL_dmean2D_abs) {
    return dgr_light_backward_batch_silhouette(stream, n_views, views, P, D, M, background, width, height, means3D, shs,
                                               colors_precomp, scales, scale_modifier, rotations, cov3D_precomp, tan_fovx, tan_fovy,
                                               dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, track_off,
                                               map_off, dL_dmean2D_abs, nullptr);
}
int dgr_light_backward_batch_silhouette(void* stream, int n_views, const dgr_light_view_grad* views, int P, int D, int M,
                                        const float* background, int width, int height, const float* means3D, const float* shs,
                                        const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                                        const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity,
                                        float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                                        float* dL_drot, int track_off, int map_off, float* const* dL_dmean2D_abs,
                                        const float* const* dL_dpix_silhouette) {
    (void)colors_precomp;
    const dgr::PreprocessBwdArgs b = bwd_scene(P, D, M, width, height, means3D, shs, scales, scale_modifier, rotations, cov3D_precomp,
                                               tan_fovx, tan_fovy, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale,
                                               dL_drot, track_off, map_off, 0);
    return backward_batch_views((hipStream_t)stream, b, background, n_views, views, dL_dmean2D_abs, dL_dpix_silhouette);
}

int dgr_full_backward_batch(void* stream, int n_views, const dgr_full_view_grad* views, int P, int D, int M,
                            const float* background, int width, int height, const float* means3D, const float* shs,
                            const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                            const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity, float* dL_dcolor,
                            float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot) {
    return dgr_full_backward_batch_absgrad(stream, n_views, views, P, D, M, background, width, height, means3D, shs, colors_precomp,
                                           scales, scale_modifier, rotations, cov3D_precomp, tan_fovx, tan_fovy, dL_dopacity,
                                           dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, nullptr);
}
int dgr_full_backward_batch_absgrad(void* stream, int n_views, const dgr_full_view_grad* views, int P, int D, int M,
                                    const float* background, int width, int height, const float* means3D, const float* shs,
                                    const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                                    const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity, float* dL_dcolor,
                                    float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, float* const* dL_dmean2D_abs) {
    return dgr_full_backward_batch_silhouette(stream, n_views, views, P, D, M, background, width, height, means3D, shs,
                                              colors_precomp, scales, scale_modifier, rotations, cov3D_precomp, tan_fovx, tan_fovy,
                                              dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot,
                                              dL_dmean2D_abs, nullptr);
}
int dgr_full_backward_batch_silhouette(void* stream, int n_views, const dgr_full_view_grad* views, int P, int D, int M,
                                       const float* background, int width, int height, const float* means3D, const float* shs,
                                       const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                                       const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity,
                                       float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                                       float* dL_drot, float* const* dL_dmean2D_abs, const float* const* dL_dpix_silhouette) {
    (void)colors_precomp;
    const dgr::PreprocessBwdArgs b = bwd_scene(P, D, M, width, height, means3D, shs, scales, scale_modifier, rotations, cov3D_precomp,
                                               tan_fovx, tan_fovy, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale,
                                               dL_drot, 0, 0, 1);
    return backward_batch_views((hipStream_t)stream, b, background, n_views, views, dL_dmean2D_abs, dL_dpix_silhouette);
}

int dgr_debug_bin_tiles_trace(unsigned long long* device_words) {
    dgr::g_bin_tiles_trace = device_words;
    return DGR_OK;
}
int dgr_debug_wave_reduce(void* stream, const float* in, float* out16, float* out12, float* out4, int* comp16, int* comp12,
                          int* comp4) {
    HIP_TRY(dgr::launch_wave_reduce_test(in, out16, out12, out4, comp16, comp12, comp4, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_debug_half_reduce(void* stream, const float* in, float* r0, float* r1, float* h3, int* slot0, int* slot1, int* comp3) {
    HIP_TRY(dgr::launch_half_reduce_test(in, r0, r1, h3, slot0, slot1, comp3, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_debug_half_reduce16(void* stream, const float* in, float* r0, float* r1, int* slot0, int* slot1) {
    HIP_TRY(dgr::launch_half_reduce16_test(in, r0, r1, slot0, slot1, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_debug_lane_lists(void* stream, const unsigned char* codes, unsigned* paired, unsigned* halves) {
    HIP_TRY(dgr::launch_lane_lists_test(codes, paired, halves, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_debug_exact_math(void* stream, int n, const float* x, const float* a, const float* b, float* out_exp, float* out_div) {
    if (n < 0 || (n > 0 && (!x || !a || !b || !out_exp || !out_div))) {
        set_last_error("dgr_debug_exact_math: bad argument");
        return DGR_ERR_BAD_ARGUMENT;
    }
    HIP_TRY(dgr::launch_exact_math_test(n, x, a, b, out_exp, out_div, opt_alpha_mode(), (hipStream_t)stream));
    return DGR_OK;
}
int dgr_debug_tile_sort(void* stream, int mode, int n_lists, const unsigned long long* keys, const int* offsets, unsigned* out_ids,
                        unsigned long long* out_keys) {
    const bool ids = mode == DGR_TILE_SORT_WAVE || mode == DGR_TILE_SORT_MERGE;
    if (mode < DGR_TILE_SORT_WAVE || mode > DGR_TILE_SORT_GLOBAL_256 || n_lists < 0 ||
        (n_lists > 0 && (!keys || !offsets || (ids ? !out_ids : !out_keys)))) {
        set_last_error("dgr_debug_tile_sort: bad argument");
        return DGR_ERR_BAD_ARGUMENT;
    }
    if (n_lists == 0) return DGR_OK;
    // the lengths each routine is called with in the binning kernels (and what its LDS array holds)
    const int lo = mode == DGR_TILE_SORT_MERGE ? 1025 : 1;
    const int hi = mode == DGR_TILE_SORT_WAVE ? 1024 : mode == DGR_TILE_SORT_PART ? 512 : mode == DGR_TILE_SORT_MERGE ? 6144 : 0x7fffffff;
    for (int b = 0; b < n_lists; b++) {
        const long long n = (long long)offsets[b + 1] - offsets[b];
        if (offsets[b] < 0 || n < lo || n > hi) {
            set_last_error("dgr_debug_tile_sort: list " + std::to_string(b) + " has " + std::to_string(n) + " keys, mode " +
                           std::to_string(mode) + " takes " + std::to_string(lo) + " .. " + std::to_string(hi));
            return DGR_ERR_BAD_ARGUMENT;
        }
    }
    int* d_off = nullptr;  // (a debug entry: its own allocation, and the call returns when the sort has finished)
    const size_t bytes = ((size_t)n_lists + 1) * sizeof(int);
    HIP_TRY(hipMalloc((void**)&d_off, bytes));
    hipError_t rc = hipMemcpy(d_off, offsets, bytes, hipMemcpyHostToDevice);
    if (rc == hipSuccess) rc = dgr::launch_tile_sort_test(mode, n_lists, (const uint64_t*)keys, d_off, out_ids, (uint64_t*)out_keys, (hipStream_t)stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(d_off);
    HIP_TRY(rc);
    return DGR_OK;
}
}  // extern "C"
