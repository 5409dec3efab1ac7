// kernels.h -- argument blocks and launch entry points of the gfx950 kernels (internal).
#pragma once
#include <hip/hip_ext.h>
#include "dgr_common.h"
#include "../../include/dgr_hip.h"  // dgr_densify_tensor, dgr_seed_tensor, dgr_relocate_tensor, dgr_transform_tensor

namespace dgr {

// Kernel launches go through dgr::launch().  When the profiler (dgr_profile_*) brackets a stage it sets
// `g_launch_events` for the calling thread and the next kernel is launched with hipExtLaunchKernelGGL, which puts
// the two events into the kernel's own dispatch packet: they hold the kernel's start and end, the same
// timestamps rocprofv3 reports, also when other streams keep the GPU busy (a hipEventRecord bracket would include
// the time the kernel's waves wait for compute units).
struct LaunchEvents {
    hipEvent_t start, stop;
    bool used;
};
extern thread_local LaunchEvents* g_launch_events;  // profile.hip

template <typename K, typename... Args>
inline void launch(K kernel, dim3 grid, dim3 block, hipStream_t stream, Args... args) {
    LaunchEvents* ev = g_launch_events;
    if (ev && !ev->used) {
        ev->used = true;
        hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, ev->start, ev->stop, 0, args...);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
    }
}
template <typename K, typename... Args>
inline void launch_shmem(K kernel, dim3 grid, dim3 block, size_t shmem, hipStream_t stream, Args... args) {
    LaunchEvents* ev = g_launch_events;
    if (ev && !ev->used) {
        ev->used = true;
        hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, ev->start, ev->stop, 0, args...);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, shmem, stream, args...);
    }
}

// Blend kernels, when several views are in flight: they run at 8 workgroups per CU, i.e. they hold every wave slot, the
// whole register file and 144 of the 160 KB of LDS, so another stream's kernels enter a CU only as blend workgroups drain.
// dgr_set_option("blend_wgs_per_cu", n) (3 <= n <= 7; 0 = no cap) pads each blend workgroup with unused dynamic LDS so
// that at most n fit a CU, which leaves wave slots, registers and LDS for the other views' bandwidth- and latency-bound
// kernels.  blend_pad_bytes() (options.hip) caches the kernels' static LDS sizes.
size_t blend_pad_bytes(const void* kernel);
template <typename K, typename... Args>
inline void launch_blend(K kernel, dim3 grid, dim3 block, hipStream_t stream, Args... args) {
    launch_shmem(kernel, grid, block, blend_pad_bytes(reinterpret_cast<const void*>(kernel)), stream, args...);
}

struct PreprocessFwdArgs {
    int P, D, M, W, H, grid_x, grid_y;
    const float* means3D;
    const float* scales;
    float scale_modifier;
    const float* rotations;
    const float* opacities;
    const float* shs;
    const float* cov3D_precomp;
    const float* colors_precomp;
    const float* view;
    const float* proj;
    const float* campos;
    float tan_fovx, tan_fovy, focal_x, focal_y;
    int prefiltered;
    int tight_cull;        // dgr_set_option("tight_cull"): alpha-aware tile rectangles (changes the integer path)
    bool sh_vec_ok;
    GeometryView geom;
    int* radii_out;        // caller's radii tensor (may be NULL)
    uint32_t* zero_words;  // n_zero_words 32-bit words to clear (the padded tile counters)
    int n_zero_words;
    float* gau_uncertainty;   // [P] cleared here, accumulated by the forward blend (may be NULL)
    int* gau_related_pixels;  // [P] likewise
    // presized path (binning buffer exists before the kernel runs): the block also takes the per-instance tile-counter
    // atomics and stores the arrival ranks -- count_rank.h; offsets come from a global cursor, not from a scan over P.
    // The counters and the cursor must be zero when the kernel starts (launch_zero_fill before it).
    int fused_count;
    uint32_t* tile_count;
    uint32_t* cursor;
    uint32_t* ranks;
    int capacity;
};

// ---- batched views: what differs between the views of a batch; everything else is in `base`
#ifndef DGR_MAX_BATCH_VIEWS
#define DGR_MAX_BATCH_VIEWS 8  // (also in include/dgr_hip.h)
#endif
struct FwdViewPart {
    const float* view;
    const float* proj;
    const float* campos;
    GeometryView geom;
    int* radii_out;
    float* gau_uncertainty;
    int* gau_related_pixels;
};
struct PreprocessFwdBatchArgs {
    PreprocessFwdArgs base;  // view / proj / campos / geom / radii_out / gau_* unused
    int V;
    FwdViewPart v[DGR_MAX_BATCH_VIEWS];
};

struct PreprocessBwdArgs {
    int P, D, M, W, H;
    const float* means3D;
    const int* radii;
    const float* shs;
    const float* scales;
    const float* rotations;
    float scale_modifier;
    const float* cov3D_precomp;
    const float* view;
    const float* proj;
    const float* campos;
    const float* perspec;
    float tan_fovx, tan_fovy, focal_x, focal_y;
    bool sh_vec_ok;
    int track_off, map_off;
    int full_variant;   // 1: semantics of F/cuda_rasterizer/backward.cu (computeCov2DCUDA assigns + depth term, pose from
                        //    dgc_dCampos / colour-only ndc sums / front-most depth sums); 0: light
    GeometryView geom;
    float* acc;         // [P,16] sums written by the blend backward
    double* det_pose;   // deterministic gradients: [blocks, 12] per-block pose partials (NULL: the 64 bucket rows, double atomics)
    int clear_scratch;  // 1: leave the scratch as it was found -- all zero: every accumulator row read is cleared by its reader and
                        //    the block that finishes the pose sum clears the buckets and the ticket (dgr_backward_scratch_clean_arm)
    float* dL_dmean2D;  // [P,3]
    float* dL_dconic;   // [P,4] optional
    float* dL_dopacity; // [P]
    float* dL_dcolor;   // [P,3] optional
    float* dL_ddepth;   // [P]   optional
    float* dL_dmean3D;  // [P,3]
    float* dL_dcov3D;   // [P,6]
    float* dL_dsh;      // [P,M,3] optional (M == 0)
    float* dL_dscale;   // [P,3]
    float* dL_drot;     // [P,4]
    double* pose_part;  // [DGR_POSE_BUCKETS,12], zero on entry
    uint32_t* ticket;   // zero on entry
    float* dL_dview;    // [16] written by the last block to deliver its pose partial
};

struct BwdViewPart {
    const float* view;
    const float* proj;
    const float* campos;
    const float* perspec;
    const int* radii;
    GeometryView geom;
    const float* acc;     // this view's accumulator rows (its backward scratch)
    float* dL_dmean2D;    // [P,3] per view (densification statistics are per view); may be NULL
    double* pose_part;
    uint32_t* ticket;
    float* dL_dview;      // [16]
    double* det_pose;     // deterministic gradients: this view's [blocks, 12] per-block pose partials (NULL otherwise; all views alike)
};
struct PreprocessBwdBatchArgs {
    PreprocessBwdArgs base;  // the per-view members unused; the dense outputs receive the SUM over the views; full_variant
                             // selects the kernel instance (dL_dconic / dL_ddepth: not written by a batch)
    int V;
    BwdViewPart v[DGR_MAX_BATCH_VIEWS];
};

struct RenderFwdLightArgs {
    int W, H, grid_x, grid_y;
    const uint4* sched;    // [tiles] {tile, list start, list end, -} of workgroup b (ImageView::tile_sched)
    const uint2* ranges;   // [tiles] ... and without a schedule (ImageView::cursor[3] == 0): block -> tile by the static XCD band
    const uint32_t* sched_flag;  // map, list from the range table (render_common.h: blend_slot)
    uint32_t* point_list;  // read only (the light forward keeps its contribution tags in the byte array beside it: render_common.h, half_tags)
    const float4* rec;
    const float* bg;
    const float* gt_depth;
    float* out_color;
    float* out_depth;
    float* out_median;
    float* out_alpha;
    float* out_depth_var;
    uint32_t* n_contrib;
    uint32_t* live_counts;  // [tiles] live entries of each tile (ImageView::tile_count, the binning's dead counters; the entries: render_common.h, live_list)
    float* gau_uncertainty;
    int* gau_related_pixels;
    StatusReport rep;      // armed status slot (dgr_status_arm): workgroup 0 copies the frame's status word to the host
    const int* status;
};

struct RenderBwdLightArgs {
    int W, H, grid_x, grid_y;
    const uint4* sched;    // [tiles] {tile, list start, list end, -} of workgroup b (ImageView::tile_sched)
    const uint2* ranges;   // [tiles] ... and without a schedule (ImageView::cursor[3] == 0): block -> tile by the static XCD band
    const uint32_t* sched_flag;  // map, list from the range table (render_common.h: blend_slot)
    const uint32_t* point_list;
    const float4* rec;
    const float* bg;
    const float* gt_depth;
    const float* alphas;
    const uint32_t* n_contrib;
    const uint32_t* live_counts;  // [tiles] written by the forward blend (render_common.h: live_list)
    const float* dL_dpix;
    const float* dL_dpix_depth;
    const float* dL_dpix_median;
    const float* dL_dpix_var;
    const float* dL_dpix_silhouette;  // [H,W] dL/d(opacity_map) or NULL (render_light.hip: SILHOUETTE)
    const float* means3D;
    const float* view;
    float* acc;  // [P,16]
    int track_off, map_off;
    // deterministic gradients (render_light.hip: DET): the instance-major row buffer [R,16] (NULL: off), the Gaussians' tile
    // rectangles and first-instance offsets
    float* det_rows;
    const ushort4* det_rect;
    const uint32_t* det_goff;
    uint32_t det_R;  // rows of det_rows (>= the frame's instances; a row index beyond it is dropped, not written)
};

struct RenderFwdFullArgs {
    int W, H, grid_x, grid_y;
    const uint4* sched;    // [tiles] {tile, list start, list end, -} of workgroup b (ImageView::tile_sched)
    const uint2* ranges;   // [tiles] ... and without a schedule (ImageView::cursor[3] == 0): block -> tile by the static XCD band
    const uint32_t* sched_flag;  // map, list from the range table (render_common.h: blend_slot)
    uint32_t* point_list;  // read only (the contribution tags go into the byte array beside it: render_common.h, half_tags)
    const float4* rec;
    const float* bg;
    float* out_color;
    float* out_depth;
    float* out_uncertainty;
    uint32_t* n_contrib;
    uint32_t* n_valid;
    uint32_t* first_contrib;
    float* final_T;
    int* status;  // status[3] += sum of n_valid (num_related_primitives)
    StatusReport rep;  // armed status slot (dgr_status_arm): workgroup 0 copies the frame's status word to the host
};

struct RenderBwdFullArgs {
    int W, H, grid_x, grid_y;
    const uint4* sched;    // [tiles] {tile, list start, list end, -} of workgroup b (ImageView::tile_sched)
    const uint2* ranges;   // [tiles] ... and without a schedule (ImageView::cursor[3] == 0): block -> tile by the static XCD band
    const uint32_t* sched_flag;  // map, list from the range table (render_common.h: blend_slot)
    const uint32_t* point_list;
    const float4* rec;
    const float* bg;
    const float* gt_depth;
    const float* final_T;
    const uint32_t* n_contrib;
    const uint32_t* first_contrib;
    const float* dL_dpix;
    const float* dL_depths;
    const float* dL_duncertainties;
    const float* dL_dpix_silhouette;  // [H,W] the exact gradient of the uncertainty output (sum alpha T) or NULL (render_full.hip)
    float* acc;  // [P,16]
    // deterministic gradients (render_light.hip: DET): the finished row of a (tile, Gaussian) pair is stored to det_rows instead
    float* det_rows;
    const ushort4* det_rect;
    const uint32_t* det_goff;
    uint32_t det_R;
};

// ---- launchers (each enqueues on `stream` and returns the hipError_t of the launch) ----
hipError_t launch_preprocess_fwd(const PreprocessFwdArgs& a, hipStream_t stream);
// complete_pose: dgr_set_option("pose_grad", 1) -- the instance with the complete pose gradient (preprocess_bwd.hip: bwd_view_terms)
hipError_t launch_preprocess_bwd(const PreprocessBwdArgs& a, hipStream_t stream, bool complete_pose = false);
hipError_t launch_preprocess_fwd_batch(const PreprocessFwdBatchArgs& b, hipStream_t stream);
hipError_t launch_preprocess_bwd_batch(const PreprocessBwdBatchArgs& b, hipStream_t stream, bool complete_pose = false);
// zero-fill of a 16-byte aligned buffer whose size is a multiple of 16 (a kernel rather than hipMemsetAsync: memset nodes of a
// captured hipGraph were seen to re-execute with corrupted parameters on this ROCm)
hipError_t launch_zero_fill(void* dst, size_t bytes, hipStream_t stream);
// fused sparse Adam (optim.hip): rows with visible[row] <= 0 are skipped entirely; visible == NULL updates every row
// pose.hip: (quaternion, translation) -> viewmatrix, projmatrix, campos, and dL/dviewmatrix -> (dL/dq, dL/dt); one launch each
hipError_t launch_pose_forward(const float* q, const float* t, const float* perspec, float* view, float* proj, float* campos,
                               hipStream_t stream);
hipError_t launch_pose_backward(const float* q, const float* dview, float* dq, float* dt, hipStream_t stream);
// l1_loss.hip: w_c mean|C - C_obs| + w_d mean|D - D_obs| (`partial`: l1_loss_partials() floats) and its two gradient images
int l1_loss_partials();
hipError_t launch_l1_loss_forward(long n_c, const float* c, const float* c_obs, long n_d, const float* d, const float* d_obs,
                                  float w_c, float w_d, float* partial, float* loss, hipStream_t stream);
hipError_t launch_l1_loss_backward(long n_c, const float* c, const float* c_obs, long n_d, const float* d, const float* d_obs,
                                   float w_c, float w_d, const float* upstream, float* dc, float* dd, hipStream_t stream);
// ssim.hip: w_l1 mean|img - ref| + w_ssim (1 - SSIM(img, ref)) + w_depth mean|d - d_obs| over a [V, C, H, W] stack (11 x 11 Gaussian
// window, zero padding); scratch = 4 header floats (mean SSIM, mean|img - ref|, mean|d - d_obs|, maps flag), the partial sums
// (ssim_partial_floats() with the header) and, with want_maps, the three derivative maps the backward correlates
bool ssim_shape_ok(int V, int C, int H, int W);
long ssim_partial_floats(int V, int C, int H, int W);
long ssim_scratch_floats(int V, int C, int H, int W);
hipError_t launch_ssim_loss_forward(int V, int C, int H, int W, const float* img, const float* ref, long n_d, const float* d,
                                    const float* d_obs, float w_l1, float w_ssim, float w_depth, float* scratch, bool want_maps,
                                    float* loss, hipStream_t stream);
hipError_t launch_ssim_loss_backward(int V, int C, int H, int W, const float* img, const float* ref, long n_d, const float* d,
                                     const float* d_obs, float w_l1, float w_ssim, float w_depth, const float* scratch,
                                     const float* upstream, float* dimg, float* ddepth, hipStream_t stream);
// masked_loss.hip: the masked L1 loss with the per-view median outlier test (include/dgr_hip.h: dgr_masked_loss_*).  The scratch,
// in bytes from its start: 16 header floats ([0] w_d / N_d, [1] w_c / N_c for the backward), then median / base / kept per view,
// the views' sums, 3 x V histograms of 2048 bins, the workgroups' slots, the kept mask (a byte per pixel)
struct MaskedLossArgs {
    int V, C, H, W;
    const float *color, *color_obs, *depth, *depth_obs, *opacity;  // opacity: NULL = no silhouette test
    const unsigned char* mask;                                      // NULL = no user mask
    float lo, hi, silhouette, factor, w_color, w_depth;
    bool reject, mask_color, mean;
};
struct MaskedLossLayout {
    long median, base, kept, view_sums, hist, slots, mask, total;  // byte offsets; total = 0 for a refused shape
    long chunk;                                                    // pixels of a view per workgroup
    int blocks;                                                    // workgroups per view
};
bool masked_loss_shape_ok(int V, int H, int W);
MaskedLossLayout masked_loss_layout(int V, int H, int W);
hipError_t launch_masked_loss_forward(const MaskedLossArgs& a, void* scratch, float* loss, hipStream_t stream);
hipError_t launch_masked_loss_backward(const MaskedLossArgs& a, const void* scratch, const float* upstream, float* dcolor,
                                       float* ddepth, hipStream_t stream);
hipError_t launch_densification_stats(int rows, const float* dmeans2D, const int* radii, float* grad_accum, float* denom,
                                      float* max_radii2D, hipStream_t stream);
hipError_t launch_sparse_adam(size_t rows, int k, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                              const int* visible, float lr, float beta1, float beta2, float eps, int step,
                              const int* step_dev, hipStream_t stream);
// fused densify-and-prune (optim.hip): decide + scan into `plan` and counts[8] (device), then one apply launch for n tensors
size_t densify_plan_bytes(size_t rows);
hipError_t launch_densify_plan(size_t rows, const float* grad_accum, const float* denom, const float* max_radii2D,
                               const float* opacity_raw, const float* scaling_raw, float grad_threshold,
                               float opacity_raw_min, float log_scale_split, float log_scale_prune, float max_screen_size,
                               void* plan, int* counts, hipStream_t stream);
hipError_t launch_densify_apply(size_t rows, size_t rows_out, const void* plan, int n, const dgr_densify_tensor* tensors,
                                const float* scaling_raw, const float* rotation_raw, const float* noise,
                                unsigned long long seed, hipStream_t stream);
// fixed-size map upkeep (relocate.hip): relocation's plan (weights, scan, draws, the hit sources' new values) into `scratch`,
// counts[8] and source[P] (device), its in-place apply over n tensors (two launches), and the gated position noise
size_t relocate_scratch_bytes(size_t P);
hipError_t launch_relocate_plan(size_t P, const float* opacity_raw, float opacity_raw_min, const long long* draws,
                                unsigned long long seed, int step, const int* step_dev, void* scratch, int* counts, int* source,
                                hipStream_t stream);
hipError_t launch_relocate_apply(size_t P, const void* scratch, int n, const dgr_relocate_tensor* tensors, double min_opacity,
                                 hipStream_t stream);
hipError_t launch_position_noise(size_t P, float* xyz, const float* scaling_raw, const float* rotation, const float* opacity_raw,
                                 const float* noise, unsigned long long seed, int step, const int* step_dev, float lr,
                                 const float* lr_dev, float scale, float k, float x0, hipStream_t stream);
// map correction (transform.hip): the transforms' fp32 records into `scratch` and counts[4] = {0, 0, invalid, 0} (two launches),
// and the in-place apply over n tensors (the counts' reset and one launch)
size_t transform_scratch_bytes(size_t K);
hipError_t launch_transform_plan(int K, const float* transforms, void* scratch, int* counts, hipStream_t stream);
hipError_t launch_transform_apply(size_t P, int K, const void* scratch, const float* anchor, int n,
                                  const dgr_transform_tensor* tensors, int* counts, hipStream_t stream);
// fused map expansion from an RGB-D keyframe (seed.hip): decide + scan over the candidate pixels into `plan` and counts[8]
// (device), then one apply launch for n tensors (old rows copied, one new row per selected pixel)
size_t seed_candidates(int W, int H, int stride);
size_t seed_plan_bytes(int W, int H, int stride);
hipError_t launch_seed_plan(int W, int H, int stride, const float* depth_obs, const float* opacity_map, const float* depth,
                            float depth_min, float depth_max, float silhouette_threshold, float depth_error_min,
                            const float* depth_error_min_dev, size_t rows, void* plan, int* counts, hipStream_t stream);
hipError_t launch_seed_apply(int W, int H, int stride, size_t rows, size_t rows_out, const void* plan, int n,
                             const dgr_seed_tensor* tensors, const float* color_obs, const float* depth_obs,
                             const float* viewmatrix, float inv_fx, float inv_fy, float cx, float cy, float pix,
                             hipStream_t stream);
// keyframe overlap scores (keyframe_overlap.hip; include/dgr_hip.h: dgr_keyframe_overlap): the candidates are seed.hip's grid (candidate_grid.h).
// One launch, or two with more than one block of candidates per keyframe; `scratch`: keyframe_overlap_scratch_bytes() bytes
struct KeyframeOverlapArgs {
    int W, H, stride, K;
    const float *depth_obs, *viewmatrix, *keyframe_viewmatrices, *keyframe_depths;  // keyframe_depths: NULL = visible is inside
    float fx, fy, inv_fx, inv_fy, cx, cy, depth_min, depth_max, edge, near_z, depth_tolerance;
    int *inside, *visible, *valid;
    float* score;
    unsigned char* flags;  // NULL: not stored
    size_t candidates;     // filled in by the launcher, as wc (candidates per grid row)
    int wc;
};
size_t keyframe_overlap_scratch_bytes(int W, int H, int stride, int K);
hipError_t launch_keyframe_overlap(const KeyframeOverlapArgs& args, void* scratch, hipStream_t stream);
// frame-to-model ICP (icp.hip; include/dgr_hip.h: dgr_depth_normals, dgr_icp_step): the packed vertex-normal map of a depth image
// (one launch) and one Gauss-Newton iteration of projective point-to-plane ICP over the candidate grid (one launch; `scratch`:
// icp_scratch_bytes() bytes whose first word is zero between calls)
struct DepthNormalsArgs {
    int W, H;
    const float *depth, *mask;  // mask: NULL = no mask image
    float mask_threshold, inv_fx, inv_fy, cx, cy, depth_min, depth_max, max_jump;
    float4* vnmap;
};
hipError_t launch_depth_normals(const DepthNormalsArgs& a, hipStream_t stream);
struct IcpStepArgs {
    int W, H, stride;
    const float* depth_obs;
    const float4 *vn_obs, *vn_model;  // vn_obs: NULL = no normal-compatibility test
    const float *model_viewmatrix, *viewmatrix_in;
    float fx, fy, inv_fx, inv_fy, cx, cy, depth_min, depth_max, dist_max, normal_cos_min, huber_delta;
    double damping, rcond;
    int min_points;
    float *viewmatrix_out, *quat_out, *trans_out;  // quat_out, trans_out: NULL = not stored
    double* stats;
    unsigned char* flags;  // NULL: not stored
    size_t candidates;     // filled in by the launcher, as wc (candidates per grid row)
    int wc;
    static constexpr bool rgbd = false;
};
size_t icp_scratch_bytes(int W, int H, int stride);
hipError_t launch_icp_step(const IcpStepArgs& args, void* scratch, hipStream_t stream);
// hybrid RGB-D alignment (icp.hip; include/dgr_hip.h: dgr_intensity_map, dgr_frame_halve, dgr_rgbd_step): the packed
// intensity-gradient map of an image (one launch), one pyramid level of a frame (one launch), and the ICP step with the
// photometric pair beside the geometric one: the same kernel body, instantiated on this argument struct (scratch: icp_scratch_bytes())
struct IntensityMapArgs {
    int W, H, C;                // C: 1 or 3 channel planes of W * H floats
    const float *image, *mask;  // mask: NULL = no mask image
    float mask_threshold;
    float4* imap;      // NULL: not stored
    float* intensity;  // NULL: not stored
};
hipError_t launch_intensity_map(const IntensityMapArgs& a, hipStream_t stream);
struct FrameHalveArgs {
    int W, H, planes;  // the input's size; the output is (W / 2) x (H / 2)
    const float *planes_in, *depth_in;  // planes_in [planes, H, W] or NULL with planes = 0; depth_in: NULL = no depth plane
    float depth_min, depth_max, max_jump;
    float *planes_out, *depth_out;
};
hipError_t launch_frame_halve(const FrameHalveArgs& a, hipStream_t stream);
struct RgbdStepArgs : IcpStepArgs {
    const float* intensity_obs;
    const float4* imap_model;
    float geo_weight, photo_weight, photo_max, photo_huber;
    static constexpr bool rgbd = true;
};
hipError_t launch_rgbd_step(const RgbdStepArgs& args, void* scratch, hipStream_t stream);
// pose-graph optimisation (pgo.hip; include/dgr_hip.h: dgr_pgo_plan, dgr_pgo_solve): the nodes' incidence lists into `scratch`
// (one launch of one workgroup), and the whole Levenberg-Marquardt solve over them (one launch of one workgroup; `scratch`:
// pgo_scratch_bytes() bytes that a plan call for the same K, E and edges filled)
struct PgoArgs {
    int K, E;
    const float* poses_in;      // [K,16], W2C^T
    const int* edges;           // [E,2]
    const float* measurements;  // [E,16], Z^T
    const float* information;   // NULL with kind 0, [E,2] with kind 2, [E,36] with kind 36
    int information_kind;
    const unsigned char* fixed;  // [K] or NULL: only pose 0 is fixed
    int iterations, cg_iterations;
    double cg_tolerance, huber_delta, damping, rcond, step_tolerance, cost_tolerance;
    float* poses_out;  // [K,16]; may be poses_in
    float* chi2;       // [E] or NULL
    double* stats;     // [16]
    int* flags;        // [1]
};
size_t pgo_scratch_bytes(int K, int E);
hipError_t launch_pgo_plan(int K, int E, const int* edges, void* scratch, hipStream_t stream);
hipError_t launch_pgo_solve(const PgoArgs& args, void* scratch, hipStream_t stream);
// per-Gaussian contribution statistics of a rendered view (contrib.hip; include/dgr_hip.h: dgr_contribution_stats): the clear of the
// per-view arrays and counts[4], the replay of the forward's blend over the tiles, and the fold into counts and the running accumulators
struct ContribTilesArgs {
    int W, H, grid_x, grid_y;
    const uint4* sched;    // as the blend kernels' (render_common.h: blend_slot)
    const uint2* ranges;
    const uint32_t* sched_flag;
    const uint32_t* point_list;
    const float4* rec;
    const uint32_t* n_contrib;
    int* n_touched;                  // [P], zero on entry
    uint32_t* max_weight_bits;       // [P] float32 bits, zero on entry
    unsigned long long* sum_weight;  // [P] Q32, zero on entry
};
struct ContribFoldArgs {
    long P;
    const uint32_t* sched_flag;  // the frame's blend flags (NULL: P == 0, no frame)
    const int* n_touched;
    const float* max_weight;
    const long long* sum_weight;
    int min_pixels;
    float weight_min;
    int frame_id;
    long long* touched_total;   // the accumulators, [P] each, any of them NULL
    float* max_weight_total;
    long long* sum_weight_total;
    int* views;
    int* last_seen;
    int* counts;  // [4] or NULL; cleared by launch_contrib_clear
};
hipError_t launch_contrib_clear(long P, int* n_touched, float* max_weight, long long* sum_weight, int* counts, hipStream_t stream);
hipError_t launch_contrib_tiles(const ContribTilesArgs& a, int alpha_mode, hipStream_t stream);
hipError_t launch_contrib_fold(const ContribFoldArgs& a, hipStream_t stream);
// TSDF fusion of rendered views and marching-tetrahedra extraction (tsdf.hip; include/dgr_hip.h: dgr_tsdf_integrate, dgr_mesh_plan,
// dgr_mesh_emit): one integrate launch for any number of views; count, scan and emit of the mesh
struct TsdfIntegrateArgs {
    int nx, ny, nz;
    float ox, oy, oz, voxel;
    float2* volume;  // [nz, ny, nx] (tsdf, weight)
    float4* color;   // [nz, ny, nx] (r, g, b, 0) or NULL
    int V, W, H;
    const float* depth;  // [V, H, W]
    const float* image;  // [V, 3, H, W] or NULL (with color)
    const float* mask;   // [V, H, W] or NULL
    const float* view;   // [V, 16] W2C^T
    float fx, fy, cx, cy, truncation, weight, max_weight, depth_min, depth_max, near_z, mask_threshold;
    unsigned bricks_x, bricks_y;  // filled by the launcher
};
hipError_t launch_tsdf_integrate(const TsdfIntegrateArgs& args, hipStream_t stream);
struct MeshArgs {
    int nx, ny, nz;
    float ox, oy, oz, voxel;
    const float2* volume;
    const float4* color;  // or NULL
    float min_weight;
    size_t cells;  // filled by the launchers
};
size_t mesh_scratch_bytes(int nx, int ny, int nz);
hipError_t launch_mesh_plan(const MeshArgs& args, int max_triangles, void* scratch, int* count, int* flags, hipStream_t stream);
hipError_t launch_mesh_emit(const MeshArgs& args, int max_triangles, const void* scratch, float* vertices, float* colors,
                            hipStream_t stream);
// ray-casting the TSDF volume (raycast.hip; include/dgr_hip.h: dgr_tsdf_bricks, dgr_tsdf_raycast): the map of live bricks in one
// launch, the march of V views in one launch
struct BricksArgs {
    int nx, ny, nz;
    const float2* volume;
    float min_weight;
    unsigned char* bricks;  // [ceil((nz-1)/8), ceil((ny-1)/8), ceil((nx-1)/8)]
    unsigned bnx, bny;      // filled by the launcher
};
size_t tsdf_brick_count(int nx, int ny, int nz);
hipError_t launch_tsdf_bricks(const BricksArgs& args, hipStream_t stream);
struct RaycastArgs {
    int nx, ny, nz;
    float ox, oy, oz, voxel;
    const float2* volume;
    const float4* color;           // or NULL
    const unsigned char* bricks;   // or NULL
    int V, W, H;
    const float* view;             // [V, 16] W2C^T
    float fx, fy, cx, cy, depth_min, depth_max, step, min_weight;
    float* depth;                  // [V, H, W] or NULL
    float4* vnmap;                 // [V, H, W] (n_c, z) or NULL
    float* color_out;              // [V, 3, H, W] or NULL
    unsigned char* flags;          // [V, H, W] or NULL
};
hipError_t launch_tsdf_raycast(const RaycastArgs& args, hipStream_t stream);
// exact k-nearest-neighbour search (knn.hip): the index (sorted records and 256-record leaves) and the pruned scan over it
size_t knn_index_bytes(int n_points);                  // 0: refused (n_points outside 1 .. 2^24)
size_t knn_scratch_bytes(int n_points, int n_queries);  // 0: refused
hipError_t launch_knn_build(int n_points, const float* points, void* index, void* scratch, hipStream_t stream);
struct KnnSearchCall {
    const void* index;
    int n_points, n_queries;
    const float* queries;  // [Q, 3] or NULL: the indexed points, query i is point i
    int k, exclude_self;
    float max_dist2;
    void* scratch;
    float* dist2;       // [Q, k] or NULL
    int* idx;           // [Q, k] or NULL
    int* count;         // [Q] or NULL
    float* mean_dist2;  // [Q] or NULL
};
hipError_t launch_knn_search(const KnnSearchCall& call, hipStream_t stream);
// generalized ICP over the kNN index (gicp.hip; include/dgr_hip.h: dgr_point_covariances, dgr_gicp_step): the neighbourhood
// covariances of a cloud (one launch), and one Gauss-Newton iteration: the source moved by the estimate, the cross-mode search with
// k = 1, the fused step (`scratch`: gicp_scratch_bytes() bytes whose first word is zero between calls)
struct PointCovArgs {
    int P, k;
    const float* points;  // [P,3]
    const int* idx;       // [P,k]
    int mode, min_neighbours, has_viewpoint;
    float epsilon, scale_floor, viewpoint[3];
    float4* cov;  // [P,2] or NULL, as every output
    float *normals, *log_scales, *quats;
    unsigned char* flags;
};
hipError_t launch_point_covariances(const PointCovArgs& a, hipStream_t stream);
struct GicpStepArgs {
    int N, S;
    const float *target, *source;           // [N,3], [S,3]
    const float4 *target_cov, *source_cov;  // [N,2], [S,2] or NULL
    const float* transform_in;
    float huber_delta;
    double damping, rcond;
    int min_points;
    float *transform_out, *quat_out, *trans_out;  // quat_out, trans_out: NULL = not stored
    double* stats;
    unsigned char* flags;  // NULL: not stored
    const float* q;        // filled in by the launcher: the moved source and its association, in the scratch
    const int* idx;
};
size_t gicp_scratch_bytes(int n_target, int n_source);  // 0: refused (a size outside 1 .. 2^24)
hipError_t launch_gicp_step(const GicpStepArgs& args, const void* index, float dist_max, int* idx_out, void* scratch,
                            hipStream_t stream);
// view-independent covariance of a batch of views (preprocess_fwd.hip, preprocess_bwd.hip)
hipError_t launch_cov3d_forward(int P, const float* scales, const float* rotations, float mod, float* cov3D, hipStream_t stream);
hipError_t launch_cov3d_backward(int P, const float* scales, const float* rotations, float mod, const float* dL_dcov3D,
                                 float* dL_dscale, float* dL_drot, hipStream_t stream);
hipError_t launch_mark_visible(int P, const float* means, const float* view, uint8_t* present, hipStream_t stream);

// binning: tile_count -> ranges (+ total in status[0], overflow in status[1]); emit keys; sort tiles
// Which binning runs behind preprocess and from which entry point: the one description api.hip decides (bin_path) and the
// launchers below read.
//   segments: the two-level segment binning (segment_binning.hip; frames whose segment tables fit LDS); otherwise the global
//             tile counters (binning.hip).
//   callback: the binning buffer is sized after a host read of num_rendered: scan_blocks has run, so geom.block_tiles is already
//             the exclusive prefix of the block totals and the status word is initialised.  Otherwise (presized) preprocess_fwd
//             left raw block totals (segments) or counted itself (counters), and the kernel that completes the status word --
//             bin_tiles, scan_tiles -- also fills status[2..3].
struct BinPath {
    bool segments, callback;
};
hipError_t launch_scan_tiles(ImageView img, int tiles, int grid_x, int capacity, BinPath path, int blend_flags, StatusReport rep,
                             hipStream_t stream);
hipError_t launch_count_rank(int P, GeometryView geom, ImageView img, BinningView bin, int grid_x, int capacity,
                             hipStream_t stream);
hipError_t launch_scan_blocks(int P, GeometryView geom, ImageView img, hipStream_t stream);
hipError_t launch_emit_instances(int P, GeometryView geom, ImageView img, BinningView bin, int grid_x, hipStream_t stream);
// two-level binning (segment_binning.hip): presized and callback paths, frames whose segment tables fit LDS.
bool segment_binning_fits(int W, int H);
int segment_binning_workgroups(int P);
int segment_shift(int W, int H, int capacity, int longest_list = -1);  // log2 of the tiles per segment (4, 3 or 2) for this frame, capacity and (if known) longest list
hipError_t launch_bin_segments(int P, GeometryView geom, BinningView bin, SegmentTables tb, int grid_x, int grid_y, int seg_shift,
                               int capacity, BinPath path, hipStream_t stream);
extern unsigned long long* g_bin_tiles_trace;  // debug: phase time stamps per bin_tiles workgroup (segment_binning.hip)
hipError_t launch_bin_tiles(int P, GeometryView geom, ImageView img, BinningView bin, SegmentTables tb, int grid_x, int grid_y,
                            int seg_shift, int capacity, BinPath path, int blend_flags, StatusReport rep, hipStream_t stream);
hipError_t launch_sort_tiles(ImageView img, BinningView bin, int tiles, hipStream_t stream);
// ranges -> the blend kernels' schedule (img.tile_sched): tiles by descending list length, so that the longest lists
// start first and every XCD gets its share of a cluster (tile_schedule.hip)
hipError_t launch_tile_schedule(ImageView img, int tiles, hipStream_t stream);

// alpha_mode: render_common.h (0 = ALPHA_REF, the restatement's bits; 1 = ALPHA_FAST; 2 = ALPHA_GLIBC)
hipError_t launch_render_fwd_light(const RenderFwdLightArgs& a, int alpha_mode, hipStream_t stream);
hipError_t launch_render_bwd_light(const RenderBwdLightArgs& a, int alpha_mode, hipStream_t stream);
hipError_t launch_render_fwd_full(const RenderFwdFullArgs& a, int alpha_mode, hipStream_t stream);
hipError_t launch_render_bwd_full(const RenderBwdFullArgs& a, int alpha_mode, hipStream_t stream, bool deterministic = false);
// absgrad (AbsGS): opt-in instances of the two MAPPING blend backwards that also sum the absolute value of each pixel's dL/dmean2D
// per Gaussian (render_light.hip: ABS) and add the totals, x and y, into dL_dmean2D_abs [P,3] -- which the caller zero-fills first
// (launch_zero_floats).  alpha_mode 0 and 1, not deterministic, not with map_off (api.hip checks).
hipError_t launch_render_bwd_light_abs(const RenderBwdLightArgs& a, float* dL_dmean2D_abs, int alpha_mode, hipStream_t stream);
hipError_t launch_render_bwd_full_abs(const RenderBwdFullArgs& a, float* dL_dmean2D_abs, int alpha_mode, hipStream_t stream);
// zero-fill of n floats at any 4-byte aligned address
hipError_t launch_zero_floats(float* dst, size_t n, hipStream_t stream);
hipError_t launch_det_offsets(int P, const ushort4* rect, uint32_t* blk, uint32_t* goff, hipStream_t stream);
hipError_t launch_det_gather(int P, const ushort4* rect, const uint32_t* goff, const float* rows, uint32_t R, float* acc, hipStream_t stream);
hipError_t launch_half_reduce16_test(const float* in, float* r0, float* r1, int* slot0, int* slot1, hipStream_t stream);
hipError_t launch_half_reduce_test(const float* in, float* r0, float* r1, float* h3, int* slot0, int* slot1, int* comp3, hipStream_t stream);
hipError_t launch_lane_lists_test(const unsigned char* codes, uint32_t* paired, uint32_t* halves, hipStream_t stream);
hipError_t launch_wave_reduce_test(const float* in, float* out16, float* out12, float* out4, int* comp16, int* comp12, int* comp4,
                                   hipStream_t stream);
hipError_t launch_exact_math_test(int n, const float* x, const float* a, const float* b, float* out_exp, float* out_div, int alpha_mode,
                                  hipStream_t stream);
// offsets: n_lists + 1 DEVICE ints (api.hip copies the caller's host array)
hipError_t launch_tile_sort_test(int mode, int n_lists, const uint64_t* keys, const int* offsets, uint32_t* out_ids, uint64_t* out_keys,
                                 hipStream_t stream);

}  // namespace dgr
