// options.h -- the library options (include/dgr_hip.h: dgr_set_option and friends): the table, and the readers of the call path.
#pragma once
#include <atomic>
#include <climits>

#include "../../include/dgr_hip.h"

namespace dgr {

// ---- THE TABLE.  One row per option: id, name, environment variable (read once, when the library is loaded; nullptr = none),
// default, accepted range lo .. hi, what a value outside the range becomes (Outside, below), the option's field in the
// per-thread options word (DGR_OPT_SHIFT_*; -1 = process-wide only) and, for OUT_REFUSE, the text of the refusal.
// Adding an option is: one row here, one line in the comment above dgr_set_option in include/dgr_hip.h, and the code that reads
// it (dgr::option(OPT_x), or dgr::thread_option(OPT_x) for a row with a field).  Everything else -- the setters and getters, the
// per-thread overrides, the options word, the environment -- is a loop over this table (options.hip).
//
// "alpha_mode": how the blend kernels evaluate alpha and T / (1 - alpha) (csrc/render_common.h).
//   0 (default) = the reference's expression with the CPU restatement's bits (exp_p32 / div_ref, csrc/exact_math.h): alpha
//       image, n_contrib and median depth bit-identical to the restatement, gradients within 1e-5 of it;
//   1 (= "fast_alpha", 1) = log2(e)-scaled conic, one v_exp_f32, v_rcp_f32: every operation good to an ulp, but the light
//       backward's T_final = 1 - alpha and its divisions by (1 - alpha) amplify the last-bit differences to 6e-5 abs at config 3;
//   2 = as 0 with glibc's expf algorithm in the double pipe (exp_glibc; rounds 5-7's default, the oracle's exp mode 1), for A/B.
//   Set it before the forward whose backward should use it (forward and backward of a view must use the same mode).
// "tight_cull": 1 = alpha-aware tile rectangles (preprocess_fwd.hip); default off.
// "deterministic_grads": 1 = the light backward (one-view entry point, alpha_mode 0) forms its gradients without
//   order-dependent float atomics (csrc/render_light.hip: DET): bit-identical run after run, at the price of an instance-major row
//   buffer (64 bytes per tile instance: zero-filled, written and read once) and a smaller batch in the blend backward.  The backward
//   then needs dgr_light_backward_scratch_bytes_r(P, W, H, R) bytes of scratch, R = the value passed as `R` (>= num_rendered).
// "pose_grad": 0 (default) = the reference's pose-gradient terms; 1 = the complete pose gradient, the view-matrix counterpart of
//   dL_dmeans3D (csrc/preprocess_bwd.hip: bwd_view_terms<true>; include/dgr_hip.h).  A light map_off backward then runs the mapping
//   blend backward (its per-Gaussian outputs are dropped).
// "silhouette_grad": 0 (default) / 1.  No entry point reads it: it is the bindings' switch (include/dgr_hip.h), kept here so
//   that both bindings and every thread share one value and a backward runs under its forward's snapshot.  1: the bindings pass
//   the opacity_map (light) / uncertainty (full) gradient as the dL_dpix_silhouette image of the _silhouette entry points.
// "tile_schedule": 1 = every forward runs tile_schedule_kernel (the blend kernels take their tiles classes of long lists
//   first), 0 = never (static XCD band map), 2 (default) = by the frame (status.hip: want_schedule).
// "lane_lists": the lists the LIGHT blend kernels walk (csrc/render_light.hip).
//   1 = one list per half of a quadrant wave in the forward and the tracking backward, paired lists in the mapping backward (round 8);
//   0 = one list per quadrant wave everywhere (rounds 1-7);
//   2 (default) = decided per FRAME on the device by the binning kernel, from the frame's own run statistics (segment_binning.hip:
//       bin_tiles_kernel; big splats -> 0) and recorded in the frame's state, where forward and backward read it.
//   Its variable is DGR_FWD_HALVES (the switch's name when it was per process; A/B runs).
// "lds_count": how the forward bins tile instances.
//   1 (default) = the two-level segment binning (csrc/segment_binning.hip) whenever the frame's segment tables fit LDS;
//   0 = returning global atomics on per-tile counters (csrc/binning.hip; inside preprocess_fwd when presized), which also
//       serves frames too large for the segment tables.  (2 is accepted as a synonym of 1.)
//   Measured, round 5 (profiles/r5/): the segment binning is faster one view at a time at every size (config 3: 0.51 against
//   0.59 ms per view, config 4: 1.71 / 1.85, config 5: 4.54 / 4.86) and equal or faster with three views in flight (0.455 /
//   0.466, 1.57 / 1.57, 4.27 / 4.53), so nothing switches by job size or by the number of views in flight any more.
// "blend_wgs_per_cu": cap on the blend kernels' workgroups per CU (kernels.h: launch_blend); 0 = none, 3 .. 7.
// "profile_every": n = the stage profiler brackets every n-th launch only (profile.hip).
// "batch_streams", "batch_order": how the per-view stages of a batch are spread over streams (api.hip: the batch stream pool).
enum Outside {
    OUT_CLAMP,   // below lo -> lo, above hi -> hi
    OUT_TRUTH,   // any non-zero value -> 1
    OUT_OFF,     // outside lo .. hi -> 0 (a window above "off")
    OUT_REFUSE,  // DGR_ERR_BAD_ARGUMENT, the option keeps its value
};
constexpr int DGR_BATCH_MAX_STREAMS = 8;
// clang-format off
#define DGR_OPTIONS(X)                                                                                                              \
    X(ALPHA_MODE,       "alpha_mode",          "DGR_ALPHA_MODE",          0, 0, 2, OUT_REFUSE, DGR_OPT_SHIFT_ALPHA_MODE,            \
      "0 (restatement's bits, fp32 expf), 1 (fast), 2 (glibc's expf form)")                                                        \
    X(TIGHT_CULL,       "tight_cull",          nullptr,                   0, 0, 1, OUT_TRUTH,  DGR_OPT_SHIFT_TIGHT_CULL, "")        \
    X(DET_GRADS,        "deterministic_grads", "DGR_DETERMINISTIC_GRADS", 0, 0, 1, OUT_TRUTH,  DGR_OPT_SHIFT_DETERMINISTIC_GRADS, "") \
    X(POSE_GRAD,        "pose_grad",           "DGR_POSE_GRAD",           0, 0, 1, OUT_REFUSE, DGR_OPT_SHIFT_POSE_GRAD,             \
      "0 (the reference's pose terms) or 1 (complete)")                                                                            \
    X(SILHOUETTE_GRAD,  "silhouette_grad",     "DGR_SILHOUETTE_GRAD",     0, 0, 1, OUT_REFUSE, DGR_OPT_SHIFT_SILHOUETTE_GRAD,       \
      "0 (the reference's gradients) or 1 (exact silhouette gradient)")                                                            \
    X(TILE_SCHEDULE,    "tile_schedule",       "DGR_TILE_SCHEDULE",       2, 0, 2, OUT_CLAMP,  -1, "")                              \
    X(LANE_LISTS,       "lane_lists",          "DGR_FWD_HALVES",          2, 0, 2, OUT_CLAMP,  -1, "")                              \
    X(LDS_COUNT,        "lds_count",           "DGR_LDS_COUNT",           1, 0, 2, OUT_CLAMP,  -1, "")                              \
    X(BLEND_WGS_PER_CU, "blend_wgs_per_cu",    "DGR_BLEND_WGS_PER_CU",    0, 3, 7, OUT_OFF,    -1, "")                              \
    X(PROFILE_EVERY,    "profile_every",       nullptr,                   1, 1, INT_MAX, OUT_CLAMP, -1, "")                         \
    X(BATCH_STREAMS,    "batch_streams",       nullptr,                   2, 1, DGR_BATCH_MAX_STREAMS, OUT_CLAMP, -1, "")           \
    X(BATCH_ORDER,      "batch_order",         nullptr,                   0, 0, 1, OUT_TRUTH,  -1, "")
// clang-format on

#define DGR_OPTION_ID(id, name, env, def, lo, hi, outside, shift, accepted) OPT_##id,
enum Option { DGR_OPTIONS(DGR_OPTION_ID) OPT_COUNT };
#undef DGR_OPTION_ID
#define DGR_OPTION_SHIFT(id, name, env, def, lo, hi, outside, shift, accepted) shift,
constexpr int k_option_shift[OPT_COUNT] = {DGR_OPTIONS(DGR_OPTION_SHIFT)};
#undef DGR_OPTION_SHIFT

// ---- the values.  Process-wide: one atomic per row.  Per THREAD: the options that change what a call computes have a field in
// the options word, and a thread holds its overrides as that word's fields (value + 1; 0 = inherit): a tracker thread and a
// mapper thread of one process -- or a test beside a training loop -- hold their own values.  Every entry point reads its options
// ONCE, when it is called, and hands them to its launches as template choices / kernel arguments: launches already queued (on
// any stream) are not affected by a later change.  A backward must run with its forward's alpha mode: the autograd bindings
// snapshot dgr_thread_options_effective() in the forward and swap it in around the backward (which the autograd engine may run
// on another thread).
constexpr int DGR_OPT_FIELDS = 5;  // fields of the options word, 4 bits each
extern std::atomic<int> g_option_value[OPT_COUNT];
extern __thread int t_option_field[DGR_OPT_FIELDS];  // (__thread: zero-initialised, read without an initialisation wrapper)

inline int option(Option o) { return g_option_value[o].load(std::memory_order_relaxed); }
// (only for rows with a field)
inline int thread_option(Option o) {
    const int f = t_option_field[k_option_shift[o] / 4];
    return f ? f - 1 : option(o);
}
inline int opt_alpha_mode() { return thread_option(OPT_ALPHA_MODE); }
inline int opt_tight_cull() { return thread_option(OPT_TIGHT_CULL); }
inline int opt_det_grads() { return thread_option(OPT_DET_GRADS); }
inline int opt_pose_grad() { return thread_option(OPT_POSE_GRAD); }

}  // namespace dgr
