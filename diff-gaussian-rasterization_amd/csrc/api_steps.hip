// api_steps.hip -- C-ABI entry points (include/dgr_hip.h) of the steps around the rasteriser (optimiser, map resize, pose, losses,
// keyframe overlap, ICP).  Host code: each checks its arguments, leaves a refusal's text for dgr_last_error() and calls its launcher.
#include <cmath>
#include <string>

#include "host_util.h"
#include "kernels.h"
#include "options.h"

using namespace dgr;

namespace {

int refuse(const char* who, const char* bad) {  // a refusal: "<entry point>: <what is wrong>" for dgr_last_error()
    set_last_error(std::string(who) + ": " + bad);
    return DGR_ERR_BAD_ARGUMENT;
}

// What the plan and apply entry points of the map steps (densify-and-prune, map expansion, relocation, position noise, map
// correction) check alike:
const long PLAN_MAX_ROWS = 0x3fffffffL;  // densify's P' <= 2 rows and seed's rows + candidates must fit the int counts

thread_local std::string named_error;  // a message that names the caller's argument, kept until the thread's next one
// the row range, under the name the entry point gives its row count: the message, or NULL
const char* rows_error(long rows, const char* name) {
    return rows >= 0 && rows <= PLAN_MAX_ROWS ? nullptr : (named_error = std::string(name) + " must be 0 .. 2^30 - 1").c_str();
}
// the row range, then `between` (the caller's own refusal reported at this place, or NULL), the plan (or scratch) pointer and, for
// a plan call, counts8_device: the message, or NULL
const char* plan_args_error(long rows, const char* between, const void* plan, bool plans, const int* counts8_device,
                            const char* rows_name = "rows", const char* plan_name = "plan") {
    if (const char* bad = rows_error(rows, rows_name)) return bad;
    if (between) return between;
    if (!plan || !dgr::aligned16(plan)) return (named_error = std::string(plan_name) + " is NULL or not 16-byte aligned").c_str();
    if (plans && !counts8_device) return "counts8_device is NULL";
    return nullptr;
}

// the descriptor table of an apply call: the message, or NULL.  Modes mode_first .. mode_last, mode_xyz the one XYZ tensor's
// (n_xyz: how many were seen); extra(t): the step's own rules for a descriptor, checked after these
template <typename Desc, typename Extra>
const char* tensor_table_error(int n, const Desc* tensors, int max_n, const char* n_error, int mode_first, int mode_last,
                               int mode_xyz, int& n_xyz, Extra extra) {
    if (n < 1 || n > max_n) return n_error;
    if (!tensors) return "tensors is NULL";
    for (int i = 0; i < n; ++i) {
        const Desc& t = tensors[i];
        if (t.k < 1 || t.k > (1 << 22)) return "a tensor with k < 1 or k > 2^22";
        if (t.mode < mode_first || t.mode > mode_last) return "unknown mode";
        if (t.mode == mode_xyz && t.k != 3) return "the XYZ tensor must have k = 3";
        if (t.mode == mode_xyz && ++n_xyz > 1) return "more than one XYZ tensor";
        if (const char* bad = extra(t)) return bad;
    }
    return nullptr;
}

}  // namespace

extern "C" {

int dgr_cov3d_forward(void* stream, int P, const float* scales, const float* rotations, float scale_modifier, float* cov3D) {
    if (P < 0 || (P > 0 && (!scales || !rotations || !cov3D))) return refuse("dgr_cov3d_forward", "bad argument");
    HIP_TRY(dgr::launch_cov3d_forward(P, scales, rotations, scale_modifier, cov3D, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_cov3d_backward(void* stream, int P, const float* scales, const float* rotations, float scale_modifier,
                       const float* dL_dcov3D, float* dL_dscales, float* dL_drotations) {
    if (P < 0 || (P > 0 && (!scales || !rotations || !dL_dcov3D || !dL_dscales || !dL_drotations)))
        return refuse("dgr_cov3d_backward", "bad argument");
    HIP_TRY(dgr::launch_cov3d_backward(P, scales, rotations, scale_modifier, dL_dcov3D, dL_dscales, dL_drotations, (hipStream_t)stream));
    return DGR_OK;
}

int dgr_sparse_adam(void* stream, long rows, int k, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                    const int* visible, float lr, float beta1, float beta2, float eps, int step) {
    if (rows < 0 || k <= 0 || step < 1 || (rows > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)))
        return refuse("dgr_sparse_adam", "bad argument");
    HIP_TRY(dgr::launch_sparse_adam((size_t)rows, k, param, grad, exp_avg, exp_avg_sq, visible, lr, beta1, beta2, eps, step,
                                    nullptr, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_sparse_adam_capturable(void* stream, long rows, int k, float* param, const float* grad, float* exp_avg,
                               float* exp_avg_sq, const int* visible, float lr, float beta1, float beta2, float eps,
                               const int* step_device) {
    if (rows < 0 || k <= 0 || !step_device || (rows > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)))
        return refuse("dgr_sparse_adam_capturable", "bad argument");
    HIP_TRY(dgr::launch_sparse_adam((size_t)rows, k, param, grad, exp_avg, exp_avg_sq, visible, lr, beta1, beta2, eps, 1,
                                    step_device, (hipStream_t)stream));
    return DGR_OK;
}

int dgr_densification_stats(void* stream, long rows, const float* dmeans2D, const int* radii, float* grad_accum, float* denom,
                            float* max_radii2D) {
    if (rows < 0 || rows > 0x7fffffffL || (rows > 0 && (!radii || (grad_accum && !dmeans2D))))
        return refuse("dgr_densification_stats", "bad argument");
    HIP_TRY(dgr::launch_densification_stats((int)rows, dmeans2D, radii, grad_accum, denom, max_radii2D, (hipStream_t)stream));
    return DGR_OK;
}

size_t dgr_densify_plan_bytes(long rows) { return rows < 0 ? 0 : dgr::densify_plan_bytes((size_t)rows); }

int dgr_densify_plan(void* stream, long rows, const float* grad_accum, const float* denom, const float* max_radii2D,
                     const float* opacity_raw, const float* scaling_raw, float grad_threshold, float opacity_raw_min,
                     float log_scale_split, float log_scale_prune, float max_screen_size, void* plan, int* counts8_device) {
    const char* bad = plan_args_error(rows, nullptr, plan, true, counts8_device);
    if (!bad && rows > 0 && (!grad_accum || !denom || !opacity_raw || !scaling_raw)) bad = "a NULL input";
    if (bad) return refuse("dgr_densify_plan", bad);
    HIP_TRY(dgr::launch_densify_plan((size_t)rows, grad_accum, denom, max_radii2D, opacity_raw, scaling_raw, grad_threshold,
                                     opacity_raw_min, log_scale_split, log_scale_prune, max_screen_size, plan, counts8_device,
                                     (hipStream_t)stream));
    return DGR_OK;
}

int dgr_densify_apply(void* stream, long rows, long rows_out, const void* plan, int n, const dgr_densify_tensor* tensors,
                      const float* scaling_raw, const float* rotation_raw, const float* noise, unsigned long long seed) {
    int n_xyz = 0;
    const char* bad = plan_args_error(rows, rows_out < 0 || rows_out > 2 * rows ? "rows_out must be 0 .. 2 rows" : nullptr, plan,
                                      false, nullptr);
    if (!bad)
        bad = tensor_table_error(n, tensors, DGR_DENSIFY_MAX_TENSORS, "n must be 1 .. DGR_DENSIFY_MAX_TENSORS (24) tensors",
                                 DGR_DENSIFY_COPY, DGR_DENSIFY_LOG_SCALE, DGR_DENSIFY_XYZ, n_xyz,
                                 [&](const dgr_densify_tensor& t) -> const char* {
                                     const bool null = rows_out > 0 && (!t.dst || (t.mode != DGR_DENSIFY_ZERO && !t.src));
                                     return null ? "a tensor with a NULL src or dst" : nullptr;
                                 });
    if (!bad && n_xyz && rows_out > 0 && (!scaling_raw || !rotation_raw)) bad = "XYZ needs scaling_raw and rotation_raw";
    if (bad) return refuse("dgr_densify_apply", bad);
    HIP_TRY(dgr::launch_densify_apply((size_t)rows, (size_t)rows_out, plan, n, tensors, scaling_raw, rotation_raw, noise, seed,
                                      (hipStream_t)stream));
    return DGR_OK;
}

size_t dgr_relocate_scratch_bytes(long P) { return P < 0 || P > PLAN_MAX_ROWS ? 0 : dgr::relocate_scratch_bytes((size_t)P); }

int dgr_relocate_plan(void* stream, long P, const float* opacity_raw, float opacity_raw_min, const long long* draws,
                      unsigned long long seed, int step, const int* step_device, void* scratch, int* counts8_device, int* source) {
    const char* bad = plan_args_error(P, nullptr, scratch, true, counts8_device, "P", "scratch");
    if (!bad && P > 0 && !opacity_raw) bad = "opacity_raw is NULL";
    if (!bad && P > 0 && !source) bad = "source is NULL";
    if (!bad && std::isnan(opacity_raw_min)) bad = "opacity_raw_min is NaN";
    if (!bad && !step_device && step < 0) bad = "step is negative";
    if (bad) return refuse("dgr_relocate_plan", bad);
    HIP_TRY(dgr::launch_relocate_plan((size_t)P, opacity_raw, opacity_raw_min, draws, seed, step, step_device, scratch,
                                      counts8_device, source, (hipStream_t)stream));
    return DGR_OK;
}

int dgr_relocate_apply(void* stream, long P, const void* scratch, int n, const dgr_relocate_tensor* tensors, float* scaling_raw,
                       float* opacity_raw, double min_opacity) {
    const char* bad = plan_args_error(P, nullptr, scratch, false, nullptr, "P", "scratch");
    if (!bad && !(min_opacity >= 0.0 && min_opacity < 1.0)) bad = "min_opacity must lie in [0, 1)";
    int n_opacity = 0, n_scale = 0, unused = 0;
    if (!bad)
        bad = tensor_table_error(n, tensors, DGR_RELOCATE_MAX_TENSORS, "n must be 1 .. DGR_RELOCATE_MAX_TENSORS (24) tensors",
                                 DGR_RELOCATE_COPY, DGR_RELOCATE_ZERO_RELOCATED, -1, unused,
                                 [&](const dgr_relocate_tensor& t) -> const char* {
                                     if (P > 0 && !t.data) return "a tensor with NULL data";
                                     if (t.mode == DGR_RELOCATE_OPACITY) {
                                         if (t.k != 1) return "the OPACITY tensor must have k = 1";
                                         if (++n_opacity > 1) return "more than one OPACITY tensor";
                                         if (t.data != opacity_raw) return "the OPACITY tensor must be opacity_raw, which the plan was made from";
                                     }
                                     if (t.mode == DGR_RELOCATE_LOG_SCALE) {
                                         if (++n_scale > 1) return "more than one LOG_SCALE tensor";
                                         if (t.data != scaling_raw) return "the LOG_SCALE tensor must be scaling_raw";
                                     }
                                     return nullptr;
                                 });
    if (bad) return refuse("dgr_relocate_apply", bad);
    HIP_TRY(dgr::launch_relocate_apply((size_t)P, scratch, n, tensors, min_opacity, (hipStream_t)stream));
    return DGR_OK;
}

int dgr_position_noise(void* stream, long P, float* xyz, const float* scaling_raw, const float* rotation, const float* opacity_raw,
                       const float* noise, unsigned long long seed, int step, const int* step_device, float lr,
                       const float* lr_device, float scale, float k, float x0) {
    const char* bad = rows_error(P, "P");
    if (!bad && P > 0 && (!xyz || !scaling_raw || !rotation || !opacity_raw)) bad = "xyz, scaling_raw, rotation or opacity_raw is NULL";
    if (!bad && !step_device && step < 0) bad = "step is negative";
    if (!bad && !lr_device && !std::isfinite(lr)) bad = "lr is not finite";
    if (!bad && !(std::isfinite(scale) && std::isfinite(k) && std::isfinite(x0))) bad = "scale, k or x0 is not finite";
    if (bad) return refuse("dgr_position_noise", bad);
    HIP_TRY(dgr::launch_position_noise((size_t)P, xyz, scaling_raw, rotation, opacity_raw, noise, seed, step, step_device, lr,
                                       lr_device, scale, k, x0, (hipStream_t)stream));
    return DGR_OK;
}

static const long TRANSFORM_MAX_K = 1L << 20;
size_t dgr_transform_scratch_bytes(long K) { return K < 1 || K > TRANSFORM_MAX_K ? 0 : dgr::transform_scratch_bytes((size_t)K); }

int dgr_transform_plan(void* stream, long K, const float* transforms, void* scratch, int* counts4_device) {
    const char* bad = K < 1 || K > TRANSFORM_MAX_K ? "K must be 1 .. 2^20" : nullptr;
    if (!bad && !transforms) bad = "transforms is NULL";
    if (!bad && (!scratch || !dgr::aligned16(scratch))) bad = "scratch is NULL or not 16-byte aligned";
    if (!bad && !counts4_device) bad = "counts4_device is NULL";
    if (bad) return refuse("dgr_transform_plan", bad);
    HIP_TRY(dgr::launch_transform_plan((int)K, transforms, scratch, counts4_device, (hipStream_t)stream));
    return DGR_OK;
}

int dgr_transform_apply(void* stream, long P, long K, const void* scratch, const float* anchor, int n,
                        const dgr_transform_tensor* tensors, int* counts4_device) {
    const char* bad = plan_args_error(P, K < 1 || K > TRANSFORM_MAX_K ? "K must be 1 .. 2^20" : nullptr, scratch, false, nullptr, "P",
                                      "scratch");
    if (!bad && !counts4_device) bad = "counts4_device is NULL";
    int n_xyz = 0, n_quat = 0, n_scale = 0;
    if (!bad)
        bad = tensor_table_error(
            n, tensors, DGR_TRANSFORM_MAX_TENSORS, "n must be 1 .. DGR_TRANSFORM_MAX_TENSORS (24) tensors", DGR_TRANSFORM_XYZ,
            DGR_TRANSFORM_SH + DGR_TRANSFORM_MOMENT2, DGR_TRANSFORM_XYZ, n_xyz, [&](const dgr_transform_tensor& t) -> const char* {
                const int kind = t.mode & ~3, order = t.mode & 3;
                if (order > DGR_TRANSFORM_MOMENT2 || (kind == DGR_TRANSFORM_LOG_SCALE && order != DGR_TRANSFORM_VALUE)) return "unknown mode";
                if (P > 0 && !t.data) return "a tensor with NULL data";
                if (kind == DGR_TRANSFORM_XYZ && t.k != 3) return "an XYZ tensor must have k = 3";
                if (kind == DGR_TRANSFORM_QUAT && t.k != 4) return "a QUAT tensor must have k = 4";
                if (kind == DGR_TRANSFORM_LOG_SCALE && t.k != 3) return "a LOG_SCALE tensor must have k = 3";
                if (kind != DGR_TRANSFORM_SH && t.skip != 0) return "skip must be 0 for a tensor that is not SH";
                if (kind == DGR_TRANSFORM_SH) {
                    if (t.skip != 0 && t.skip != 3) return "an SH tensor's skip must be 0 or 3";
                    const int width = t.k - t.skip;
                    if (width != 9 && width != 24 && width != 45) return "an SH tensor must hold the complete bands of degree 1, 2 or 3 (k - skip = 9, 24 or 45)";
                }
                if (t.mode == DGR_TRANSFORM_QUAT && ++n_quat > 1) return "more than one QUAT tensor";
                if (t.mode == DGR_TRANSFORM_LOG_SCALE && ++n_scale > 1) return "more than one LOG_SCALE tensor";
                return nullptr;
            });
    if (bad) return refuse("dgr_transform_apply", bad);
    HIP_TRY(dgr::launch_transform_apply((size_t)P, (int)K, scratch, anchor, n, tensors, counts4_device, (hipStream_t)stream));
    return DGR_OK;
}

static const char* seed_shape_error(int width, int height, int stride) {
    if (width < 1 || height < 1) return "width and height must be positive";
    if (stride < 1) return "stride must be positive";
    if (dgr::seed_candidates(width, height, stride) > (size_t)PLAN_MAX_ROWS) return "2^30 candidates or more";
    return nullptr;
}
size_t dgr_seed_plan_bytes(int width, int height, int stride) {
    return seed_shape_error(width, height, stride) ? 0 : dgr::seed_plan_bytes(width, height, stride);
}

int dgr_seed_plan(void* stream, int width, int height, int stride, const float* depth_obs, const float* opacity_map,
                  const float* depth, float depth_min, float depth_max, float silhouette_threshold, float depth_error_min,
                  const float* depth_error_min_device, long rows, void* plan, int* counts8_device) {
    const char* bad = seed_shape_error(width, height, stride);
    if (!bad) bad = plan_args_error(rows, nullptr, plan, true, counts8_device);
    if (!bad && (!depth_obs)) bad = "depth_obs is NULL";
    if (bad) return refuse("dgr_seed_plan", bad);
    HIP_TRY(dgr::launch_seed_plan(width, height, stride, depth_obs, opacity_map, depth, depth_min, depth_max, silhouette_threshold,
                                  depth_error_min, depth_error_min_device, (size_t)rows, plan, counts8_device,
                                  (hipStream_t)stream));
    return DGR_OK;
}

int dgr_seed_apply(void* stream, int width, int height, int stride, long rows, long rows_out, const void* plan, int n,
                   const dgr_seed_tensor* tensors, const float* color_obs, const float* depth_obs, const float* viewmatrix,
                   float fx, float fy, float cx, float cy, float pix) {
    const char* bad = seed_shape_error(width, height, stride);
    int n_xyz = 0;
    if (!bad) {
        const bool fits = rows_out >= rows && rows_out - rows <= (long)dgr::seed_candidates(width, height, stride);
        bad = plan_args_error(rows, fits ? nullptr : "rows_out must be rows + the plan's count of new rows (rows .. rows + candidates)",
                              plan, false, nullptr);
    }
    if (!bad && (!depth_obs)) bad = "depth_obs is NULL";
    if (!bad && (!viewmatrix)) bad = "viewmatrix is NULL";
    if (!bad && (!(fx > 0.0f && fy > 0.0f && std::isfinite(fx) && std::isfinite(fy)))) bad = "fx and fy must be finite and positive";
    if (!bad)
        bad = tensor_table_error(
            n, tensors, DGR_SEED_MAX_TENSORS, "n must be 1 .. DGR_SEED_MAX_TENSORS (24) tensors", DGR_SEED_XYZ, DGR_SEED_CONST,
            DGR_SEED_XYZ, n_xyz, [&](const dgr_seed_tensor& t) -> const char* {
                if (t.mode == DGR_SEED_LOG_SCALE && t.k != 3 && t.k != 1) return "a LOG_SCALE tensor must have k = 3 or k = 1";
                if (t.mode == DGR_SEED_RGB_DC && t.k != 3) return "an RGB_DC tensor must have k = 3";
                if (t.mode == DGR_SEED_RGB_DC && !color_obs) return "RGB_DC needs color_obs";
                if (t.mode == DGR_SEED_QUAT_IDENTITY && t.k != 4) return "a QUAT_IDENTITY tensor must have k = 4";
                if (rows_out > 0 && (!t.dst || (rows > 0 && !t.src))) return "a tensor with a NULL dst, or a NULL src with rows > 0";
                return nullptr;
            });
    if (bad) return refuse("dgr_seed_apply", bad);
    HIP_TRY(dgr::launch_seed_apply(width, height, stride, (size_t)rows, (size_t)rows_out, plan, n, tensors, color_obs, depth_obs,
                                   viewmatrix, (float)(1.0 / (double)fx), (float)(1.0 / (double)fy), cx, cy, pix,
                                   (hipStream_t)stream));
    return DGR_OK;
}

int dgr_pose_forward(void* stream, const float* quat, const float* trans, const float* perspec_matrix, float* viewmatrix,
                     float* projmatrix, float* campos) {
    if (!quat || !trans || !perspec_matrix || !viewmatrix || !projmatrix || !campos) return refuse("dgr_pose_forward", "NULL argument");
    HIP_TRY(dgr::launch_pose_forward(quat, trans, perspec_matrix, viewmatrix, projmatrix, campos, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_pose_backward(void* stream, const float* quat, const float* dL_dviewmatrix, float* dL_dquat, float* dL_dtrans) {
    if (!quat || !dL_dviewmatrix || !dL_dquat || !dL_dtrans) return refuse("dgr_pose_backward", "NULL argument");
    HIP_TRY(dgr::launch_pose_backward(quat, dL_dviewmatrix, dL_dquat, dL_dtrans, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_l1_loss_scratch_floats(void) { return dgr::l1_loss_partials(); }
int dgr_l1_loss_forward(void* stream, long n_color, const float* color, const float* color_obs, long n_depth, const float* depth,
                        const float* depth_obs, float w_color, float w_depth, float* scratch, float* loss) {
    if (n_color < 0 || n_depth < 0 || !scratch || !loss || (n_color > 0 && (!color || !color_obs)) ||
        (n_depth > 0 && (!depth || !depth_obs))) return refuse("dgr_l1_loss_forward", "bad argument");
    HIP_TRY(dgr::launch_l1_loss_forward(n_color, color, color_obs, n_depth, depth, depth_obs, w_color, w_depth, scratch, loss,
                                        (hipStream_t)stream));
    return DGR_OK;
}
int dgr_l1_loss_backward(void* stream, long n_color, const float* color, const float* color_obs, long n_depth, const float* depth,
                         const float* depth_obs, float w_color, float w_depth, const float* upstream, float* dL_dcolor,
                         float* dL_ddepth) {
    if (n_color < 0 || n_depth < 0 || (n_color > 0 && (!color || !color_obs || !dL_dcolor)) ||
        (n_depth > 0 && (!depth || !depth_obs || !dL_ddepth))) return refuse("dgr_l1_loss_backward", "bad argument");
    HIP_TRY(dgr::launch_l1_loss_backward(n_color, color, color_obs, n_depth, depth, depth_obs, w_color, w_depth, upstream,
                                         dL_dcolor, dL_ddepth, (hipStream_t)stream));
    return DGR_OK;
}

// the shared argument checks of dgr_ssim_loss_forward / _backward: the message, or NULL
static const char* ssim_bad_argument(int n_images, int channels, int height, int width, const float* img, const float* ref,
                                     long n_depth, const float* depth, const float* depth_obs, const float* scratch) {
    if (n_images <= 0 || channels <= 0 || height <= 0 || width <= 0) return "n_images, channels, height and width must be positive";
    if (!dgr::ssim_shape_ok(n_images, channels, height, width))
        return "n_images * channels must be at most 65535 (one grid plane each) and height, width at most 2^20";
    if (!img || !ref) return "img or ref is NULL";
    if (n_depth < 0) return "n_depth is negative";
    if (n_depth > 0 && (!depth || !depth_obs)) return "n_depth > 0 with a NULL depth or depth_obs";
    if (!scratch || !dgr::aligned16(scratch)) return "scratch is NULL or not 16-byte aligned";
    return nullptr;
}
long dgr_ssim_scratch_floats(int n_images, int channels, int height, int width) {
    return dgr::ssim_scratch_floats(n_images, channels, height, width);
}
int dgr_ssim_loss_forward(void* stream, int n_images, int channels, int height, int width, const float* img, const float* ref,
                          long n_depth, const float* depth, const float* depth_obs, float w_l1, float w_ssim, float w_depth,
                          float* scratch, int want_maps, float* loss) {
    const char* bad = ssim_bad_argument(n_images, channels, height, width, img, ref, n_depth, depth, depth_obs, scratch);
    if (!bad && !loss) bad = "loss is NULL";
    if (bad) return refuse("dgr_ssim_loss_forward", bad);
    HIP_TRY(dgr::launch_ssim_loss_forward(n_images, channels, height, width, img, ref, n_depth, depth, depth_obs, w_l1, w_ssim,
                                          w_depth, scratch, want_maps != 0, loss, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_ssim_loss_backward(void* stream, int n_images, int channels, int height, int width, const float* img, const float* ref,
                           long n_depth, const float* depth, const float* depth_obs, float w_l1, float w_ssim, float w_depth,
                           const float* scratch, const float* upstream, float* dL_dimg, float* dL_ddepth) {
    const char* bad = ssim_bad_argument(n_images, channels, height, width, img, ref, n_depth, depth, depth_obs, scratch);
    if (!bad && !dL_dimg) bad = "dL_dimg is NULL";
    if (!bad && n_depth > 0 && !dL_ddepth) bad = "n_depth > 0 with a NULL dL_ddepth";
    if (bad) return refuse("dgr_ssim_loss_backward", bad);
    HIP_TRY(dgr::launch_ssim_loss_backward(n_images, channels, height, width, img, ref, n_depth, depth, depth_obs, w_l1, w_ssim,
                                           w_depth, scratch, upstream, dL_dimg, dL_ddepth, (hipStream_t)stream));
    return DGR_OK;
}

// the shared argument checks of dgr_masked_loss_forward / _backward: the message, or NULL
static const char* masked_loss_bad_argument(int n_views, int channels, int height, int width, const float* color,
                                            const float* color_obs, const float* depth, const float* depth_obs,
                                            const dgr_masked_loss_params* p, const void* scratch) {
    if (n_views <= 0 || channels <= 0 || height <= 0 || width <= 0) return "n_views, channels, height and width must be positive";
    if (!dgr::masked_loss_shape_ok(n_views, height, width)) return "n_views must be at most 65535 and height * width at most 2^30";
    if (!color || !color_obs) return "color or color_obs is NULL";
    if (!depth || !depth_obs) return "depth or depth_obs is NULL";
    if (!p) return "params is NULL";
    if (std::isnan(p->depth_lo) || std::isnan(p->depth_hi)) return "depth_lo or depth_hi is NaN";
    if (std::isnan(p->silhouette_threshold)) return "silhouette_threshold is NaN";
    if (std::isnan(p->outlier_factor)) return "outlier_factor is NaN";
    if (p->reject_outliers && p->outlier_factor < 0.f) return "outlier_factor is negative";
    if (p->reduction != DGR_MASKED_LOSS_SUM && p->reduction != DGR_MASKED_LOSS_MEAN) return "unknown reduction";
    if (!scratch || !dgr::aligned16(scratch)) return "scratch is NULL or not 16-byte aligned";
    return nullptr;
}
static dgr::MaskedLossArgs masked_loss_args(int n_views, int channels, int height, int width, const float* color,
                                            const float* color_obs, const float* depth, const float* depth_obs,
                                            const float* opacity_map, const unsigned char* mask, const dgr_masked_loss_params& p) {
    dgr::MaskedLossArgs a{};
    a.V = n_views, a.C = channels, a.H = height, a.W = width;
    a.color = color, a.color_obs = color_obs, a.depth = depth, a.depth_obs = depth_obs, a.opacity = opacity_map, a.mask = mask;
    a.lo = p.depth_lo, a.hi = p.depth_hi, a.silhouette = p.silhouette_threshold, a.factor = p.outlier_factor;
    a.w_color = p.w_color, a.w_depth = p.w_depth;
    a.reject = p.reject_outliers != 0, a.mask_color = p.mask_color != 0, a.mean = p.reduction == DGR_MASKED_LOSS_MEAN;
    return a;
}
size_t dgr_masked_loss_scratch_bytes(int n_views, int height, int width) {
    return (size_t)dgr::masked_loss_layout(n_views, height, width).total;
}
int dgr_masked_loss_forward(void* stream, int n_views, int channels, int height, int width, const float* color,
                            const float* color_obs, const float* depth, const float* depth_obs, const float* opacity_map,
                            const unsigned char* mask, const dgr_masked_loss_params* params, void* scratch, float* loss) {
    const char* bad = masked_loss_bad_argument(n_views, channels, height, width, color, color_obs, depth, depth_obs, params, scratch);
    if (!bad && !loss) bad = "loss is NULL";
    if (bad) return refuse("dgr_masked_loss_forward", bad);
    HIP_TRY(dgr::launch_masked_loss_forward(masked_loss_args(n_views, channels, height, width, color, color_obs, depth, depth_obs,
                                                             opacity_map, mask, *params),
                                            scratch, loss, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_masked_loss_backward(void* stream, int n_views, int channels, int height, int width, const float* color,
                             const float* color_obs, const float* depth, const float* depth_obs, const float* opacity_map,
                             const unsigned char* mask, const dgr_masked_loss_params* params, const void* scratch,
                             const float* upstream, float* dL_dcolor, float* dL_ddepth) {
    const char* bad = masked_loss_bad_argument(n_views, channels, height, width, color, color_obs, depth, depth_obs, params, scratch);
    if (!bad && !dL_dcolor && !dL_ddepth) bad = "dL_dcolor and dL_ddepth are both NULL";
    if (bad) return refuse("dgr_masked_loss_backward", bad);
    HIP_TRY(dgr::launch_masked_loss_backward(masked_loss_args(n_views, channels, height, width, color, color_obs, depth, depth_obs,
                                                              opacity_map, mask, *params),
                                             scratch, upstream, dL_dcolor, dL_ddepth, (hipStream_t)stream));
    return DGR_OK;
}

// 2^20 keyframes at most: with n_keyframes * candidates below 2^31 the count launch then stays under 2^21 workgroups
static const int OVERLAP_MAX_KEYFRAMES = 1 << 20;
static const char* keyframe_overlap_shape_error(int width, int height, int stride, int n_keyframes) {
    if (width < 1 || height < 1) return "width and height must be positive";
    if (stride < 1) return "stride must be positive";
    if (n_keyframes < 1) return "n_keyframes must be positive";
    if (n_keyframes > OVERLAP_MAX_KEYFRAMES) return "n_keyframes must be at most 2^20";
    if (dgr::seed_candidates(width, height, stride) * (size_t)n_keyframes >= ((size_t)1 << 31))
        return "n_keyframes * candidates must be below 2^31";
    return nullptr;
}
size_t dgr_keyframe_overlap_scratch_bytes(int width, int height, int stride, int n_keyframes) {
    return keyframe_overlap_shape_error(width, height, stride, n_keyframes)
               ? 0
               : dgr::keyframe_overlap_scratch_bytes(width, height, stride, n_keyframes);
}
int dgr_keyframe_overlap(void* stream, int width, int height, const float* depth_obs, const float* viewmatrix, int n_keyframes,
                         const float* keyframe_viewmatrices, const float* keyframe_depths,
                         const dgr_keyframe_overlap_params* params, void* scratch, int* inside, int* visible, int* valid,
                         float* score, unsigned char* flags) {
    const dgr_keyframe_overlap_params* p = params;
    const char* bad = !p ? "params is NULL" : keyframe_overlap_shape_error(width, height, p->stride, n_keyframes);
    if (!bad && !depth_obs) bad = "depth_obs is NULL";
    if (!bad && !viewmatrix) bad = "viewmatrix is NULL";
    if (!bad && !keyframe_viewmatrices) bad = "keyframe_viewmatrices is NULL";
    if (!bad && (!scratch || !dgr::aligned16(scratch))) bad = "scratch is NULL or not 16-byte aligned";
    if (!bad && (!inside || !visible || !valid || !score)) bad = "inside, visible, valid or score is NULL";
    if (!bad && !(p->fx > 0.0f && p->fy > 0.0f && std::isfinite(p->fx) && std::isfinite(p->fy)))
        bad = "fx and fy must be finite and positive";
    if (!bad && (std::isnan(p->cx) || std::isnan(p->cy))) bad = "cx or cy is NaN";
    if (!bad && (std::isnan(p->depth_min) || std::isnan(p->depth_max))) bad = "depth_min or depth_max is NaN";
    if (!bad && std::isnan(p->near_z)) bad = "near_z is NaN";
    if (!bad && !(p->edge >= 0.0f)) bad = "edge is NaN or negative";
    if (!bad && !(p->depth_tolerance >= 0.0f)) bad = "depth_tolerance is NaN or negative";
    if (bad) return refuse("dgr_keyframe_overlap", bad);
    dgr::KeyframeOverlapArgs a{};
    a.W = width, a.H = height, a.stride = p->stride, a.K = n_keyframes;
    a.depth_obs = depth_obs, a.viewmatrix = viewmatrix, a.keyframe_viewmatrices = keyframe_viewmatrices;
    a.keyframe_depths = keyframe_depths;
    a.fx = p->fx, a.fy = p->fy, a.inv_fx = (float)(1.0 / (double)p->fx), a.inv_fy = (float)(1.0 / (double)p->fy);
    a.cx = p->cx, a.cy = p->cy, a.depth_min = p->depth_min, a.depth_max = p->depth_max;
    a.edge = p->edge, a.near_z = p->near_z, a.depth_tolerance = p->depth_tolerance;
    a.inside = inside, a.visible = visible, a.valid = valid, a.score = score, a.flags = flags;
    HIP_TRY(dgr::launch_keyframe_overlap(a, scratch, (hipStream_t)stream));
    return DGR_OK;
}

int dgr_depth_normals(void* stream, int width, int height, const float* depth, const float* mask_image, float mask_threshold,
                      float fx, float fy, float cx, float cy, float depth_min, float depth_max, float max_jump, float* vnmap) {
    const char* bad = width < 1 || height < 1 ? "width and height must be positive" : nullptr;
    if (!bad && (size_t)width * (size_t)height > (size_t)PLAN_MAX_ROWS) bad = "2^30 pixels or more";
    if (!bad && !depth) bad = "depth is NULL";
    if (!bad && (!vnmap || !dgr::aligned16(vnmap))) bad = "vnmap is NULL or not 16-byte aligned";
    if (!bad && !(fx > 0.0f && fy > 0.0f && std::isfinite(fx) && std::isfinite(fy))) bad = "fx and fy must be finite and positive";
    if (!bad && (std::isnan(cx) || std::isnan(cy))) bad = "cx or cy is NaN";
    if (!bad && (std::isnan(depth_min) || std::isnan(depth_max))) bad = "depth_min or depth_max is NaN";
    if (!bad && !(max_jump >= 0.0f)) bad = "max_jump is NaN or negative";
    if (!bad && mask_image && std::isnan(mask_threshold)) bad = "mask_threshold is NaN";
    if (bad) return refuse("dgr_depth_normals", bad);
    dgr::DepthNormalsArgs a{};
    a.W = width, a.H = height, a.depth = depth, a.mask = mask_image, a.mask_threshold = mask_threshold;
    a.inv_fx = (float)(1.0 / (double)fx), a.inv_fy = (float)(1.0 / (double)fy), a.cx = cx, a.cy = cy;
    a.depth_min = depth_min, a.depth_max = depth_max, a.max_jump = max_jump, a.vnmap = reinterpret_cast<float4*>(vnmap);
    HIP_TRY(dgr::launch_depth_normals(a, (hipStream_t)stream));
    return DGR_OK;
}

size_t dgr_icp_scratch_bytes(int width, int height, int stride) {
    return seed_shape_error(width, height, stride) ? 0 : dgr::icp_scratch_bytes(width, height, stride);
}
// what dgr_icp_step and dgr_rgbd_step check alike (the message, or NULL) and fill in alike
static const char* icp_step_bad_argument(int width, int height, const float* depth_obs, const float* vn_obs, const float* vn_model,
                                         const float* model_viewmatrix, const float* viewmatrix_in, const dgr_icp_params* p,
                                         void* scratch, float* viewmatrix_out, double* stats) {
    const char* bad = !p ? "params is NULL" : seed_shape_error(width, height, p->stride);
    if (!bad && !depth_obs) bad = "depth_obs is NULL";
    if (!bad && vn_obs && !dgr::aligned16(vn_obs)) bad = "vn_obs is not 16-byte aligned";
    if (!bad && (!vn_model || !dgr::aligned16(vn_model))) bad = "vn_model is NULL or not 16-byte aligned";
    if (!bad && !model_viewmatrix) bad = "model_viewmatrix is NULL";
    if (!bad && !viewmatrix_in) bad = "viewmatrix_in is NULL";
    if (!bad && (!scratch || !dgr::aligned16(scratch))) bad = "scratch is NULL or not 16-byte aligned";
    if (!bad && !viewmatrix_out) bad = "viewmatrix_out is NULL";
    if (!bad && (!stats || (reinterpret_cast<uintptr_t>(stats) & 7u))) bad = "stats is NULL or not 8-byte aligned";
    if (!bad && !(p->fx > 0.0f && p->fy > 0.0f && std::isfinite(p->fx) && std::isfinite(p->fy)))
        bad = "fx and fy must be finite and positive";
    if (!bad && (std::isnan(p->cx) || std::isnan(p->cy))) bad = "cx or cy is NaN";
    if (!bad && (std::isnan(p->depth_min) || std::isnan(p->depth_max))) bad = "depth_min or depth_max is NaN";
    if (!bad && !(p->dist_max >= 0.0f)) bad = "dist_max is NaN or negative";
    if (!bad && !(p->normal_cos_min >= -1.0f && p->normal_cos_min <= 1.0f)) bad = "normal_cos_min must lie in [-1, 1]";
    if (!bad && !(p->huber_delta >= 0.0f)) bad = "huber_delta is NaN or negative";
    if (!bad && !(p->damping >= 0.0f)) bad = "damping is NaN or negative";
    if (!bad && !(p->rcond >= 0.0f)) bad = "rcond is NaN or negative";
    if (!bad && p->min_points < 1) bad = "min_points must be at least 1";
    return bad;
}
static void icp_step_fill(dgr::IcpStepArgs& a, int width, int height, const float* depth_obs, const float* vn_obs,
                          const float* vn_model, const float* model_viewmatrix, const float* viewmatrix_in, const dgr_icp_params* p,
                          float* viewmatrix_out, float* quat_out, float* trans_out, double* stats, unsigned char* flags) {
    a.W = width, a.H = height, a.stride = p->stride, a.depth_obs = depth_obs;
    a.vn_obs = reinterpret_cast<const float4*>(vn_obs), a.vn_model = reinterpret_cast<const float4*>(vn_model);
    a.model_viewmatrix = model_viewmatrix, a.viewmatrix_in = viewmatrix_in;
    a.fx = p->fx, a.fy = p->fy, a.inv_fx = (float)(1.0 / (double)p->fx), a.inv_fy = (float)(1.0 / (double)p->fy);
    a.cx = p->cx, a.cy = p->cy, a.depth_min = p->depth_min, a.depth_max = p->depth_max, a.dist_max = p->dist_max;
    a.normal_cos_min = p->normal_cos_min, a.huber_delta = p->huber_delta, a.damping = (double)p->damping, a.rcond = (double)p->rcond;
    a.min_points = p->min_points;
    a.viewmatrix_out = viewmatrix_out, a.quat_out = quat_out, a.trans_out = trans_out, a.stats = stats, a.flags = flags;
}
int dgr_icp_step(void* stream, int width, int height, const float* depth_obs, const float* vn_obs, const float* vn_model,
                 const float* model_viewmatrix, const float* viewmatrix_in, const dgr_icp_params* params, void* scratch,
                 float* viewmatrix_out, float* quat_out, float* trans_out, double* stats, unsigned char* flags) {
    const char* bad = icp_step_bad_argument(width, height, depth_obs, vn_obs, vn_model, model_viewmatrix, viewmatrix_in, params, scratch,
                                            viewmatrix_out, stats);
    if (bad) return refuse("dgr_icp_step", bad);
    dgr::IcpStepArgs a{};
    icp_step_fill(a, width, height, depth_obs, vn_obs, vn_model, model_viewmatrix, viewmatrix_in, params, viewmatrix_out, quat_out,
                  trans_out, stats, flags);
    HIP_TRY(dgr::launch_icp_step(a, scratch, (hipStream_t)stream));
    return DGR_OK;
}

int dgr_intensity_map(void* stream, int width, int height, int channels, const float* image, const float* mask_image,
                      float mask_threshold, float* imap, float* intensity) {
    const char* bad = width < 1 || height < 1 ? "width and height must be positive" : nullptr;
    if (!bad && (size_t)width * (size_t)height > (size_t)PLAN_MAX_ROWS) bad = "2^30 pixels or more";
    if (!bad && channels != 1 && channels != 3) bad = "channels must be 1 or 3";
    if (!bad && !image) bad = "image is NULL";
    if (!bad && !imap && !intensity) bad = "imap and intensity are both NULL";
    if (!bad && imap && !dgr::aligned16(imap)) bad = "imap is not 16-byte aligned";
    if (!bad && mask_image && std::isnan(mask_threshold)) bad = "mask_threshold is NaN";
    if (bad) return refuse("dgr_intensity_map", bad);
    dgr::IntensityMapArgs a{};
    a.W = width, a.H = height, a.C = channels, a.image = image, a.mask = mask_image, a.mask_threshold = mask_threshold;
    a.imap = reinterpret_cast<float4*>(imap), a.intensity = intensity;
    HIP_TRY(dgr::launch_intensity_map(a, (hipStream_t)stream));
    return DGR_OK;
}

int dgr_frame_halve(void* stream, int width, int height, int n_planes, const float* planes, const float* depth, float depth_min,
                    float depth_max, float max_jump, float* planes_out, float* depth_out) {
    const char* bad = width < 2 || height < 2 ? "width and height must be at least 2" : nullptr;
    if (!bad && (size_t)width * (size_t)height > (size_t)PLAN_MAX_ROWS) bad = "2^30 pixels or more";
    if (!bad && (n_planes < 0 || n_planes > 64)) bad = "n_planes must be 0 .. 64";
    if (!bad && n_planes == 0 && !depth) bad = "nothing to halve: n_planes is 0 and depth is NULL";
    if (!bad && n_planes > 0 && (!planes || !planes_out)) bad = "planes or planes_out is NULL";
    if (!bad && depth && !depth_out) bad = "depth_out is NULL";
    if (!bad && depth && (std::isnan(depth_min) || std::isnan(depth_max))) bad = "depth_min or depth_max is NaN";
    if (!bad && depth && !(max_jump >= 0.0f)) bad = "max_jump is NaN or negative";
    if (bad) return refuse("dgr_frame_halve", bad);
    dgr::FrameHalveArgs a{};
    a.W = width, a.H = height, a.planes = n_planes, a.planes_in = planes, a.depth_in = depth;
    a.depth_min = depth_min, a.depth_max = depth_max, a.max_jump = max_jump, a.planes_out = planes_out, a.depth_out = depth_out;
    HIP_TRY(dgr::launch_frame_halve(a, (hipStream_t)stream));
    return DGR_OK;
}

size_t dgr_rgbd_scratch_bytes(int width, int height, int stride) { return dgr_icp_scratch_bytes(width, height, stride); }
int dgr_rgbd_step(void* stream, int width, int height, const float* depth_obs, const float* vn_obs, const float* vn_model,
                  const float* intensity_obs, const float* imap_model, const float* model_viewmatrix, const float* viewmatrix_in,
                  const dgr_rgbd_params* params, void* scratch, float* viewmatrix_out, float* quat_out, float* trans_out,
                  double* stats, unsigned char* flags) {
    const dgr_rgbd_params* p = params;
    dgr_icp_params icp{};
    if (p)
        icp = dgr_icp_params{p->fx, p->fy, p->cx, p->cy, p->depth_min, p->depth_max, p->dist_max, p->normal_cos_min, p->huber_delta,
                             p->damping, p->rcond, p->min_points, p->stride};
    const char* bad = icp_step_bad_argument(width, height, depth_obs, vn_obs, vn_model, model_viewmatrix, viewmatrix_in, p ? &icp : nullptr,
                                            scratch, viewmatrix_out, stats);
    if (!bad && !intensity_obs) bad = "intensity_obs is NULL";
    if (!bad && (!imap_model || !dgr::aligned16(imap_model))) bad = "imap_model is NULL or not 16-byte aligned";
    if (!bad && !(p->geo_weight >= 0.0f)) bad = "geo_weight is NaN or negative";
    if (!bad && !(p->photo_weight >= 0.0f)) bad = "photo_weight is NaN or negative";
    if (!bad && !(p->photo_max >= 0.0f)) bad = "photo_max is NaN or negative";
    if (!bad && !(p->photo_huber >= 0.0f)) bad = "photo_huber is NaN or negative";
    if (bad) return refuse("dgr_rgbd_step", bad);
    dgr::RgbdStepArgs a{};
    icp_step_fill(a, width, height, depth_obs, vn_obs, vn_model, model_viewmatrix, viewmatrix_in, &icp, viewmatrix_out, quat_out,
                  trans_out, stats, flags);
    a.intensity_obs = intensity_obs, a.imap_model = reinterpret_cast<const float4*>(imap_model);
    a.geo_weight = p->geo_weight, a.photo_weight = p->photo_weight, a.photo_max = p->photo_max, a.photo_huber = p->photo_huber;
    HIP_TRY(dgr::launch_rgbd_step(a, scratch, (hipStream_t)stream));
    return DGR_OK;
}

static const int PGO_MAX_POSES = 1 << 16, PGO_MAX_EDGES = 1 << 18, PGO_MAX_ITERATIONS = 1000;
// 12 * 65 536 (the Python default at the largest graph) fits; one launch runs at most iterations * cg_iterations CG iterations
static const int PGO_MAX_CG_ITERATIONS = 1 << 20;
static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
static const char* pgo_shape_error(int n_poses, int n_edges) {
    if (n_poses < 1 || n_poses > PGO_MAX_POSES) return "n_poses must be 1 .. 65536";
    if (n_edges < 0 || n_edges > PGO_MAX_EDGES) return "n_edges must be 0 .. 2^18";
    return nullptr;
}
size_t dgr_pgo_scratch_bytes(int n_poses, int n_edges) {
    return pgo_shape_error(n_poses, n_edges) ? 0 : dgr::pgo_scratch_bytes(n_poses, n_edges);
}
int dgr_pgo_plan(void* stream, int n_poses, int n_edges, const int* edges, void* scratch) {
    const char* bad = pgo_shape_error(n_poses, n_edges);
    if (!bad && n_edges > 0 && !edges) bad = "edges is NULL";
    if (!bad && !aligned4(edges)) bad = "edges is not 4-byte aligned";
    if (!bad && (!scratch || !dgr::aligned16(scratch))) bad = "scratch is NULL or not 16-byte aligned";
    if (bad) return refuse("dgr_pgo_plan", bad);
    HIP_TRY(dgr::launch_pgo_plan(n_poses, n_edges, edges, scratch, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_pgo_solve(void* stream, int n_poses, int n_edges, const float* poses_in, const int* edges, const float* measurements,
                  const float* information, int information_kind, const unsigned char* fixed, const dgr_pgo_params* params,
                  void* scratch, float* poses_out, float* chi2, double* stats, int* flags) {
    const dgr_pgo_params* p = params;
    const char* bad = !p ? "params is NULL" : pgo_shape_error(n_poses, n_edges);
    if (!bad && !poses_in) bad = "poses_in is NULL";
    if (!bad && n_edges > 0 && !edges) bad = "edges is NULL";
    if (!bad && n_edges > 0 && !measurements) bad = "measurements is NULL";
    if (!bad && information_kind != 0 && information_kind != 2 && information_kind != 36) bad = "information_kind must be 0, 2 or 36";
    if (!bad && information_kind != 0 && n_edges > 0 && !information) bad = "information is NULL";
    if (!bad && (!scratch || !dgr::aligned16(scratch))) bad = "scratch is NULL or not 16-byte aligned";
    if (!bad && !poses_out) bad = "poses_out is NULL";
    if (!bad && (!stats || (reinterpret_cast<uintptr_t>(stats) & 7u))) bad = "stats is NULL or not 8-byte aligned";
    if (!bad && !flags) bad = "flags is NULL";
    if (!bad && !(aligned4(poses_in) && aligned4(edges) && aligned4(measurements) && aligned4(information) && aligned4(poses_out) &&
                  aligned4(chi2) && aligned4(flags)))
        bad = "poses_in, edges, measurements, information, poses_out, chi2 or flags is not 4-byte aligned";
    if (!bad && (p->iterations < 0 || p->iterations > PGO_MAX_ITERATIONS)) bad = "iterations must be 0 .. 1000";
    if (!bad && (p->cg_iterations < 1 || p->cg_iterations > PGO_MAX_CG_ITERATIONS)) bad = "cg_iterations must be 1 .. 2^20";
    if (!bad && !(p->cg_tolerance >= 0.0f)) bad = "cg_tolerance is NaN or negative";
    if (!bad && !(p->huber_delta >= 0.0f)) bad = "huber_delta is NaN or negative";
    if (!bad && !(p->damping >= 0.0f)) bad = "damping is NaN or negative";
    if (!bad && !(p->rcond >= 0.0f)) bad = "rcond is NaN or negative";
    if (!bad && !(p->step_tolerance >= 0.0f)) bad = "step_tolerance is NaN or negative";
    if (!bad && !(p->cost_tolerance >= 0.0f)) bad = "cost_tolerance is NaN or negative";
    if (bad) return refuse("dgr_pgo_solve", bad);
    dgr::PgoArgs a{};
    a.K = n_poses, a.E = n_edges, a.poses_in = poses_in, a.edges = edges, a.measurements = measurements;
    a.information = information, a.information_kind = information_kind, a.fixed = fixed;
    a.iterations = p->iterations, a.cg_iterations = p->cg_iterations;
    a.cg_tolerance = (double)p->cg_tolerance, a.huber_delta = (double)p->huber_delta, a.damping = (double)p->damping;
    a.rcond = (double)p->rcond, a.step_tolerance = (double)p->step_tolerance, a.cost_tolerance = (double)p->cost_tolerance;
    a.poses_out = poses_out, a.chi2 = chi2, a.stats = stats, a.flags = flags;
    HIP_TRY(dgr::launch_pgo_solve(a, scratch, (hipStream_t)stream));
    return DGR_OK;
}

// ---- contribution statistics (contrib.hip)
static bool aligned_to(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }
static size_t contribution_plane(long P, size_t elem) { return dgr::align_up(elem * (size_t)P, 256); }
size_t dgr_contribution_scratch_bytes(long P) {
    if (P < 0 || P > (long)DGR_ID_MASK) return 0;
    return contribution_plane(P, 4) + contribution_plane(P, 4) + contribution_plane(P, 8) + 256;  // (never 0 for a valid P)
}
int dgr_contribution_stats(void* stream, long P, int width, int height, int R, const char* geometry_buffer,
                           const char* binning_buffer, const char* image_buffer, const dgr_contribution_params* params,
                           void* scratch, int* n_touched, float* max_weight, long long* sum_weight, long long* touched_total,
                           float* max_weight_total, long long* sum_weight_total, int* views, int* last_seen,
                           int* counts4_device) {
    const dgr_contribution_params* p = params;
    const bool all_views = n_touched && max_weight && sum_weight;
    const char* bad = !p ? "params is NULL" : nullptr;
    if (!bad && (P < 0 || P > (long)DGR_ID_MASK)) bad = "P must be 0 .. 2^28 - 1";
    if (!bad && (width <= 0 || height <= 0 || (long long)width * height > (1ll << 30))) bad = "width and height must be positive (and width * height at most 2^30)";
    if (!bad && R < 0) bad = "R is negative";
    if (!bad && P > 0 && (!geometry_buffer || !binning_buffer || !image_buffer)) bad = "the forward's three state buffers are required";
    if (!bad && p->min_pixels < 0) bad = "min_pixels is negative";
    if (!bad && !(p->weight_min >= 0.0f)) bad = "weight_min is NaN or negative";
    if (!bad && P > 0 && !all_views && !scratch) bad = "scratch is NULL (a per-view output is NULL: it lives there)";
    if (!bad && !dgr::aligned16(scratch)) bad = "scratch is not 16-byte aligned";
    if (!bad && !(aligned_to(n_touched, 4) && aligned_to(max_weight, 4) && aligned_to(views, 4) && aligned_to(last_seen, 4) &&
                  aligned_to(max_weight_total, 4) && aligned_to(counts4_device, 4)))
        bad = "n_touched, max_weight, max_weight_total, views, last_seen or counts4_device is not 4-byte aligned";
    if (!bad && !(aligned_to(sum_weight, 8) && aligned_to(touched_total, 8) && aligned_to(sum_weight_total, 8)))
        bad = "sum_weight, touched_total or sum_weight_total is not 8-byte aligned";
    if (!bad && !n_touched && !max_weight && !sum_weight && !touched_total && !max_weight_total && !sum_weight_total && !views &&
        !last_seen && !counts4_device)
        bad = "nothing to write (every output is NULL)";
    if (bad) return refuse("dgr_contribution_stats", bad);
    hipStream_t st = (hipStream_t)stream;
    if (P == 0) {  // no Gaussians, no frame: only the counts
        if (counts4_device) HIP_TRY(dgr::launch_contrib_clear(0, nullptr, nullptr, nullptr, counts4_device, st));
        return DGR_OK;
    }
    char* sc = static_cast<char*>(scratch);
    if (!n_touched) n_touched = reinterpret_cast<int*>(sc);
    if (!max_weight) max_weight = reinterpret_cast<float*>(sc + contribution_plane(P, 4));
    if (!sum_weight) sum_weight = reinterpret_cast<long long*>(sc + 2 * contribution_plane(P, 4));
    const dgr::GeometryView geom = dgr::carve_geometry(const_cast<char*>(geometry_buffer), (int)P);
    const dgr::ImageView img = dgr::carve_image(const_cast<char*>(image_buffer), width, height);
    HIP_TRY(dgr::launch_contrib_clear(P, n_touched, max_weight, sum_weight, counts4_device, st));
    dgr::ContribTilesArgs t{};
    t.W = width, t.H = height, t.grid_x = dgr::tiles_x(width), t.grid_y = dgr::tiles_y(height);
    t.sched = img.tile_sched, t.ranges = img.ranges, t.sched_flag = img.cursor + 3;
    t.point_list = reinterpret_cast<const uint32_t*>(binning_buffer), t.rec = geom.rec, t.n_contrib = img.n_contrib;
    t.n_touched = n_touched, t.max_weight_bits = reinterpret_cast<uint32_t*>(max_weight);
    t.sum_weight = reinterpret_cast<unsigned long long*>(sum_weight);
    HIP_TRY(dgr::launch_contrib_tiles(t, dgr::opt_alpha_mode(), st));
    dgr::ContribFoldArgs f{};
    f.P = P, f.sched_flag = img.cursor + 3, f.n_touched = n_touched, f.max_weight = max_weight, f.sum_weight = sum_weight;
    f.min_pixels = p->min_pixels, f.weight_min = p->weight_min, f.frame_id = p->frame_id;
    f.touched_total = touched_total, f.max_weight_total = max_weight_total, f.sum_weight_total = sum_weight_total;
    f.views = views, f.last_seen = last_seen, f.counts = counts4_device;
    if (touched_total || max_weight_total || sum_weight_total || views || last_seen || counts4_device) HIP_TRY(dgr::launch_contrib_fold(f, st));
    return DGR_OK;
}

// ---- TSDF fusion and mesh extraction (tsdf.hip)
static const char* tsdf_grid_error(const dgr_tsdf_grid* g) {
    if (!g) return "grid is NULL";
    if (g->nx < 1 || g->ny < 1 || g->nz < 1) return "the grid's nx, ny and nz must be positive";
    if ((unsigned long long)g->nx * (unsigned long long)g->ny >= (1ull << 31) ||
        (unsigned long long)g->nx * (unsigned long long)g->ny * (unsigned long long)g->nz >= (1ull << 31))
        return "the grid must hold fewer than 2^31 samples";
    if (!(g->voxel_size > 0.0f) || !std::isfinite(g->voxel_size)) return "voxel_size must be finite and positive";
    return nullptr;
}
int dgr_tsdf_integrate(void* stream, const dgr_tsdf_grid* grid, float* volume, float* color, int n_views, int width, int height,
                       const float* depth, const float* image, const float* mask, const float* viewmatrices,
                       const dgr_tsdf_params* params) {
    const dgr_tsdf_params* p = params;
    const char* bad = tsdf_grid_error(grid);
    if (!bad && !p) bad = "params is NULL";
    if (!bad && n_views < 1) bad = "n_views must be at least 1";
    if (!bad && (width < 1 || height < 1 || (long long)width * height > (1ll << 30))) bad = "width and height must be positive (and width * height at most 2^30)";
    if (!bad && !volume) bad = "volume is NULL";
    if (!bad && !depth) bad = "depth is NULL";
    if (!bad && !viewmatrices) bad = "viewmatrices is NULL";
    if (!bad && ((color != nullptr) != (image != nullptr))) bad = "the colour volume and the colour images go together: one of them is NULL";
    if (!bad && (!aligned_to(volume, 8) || !dgr::aligned16(color))) bad = "volume is not 8-byte aligned or color is not 16-byte aligned";
    if (!bad && !(aligned_to(depth, 4) && aligned_to(image, 4) && aligned_to(mask, 4) && aligned_to(viewmatrices, 4)))
        bad = "depth, image, mask or viewmatrices is not 4-byte aligned";
    if (!bad && !(p->fx > 0.0f && p->fy > 0.0f && std::isfinite(p->fx) && std::isfinite(p->fy))) bad = "fx and fy must be finite and positive";
    if (!bad && (!(p->truncation > 0.0f) || !std::isfinite(p->truncation))) bad = "truncation must be finite and positive";
    if (bad) return refuse("dgr_tsdf_integrate", bad);
    dgr::TsdfIntegrateArgs a{};
    a.nx = grid->nx, a.ny = grid->ny, a.nz = grid->nz;
    a.ox = grid->origin[0], a.oy = grid->origin[1], a.oz = grid->origin[2], a.voxel = grid->voxel_size;
    a.volume = reinterpret_cast<float2*>(volume), a.color = reinterpret_cast<float4*>(color);
    a.V = n_views, a.W = width, a.H = height, a.depth = depth, a.image = image, a.mask = mask, a.view = viewmatrices;
    a.fx = p->fx, a.fy = p->fy, a.cx = p->cx, a.cy = p->cy, a.truncation = p->truncation, a.weight = p->weight;
    a.max_weight = p->max_weight, a.depth_min = p->depth_min, a.depth_max = p->depth_max, a.near_z = p->near_z;
    a.mask_threshold = p->mask_threshold;
    HIP_TRY(dgr::launch_tsdf_integrate(a, (hipStream_t)stream));
    return DGR_OK;
}

size_t dgr_mesh_scratch_bytes(const dgr_tsdf_grid* grid) {
    return tsdf_grid_error(grid) ? 0 : dgr::mesh_scratch_bytes(grid->nx, grid->ny, grid->nz);
}
static dgr::MeshArgs mesh_args(const dgr_tsdf_grid* grid, const float* volume, const float* color, float min_weight) {
    dgr::MeshArgs a{};
    a.nx = grid->nx, a.ny = grid->ny, a.nz = grid->nz;
    a.ox = grid->origin[0], a.oy = grid->origin[1], a.oz = grid->origin[2], a.voxel = grid->voxel_size;
    a.volume = reinterpret_cast<const float2*>(volume), a.color = reinterpret_cast<const float4*>(color), a.min_weight = min_weight;
    return a;
}
int dgr_mesh_plan(void* stream, const dgr_tsdf_grid* grid, const float* volume, float min_weight, int max_triangles, void* scratch,
                  int* count, int* flags) {
    const char* bad = tsdf_grid_error(grid);
    if (!bad && !volume) bad = "volume is NULL";
    if (!bad && !aligned_to(volume, 8)) bad = "volume is not 8-byte aligned";
    if (!bad && std::isnan(min_weight)) bad = "min_weight is NaN";
    if (!bad && max_triangles < 0) bad = "max_triangles is negative";
    if (!bad && (!scratch || !dgr::aligned16(scratch))) bad = "scratch is NULL or not 16-byte aligned";
    if (!bad && (!count || !flags)) bad = "count or flags is NULL";
    if (!bad && !(aligned_to(count, 4) && aligned_to(flags, 4))) bad = "count or flags is not 4-byte aligned";
    if (bad) return refuse("dgr_mesh_plan", bad);
    HIP_TRY(dgr::launch_mesh_plan(mesh_args(grid, volume, nullptr, min_weight), max_triangles, scratch, count, flags, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_mesh_emit(void* stream, const dgr_tsdf_grid* grid, const float* volume, const float* color, float min_weight,
                  int max_triangles, const void* scratch, float* vertices, float* colors) {
    const char* bad = tsdf_grid_error(grid);
    if (!bad && !volume) bad = "volume is NULL";
    if (!bad && (!aligned_to(volume, 8) || !dgr::aligned16(color))) bad = "volume is not 8-byte aligned or color is not 16-byte aligned";
    if (!bad && std::isnan(min_weight)) bad = "min_weight is NaN";
    if (!bad && max_triangles < 0) bad = "max_triangles is negative";
    if (!bad && (!scratch || !dgr::aligned16(scratch))) bad = "scratch is NULL or not 16-byte aligned";
    if (!bad && max_triangles > 0 && !vertices) bad = "vertices is NULL";
    if (!bad && colors && !color) bad = "colors asked for of a volume without colour";
    if (!bad && !(aligned_to(vertices, 4) && aligned_to(colors, 4))) bad = "vertices or colors is not 4-byte aligned";
    if (bad) return refuse("dgr_mesh_emit", bad);
    HIP_TRY(dgr::launch_mesh_emit(mesh_args(grid, volume, colors ? color : nullptr, min_weight), max_triangles, scratch, vertices, colors,
                                  (hipStream_t)stream));
    return DGR_OK;
}

// ---- ray-casting the TSDF volume (raycast.hip)
size_t dgr_tsdf_brick_bytes(const dgr_tsdf_grid* grid) {
    return tsdf_grid_error(grid) ? 0 : dgr::tsdf_brick_count(grid->nx, grid->ny, grid->nz);
}
int dgr_tsdf_bricks(void* stream, const dgr_tsdf_grid* grid, const float* volume, float min_weight, unsigned char* bricks) {
    const char* bad = tsdf_grid_error(grid);
    if (!bad && !volume) bad = "volume is NULL";
    if (!bad && !aligned_to(volume, 8)) bad = "volume is not 8-byte aligned";
    if (!bad && std::isnan(min_weight)) bad = "min_weight is NaN";
    if (!bad && !bricks && dgr::tsdf_brick_count(grid->nx, grid->ny, grid->nz) > 0) bad = "bricks is NULL";
    if (bad) return refuse("dgr_tsdf_bricks", bad);
    dgr::BricksArgs a{};
    a.nx = grid->nx, a.ny = grid->ny, a.nz = grid->nz;
    a.volume = reinterpret_cast<const float2*>(volume), a.min_weight = min_weight, a.bricks = bricks;
    HIP_TRY(dgr::launch_tsdf_bricks(a, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_tsdf_raycast(void* stream, const dgr_tsdf_grid* grid, const float* volume, const float* color, const unsigned char* bricks,
                     int n_views, int width, int height, const float* viewmatrices, const dgr_raycast_params* params, float* depth,
                     float* vnmap, float* color_out, unsigned char* flags) {
    const dgr_raycast_params* p = params;
    const char* bad = tsdf_grid_error(grid);
    if (!bad && !p) bad = "params is NULL";
    if (!bad && (n_views < 1 || n_views > 65535)) bad = "n_views must be at least 1 (and at most 65535)";
    if (!bad && (width < 1 || height < 1 || (long long)width * height > (1ll << 30))) bad = "width and height must be positive (and width * height at most 2^30)";
    if (!bad && !volume) bad = "volume is NULL";
    if (!bad && !viewmatrices) bad = "viewmatrices is NULL";
    if (!bad && !depth && !vnmap && !color_out && !flags) bad = "no output given: depth, vnmap, color_out and flags are all NULL";
    if (!bad && color_out && !color) bad = "color_out asked for of a volume without colour";
    if (!bad && (!aligned_to(volume, 8) || !dgr::aligned16(color))) bad = "volume is not 8-byte aligned or color is not 16-byte aligned";
    if (!bad && !dgr::aligned16(vnmap)) bad = "vnmap is not 16-byte aligned";
    if (!bad && !(aligned_to(viewmatrices, 4) && aligned_to(depth, 4) && aligned_to(color_out, 4))) bad = "viewmatrices, depth or color_out is not 4-byte aligned";
    if (!bad && !(p->fx > 0.0f && p->fy > 0.0f && std::isfinite(p->fx) && std::isfinite(p->fy))) bad = "fx and fy must be finite and positive";
    if (!bad && (!(p->step > 0.0f) || !std::isfinite(p->step))) bad = "step must be finite and positive";
    if (!bad && std::isnan(p->min_weight)) bad = "min_weight is NaN";
    if (!bad && (!std::isfinite(p->depth_min) || std::isnan(p->depth_max))) bad = "depth_min must be finite and depth_max not NaN";
    if (bad) return refuse("dgr_tsdf_raycast", bad);
    dgr::RaycastArgs a{};
    a.nx = grid->nx, a.ny = grid->ny, a.nz = grid->nz;
    a.ox = grid->origin[0], a.oy = grid->origin[1], a.oz = grid->origin[2], a.voxel = grid->voxel_size;
    a.volume = reinterpret_cast<const float2*>(volume), a.color = reinterpret_cast<const float4*>(color), a.bricks = bricks;
    a.V = n_views, a.W = width, a.H = height, a.view = viewmatrices;
    a.fx = p->fx, a.fy = p->fy, a.cx = p->cx, a.cy = p->cy, a.depth_min = p->depth_min, a.depth_max = p->depth_max;
    a.step = p->step, a.min_weight = p->min_weight;
    a.depth = depth, a.vnmap = reinterpret_cast<float4*>(vnmap), a.color_out = color_out, a.flags = flags;
    HIP_TRY(dgr::launch_tsdf_raycast(a, (hipStream_t)stream));
    return DGR_OK;
}

// ---- exact k-nearest-neighbour search (knn.hip)
size_t dgr_knn_index_bytes(int n_points) { return dgr::knn_index_bytes(n_points); }
size_t dgr_knn_scratch_bytes(int n_points, int n_queries) { return dgr::knn_scratch_bytes(n_points, n_queries); }
int dgr_knn_build(void* stream, int n_points, const float* points, void* index, void* scratch) {
    const char* bad = nullptr;
    if (dgr::knn_index_bytes(n_points) == 0) bad = "n_points must be 1 .. 2^24";
    if (!bad && !points) bad = "points is NULL";
    if (!bad && !aligned_to(points, 4)) bad = "points is not 4-byte aligned";
    if (!bad && (!index || !dgr::aligned16(index))) bad = "index is NULL or not 16-byte aligned";
    if (!bad && (!scratch || !dgr::aligned16(scratch))) bad = "scratch is NULL or not 16-byte aligned";
    if (bad) return refuse("dgr_knn_build", bad);
    HIP_TRY(dgr::launch_knn_build(n_points, points, index, scratch, (hipStream_t)stream));
    return DGR_OK;
}
int dgr_knn_search(void* stream, const void* index, int n_points, const float* points, int n_queries, const float* queries,
                   const dgr_knn_params* params, void* scratch, float* dist2, int* idx, int* count, float* mean_dist2) {
    const dgr_knn_params* p = params;
    const char* bad = nullptr;
    if (dgr::knn_index_bytes(n_points) == 0) bad = "n_points must be 1 .. 2^24";
    if (!bad && (n_queries < 1 || n_queries > (1 << 24))) bad = "n_queries must be 1 .. 2^24";
    if (!bad && !p) bad = "params is NULL";
    if (!bad && (p->k < 1 || p->k > DGR_KNN_MAX_K)) bad = "k must be 1 .. 16";
    if (!bad && (std::isnan(p->max_dist2) || p->max_dist2 < 0.0f)) bad = "max_dist2 is NaN or negative";
    if (!bad && queries && p->exclude_self) bad = "exclude_self with queries given: it is defined in self mode only";
    if (!bad && !queries && n_queries != n_points) bad = "n_queries must equal n_points in self mode (queries is NULL)";
    if (!bad && (!index || !dgr::aligned16(index))) bad = "index is NULL or not 16-byte aligned";
    if (!bad && !points) bad = "points is NULL";
    if (!bad && (!scratch || !dgr::aligned16(scratch))) bad = "scratch is NULL or not 16-byte aligned";
    if (!bad && !dist2 && !idx && !count && !mean_dist2) bad = "no output given: dist2, idx, count and mean_dist2 are all NULL";
    if (!bad && !(aligned_to(points, 4) && aligned_to(queries, 4) && aligned_to(dist2, 4) && aligned_to(idx, 4) && aligned_to(count, 4) &&
                  aligned_to(mean_dist2, 4)))
        bad = "points, queries or an output is not 4-byte aligned";
    if (bad) return refuse("dgr_knn_search", bad);
    dgr::KnnSearchCall c{};
    c.index = index, c.n_points = n_points, c.n_queries = n_queries, c.queries = queries;
    c.k = p->k, c.exclude_self = p->exclude_self ? 1 : 0, c.max_dist2 = p->max_dist2, c.scratch = scratch;
    c.dist2 = dist2, c.idx = idx, c.count = count, c.mean_dist2 = mean_dist2;
    HIP_TRY(dgr::launch_knn_search(c, (hipStream_t)stream));
    return DGR_OK;
}

// ---- generalized ICP over the kNN index (gicp.hip)
int dgr_point_covariances(void* stream, int n_points, const float* points, int k, const int* idx,
                          const dgr_covariance_params* params, float* cov, float* normals, float* log_scales, float* quats,
                          unsigned char* flags) {
    const dgr_covariance_params* p = params;
    const char* bad = nullptr;
    if (n_points < 1 || n_points > (1 << 24)) bad = "n_points must be 1 .. 2^24";
    if (!bad && (k < 1 || k > DGR_KNN_MAX_K)) bad = "k must be 1 .. 16";
    if (!bad && !points) bad = "points is NULL";
    if (!bad && !idx) bad = "idx is NULL";
    if (!bad && !p) bad = "params is NULL";
    if (!bad && !cov && !normals && !log_scales && !quats && !flags)
        bad = "no output given: cov, normals, log_scales, quats and flags are all NULL";
    if (!bad && !dgr::aligned16(cov)) bad = "cov is not 16-byte aligned";
    if (!bad && !(aligned_to(points, 4) && aligned_to(idx, 4) && aligned_to(normals, 4) && aligned_to(log_scales, 4) && aligned_to(quats, 4)))
        bad = "points, idx or an output is not 4-byte aligned";
    if (!bad && p->mode != DGR_COV_RAW && p->mode != DGR_COV_PLANE) bad = "unknown mode";
    if (!bad && !(p->epsilon > 0.0f && p->epsilon <= 1.0f)) bad = "epsilon must lie in (0, 1]";
    if (!bad && (p->min_neighbours < 3 || p->min_neighbours > k)) bad = "min_neighbours must be 3 .. k";
    if (!bad && std::isnan(p->scale_floor)) bad = "scale_floor is NaN";
    if (!bad && p->has_viewpoint && (std::isnan(p->viewpoint[0]) || std::isnan(p->viewpoint[1]) || std::isnan(p->viewpoint[2])))
        bad = "viewpoint holds a NaN";
    if (bad) return refuse("dgr_point_covariances", bad);
    dgr::PointCovArgs a{};
    a.P = n_points, a.k = k, a.points = points, a.idx = idx;
    a.mode = p->mode, a.min_neighbours = p->min_neighbours, a.has_viewpoint = p->has_viewpoint ? 1 : 0;
    a.epsilon = p->epsilon, a.scale_floor = p->scale_floor;
    for (int i = 0; i < 3; ++i) a.viewpoint[i] = p->has_viewpoint ? p->viewpoint[i] : 0.0f;
    a.cov = reinterpret_cast<float4*>(cov), a.normals = normals, a.log_scales = log_scales, a.quats = quats, a.flags = flags;
    HIP_TRY(dgr::launch_point_covariances(a, (hipStream_t)stream));
    return DGR_OK;
}
size_t dgr_gicp_scratch_bytes(int n_target, int n_source) { return dgr::gicp_scratch_bytes(n_target, n_source); }
int dgr_gicp_step(void* stream, const void* target_index, int n_target, const float* target, const float* target_cov, int n_source,
                  const float* source, const float* source_cov, const float* transform_in, const dgr_gicp_params* params,
                  void* scratch, float* transform_out, float* quat_out, float* trans_out, double* stats, int* idx_out,
                  unsigned char* flags) {
    const dgr_gicp_params* p = params;
    const char* bad = nullptr;
    if (n_target < 1 || n_target > (1 << 24)) bad = "n_target must be 1 .. 2^24";
    if (!bad && (n_source < 1 || n_source > (1 << 24))) bad = "n_source must be 1 .. 2^24";
    if (!bad && !p) bad = "params is NULL";
    if (!bad && (!target_index || !dgr::aligned16(target_index))) bad = "target_index is NULL or not 16-byte aligned";
    if (!bad && !target) bad = "target is NULL";
    if (!bad && !source) bad = "source is NULL";
    if (!bad && !dgr::aligned16(target_cov)) bad = "target_cov is not 16-byte aligned";
    if (!bad && !dgr::aligned16(source_cov)) bad = "source_cov is not 16-byte aligned";
    if (!bad && !transform_in) bad = "transform_in is NULL";
    if (!bad && (!scratch || !dgr::aligned16(scratch))) bad = "scratch is NULL or not 16-byte aligned";
    if (!bad && !transform_out) bad = "transform_out is NULL";
    if (!bad && (!stats || (reinterpret_cast<uintptr_t>(stats) & 7u))) bad = "stats is NULL or not 8-byte aligned";
    if (!bad && !(aligned_to(target, 4) && aligned_to(source, 4) && aligned_to(transform_in, 4) && aligned_to(transform_out, 4) &&
                  aligned_to(quat_out, 4) && aligned_to(trans_out, 4) && aligned_to(idx_out, 4)))
        bad = "target, source, a transform or an output is not 4-byte aligned";
    if (!bad && !(p->dist_max >= 0.0f)) bad = "dist_max is NaN or negative";
    if (!bad && !(p->huber_delta >= 0.0f)) bad = "huber_delta is NaN or negative";
    if (!bad && !(p->damping >= 0.0f)) bad = "damping is NaN or negative";
    if (!bad && !(p->rcond >= 0.0f)) bad = "rcond is NaN or negative";
    if (!bad && p->min_points < 1) bad = "min_points must be at least 1";
    if (bad) return refuse("dgr_gicp_step", bad);
    dgr::GicpStepArgs a{};
    a.N = n_target, a.S = n_source, a.target = target, a.source = source;
    a.target_cov = reinterpret_cast<const float4*>(target_cov), a.source_cov = reinterpret_cast<const float4*>(source_cov);
    a.transform_in = transform_in, a.huber_delta = p->huber_delta, a.damping = (double)p->damping, a.rcond = (double)p->rcond;
    a.min_points = p->min_points;
    a.transform_out = transform_out, a.quat_out = quat_out, a.trans_out = trans_out, a.stats = stats, a.flags = flags;
    HIP_TRY(dgr::launch_gicp_step(a, target_index, p->dist_max, idx_out, scratch, (hipStream_t)stream));
    return DGR_OK;
}

}  // extern "C"
