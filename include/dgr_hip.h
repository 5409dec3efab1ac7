/* dgr_hip.h -- C ABI of the MI355X (gfx950) differentiable Gaussian rasterizer.
 *
 * This is the drop-in boundary for the reference's hot path.  Each entry point replaces one
 * member of `CudaRasterizer::Rasterizer` (the raw-pointer layer the reference's torch binding
 * calls) and keeps its argument order and meaning; what changes is stated per function.
 * Reference paths: L = diff-gaussian-rasterization-light, F = diff-gaussian-rasterization-full.
 *
 * Conventions
 *  - every `float*` / `int*` / `char*` argument is a DEVICE pointer unless marked "host";
 *    optional inputs are NULL exactly where the reference passes nullptr (empty tensors);
 *  - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream the reference uses);
 *  - 4x4 matrices are 16 floats read column-major: x' = m[0]x + m[4]y + m[8]z + m[12]
 *    (cuda_rasterizer/auxiliary.h:58-77);
 *  - the three state buffers (geometry / binning / image) are opaque to the caller, as in the
 *    reference (L/cuda_rasterizer/rasterizer_impl.h:29-64); their layout here is different and
 *    documented in DESIGN.md;
 *  - return value: >= 0 success (forward: num_rendered), < 0 one of DGR_ERR_*.
 */
#ifndef DGR_HIP_H
#define DGR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGR_OK 0
#define DGR_ERR_BAD_ARGUMENT (-1)       /* e.g. non-RGB without precomputed colours (L/cr/rasterizer_impl.cu:248-251) */
#define DGR_ERR_PREFILTERED (-2)        /* a point was culled although `prefiltered` is set (cr/auxiliary.h:154-161: __trap there) */
#define DGR_ERR_BINNING_OVERFLOW (-3)   /* presized binning buffer too small; *num_rendered holds the required count */
#define DGR_ERR_HIP (-4)                /* a HIP runtime call failed; see dgr_last_error() */
#define DGR_ERR_ALLOC (-5)              /* an allocation callback returned NULL */

/* Replaces std::function<char*(size_t)> (L/cr/rasterizer.h:41-43, L/rasterize_points.cu:27-33):
 * called with the number of bytes needed, returns a device pointer (>= 256-byte aligned). */
typedef char* (*dgr_alloc_fn)(size_t bytes, void* user);

/* Human-readable text of the last DGR_ERR_HIP on this thread (host string, never NULL). */
const char* dgr_last_error(void);

/* Version / target string of the built library, e.g. "dgr_hip 0.1 gfx950". */
const char* dgr_version(void);

/* ---- state buffer sizes (the reference's `required<T>(n)`, L/cr/rasterizer_impl.h:66-72) ---- */
size_t dgr_geometry_bytes(int P);
size_t dgr_image_bytes(int width, int height);
/* 24 bytes per instance of capacity (sorted list, key scratch, arrival ranks / pair columns, pair keys) plus the segment
 * binning's forward-only tables (csrc/segment_binning.hip: 2 KB per 16-tile row segment), i.e. NON-ZERO for a capacity of 0:
 * the presized entry points need a binning buffer of this size for every P > 0 and reject NULL. */
size_t dgr_binning_bytes(int num_rendered_capacity, int width, int height);
/* scratch the backward needs (per-Gaussian accumulator rows + reduction partials) */
size_t dgr_light_backward_scratch_bytes(int P, int width, int height);
/* ... with the option "deterministic_grads" on: the scratch also holds the instance-major row buffer, 64 bytes per tile
 * instance -- R = the value the backward will be given as `R`, at least the forward's num_rendered (a lazy caller passes its
 * binning capacity).  Equals dgr_light_backward_scratch_bytes(P, W, H) while the option is off. */
size_t dgr_light_backward_scratch_bytes_r(int P, int W, int H, int R);

/* Replaces CudaRasterizer::Rasterizer::markVisible (L/cr/rasterizer.h:33-38,
 * L/cr/rasterizer_impl.cu:54-66,141-153).  present[i] = (view * p_i).z > 0.2.  `present` is P bytes (bool). */
int dgr_mark_visible(void* stream, int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present);

/* Replaces CudaRasterizer::Rasterizer::forward of the light variant (L/cr/rasterizer.h:40-70,
 * L/cr/rasterizer_impl.cu:197-350).  Same arguments in the same order, with `stream` prepended and
 * the three std::function allocators replaced by C callbacks sharing one `alloc_user`.
 * Like the reference it blocks the host once (to size the binning buffer) and returns num_rendered.
 * Outputs need NOT be zero-initialised (the reference's binding zero-fills them first,
 * L/rasterize_points.cu:69-76; here every element is written).  `out_depth_var` is written as 0
 * (L/cr/forward.cu:317,410).  `radii` may be NULL (L/cr/rasterizer_impl.cu:235-238).
 * SH layout, here and in every entry point that takes (D, M, shs): `shs` is [P, M, 3] with any M >= 1 and any alignment; D = 0 .. 3
 * (else DGR_ERR_BAD_ARGUMENT); coefficients beyond M count as zero; dL_dsh is [P, M, 3] and coefficients beyond 16 get zero gradient.
 * (The map steps below refuse a tensor with k < 1 values per row: dgr_amd.map_steps hands them no leaf of zero width, which is legal there.) */
int dgr_light_forward(void* stream, dgr_alloc_fn geometryBuffer, dgr_alloc_fn binningBuffer, dgr_alloc_fn imageBuffer,
                      void* alloc_user, int P, int D, int M, const float* background, int width, int height,
                      const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                      const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                      const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                      float tan_fovy, int prefiltered, float* out_color, float* out_depth, float* out_median_depth,
                      float* out_alpha, const float* gt_depth, float* out_depth_var, float* gau_uncertainty,
                      int* gau_related_pixels, int* radii, int debug);

/* Same computation with caller-provided state buffers and NO host synchronisation (hipGraph-capturable):
 * `binning_buffer` holds at most `binning_capacity` instances.  `status` is a device int[4] written by the
 * kernels: {num_rendered, overflow flag, prefiltered-violation flag, reserved}.  When the capacity is too
 * small the blend kernels see empty tile lists and the caller must re-run with a larger buffer. */
int dgr_light_forward_presized(void* stream, char* geometry_buffer, char* binning_buffer, int binning_capacity,
                               char* image_buffer, int* status, int P, int D, int M, const float* background,
                               int width, int height, const float* means3D, const float* shs,
                               const float* colors_precomp, const float* opacities, const float* scales,
                               float scale_modifier, const float* rotations, const float* cov3D_precomp,
                               const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                               float tan_fovx, float tan_fovy, int prefiltered, float* out_color, float* out_depth,
                               float* out_median_depth, float* out_alpha, const float* gt_depth,
                               float* out_depth_var, float* gau_uncertainty, int* gau_related_pixels, int* radii);

/* Replaces CudaRasterizer::Rasterizer::backward of the light variant (L/cr/rasterizer.h:72-104,
 * L/cr/rasterizer_impl.cu:354-495).  Same arguments in the same order with `stream` prepended and a
 * scratch buffer appended.  Differences, all on buffers the reference's Python never sees:
 *  - `dL_dview` receives the 16 reduced entries (entries 3,7,11,15 = 0), i.e. what
 *    L/diff_gaussian_rasterization/__init__.py:160-161 obtains by summing the reference's [H*W,4,4] buffer;
 *  - `dgndcs_dviewmatrix` / `dg_camd_dviewmatrix` (per-Gaussian pose Jacobians, L/cr/backward.cu:701-751)
 *    are not materialised and may be NULL;
 *  - `dL_dconic` ([P,2,2]) and `dL_ddepth` ([P,1]) may be NULL; when given they receive the same sums
 *    the reference accumulates there;
 *  - gradient outputs need not be zero-initialised: rows of invisible Gaussians are written as 0;
 *  - every per-Gaussian gradient output may be NULL and is then not written.  A tracking step (only `viewmatrix` requires
 *    a gradient) passes them all as NULL together with map_off = 1: the backward then forms the pose gradient alone and
 *    moves no dense per-Gaussian rows (248 bytes per Gaussian at SH degree 3);
 *  - `dL_dpix_median_depth` and `dL_dpix_depth_var` may each be NULL (the loss did not use that output: an all-zero image).
 *    With both NULL the blend backward runs a leaner kernel -- no variance term, no median test: 8 % fewer issue cycles per
 *    list entry, bit-identical to all-zero images -- which is what the compiled autograd node passes when autograd hands it
 *    no gradient for those outputs (CG-SLAM's losses use neither: depth_var is identically zero, L/cr/forward.cu:317,410).
 * `R` is the value forward returned; `radii` may be NULL (internal copy is used).
 * The forward does not keep the 3D covariance: unless `cov3D_precomp` is given, `scales`, `rotations` and `scale_modifier`
 * must be the forward's (the backward re-forms the covariance from them, same expression, same bits) and may not be NULL
 * (DGR_ERR_BAD_ARGUMENT); likewise the three state buffers. */
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
                       const float* gt_depth, int track_off, int map_off, char* scratch, size_t scratch_bytes);

/* Resident scratch.  dgr_light_backward / dgr_full_backward clear `scratch` with one launch before the blend backward.  A caller
 * that keeps a scratch buffer across calls (one per stream: calls that share one must be ordered on a stream) can skip that launch:
 * after dgr_backward_scratch_clean_arm() the NEXT backward call of this thread takes `scratch` as ALL ZERO on entry and leaves it
 * all zero when its kernels have completed -- the per-Gaussian kernel clears every accumulator row it reads, the block that
 * finishes the pose sum clears the partials.  Start from a zero-filled buffer; after a call that returned an error, zero it again. */
int dgr_backward_scratch_clean_arm(void);

/* ---- -full variant -------------------------------------------------------------------------------
 * Replaces CudaRasterizer::Rasterizer::forward of the full variant (F/cr/rasterizer.h:31-62,
 * F/cr/rasterizer_impl.cu:349-500): returns num_rendered; the tuple's second member (num_related_primitives,
 * the total of n_valid_contrib) is written to *num_related_primitives (host int, may be NULL to skip the second
 * blocking read).  `out_uncertainty` is sum alpha*T (F/cr/forward.cu:367,394); gt_depth is accepted and unused in
 * the forward, as there (quirk F6). */
int dgr_full_forward(void* stream, dgr_alloc_fn geometryBuffer, dgr_alloc_fn binningBuffer, dgr_alloc_fn imageBuffer,
                     void* alloc_user, int P, int D, int M, const float* background, int width, int height,
                     const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                     const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                     const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                     float tan_fovy, int prefiltered, float* out_color, float* out_depth, const float* gt_depth,
                     float* out_uncertainty, int* radii, int* num_related_primitives);

/* No-sync form; status = device int[4] {num_rendered, overflow, prefiltered violation, num_related_primitives}. */
int dgr_full_forward_presized(void* stream, char* geometry_buffer, char* binning_buffer, int binning_capacity,
                              char* image_buffer, int* status, int P, int D, int M, const float* background, int width,
                              int height, const float* means3D, const float* shs, const float* colors_precomp,
                              const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                              const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                              const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                              float* out_depth, const float* gt_depth, float* out_uncertainty, int* radii);

/* Replaces CudaRasterizer::Rasterizer::backward of the full variant (F/cr/rasterizer.h:64-102,
 * F/cr/rasterizer_impl.cu:504-666), same arguments in the same order (+ stream, + scratch).  The NG-sized pair
 * lists (dpixel_dgc, gau_id_list, pix_id_list, dpixel_dndcs, dpixel_dinvcovs, ddepth_dndcs, ddepth_dinvcovs) and
 * the per-Gaussian Jacobian tables (dgc_dCam_position, dgndcs_dviewmatrix, dgc_invcovs_dT) are implementation
 * scratch of the reference; they are not materialised here and may be NULL.  dL_dview receives the 4x4 gradient
 * with the well-defined semantics of ComputePG: every recorded (pixel, Gaussian) pair is consumed.  (The reference
 * lets threads of pixels without a valid contributor return before the block-wide loads, F/cr/backward.cu:875-878,
 * 935-938, which makes its own result undefined for the other pixels of such a tile; DESIGN.md "full variant".)
 * dL_duncertainties may be NULL (the loss did not use the uncertainty output): it reads as zero, and the blend backward
 * drops the variance recurrence (bit-identical to an all-zero image).  R: as in dgr_light_backward; read only with
 * "deterministic_grads", where it sizes the instance-major row buffer (scratch: dgr_light_backward_scratch_bytes_r). */
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
                      size_t scratch_bytes);

/* ---- stage-wise access for tests and profiling (views into the opaque state buffers) ---- */
/* Copies one named array of a state buffer to `dst` (device or host pointer).  Names: "depths", "radii",
 * "means2D", "conic_opacity", "rgb", "clamped", "tiles_touched" (geometry); "point_list", "keys" (binning); "contribution_tags"
 * (one byte per list entry, bit w = some pixel of quadrant w of the tile blended it: the forward blend's tag bytes folded),
 * "half_tags" (those bytes as they are: bit 2 w + h = half h of quadrant w); "live_list" (light variant: two words per instance
 * slot, {Gaussian id, list position << 8 | tag byte} -- the entries the forward blended, compacted per tile from the tile's range
 * start on) with "live_counts" (image: one word per tile, how many of them the tile has).  LIMIT (light variant): a live entry
 * keeps its list position in 24 bits, so ONE tile's list must stay below 2^24 = 16 777 216 entries (16.7 M Gaussians reaching
 * the same 16x16 tile; config 5's whole frame has 16.4 M instances over 32 400 tiles).  It is not checked: beyond it the
 * light backward's gradients for that tile are wrong;
 * "ranges", "tile_sched", "sched_flag" (one word, the frame's blend flags: bit 0 = its blend kernels use the schedule, bit 1 = the
 * binning buffer overflowed, bit 2 = quadrant lane lists: option "lane_lists"), "n_contrib", "n_valid",
 * "first_contrib" (uint32 per pixel: the 1-based list position of the pixel's front-most valid Gaussian, 0 = none),
 * "final_T" (image; the last three: full variant).  Layout conversion to the reference's element types is done on the fly.
 * `num_rendered` instances are exported; `binning_capacity` is the capacity the binning buffer was carved with
 * (= num_rendered after dgr_*_forward, the caller's capacity after *_presized).  Returns the element count, or < 0. */
long dgr_state_export(void* stream, const char* name, int P, int width, int height, int num_rendered,
                      int binning_capacity, const char* geom_buffer, const char* binning_buffer,
                      const char* image_buffer, void* dst_device);

/* Early status.  The reference blocks the host once per forward to read num_rendered (L/cr/rasterizer_impl.cu:287).  That
 * number and the prefiltered-violation flag are final after the per-block scan, about a tenth of the way into the forward:
 * dgr_early_status_arm() makes the NEXT *_forward_presized call of this thread copy the status word to pinned host memory
 * at that point, and dgr_early_status_wait() blocks until that copy -- not the rest of the forward -- has completed and
 * returns {num_rendered, 0, prefiltered violation, 0} (the overflow flag is the caller's own num_rendered > capacity).
 * Returns 1 when nothing was posted (P == 0). */
/* Asynchronous read-back of a device status word (the bindings' lazy mode): dgr_status_post enqueues a copy of
 * device_status[0..3] to pinned host memory behind an event on `stream` and returns a ticket (>= 0) or an error code;
 * dgr_status_poll returns 1 and fills host_status4 once the copy has landed (the ticket is then released), 0 when
 * `wait` == 0 and it has not yet.  dgr_stream_is_capturing: 1 while `stream` records a hipGraph (nothing can be read
 * back then). */
long dgr_status_post(void* stream, const int* device_status);
int dgr_status_poll(long ticket, int wait, int* host_status4);
/* The same read-back without the copy and the event: dgr_status_arm() returns a ticket and hands its slot to the NEXT
 * *_forward_presized call of this thread (whichever stream it runs on).  That forward's blend kernel (its first workgroup, before anything else) writes {num_rendered,
 * overflow, prefiltered violation, 0} straight into the slot's pinned host memory (mapped into the device's address space),
 * a tag last; dgr_status_poll on the ticket then reads host memory -- no HIP call unless it has to wait.  num_related_primitives
 * (full variant; completed by the forward blend, later than the rest) is NOT reported this way: read the device word when it
 * is needed.  A forward that enqueues no binning kernel (P == 0, an argument error) completes the word itself, all zero.  The
 * armed forward also reports its longest tile list, which feeds the "tile_schedule" policy below.  Not while `stream` records
 * a hipGraph (nothing can be read back then: do not arm).
 * A blocking poll (wait != 0) of an armed ticket cannot spin for ever: every millisecond it asks the forward's stream -- a HIP
 * error there ends the wait with DGR_ERR_HIP, and so does a stream that has finished all its work without the word having
 * arrived (a forward issued into a capturing stream, a faulted kernel) -- and it gives up after DGR_STATUS_TIMEOUT_MS
 * (environment, default 30 000; 0 = no limit: profiler replays and a collective's stragglers can hold a queue for longer).  The
 * stream is not asked while it records a hipGraph (a query would invalidate the capture).  The ticket is released on every such
 * return; after a timeout or a stream error its slot stays out of use until that stream has drained (the forward may still be
 * queued and would write into a slot that had been handed to another forward meanwhile). */
long dgr_status_arm(void);
int dgr_stream_is_capturing(void* stream);
int dgr_early_status_arm(void);
int dgr_early_status_wait(int* host_status4);

/* Fused sparse Adam step on one per-Gaussian tensor [rows, k] (the reference leaves the optimiser
 * to torch).  torch.optim.Adam's update (no weight decay, no amsgrad) with bias correction for the 1-based `step`;
 * rows with visible[row] <= 0 are skipped -- parameter and both moments untouched, as in 3DGS's sparse Adam -- and
 * `visible` == NULL updates every row.  `visible` is typically the forward's `radii`. */
int dgr_sparse_adam(void* stream, long rows, int k, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                    const int* visible, float lr, float beta1, float beta2, float eps, int step);
/* The same with the 1-based step count read from device memory when the kernel runs, so that a step recorded into a
 * hipGraph keeps its bias correction right on every replay (the caller increments *step_device before, on the stream). */
int dgr_sparse_adam_capturable(void* stream, long rows, int k, float* param, const float* grad, float* exp_avg,
                               float* exp_avg_sq, const int* visible, float lr, float beta1, float beta2, float eps,
                               const int* step_device);

/* Densification bookkeeping for the rows one view saw (radii[row] > 0), as 3DGS's GaussianModel.add_densification_stats
 * and the training loop's max_radii2D update do with indexed torch ops (the reference's caller; the rasterizer only
 * hands back dL_dmeans2D for this purpose, diff_gaussian_rasterization/__init__.py L:164-176):
 *   grad_accum[row] += |dmeans2D[row, 0:2]|;  denom[row] += 1;  max_radii2D[row] = max(max_radii2D[row], radii[row]).
 * dmeans2D is [rows, 3]; each of the three outputs ([rows] floats) may be NULL to skip it. */
int dgr_densification_stats(void* stream, long rows, const float* dmeans2D, const int* radii, float* grad_accum, float* denom,
                            float* max_radii2D);

/* Fused densify-and-prune: 3DGS's densify_and_clone, densify_and_split and prune_points over every per-Gaussian tensor of
 * the model, in three launches (csrc/optim.hip).  All decisions are fp32 comparisons on the raw values against thresholds
 * the caller forms (in float64, rounded once), so that a restatement with plain tensor comparisons takes the same ones:
 *   hot   = denom > 0 && grad_accum >= grad_threshold * denom      (one rounded fp32 multiply; a NaN is not hot)
 *   m     = max_k scaling_raw[row, k];   split = hot && m > log_scale_split;   clone = hot && !split
 * The result is that of: append a copy of every clone row (row order); append the children of every split row (sample 0 of
 * all split rows, then sample 1), child xyz = xyz + R(q / |q|) (exp(scaling_raw) * n), child scaling_raw = scaling_raw -
 * logf(1.6f) (one fp32 subtraction of 0x1.e148a2p-2f), everything else the parent's; remove the split originals; then prune
 * every row, new ones included, with opacity_raw < opacity_raw_min, or max_radii2D > max_screen_size (new rows carry 0), or
 * its own max_k scaling_raw > log_scale_prune.  Pass +inf for the last two thresholds to switch those rules off.
 * Output order: surviving originals, clones, children of sample 0, children of sample 1, each in original row order; no
 * atomic decides a position, so the result is the same bits on every run.
 *
 * dgr_densify_plan decides (one action per row) into `plan`, an opaque 16-byte aligned device buffer of
 * dgr_densify_plan_bytes(rows) bytes, and writes counts8_device[0..7] (device memory) = {rows after the step, surviving
 * originals, clones kept, children kept, rows split, 0, 0, 0}.  The caller reads counts[0], allocates, and calls
 * dgr_densify_apply with rows_out = counts[0] and a table of 1 .. DGR_DENSIFY_MAX_TENSORS tensors {src [rows, k], dst
 * [rows_out, k]}: ONE launch moves them all (call it again with the same plan for more tensors).  Modes: COPY (every emitted
 * row takes its source row), ZERO_NEW (Adam moments: survivors copied, new rows zero), ZERO (accumulators: dst zeroed, src
 * unused), XYZ (k = 3, at most one: children displaced as above), LOG_SCALE (children shifted by -logf(1.6f)).
 * `noise`: [rows, 2, 3] standard normals indexed by the ORIGINAL row (sample, component), or NULL: the kernel then draws
 * them with Philox4x32-10 keyed by `seed` with the counter (row, sample) and Box-Muller -- the values do not depend on the
 * grid or on which other rows split.  scaling_raw [rows, 3] / rotation_raw [rows, 4] (r, x, y, z; not unit) are read by XYZ.
 * rows == 0 succeeds (zero counts).  Argument errors are reported before any HIP call.  Not capturable as a whole: the
 * caller reads counts between the two calls. */
#define DGR_DENSIFY_MAX_TENSORS 24
#define DGR_DENSIFY_COPY 0
#define DGR_DENSIFY_ZERO_NEW 1
#define DGR_DENSIFY_ZERO 2
#define DGR_DENSIFY_XYZ 3
#define DGR_DENSIFY_LOG_SCALE 4
typedef struct {
    const float* src;
    float* dst;
    int k;
    int mode;
} dgr_densify_tensor;
size_t dgr_densify_plan_bytes(long rows);
int dgr_densify_plan(void* stream, long rows, const float* grad_accum, const float* denom, const float* max_radii2D /* or NULL */,
                     const float* opacity_raw, const float* scaling_raw, float grad_threshold, float opacity_raw_min,
                     float log_scale_split, float log_scale_prune, float max_screen_size, void* plan, int* counts8_device);
int dgr_densify_apply(void* stream, long rows, long rows_out, const void* plan, int n, const dgr_densify_tensor* tensors,
                      const float* scaling_raw, const float* rotation_raw, const float* noise /* or NULL */,
                      unsigned long long seed);

/* Fixed-size map upkeep: 3DGS-MCMC's relocation of dead Gaussians and its position noise (Kheradmand et al., NeurIPS 2024), in
 * place (csrc/relocate.hip).  Neither changes the number of rows P: no tensor is reallocated and nothing is read on the host, so
 * both can be recorded into a hipGraph.  Raw leaves as above: opacity_raw a logit, scaling_raw the log of the scale.
 *
 * Relocation.  thr = opacity_raw_min (the caller's logit(min_opacity), formed in float64 and rounded once).
 *   dead   = opacity_raw < thr (an fp32 comparison, false on a NaN), and opacity_raw finite;
 *   live   = opacity_raw finite and not dead, with the integer weight w = rint(2^20 o), o = 1 / (1 + exp(-opacity_raw)) in
 *            float64; a row whose opacity_raw is not finite is neither: weight 0, never read, never written;
 *   S      = sum of w (exact, 64-bit; below 2^48 for P <= 2^28), C_i = the exclusive prefix of w in row order;
 *   draw   = every dead row r owns one 32-bit draw d_r: draws[r] (int64 [P], values 0 .. 2^32 - 1) or, with draws == NULL, word 0
 *            of Philox4x32-10 under key `seed` with the counter (r, step, 1); its target is t_r = (d_r S) >> 32 (exact) and its
 *            source the live row i with C_i <= t_r < C_i + w_i.  Integer arithmetic only: the result does not depend on the grid
 *            or the launch order.  With S == 0 nothing is relocated;
 *   hits_i = how many dead rows drew i (an integer atomic), N_i = min(hits_i + 1, 51).
 * For a source with hits_i > 0, in float64: o' = 1 - (1 - o)^(1 / N); D = sum_{m=1..N} sum_{k=0..m-1} C(m-1, k) (-1)^k
 * (k + 1)^(-1/2) o'^(k+1); coeff = o / D; o' is then clamped to [min_opacity, 1 - 2^-23].  The new raw opacity is log(o' / (1 -
 * o')) and the new raw scale scaling_raw + log(coeff) per component, each rounded once to fp32: the N copies together render what
 * the one did.  (fp32 loses up to 1.9e-4 relative here, to the cancellation in 1 - (1 - o)^(1/N).)
 * Writes, all in place: a relocated row takes every tensor of its source bit for bit (COPY), the source's NEW opacity (OPACITY) and
 * scale (LOG_SCALE); the source takes the same new opacity and scale; ZERO_TOUCHED tensors (the Adam moments: a stale moment belongs
 * to neither the old place nor the new shape) become 0 at relocated rows and hit sources, ZERO_RELOCATED ones (the densification
 * accumulators) at relocated rows only.  Every other row keeps its bits in every tensor.
 *
 * dgr_relocate_plan (four launches: weights and block totals, a one-workgroup scan, the draws, the hit sources' new values) fills
 * `scratch`, an opaque 16-byte aligned device buffer of dgr_relocate_scratch_bytes(P) bytes (0 for a P it refuses), and writes
 * counts8_device[0..7] = {dead, live, relocated, sources hit, largest hits, 0, 0, 0} and source[P] (the source row of a relocated
 * row, -1 elsewhere), both device memory.  `step` is read from *step_device when that is not NULL (a recorded graph then draws
 * fresh numbers on every replay).  dgr_relocate_apply then rewrites a table of 1 .. DGR_RELOCATE_MAX_TENSORS tensors {data [P, k]}
 * in two launches -- the relocated rows, which only read live rows and only write dead ones, then the sources -- from the values
 * the plan saved, so that no row is read while it is rewritten; call it again with the same scratch for more tensors.  The plan
 * belongs to the opacity it was made from: an OPACITY tensor must be `opacity_raw` (k = 1, at most one), a LOG_SCALE tensor
 * `scaling_raw` (at most one).  Argument errors are reported before any HIP call. */
#define DGR_RELOCATE_MAX_TENSORS 24
#define DGR_RELOCATE_COPY 0
#define DGR_RELOCATE_OPACITY 1
#define DGR_RELOCATE_LOG_SCALE 2
#define DGR_RELOCATE_ZERO_TOUCHED 3
#define DGR_RELOCATE_ZERO_RELOCATED 4
typedef struct {
    float* data;
    int k;
    int mode;
} dgr_relocate_tensor;
size_t dgr_relocate_scratch_bytes(long P);
int dgr_relocate_plan(void* stream, long P, const float* opacity_raw, float opacity_raw_min, const long long* draws /* or NULL */,
                      unsigned long long seed, int step, const int* step_device /* or NULL */, void* scratch, int* counts8_device,
                      int* source);
int dgr_relocate_apply(void* stream, long P, const void* scratch, int n, const dgr_relocate_tensor* tensors, float* scaling_raw,
                       float* opacity_raw, double min_opacity);
/* Position noise (SGLD), one launch, fp32, in place: xyz_c += g sum_j Sigma_cj n_j with Sigma = R S^2 R^T from the normalised
 * quaternion rotation [P, 4] (r, x, y, z) and S = diag(exp(scaling_raw)); g = scale lr / (1 + exp(-k (1 - o - x0))), o =
 * sigmoid(opacity_raw): the gate opens for the near-transparent rows only (3DGS-MCMC: scale 5e5, k 100, x0 0.995).  `noise`: [P,
 * 3] standard normals, or NULL: Philox normals (Box-Muller) under key `seed` with the counter (row, step, 0), components 0 .. 2.
 * `step` / `lr` are read from *step_device / *lr_device when those are not NULL. */
int dgr_position_noise(void* stream, long P, float* xyz, const float* scaling_raw, const float* rotation, const float* opacity_raw,
                       const float* noise /* or NULL */, unsigned long long seed, int step, const int* step_device /* or NULL */,
                       float lr, const float* lr_device /* or NULL */, float scale, float k, float x0);

/* Map correction after a pose-graph update (loop closure, global bundle adjustment): every Gaussian moves with the keyframe it was
 * created from, by that keyframe's Sim(3) transform (csrc/transform.hip).  In place on P rows, no host read and no allocation: the
 * step can be recorded into a hipGraph, and `transforms` is read when the graph is replayed.
 * transforms [K, 4, 4]: float32 on the device, row-major, old world coordinates -> new ones; of transform k, A is the upper-left
 * 3 x 3 block and t the translation column (the bottom row is only tested for being finite).  anchor [P]: float32 on the device,
 * the transform of each row (what seed_from_frame's `fill` wrote and the other steps copied), or NULL: every row takes transform 0.
 *
 * Plan, per transform, in float64, each result rounded once to fp32: s = cbrt(det A); q_R = (r, x, y, z), the unit quaternion of
 * A / s (Shepperd: the largest of the trace and the diagonal entries picks the branch; then normalised; the sign is the branch's);
 * R, the rotation matrix of q_R; 1 / s, 1 / s^2, log s; and M_1 (3 x 3), M_2 (5 x 5), M_3 (7 x 7) with B_l(R d) = M_l B_l(d) for
 * every unit d, B_l being the band-l spherical-harmonic basis as csrc/gaussian_math.h evaluates it (SH_C1, SH_C2[], SH_C3[] as
 * fp32 constants, its signs, its order): coefficients rotate as c'_l = M_l c_l per colour channel.  M_l is formed as
 * Y_l(R d) Y_l^-1 over 2 l + 1 fixed directions (csrc/sh_rotation_table.h).  A transform is INVALID, and its rows are left
 * untouched, when one of its 16 values is not finite, det A <= 0, or max |A^T A / s^2 - I| > 1e-3.
 *
 * Apply.  Row i is transformed when its anchor a is an integer value with 0 <= a < K and transform a is valid; every other row (a
 * NaN, negative, fractional or too large anchor, an invalid transform) keeps its bits in every tensor, and nothing is read out of
 * range.  Each tensor {data [P, k], mode, skip} has mode = kind + order, fp32 arithmetic on the records:
 *   XYZ (k = 3)        VALUE x' = A x + t;  MOMENT1 m' = (R m) / s (a gradient is a covector: the inverse transpose of the value's
 *                      linear part);  MOMENT2 v'_i = (sum_j R_ij^2 v_j) / s^2 (the diagonal of the rotated second moment without
 *                      the cross terms Adam never tracked; it stays >= 0)
 *   QUAT (k = 4)       VALUE q' = q_R (x) q (Hamilton product; the row's norm is kept, its sign not canonicalised);  MOMENT1 L(q_R) m
 *                      with L the (orthogonal) 4 x 4 matrix of the left multiplication;  MOMENT2 (L o L) v, o the element-wise product
 *   LOG_SCALE (k = 3)  VALUE only: + log s per component (a shift leaves the gradients alone: the moments are not in the table)
 *   SH                 skip = 0: an f_rest leaf [P, M, 3] (k = 3 M), skip = 3: a combined shs leaf [P, M + 1, 3] (k = 3 M + 3) whose
 *                      DC row is left alone; M = 3, 8 or 15, coefficient-major, channel-minor.  VALUE and MOMENT1: c'_l = M_l c_l per
 *                      complete band and channel;  MOMENT2: (M_l o M_l)
 * Opacity, the DC colour, leaves without a role and the densification accumulators are invariant: they are not in the table.
 * counts4_device [4] int32 = {rows transformed, rows whose anchor names no transform, invalid transforms, rows anchored to an
 * invalid transform}: dgr_transform_plan writes {0, 0, invalid, 0}; every dgr_transform_apply rewrites all four (so a second apply
 * call with the same scratch for more tensors leaves the same counts).
 *
 * dgr_transform_plan (the transforms' launch and a one-workgroup count) fills `scratch`, an opaque 16-byte aligned device buffer of
 * dgr_transform_scratch_bytes(K) bytes (0 for a refused K: K must be 1 .. 2^20).  dgr_transform_apply: the count's reset and one
 * launch over 1 .. DGR_TRANSFORM_MAX_TENSORS tensors.  At most one XYZ, one QUAT and one LOG_SCALE VALUE tensor per call.  Argument
 * errors are reported before any HIP call. */
#define DGR_TRANSFORM_MAX_TENSORS 24
#define DGR_TRANSFORM_VALUE 0
#define DGR_TRANSFORM_MOMENT1 1
#define DGR_TRANSFORM_MOMENT2 2
#define DGR_TRANSFORM_XYZ 0
#define DGR_TRANSFORM_QUAT 4
#define DGR_TRANSFORM_LOG_SCALE 8
#define DGR_TRANSFORM_SH 12
typedef struct {
    float* data;
    int k;
    int mode; /* DGR_TRANSFORM_<kind> + DGR_TRANSFORM_<order> */
    int skip; /* SH: 0 or 3 leading values of each row that stay; 0 for the other kinds */
} dgr_transform_tensor;
size_t dgr_transform_scratch_bytes(long K);
int dgr_transform_plan(void* stream, long K, const float* transforms, void* scratch, int* counts4_device);
int dgr_transform_apply(void* stream, long P, long K, const void* scratch, const float* anchor /* or NULL */, int n,
                        const dgr_transform_tensor* tensors, int* counts4_device);

/* Fused map expansion: new Gaussians from an RGB-D keyframe, appended to every per-Gaussian tensor of the model in three
 * launches (csrc/seed.hip) -- what an RGB-D SLAM system (CG-SLAM, SplaTAM, MonoGS) does when a keyframe arrives: unproject the
 * pixels the current map does not explain.  The sibling of densify-and-prune above: decide, scan, one host read, one apply.
 * Images are float32 on the device: color_obs [3, H, W], depth_obs [H, W], and the optional opacity_map [H, W] (the forward's
 * silhouette) and depth [H, W] (the rendered depth).  viewmatrix: 16 floats on the device holding W2C^T, what the rasterizer
 * takes and dgr_pose_forward writes; the pose is taken as rigid.  fx, fy, cx, cy: pixels, in the convention in which a point on
 * the optical axis lands on pixel (cx, cy) under ndc2Pix: pixel (x, y) at depth d is the camera-space point
 * p = ((x - cx) / fx * d, (y - cy) / fy * d, d).
 * Candidates: the pixels with x % stride == 0 && y % stride == 0.  Every decision is an fp32 comparison on the raw values
 * against thresholds the caller forms (in float64, rounded once); a NaN compares false:
 *   valid   = depth_obs > depth_min && depth_obs < depth_max
 *   unseen  = opacity_map given && opacity_map < silhouette_threshold
 *   infront = depth given && depth > depth_obs && (depth - depth_obs) > depth_error_min     (one rounded fp32 subtraction)
 *   select  = valid && (unseen || infront);   select = valid when neither image is given (the first frame)
 * depth_error_min_device (one float on the device, or NULL) overrides depth_error_min when non-NULL, so that a caller's
 * k * median(error) needs no host read.
 * The result is the old `rows` rows unchanged, followed by one new row per selected pixel in row-major pixel order (y, then x);
 * no atomic decides a position, so the result is the same bits on every run.
 *
 * dgr_seed_plan decides (one flag byte per candidate) into `plan`, an opaque 16-byte aligned device buffer of
 * dgr_seed_plan_bytes(width, height, stride) bytes (0 for a shape it refuses: a non-positive dimension or stride, 2^30
 * candidates or more), and writes counts8_device[0..7] (device memory) = {rows after the step, new rows, valid candidates,
 * valid candidates that are unseen, valid candidates that are in front, 0, 0, 0}.  The caller reads counts[0], allocates, and
 * calls dgr_seed_apply with rows_out = counts[0] and a table of 1 .. DGR_SEED_MAX_TENSORS tensors {src [rows, k], dst
 * [rows_out, k], mode, value}: ONE launch copies the old rows of them all and writes their new rows (call it again with the same
 * plan for more tensors).  src may be NULL only when rows == 0.  Nothing is written past rows_out.  What `mode` puts into a new
 * row:
 *   XYZ (k = 3, at most one per table): p taken to the world, world_i = sum_j view[i][j] (p_j - view[3][j]), view[i][j] =
 *     viewmatrix[4 i + j], in fp32 (fused multiply-adds allowed);
 *   LOG_SCALE (k = 3 or 1): every component logf(d * pix), d = depth_obs, one rounded fp32 multiply and the full-precision logf;
 *     the caller forms pix = scale_factor * stride * 0.5 * (1 / fx + 1 / fy): the Gaussian is as large as the pixel's footprint at
 *     its depth;
 *   RGB_DC (k = 3; reads color_obs): the degree-0 SH coefficients of the observed colour, (rgb - 0.5f) * inv_C0 with one rounded
 *     subtraction, one rounded multiply and inv_C0 = (float)(1 / 0.28209479177387814);
 *   QUAT_IDENTITY (k = 4): (1, 0, 0, 0);
 *   CONST (any k): `value` in every component -- logit(init_opacity) for opacity_raw, 0 for the higher SH coefficients, the Adam
 *     moments and xyz_gradient_accum / denom / max_radii2D.  (Unlike densify-and-prune, which zeroes the accumulators, their old
 *     rows are copied: a keyframe arriving must not wipe the statistics of the rows that stay.)
 * Argument errors return DGR_ERR_BAD_ARGUMENT with a message before any device call: a NULL or misaligned plan, NULL depth_obs
 * or viewmatrix, non-positive width, height or stride, fx or fy not finite and positive, rows_out outside rows .. rows + the
 * number of candidates (what can be checked of rows_out == rows + the plan's count without reading the device), n outside
 * 1 .. DGR_SEED_MAX_TENSORS, k < 1, an unknown mode, two XYZ descriptors, a wrong k for a mode, RGB_DC without color_obs.  Not
 * capturable as a whole: the caller reads counts between the two calls. */
#define DGR_SEED_MAX_TENSORS 24
#define DGR_SEED_XYZ 0
#define DGR_SEED_LOG_SCALE 1
#define DGR_SEED_RGB_DC 2
#define DGR_SEED_QUAT_IDENTITY 3
#define DGR_SEED_CONST 4
typedef struct {
    const float* src;
    float* dst;
    int k;
    int mode;
    float value;
} dgr_seed_tensor;
size_t dgr_seed_plan_bytes(int width, int height, int stride);
int dgr_seed_plan(void* stream, int width, int height, int stride, const float* depth_obs, const float* opacity_map /* or NULL */,
                  const float* depth /* or NULL */, float depth_min, float depth_max, float silhouette_threshold,
                  float depth_error_min, const float* depth_error_min_device /* or NULL */, long rows, void* plan,
                  int* counts8_device);
int dgr_seed_apply(void* stream, int width, int height, int stride, long rows, long rows_out, const void* plan, int n,
                   const dgr_seed_tensor* tensors, const float* color_obs /* or NULL */, const float* depth_obs,
                   const float* viewmatrix, float fx, float fy, float cx, float cy, float pix);

/* ---- the small pieces of a tracking iteration around the rasterizer, one launch each (the reference's
 * caller, CG-SLAM, does these with a dozen elementwise torch kernels each -- a 640x480 tracking step is launch-bound) ----
 * dgr_pose_forward: (quat = (r, x, y, z), not necessarily unit; trans) -> the three camera tensors the rasterizer takes,
 *   in its convention (cuda_rasterizer/auxiliary.h:58-77): viewmatrix = W2C^T, projmatrix = W2C^T * perspec_matrix with
 *   perspec_matrix = Proj^T, campos = -R^T t.  16 + 16 + 3 floats.
 * dgr_pose_backward: dL/dviewmatrix[16] (the rasterizer's pose gradient) -> dL/dquat[4], dL/dtrans[3], through the
 *   normalisation of quat.  projmatrix and campos are constants of the rasterizer call, as in the reference
 *   (diff_gaussian_rasterization/__init__.py L:164-176 returns a gradient for `viewmatrix` only). */
int dgr_pose_forward(void* stream, const float* quat, const float* trans, const float* perspec_matrix, float* viewmatrix,
                     float* projmatrix, float* campos);
int dgr_pose_backward(void* stream, const float* quat, const float* dL_dviewmatrix, float* dL_dquat, float* dL_dtrans);
/* loss = w_color * mean|color - color_obs| + w_depth * mean|depth - depth_obs| (two launches, fixed summation order);
 * `scratch` holds dgr_l1_loss_scratch_floats() floats.  The backward writes both gradient images in one launch:
 * w / n * sign(difference) * (*upstream), `upstream` == NULL meaning 1. */
int dgr_l1_loss_scratch_floats(void);
int dgr_l1_loss_forward(void* stream, long n_color, const float* color, const float* color_obs, long n_depth, const float* depth,
                        const float* depth_obs, float w_color, float w_depth, float* scratch, float* loss);
int dgr_l1_loss_backward(void* stream, long n_color, const float* color, const float* color_obs, long n_depth, const float* depth,
                         const float* depth_obs, float w_color, float w_depth, const float* upstream, float* dL_dcolor,
                         float* dL_ddepth);

/* ---- the standard mapping loss: L1 + D-SSIM on the colour images, L1 on the depth (csrc/ssim.hip) ----
 *   loss = w_l1 * mean|img - ref| + w_ssim * (1 - SSIM(img, ref)) + w_depth * mean|depth - depth_obs|
 * over a contiguous [n_images, channels, height, width] float stack.  SSIM is 3DGS's ssim(window_size=11, size_average=True):
 * per channel and image, the 11 x 11 window g g^T with g[i] ~ exp(-(i - 5)^2 / (2 * 1.5^2)) normalised to sum 1, the images
 * zero-padded by 5, C1 = 0.01^2, C2 = 0.03^2, the mean of the map over every element.  n_depth = 0 drops the depth term.
 * `scratch`: dgr_ssim_scratch_floats() floats, 16-byte aligned (0 for a shape it refuses: a non-positive dimension,
 *   n_images * channels above 65535, height or width above 2^20) = 4 header floats, the workgroups' partial sums and the three
 *   derivative maps (3 * n_images * channels * height * width floats, at the end).  After the forward scratch[0] holds the mean
 *   SSIM, scratch[1] mean|img - ref| and scratch[2] mean|depth - depth_obs|.
 * `want_maps` = 0 is the inference form: the maps are neither written nor needed (scratch may end where they would begin) and
 *   the backward must not be called: one that is fills dL_dimg with NaN.
 * The forward is at most three launches, the backward at most two; neither synchronises the host or allocates, so both can be
 * captured into a hipGraph, and neither uses atomics: the loss and both gradient images carry the same bits on every run.
 * The backward takes the forward's arguments and scratch, writes dL_dimg = d loss / d img * (*upstream) (`upstream` == NULL
 * meaning 1) once and, with n_depth > 0, dL_ddepth.  `ref` and `depth_obs` receive no gradient.  Every argument error returns
 * DGR_ERR_BAD_ARGUMENT with a message before any device call. */
long dgr_ssim_scratch_floats(int n_images, int channels, int height, int width);
int dgr_ssim_loss_forward(void* stream, int n_images, int channels, int height, int width, const float* img, const float* ref,
                          long n_depth, const float* depth, const float* depth_obs, float w_l1, float w_ssim, float w_depth,
                          float* scratch, int want_maps, float* loss);
int dgr_ssim_loss_backward(void* stream, int n_images, int channels, int height, int width, const float* img, const float* ref,
                           long n_depth, const float* depth, const float* depth_obs, float w_l1, float w_ssim, float w_depth,
                           const float* scratch, const float* upstream, float* dL_dimg, float* dL_ddepth /* NULL when n_depth == 0 */);

/* ---- the masked L1 loss of RGB-D SLAM with a per-view median outlier test (csrc/masked_loss.hip) ----
 * Over a stack of n_views views -- color, color_obs: contiguous [n_views, channels, height, width] floats; depth, depth_obs,
 * opacity_map (NULL: no silhouette test) and mask (bytes, NULL: no user mask): [n_views, height, width] -- per pixel p of view v,
 * every operation a single fp32 one (a host restatement reproduces masks, medians and counts bit for bit):
 *   e      = fabsf(depth - depth_obs)
 *   B      = depth_lo < depth_obs && depth_obs < depth_hi && isfinite(e) [&& opacity_map > silhouette_threshold] [&& mask != 0]
 *            (a NaN anywhere fails its test: the pixel drops out)
 *   median = the LOWER median of e over B_v, the element of 0-based rank (|B_v| - 1) / 2 (torch.median's), 0 for an empty B_v;
 *            exact, by a radix select over the bits of e on the device (no sort, no host read); one per view
 *   K      = B && e <= outlier_factor * median     (<=: a perfectly fitted frame, median 0, keeps its pixels);
 *            K = B with reject_outliers = 0, and then no median is computed (the stored one is NaN)
 *   loss   = w_depth * S_d / N_d + w_color * S_c / N_c,   S_d = sum_K e,   S_c = sum over the channels of |color - color_obs|
 *            over K (mask_color != 0) or over every pixel (mask_color = 0, the mapping form);
 *            DGR_MASKED_LOSS_SUM: N_d = N_c = 1;  DGR_MASKED_LOSS_MEAN: N_d = |K| over the whole stack, N_c = channels * |K|, or
 *            channels * height * width * n_views with mask_color = 0 -- counts read on the device; a zero count gives a zero term
 *   dL_ddepth = *upstream * w_depth / N_d * sign(depth - depth_obs) on K, 0 elsewhere; dL_dcolor likewise on its set.  The mask
 *            is piecewise constant: nothing flows to opacity_map, the observations or the median.
 * `scratch`: dgr_masked_loss_scratch_bytes() bytes, 16-byte aligned (0 for a shape it refuses: a non-positive dimension, n_views
 *   above 65535, height * width above 2^30).  With R(x) = x rounded up to a multiple of 16, from its start:
 *     stats header   64 bytes: float[0] = w_depth / N_d, float[1] = w_color / N_c (the backward's scales); bytes 8..63 are not
 *                    written (a caller may point `loss` there)
 *     median         float[n_views] at 64;   base = |B_v|: int[n_views] at 64 + R(4 n_views);   kept = |K_v|: int[n_views] at
 *                    64 + 2 R(4 n_views);    then 16 n_views bytes of per-view sums
 *     histograms     3 * n_views * 2048 32-bit counts (the select's three digits of 11 / 11 / 10 bits)
 *     partials       32 bytes per workgroup (sums as hi/lo float pairs, counts)
 *     mask bytes     the LAST R(n_views * height * width) bytes: 1 for a pixel in K, else 0 -- the backward reads them, so the
 *                    mask has one definition
 * The forward is at most six launches (two with reject_outliers = 0), the backward one; none of them blocks the host, both can
 * be captured into a hipGraph, sums are added in a fixed order and only integers atomically: every output carries the same bits
 * on every run.  The backward takes the forward's arguments and scratch; dL_dcolor or dL_ddepth may be NULL (not both).
 * Every argument error returns DGR_ERR_BAD_ARGUMENT with a message before any device call. */
#define DGR_MASKED_LOSS_SUM 0
#define DGR_MASKED_LOSS_MEAN 1
typedef struct dgr_masked_loss_params {
    float depth_lo, depth_hi;     /* exclusive bounds on depth_obs; (0, INFINITY) = any valid sensor depth */
    float silhouette_threshold;   /* used when opacity_map != NULL */
    float outlier_factor;         /* >= 0; used when reject_outliers != 0 */
    int reject_outliers;
    int mask_color;
    int reduction;                /* DGR_MASKED_LOSS_SUM or DGR_MASKED_LOSS_MEAN */
    float w_color, w_depth;
} dgr_masked_loss_params;
size_t dgr_masked_loss_scratch_bytes(int n_views, int height, int width);
int dgr_masked_loss_forward(void* stream, int n_views, int channels, int height, int width, const float* color,
                            const float* color_obs, const float* depth, const float* depth_obs, const float* opacity_map,
                            const unsigned char* mask, const dgr_masked_loss_params* params, void* scratch, float* loss);
int dgr_masked_loss_backward(void* stream, int n_views, int channels, int height, int width, const float* color,
                             const float* color_obs, const float* depth, const float* depth_obs, const float* opacity_map,
                             const unsigned char* mask, const dgr_masked_loss_params* params, const void* scratch,
                             const float* upstream, float* dL_dcolor, float* dL_ddepth);

/* ---- keyframe overlap scores: which stored keyframes see what the current frame sees (csrc/keyframe_overlap.hip) ----
 * What CG-SLAM, SplaTAM and the NICE-SLAM family do before a mapping phase (SplaTAM's keyframe_selection_overlap), and MonoGS
 * against the last keyframe (n_keyframes = 1) to decide whether a frame becomes a keyframe: pixels of the current frame are
 * unprojected with the measured depth, taken into every stored keyframe and counted where they land inside its image.  One call
 * for all keyframes, one launch (two when a keyframe's candidates need more than one workgroup), no host read, no atomics.
 * Inputs, float32 on the device: depth_obs [height, width]; viewmatrix: the current frame's 16 floats holding W2C^T (what the
 * rasterizer takes and dgr_pose_forward writes; taken as rigid); keyframe_viewmatrices [n_keyframes, 16], same convention;
 * keyframe_depths [n_keyframes, height, width] or NULL.  The keyframes share the frame's size and intrinsics (as the batched entry
 * points assume).
 * Candidates: the stride grid of dgr_seed_plan -- the pixels with x % stride == 0 && y % stride == 0, numbered row-major, S =
 *   ceil(width / stride) * ceil(height / stride).  No sampling, no compaction.
 *   valid   = depth_min < d && d < depth_max, d = depth_obs at the candidate: raw fp32 comparisons, false on a NaN (dgr_seed_plan's)
 * Geometry, in fp32 (fused multiply-adds allowed): pixel (x, y) at depth d is p = ((x - cx) / fx * d, (y - cy) / fy * d, d) in the
 *   current camera (dgr_seed_plan's convention); p goes to the world through the rigid inverse of the current pose and on into
 *   keyframe k, (X, Y, Z) = R_k R^T (p - t) + t_k.  The kernel forms R_k R^T and t_k - R_k R^T t from the two matrices itself, in
 *   double, rounded once: no inverse is formed on the host.  u = fx * X / Z + cx, v = fy * Y / Z + cy.
 *   inside  = valid && Z > near_z && edge < u && u < width - edge && edge < v && v < height - edge      (SplaTAM's strict tests)
 *   visible = inside without keyframe_depths; with them, inside && depth_min < d_k && d_k < depth_max &&
 *             fabsf(Z - d_k) <= depth_tolerance * d_k, d_k = keyframe k's depth at pixel (floor(u + 0.5), floor(v + 0.5)); a pixel
 *             outside the image (possible only with edge < 0.5) is not visible
 * Outputs, on the device: inside[n_keyframes], visible[n_keyframes] (int counts per keyframe), valid[1] (int, the frame's),
 * score[n_keyframes] = (float)visible[k] / (float)valid as one fp32 division, 0 when valid == 0 (never NaN); flags
 * [n_keyframes, S] bytes (bit 0 valid, bit 1 inside, bit 2 visible) or NULL.  Nothing else is written.  Counts are integer sums:
 * the same bits on every run.  Capturable into a hipGraph.
 * `scratch`: dgr_keyframe_overlap_scratch_bytes() bytes, 16-byte aligned (0 for a shape it refuses).
 * Argument errors return DGR_ERR_BAD_ARGUMENT with a message before any device call: non-positive width, height, stride or
 * n_keyframes; n_keyframes above 2^20 or n_keyframes * S at or above 2^31; a NULL params, depth_obs, viewmatrix,
 * keyframe_viewmatrices, scratch (or a misaligned one) or output other than flags; fx or fy not finite and positive; a NaN cx, cy,
 * depth_min, depth_max or near_z; an edge or depth_tolerance that is NaN or negative. */
typedef struct dgr_keyframe_overlap_params {
    float fx, fy, cx, cy;         /* the shared intrinsics, pixels */
    float depth_min, depth_max;   /* exclusive bounds on a usable depth; (0, INFINITY) = any valid sensor depth */
    float edge;                   /* >= 0: the margin inside the keyframe's image, pixels (SplaTAM: 20) */
    float near_z;                 /* Z > near_z (SplaTAM: 0) */
    float depth_tolerance;        /* >= 0; used with keyframe_depths */
    int stride;
} dgr_keyframe_overlap_params;
size_t dgr_keyframe_overlap_scratch_bytes(int width, int height, int stride, int n_keyframes);
int dgr_keyframe_overlap(void* stream, int width, int height, const float* depth_obs, const float* viewmatrix, int n_keyframes,
                         const float* keyframe_viewmatrices, const float* keyframe_depths /* or NULL */,
                         const dgr_keyframe_overlap_params* params, void* scratch, int* inside, int* visible, int* valid,
                         float* score, unsigned char* flags /* or NULL */);

/* ---- frame-to-model ICP pose alignment: the geometric pose initialisation in front of the photometric tracker (csrc/icp.hip) ----
 * KinectFusion's projective point-to-plane ICP of the sensor depth against the model's rendered depth, as RTG-SLAM and GS-ICP SLAM
 * run it on a Gaussian map.  Conventions are dgr_keyframe_overlap's and dgr_seed_plan's: float32 images on the device, pixel
 * (x, y) at depth d is the camera point V = ((x - cx) / fx * d, (y - cy) / fy * d, d), poses are 16 floats holding W2C^T taken as
 * rigid, raw fp32 comparisons that are false on a NaN, the stride grid as candidates.  No host read, no float atomics, the same
 * bits on every run, capturable into a hipGraph.
 *
 * dgr_depth_normals: depth [height, width] (and mask_image [height, width] or NULL) -> vnmap [height, width, 4] = (nx, ny, nz, d),
 * packed so that the step's gather is one 16-byte load; one launch.  A pixel is usable when it and its four neighbours x +- 1,
 * y +- 1 lie inside the image with depth_min < d && d < depth_max; with a mask, its own mask_image > mask_threshold; each
 * neighbour's depth satisfies fabsf(d_n - d) <= max_jump * d; and the cross product below is non-zero (and finite).  Its normal is
 * n = normalize((V(x+1, y) - V(x-1, y)) x (V(x, y+1) - V(x, y-1))), flipped so that n . V <= 0 (facing the camera), and d its own
 * depth's bits.  Every other pixel (the border among them) gets four zeros.
 * Argument errors: non-positive width or height, 2^30 pixels or more; a NULL depth; a NULL or misaligned vnmap (16 bytes); fx or
 * fy not finite and positive; a NaN cx, cy, depth_min, depth_max (or mask_threshold with a mask); max_jump NaN or negative.
 *
 * dgr_icp_step: one Gauss-Newton iteration, ONE launch.  Inputs: depth_obs [height, width]; vn_obs, the observation's map, or
 * NULL (used only by the normal-compatibility test); vn_model, the map of the model depth rendered at model_viewmatrix;
 * viewmatrix_in, the current estimate.  Per candidate pixel (x, y) of depth_obs, in fp32 (fused multiply-adds allowed):
 *   valid      = depth_min < d && d < depth_max, and with vn_obs its d > 0
 *   q          = R_rel p + t_rel, p the candidate's camera point, rel = T_model T_in^-1 formed by the kernel from the two matrices
 *                in double and rounded once (no inverse is formed on the host)
 *   pixel      = (floor(u + 0.5), floor(v + 0.5)), u = fx * q.x / q.z + cx, v = fy * q.y / q.z + cy
 *   inside     = valid && q.z > 0 && the pixel lies in the image && the model's d_m > 0 there
 *   e          = q - v_m, v_m the camera point of that pixel at d_m; n_m the model's normal there
 *   associated = inside && |e| <= dist_max && (no vn_obs || (R_rel n_obs) . n_m >= normal_cos_min)
 *   r = n_m . e;  J = (q x n_m, n_m), the rotation part first;  w = 1 for |r| <= huber_delta, else huber_delta / |r|
 *                (huber_delta = INFINITY: no robust weight)
 * Sums over the associated candidates, accumulated in double from the first addition in a fixed order (a thread's candidates
 * ascending, the workgroup's threads by the block sum, the workgroups of 2048 candidates in block order): the 21 upper-triangle
 * entries of A = sum w J J^T (row-major), the 6 of b = sum w J r, sum w r^2, the count.
 * Solve, one thread in double: M xi = -b by LDL^T, M = A + damping * diag(max(A_ii, 1e-3 max_i A_ii)) -- Marquardt's scaling with
 * a floor, so that a direction with an exactly zero row (a fronto-parallel plane's) has a pivot under damping > 0 and stays put.
 * Refused (ok = 0) when count < min_points, a pivot <= rcond * max_i A_ii, or anything is not finite.  E = exp(xi) on SE(3)
 * (Rodrigues, series near 0), T_out = T_in T_model^-1 E^-1 T_model, its rotation re-orthonormalised through its unit quaternion.
 * Outputs: viewmatrix_out[16] (W2C^T; may be viewmatrix_in: the finishing workgroup reads before it writes); quat_out[4]
 * (r, x, y, z; unit, r >= 0) and trans_out[3] or NULL, dgr_pose_forward's convention; stats, 32 doubles: A (21), b (6),
 * sum w r^2 [27], count [28], ok [29], |omega| [30], |v| [31] (both 0 when refused); flags [S] bytes or NULL (bit 0 valid, bit 1
 * inside, bit 2 associated).  When refused every pose output carries the input's bits (quat_out derived from the input matrix).
 * `scratch`: dgr_icp_scratch_bytes() bytes, 16-byte aligned (0 for a shape it refuses).  Its first 16 bytes hold the workgroups'
 * ticket and MUST BE ZERO before the first call that uses it; every call leaves them zero, so one zero-filled allocation serves
 * any number of calls in stream order (and a recorded graph replays).  The rest needs no initialisation.
 * Argument errors return DGR_ERR_BAD_ARGUMENT with a message before any device call: non-positive width, height or stride, 2^30
 * candidates or more; a NULL params, depth_obs, vn_model, model_viewmatrix, viewmatrix_in, scratch, viewmatrix_out or stats; a
 * vn_obs, vn_model or scratch that is not 16-byte aligned, stats not 8-byte aligned; fx or fy not finite and positive; a NaN
 * cx, cy, depth_min or depth_max; dist_max, huber_delta, damping or rcond NaN or negative; normal_cos_min outside [-1, 1] (or
 * NaN); min_points < 1. */
typedef struct dgr_icp_params {
    float fx, fy, cx, cy;         /* the shared intrinsics, pixels */
    float depth_min, depth_max;   /* exclusive bounds on a usable depth_obs; (0, INFINITY) = any valid sensor depth */
    float dist_max;               /* >= 0: largest |q - v_m| of an associated pair (KinectFusion: 0.1 m) */
    float normal_cos_min;         /* [-1, 1]; used with vn_obs (KinectFusion: cos 20 deg ~ 0.94; 0.8 here) */
    float huber_delta;            /* >= 0; INFINITY = least squares */
    float damping;                /* >= 0; 0 = Gauss-Newton */
    float rcond;                  /* >= 0: smallest pivot accepted, relative to the largest diagonal entry of A */
    int min_points;               /* >= 1 */
    int stride;
} dgr_icp_params;
int dgr_depth_normals(void* stream, int width, int height, const float* depth, const float* mask_image /* or NULL */,
                      float mask_threshold, float fx, float fy, float cx, float cy, float depth_min, float depth_max, float max_jump,
                      float* vnmap);
size_t dgr_icp_scratch_bytes(int width, int height, int stride);
int dgr_icp_step(void* stream, int width, int height, const float* depth_obs, const float* vn_obs /* or NULL */,
                 const float* vn_model, const float* model_viewmatrix, const float* viewmatrix_in, const dgr_icp_params* params,
                 void* scratch, float* viewmatrix_out, float* quat_out /* or NULL */, float* trans_out /* or NULL */, double* stats,
                 unsigned char* flags /* or NULL */);

/* ---- hybrid RGB-D pose alignment: a photometric term beside the ICP step (csrc/icp.hip) ----
 * What every classical RGB-D front end adds to point-to-plane ICP (Kerl's DVO, Open3D's hybrid odometry, the initialisers of
 * Gaussian-SLAM and LoopSplat): the model's rendered colour against the sensor's colour.  It constrains the directions a planar
 * scene leaves free.  Conventions are the ICP block's throughout; fused multiply-adds are allowed wherever a sum of products is
 * written, the operation order is the one written.
 *
 * dgr_intensity_map: image [channels, height, width], channels = 1 or 3 (the rasterizer's layout), and mask_image [height, width]
 * or NULL -> imap [height, width, 4] = (I, I_x, I_y, u), one 16-byte store per pixel, so that the step's gather is one 16-byte
 * load; one launch, a thread per pixel.
 *   I   = the single channel's bits, or (0.299f * R + 0.587f * G) + 0.114f * B
 *   I_x = (((I(x+1,y-1) - I(x-1,y-1)) + (I(x+1,y+1) - I(x-1,y+1))) + 2 * (I(x+1,y) - I(x-1,y))) * 0.125f   (Sobel / 8)
 *   I_y = (((I(x-1,y+1) - I(x-1,y-1)) + (I(x+1,y+1) - I(x+1,y-1))) + 2 * (I(x,y+1) - I(x,y-1))) * 0.125f
 *   usable (u = 1.0f): the pixel is interior (x +- 1 and y +- 1 lie inside the image), all nine intensities of its 3 x 3
 *   neighbourhood are finite, and with a mask all nine mask values > mask_threshold (a rendered image means something only where
 *   the silhouette is).  Every other pixel gets four zeros.
 * `intensity` [height, width] or NULL also receives I of every pixel as a plain plane (the observation's side of the step, and
 * what the next pyramid level is halved from); imap may then be NULL.
 * Argument errors: non-positive width or height, 2^30 pixels or more; channels other than 1 or 3; a NULL image; imap and
 * intensity both NULL; a misaligned imap (16 bytes); a NaN mask_threshold with a mask.
 *
 * dgr_frame_halve: one pyramid level, one launch: width x height -> floor(width / 2) x floor(height / 2); output pixel (x, y)
 * is made of the block a = (2x, 2y), b = (2x+1, 2y), c = (2x, 2y+1), d = (2x+1, 2y+1); an odd last row or column is dropped.
 *   mean planes: planes [n_planes, height, width] -> planes_out [n_planes, height/2, width/2], ((a + b) + (c + d)) * 0.25f
 *   depth plane (depth [height, width] or NULL -> depth_out): with usable = depth_min < d && d < depth_max per pixel of the
 *   block, n their number, lo and hi the smallest and largest usable depth: ((a' + b') + (c' + d')) / (float)n where
 *   n >= 1 && hi - lo <= max_jump * lo (v' = v when usable, else 0.0f; one fp32 division), else 0.0f.
 * Pixel centres sit at integers, so the level's intrinsics are fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2.
 * Argument errors: width or height below 2, 2^30 pixels or more; n_planes outside 0 .. 64; n_planes = 0 without a depth; a NULL
 * planes or planes_out with n_planes > 0; a depth without depth_out; with a depth, a NaN depth_min or depth_max, max_jump NaN or
 * negative.
 *
 * dgr_rgbd_step: one hybrid Gauss-Newton iteration, ONE launch: dgr_icp_step with a photometric pair per candidate beside the
 * geometric one.  Extra inputs: intensity_obs [height, width], the observation's intensity as a plain plane (only the candidate's
 * own value is read); imap_model [height, width, 4], dgr_intensity_map of the model's colour rendered at model_viewmatrix.
 * Per candidate: valid, q, u, v, the pixel (px, py) = (floor(u + 0.5), floor(v + 0.5)), inside, e, associated, r, J and w are
 * exactly dgr_icp_step's.  The geometric pair (an associated candidate) enters the sums only when geo_weight > 0.
 *   photometric = inside && |e| <= dist_max (the occlusion test; no normal test) && u_m == 1 at (px, py) && I_obs finite &&
 *                 |r_p| <= photo_max; it enters the sums only when photo_weight > 0
 *   r_p = ((I_m + I_x * (u - px)) + I_y * (v - py)) - I_obs(x, y): the nearest model pixel with its first-order sub-pixel
 *         correction: one gather, exact on a linear ramp
 *   g   = (g_x, g_y, g_z), g_x = (I_x * fx) / q.z, g_y = (I_y * fy) / q.z, g_z = -((g_x * q.x + g_y * q.y) / q.z)
 *   J_p = (q x g, g);  w_p = 1 for |r_p| <= photo_huber, else photo_huber / |r_p|
 * Sums, in dgr_icp_step's order and double accumulation, a candidate's geometric pair before its photometric one: per pair
 * s = class weight * w as one fp32 product (geo_weight * w, photo_weight * w_p), A += (s J_i) J_j, b += (s J_i) r, each product
 * rounded to fp32; kept apart and unscaled by the class weight: sum w r^2 = sum (w r) r and count_g, sum w_p r_p^2 and count_p.
 * Refused when count_g + count_p < min_points, or by dgr_icp_step's pivot and finiteness rules (sum w_p r_p^2 among the sums
 * that must be finite).  Solve, update, outputs, the aliasing guarantee and the scratch contract are dgr_icp_step's;
 * dgr_rgbd_scratch_bytes = dgr_icp_scratch_bytes, and one scratch serves both steps.
 * stats, 40 doubles: A (21), b (6), sum w r^2 [27], count_g [28], sum w_p r_p^2 [29], count_p [30], ok [31], |omega| [32],
 * |v| [33], zeros [34..39].  flags: dgr_icp_step's bits and bit 3 = photometric (whatever the class weights are).
 * With geo_weight = 1 and photo_weight = 0 every pose output, A, b, sum w r^2 and the count carry dgr_icp_step's bits (1 * w is
 * exact).
 * Argument errors: dgr_icp_step's, and a NULL intensity_obs, a NULL or misaligned imap_model (16 bytes), geo_weight,
 * photo_weight, photo_max or photo_huber NaN or negative. */
typedef struct dgr_rgbd_params {
    float fx, fy, cx, cy;         /* dgr_icp_params' fields, in its order */
    float depth_min, depth_max;
    float dist_max;
    float normal_cos_min;
    float huber_delta;
    float damping;
    float rcond;
    int min_points;
    int stride;
    float geo_weight;             /* >= 0: the geometric pairs' class weight; 0 = photometric only */
    float photo_weight;           /* >= 0: the photometric pairs' class weight (intensity^-2 against metres^-2); 0 = dgr_icp_step */
    float photo_max;              /* >= 0: largest |r_p| of a photometric pair; INFINITY = none */
    float photo_huber;            /* >= 0; INFINITY = least squares */
} dgr_rgbd_params;
int dgr_intensity_map(void* stream, int width, int height, int channels, const float* image, const float* mask_image /* or NULL */,
                      float mask_threshold, float* imap /* or NULL */, float* intensity /* or NULL */);
int dgr_frame_halve(void* stream, int width, int height, int n_planes, const float* planes /* or NULL */,
                    const float* depth /* or NULL */, float depth_min, float depth_max, float max_jump, float* planes_out,
                    float* depth_out);
size_t dgr_rgbd_scratch_bytes(int width, int height, int stride);
int dgr_rgbd_step(void* stream, int width, int height, const float* depth_obs, const float* vn_obs /* or NULL */,
                  const float* vn_model, const float* intensity_obs, const float* imap_model, const float* model_viewmatrix,
                  const float* viewmatrix_in, const dgr_rgbd_params* params, void* scratch, float* viewmatrix_out,
                  float* quat_out /* or NULL */, float* trans_out /* or NULL */, double* stats, unsigned char* flags /* or NULL */);

/* ---- pose-graph optimisation: the solver in front of the map correction (csrc/pgo.hip) ----
 * What a SLAM back end runs after a loop closure (g2o, GTSAM, Open3D's pose graph), here on the device: n_poses keyframe poses
 * T_k (16 floats holding W2C^T each, as everywhere above) and n_edges relative-pose constraints give the poses that
 * dgr_transform_plan's corrections are formed from.  No host read, no float atomics, the same bits on every run, capturable
 * into a hipGraph.
 * Problem: edge e = (i, j, Z_e, Omega_e), edges [n_edges, 2] int32 = (i, j), measures Z_e ~ T_i T_j^-1 (camera j's coordinates to
 *   camera i's); measurements [n_edges, 16] holds Z_e^T, the viewmatrix layout.  r_e = Log(Z_e^-1 T_i T_j^-1) in R^6, ordered
 *   (omega, v) as dgr_icp_step's twist; s_e = sqrt(r_e^T Omega_e r_e); minimised is sum_e rho(s_e), rho(s) = s^2 for
 *   s <= huber_delta and 2 huber_delta s - huber_delta^2 beyond (INFINITY: least squares), over the free poses with the update
 *   T_k <- Exp(d_k) T_k.  `fixed` [n_poses] bytes (non-zero = fixed) holds the gauge; NULL fixes pose 0 only.
 *   information_kind 0: Omega = I (information ignored); 2: information [n_edges, 2] = (rotation weight, translation weight),
 *   Omega = diag(a, a, a, b, b, b); 36: information [n_edges, 6, 6] row-major, its symmetric part used.
 * dgr_pgo_plan: ONE launch of one workgroup: every pose's incidence list (edge, side) into `scratch`, in ascending edge order, side
 *   i before side j.  This order is the summation order of every per-node sum below.  An edge with an index outside
 *   0 .. n_poses - 1 or with i == j is left out (and counted as skipped by the solve).  A plan serves every solve with the same
 *   n_poses, n_edges and edges, in stream order (and a recorded graph replays).
 * dgr_pgo_solve: ONE launch of one workgroup runs the whole solve, all in double: Levenberg-Marquardt with iteratively
 *   reweighted Huber, at most `iterations` trials.  Poses are read into unit quaternions and translations; the solve is REFUSED
 *   (stats ok = 0, every pose output the input's bits, chi2 NaN) when a pose is not rigid: not finite, det <= 0, or R^T R off the
 *   identity by more than 1e-3 (dgr_transform_plan's rule), or when `scratch` holds no plan for this n_poses and n_edges.
 *   Linearise: per usable edge r_e, the exact first-order Jacobians J_j = -J_r^-1(r_e), J_i = J_r^-1(r_e) Ad(T_j T_i^-1) in closed
 *   form, w_e = min(1, huber_delta / s_e), the blocks of H = sum J^T (w Omega) J and g = sum J^T (w Omega) r.  The Log goes through
 *   the sign-normalised unit quaternion (stable up to an angle of pi; a series below theta^2 = 1e-6).  An edge is skipped and
 *   counted when the plan left it out, Z_e is not rigid (the rule above) or Omega_e has a non-finite entry.
 *   Per node, in list order: its diagonal block and gradient; the damped block's 6 x 6 LDL^T.  A free node with a pivot
 *   <= rcond * (its largest diagonal entry) -- a node with no usable edge among them -- is loose: treated as fixed for the rest
 *   of the solve and counted.
 *   (H + lambda diag H) d = -g by preconditioned conjugate gradients, block-Jacobi preconditioner (those LDL^T), x0 = 0, at most
 *   cg_iterations, stopped at r^T M^-1 r <= cg_tolerance^2 r0^T M^-1 r0.  H p is a per-node gather: the damped diagonal block
 *   first, then the off-diagonal blocks in list order.  Dot products and the cost: a thread's items ascending (thread t of 256
 *   takes t, t + 256, ..), then the workgroup's fixed-order block sum.
 *   The candidate T_k <- Exp(d_k) T_k is accepted when its cost fell, then lambda <- max(lambda / 10, 1e-12); otherwise the poses
 *   are restored and lambda <- min(10 lambda, 1e12).  Stops early on an accepted step with max(|omega_k|, |v_k|) <
 *   step_tolerance or a relative cost decrease below cost_tolerance (both: converged), on a zero gradient or no free node left
 *   (converged, the trial not counted), or with lambda at its maximum.
 * Outputs: poses_out [n_poses, 16] (may be poses_in), rotations re-orthonormalised through the quaternion; fixed and loose poses
 *   -- and every pose when no step was accepted -- keep the input's bits.  chi2 [n_edges] or NULL: s_e^2 at the poses as
 *   written, NaN for a skipped edge.  stats, 16 doubles: initial cost [0], final cost (at the poses as written) [1], ok [2],
 *   trials run [3], accepted [4], rejected [5], CG iterations in total [6], final lambda [7], max_k |omega_k| [8] and max_k |v_k|
 *   [9] of the last accepted step, max |g| over the free poses at the poses as written [10] (g = sum J^T w Omega r, half the
 *   cost's gradient), edges used [11], edges skipped [12], loose poses [13], converged [14], 0 [15].  flags [1] int: bit 0
 *   refused, bit 1 an edge was skipped, bit 2 a pose is loose, bit 3 stopped with lambda at its maximum, bit 4 a CG solve ran
 *   into cg_iterations, bit 5 no plan.
 * `scratch`: dgr_pgo_scratch_bytes() bytes, 16-byte aligned (0 for a shape it refuses: n_poses outside 1 .. 65536, n_edges
 *   outside 0 .. 2^18); no initialisation needed before dgr_pgo_plan.
 * Argument errors return DGR_ERR_BAD_ARGUMENT with a message before any device call: those shapes; a NULL params, poses_in,
 *   poses_out, flags, scratch (or a misaligned one), stats (or one not 8-byte aligned); with n_edges > 0 a NULL edges,
 *   measurements, or information with a kind other than 0; an information_kind other than 0, 2, 36; iterations outside
 *   0 .. 1000; cg_iterations outside 1 .. 2^20; a poses_in, edges, measurements, information, poses_out, chi2 or flags that is not
 *   4-byte aligned; a cg_tolerance, huber_delta, damping, rcond, step_tolerance or cost_tolerance that is NaN or negative.
 * How long one launch can run: the solve is one workgroup that nothing interrupts, and it runs at most iterations * cg_iterations
 *   CG iterations, each a pass over the nodes and their lists (measured on an MI355X: 12 us at 200 poses, 64 us at 1000, growing
 *   with n_poses / 256 and with the degrees).  The caps keep that finite, not short: at the largest shapes and the Python default of
 *   12 n_poses the bound is hours on one compute unit.  Size iterations and cg_iterations to the time the device can be held;
 *   flags bit 4 says when a CG solve was cut off. */
typedef struct dgr_pgo_params {
    int iterations;               /* 0 .. 1000 trials; 0 evaluates chi2 and the costs only */
    int cg_iterations;            /* 1 .. 2^20; block-Jacobi CG needs about 2 n_poses on a chain */
    float cg_tolerance;           /* >= 0: relative, on sqrt(r^T M^-1 r) */
    float huber_delta;            /* >= 0; INFINITY = least squares */
    float damping;                /* >= 0: the initial lambda (kept inside 1e-12 .. 1e12) */
    float rcond;                  /* >= 0: smallest pivot of a node's block, relative to its largest diagonal entry */
    float step_tolerance;         /* >= 0 */
    float cost_tolerance;         /* >= 0 */
} dgr_pgo_params;
size_t dgr_pgo_scratch_bytes(int n_poses, int n_edges);
int dgr_pgo_plan(void* stream, int n_poses, int n_edges, const int* edges, void* scratch);
int dgr_pgo_solve(void* stream, int n_poses, int n_edges, const float* poses_in, const int* edges, const float* measurements,
                  const float* information /* or NULL */, int information_kind, const unsigned char* fixed /* or NULL */,
                  const dgr_pgo_params* params, void* scratch, float* poses_out, float* chi2 /* or NULL */, double* stats,
                  int* flags);

/* ---- per-Gaussian contribution statistics of a rendered view (csrc/contrib.hip) ----
 * Which Gaussians did the pixels of a finished forward actually BLEND, and how much -- what radii > 0 (a frustum and rectangle
 * test an occluded Gaussian passes) cannot say: MonoGS's n_touched, the largest / accumulated blend weight alpha T that RTG-SLAM,
 * LightGaussian and Mini-Splatting rank by.  The call replays the blend of the view whose state the three buffers hold (light or
 * full forward, one view; the buffers as the backward entry points take them, `R` as theirs: >= 0, the binning buffer is found
 * from the capacity the forward recorded) under the calling thread's alpha_mode (0, 1 and 2 all supported), as for a backward.
 *   A pair (pixel p, 1-based position k in the list of p's tile) is BLENDED iff k <= n_contrib[p], power <= 0 and
 *   alpha = min(0.99, o G) >= 15/255 (the blend kernels' ALPHA_MIN, evaluated by their own functions).  Its weight is w = alpha T,
 *   T the running product of (1 - alpha) over the pixel's earlier blended pairs in list order: the forward's bits.
 *   Per Gaussian g of this view:  n_touched[g] int32 = number of blended pairs;  max_weight[g] float32 = largest w (0 if none);
 *   sum_weight[g] int64 = sum of floor(w 2^32) (Q32 fixed point: * 2^-32 is the accumulated weight; an integer sum does not
 *   depend on the order the atomics arrive in).  Each of the three may be NULL; it then lives in `scratch`.
 *   The running accumulators [P], each of which may be NULL, receive this view in a last pass:  touched_total (int64) +=
 *   n_touched;  max_weight_total (float32) = max;  sum_weight_total (int64) += sum_weight;  views (int32) += 1 and last_seen
 *   (int32) = frame_id where the view OBSERVED g: n_touched >= min_pixels && max_weight >= weight_min.
 *   counts4_device (device int[4], may be NULL) = {Gaussians with n_touched > 0, Gaussians observed, 1 if the frame's binning had
 *   overflowed else 0, 0}.  An overflowed frame has empty lists: its per-view outputs are zero and it is NOT folded into the
 *   accumulators (nor counted as observing anything).
 * At most three launches (clear, tiles, fold), integer atomics only -- the same bits on every run --, nothing read on the host,
 * capturable into a hipGraph.  scratch: dgr_contribution_scratch_bytes(P) bytes, 16-byte aligned; needed (non-NULL) when a
 * per-view output is NULL.  P == 0 succeeds (the state buffers may then be NULL; counts4_device is cleared).  Refused before any
 * device call: params NULL, P < 0 or above 2^28 - 1, width or height <= 0, R < 0, a NULL state buffer, negative min_pixels, NaN
 * or negative weight_min, a scratch that is missing or misaligned, a misaligned output, nothing to write. */
typedef struct dgr_contribution_params {
    int min_pixels;   /* >= 0: blended pairs a view needs to have observed a Gaussian */
    float weight_min; /* >= 0: ... and the largest weight it needs */
    int frame_id;     /* what last_seen receives */
} dgr_contribution_params;
size_t dgr_contribution_scratch_bytes(long P);
int dgr_contribution_stats(void* stream, long P, int width, int height, int R, const char* geometry_buffer,
                           const char* binning_buffer, const char* image_buffer, const dgr_contribution_params* params,
                           void* scratch, int* n_touched, float* max_weight, long long* sum_weight, long long* touched_total,
                           float* max_weight_total, long long* sum_weight_total, int* views, int* last_seen,
                           int* counts4_device);

/* ---- TSDF fusion of rendered views and mesh extraction (csrc/tsdf.hip) ----
 * The surface a dense RGB-D SLAM run hands over: depth and colour rendered (or measured) at the keyframe poses, fused into a
 * truncated signed distance volume, and the zero level of that volume as a triangle mesh.
 * The volume: a dense lattice of nx x ny x nz samples, sample (ix, iy, iz) at origin + voxel_size (ix, iy, iz), x the fastest index.
 *   volume float32 [nz, ny, nx, 2] = (tsdf in [-1, 1], weight >= 0), 8-byte aligned; color float32 [nz, ny, nx, 4] = (r, g, b, 0),
 *   16-byte aligned, or NULL.  Plain memory the caller owns; all zero = empty.  nx ny nz < 2^31.
 * dgr_tsdf_integrate: n_views >= 1 views in ONE launch; every sample is read once and written at most once per call -- not at
 *   all when no view updated it -- whatever n_views is.  depth [n_views, height, width]; image [n_views, 3, height, width] or NULL
 *   (with color: both or neither); mask [n_views, height, width] or NULL; viewmatrices [n_views, 16] = W2C^T; pixel (x, y) at depth
 *   d is the camera point ((x - cx) / fx d, (y - cy) / fy d, d) (dgr_keyframe_overlap's convention).
 *   Per sample p_w and per view, in the order given:  p_c = W2C p_w, z = p_c.z, skip unless z > near_z;  u = fx x / z + cx,
 *   v = fy y / z + cy, the nearest pixel (floor(u + 0.5), floor(v + 0.5)), skip unless inside the image;  d = depth there, skip
 *   unless depth_min < d < depth_max (a NaN fails) and skip if mask there <= mask_threshold;  sdf = d - z (projective), skip if
 *   sdf < -truncation;  t = min(1, sdf / truncation);  tsdf = (tsdf w + t weight) / (w + weight), the colour likewise, then
 *   w = min(w + weight, max_weight).
 *   One thread owns a sample and applies the views in index order: no atomics, the same bits on every run, V views in one call
 *   equal the same views in V calls bit for bit.  Nothing is read on the host and nothing allocated: capturable into a hipGraph.
 *   The values of depth, image, mask and the poses are not validated: a NaN ends in a skipped update or a garbage value, never
 *   in an out-of-range read.
 * dgr_mesh_plan / dgr_mesh_emit: marching tetrahedra on Kuhn's split of every cell (the cube of 8 neighbouring samples, corners
 *   numbered by bits x = 1, y = 2, z = 4) into the six tetrahedra {0, a, a|b, 7}, (a, b) = (1,2), (1,4), (2,1), (2,4), (4,1), (4,2)
 *   in this order.  A cell is valid when all 8 weights are >= min_weight; a sample is inside when tsdf < 0 (an exact 0 is
 *   outside).  A vertex on the edge (A, B), A the corner with the smaller number, is p_A + t (p_B - p_A), t = v_A / (v_A - v_B),
 *   so every cell that shares the edge writes the same bits; colours are interpolated with the same t.  A tetrahedron with one
 *   corner apart gives a triangle, two and two a quadrilateral: its crossings in cyclic order, normal from the inside (negative)
 *   corners to the outside ones, started at the edge with the smallest (A, B), fanned from there: (e0, e1, e2), (e0, e2, e3).
 *   Degenerate triangles are kept.  Output: an unindexed list, vertices float32 [3 T, 3] and colors float32 [3 T, 3], ordered
 *   by linear cell index (x fastest, over the (nx-1)(ny-1)(nz-1) cells), then tetrahedron, then triangle.
 *   plan: two launches (count per 256-cell block, a one-workgroup scan).  count [1] int32 = the triangles needed (saturated at
 *   2^31 - 1), flags [1] int32: bit 0 = more than max_triangles.  emit: one launch; writes the first min(count, max_triangles)
 *   triangles and nothing behind them; the same volume, min_weight and scratch as the plan.  With a caller-given capacity nothing
 *   is read on the host: capturable.  scratch: dgr_mesh_scratch_bytes(grid) bytes (0 for a grid it refuses), 16-byte aligned.
 * Refused with DGR_ERR_BAD_ARGUMENT and a message before any device call: a NULL grid or params; non-positive nx, ny, nz; 2^31
 *   samples or more; a voxel_size, fx, fy or truncation that is not finite and positive; n_views < 1; width or height < 1; a NULL
 *   volume, depth or viewmatrices; color without image or image without color; a misaligned pointer; (mesh) a NaN min_weight, a
 *   negative max_triangles, a NULL or misaligned scratch, a NULL count or flags, a NULL vertices with max_triangles > 0, colors of
 *   a volume without color. */
typedef struct dgr_tsdf_grid {
    int nx, ny, nz;
    float origin[3];
    float voxel_size;
} dgr_tsdf_grid;
typedef struct dgr_tsdf_params {
    float fx, fy, cx, cy;
    float truncation;     /* > 0 */
    float weight;         /* what a view adds to a sample's weight */
    float max_weight;     /* the weight's cap; INFINITY = none */
    float depth_min, depth_max;
    float near_z;
    float mask_threshold; /* a pixel with mask <= this is not fused */
} dgr_tsdf_params;
int dgr_tsdf_integrate(void* stream, const dgr_tsdf_grid* grid, float* volume, float* color /* or NULL */, int n_views, int width,
                       int height, const float* depth, const float* image /* or NULL */, const float* mask /* or NULL */,
                       const float* viewmatrices, const dgr_tsdf_params* params);
size_t dgr_mesh_scratch_bytes(const dgr_tsdf_grid* grid);
int dgr_mesh_plan(void* stream, const dgr_tsdf_grid* grid, const float* volume, float min_weight, int max_triangles, void* scratch,
                  int* count, int* flags);
int dgr_mesh_emit(void* stream, const dgr_tsdf_grid* grid, const float* volume, const float* color /* or NULL */, float min_weight,
                  int max_triangles, const void* scratch, float* vertices, float* colors /* or NULL */);

/* ---- Ray-casting the TSDF volume: depth, normals and colour at any pose (csrc/raycast.hip) ----
 * The other half of a volumetric pipeline: the fused surface seen from a pose -- a multi-view-averaged depth with normals from the
 * field's gradient, as dgr_icp_step's vn_model and dgr_depth_normals' input; the depth the "Depth L1" tables are measured on.
 * The volume, grid and conventions are dgr_tsdf_integrate's: viewmatrices [n_views, 16] = W2C^T with W2C = [R | t]; pixel (x, y) at
 *   z-depth z is the camera point z d_c, d_c = ((x - cx) / fx, (y - cy) / fy, 1), the world point p_w = R^T (z d_c - t).
 * Samples: z_k = depth_min + k step for k = 0, 1, ... while z_k < depth_max (and k < 2^24); each z_k is ONE fused multiply-add from
 *   k, never accumulated along the ray.  step is in metres of z-depth.  Lattice coordinates q = (p_w - origin) / voxel_size, the
 *   cell i = floor(q), the fraction f = q - i.  A sample is valid iff 0 <= i <= n - 2 on every axis and all 8 corner weights are
 *   >= min_weight (dgr_mesh_plan's cell validity).  Its value F is the trilinear interpolant of the 8 tsdf values.
 * Decision: k* = the smallest k whose sample is valid with F <= 0.  None: a miss, flags = 0.  If k* >= 1 and sample k* - 1 is
 *   valid with F > 0: a hit, flags bit 0.  Otherwise the ray ends there unseen, flags bit 1, no depth: it started inside the
 *   surface or came out of unmeasured space behind it.  Nothing else ends a ray.  (Samples outside the lattice are invalid: the
 *   march starts at the box and stops behind it, which is no part of the rule.  depth_max may be INFINITY.)
 * A hit's outputs: depth z* = z_(k*-1) + step F_(k*-1) / (F_(k*-1) - F_k*), p* the world point there.  Normal: the central
 *   differences of the same validity-checked interpolant F at p* +- voxel_size along each world axis, normalised, rotated by R
 *   into the camera frame and turned to face the camera (n . p_c <= 0) as dgr_depth_normals does; if one of the six evaluations
 *   is invalid or the gradient is zero, infinite or NaN: flags bit 2, the normal stays zero, depth and colour are still written.
 *   Colour: plain trilinear interpolation of the colour volume in p*'s cell (which exists: both ends of the segment lie in the
 *   lattice's convex cell range); the weights are NOT consulted for the colour.
 * Outputs, each may be NULL but not all: depth [n_views, height, width], 0 without a hit (the sensor's "invalid"); vnmap
 *   [n_views, height, width, 4] = (n_c, z*), what dgr_depth_normals writes and dgr_icp_step reads, four zeros without a hit or
 *   without a normal, 16-byte aligned; color_out [n_views, 3, height, width], 0 without a hit; flags uint8 [n_views, height, width].
 * NaN poses and NaN volume entries end in misses or garbage values, never in an out-of-range read: comparisons are made in float
 *   (false on a NaN) and the integer indices are tested again before every gather.
 * Empty-space skipping: a brick is 8 x 8 x 8 cells; bricks uint8 [ceil((nz-1)/8), ceil((ny-1)/8), ceil((nx-1)/8)], 1 iff the brick
 *   contains a valid cell (for the min_weight given) with at least one corner tsdf <= 0 -- only such a cell can hold a valid sample
 *   with F <= 0, a trilinear value never lying below its corners' minimum.  dgr_tsdf_bricks builds it in one launch (comparisons
 *   and integer logic, no atomics); dgr_tsdf_brick_bytes(grid) is its size (0 for a grid the library refuses, and for one without
 *   a cell).  dgr_tsdf_raycast takes the map or NULL; with it, runs of samples whose cells lie in dead bricks are jumped over, and
 *   the outputs are the SAME BITS as without: every surviving sample is computed from its own k, a jump is checked against the
 *   sample it would skip last and the sample landed on has its brick tested again, and sample k* - 1 is evaluated for real
 *   wherever it lies.  The map must have been built from this volume with this min_weight.
 * One lane per ray, every view in one launch; nothing allocated, nothing read on the host: capturable into a hipGraph.
 * Refused with DGR_ERR_BAD_ARGUMENT and a message before any device call: a NULL grid, params, volume or viewmatrices; a grid
 *   dgr_tsdf_integrate refuses; fx, fy or step not finite and positive; a NaN min_weight, a NaN depth_max, a depth_min that is not
 *   finite; n_views < 1 (or > 65535), width or height < 1; no output at all; color_out without a colour volume; a misaligned
 *   pointer (vnmap and color 16 bytes, volume 8); (bricks) a NULL bricks for a grid with cells. */
typedef struct dgr_raycast_params {
    float fx, fy, cx, cy;
    float depth_min, depth_max; /* the samples' z-depths: depth_min + k step < depth_max */
    float step;                 /* > 0, metres of z-depth */
    float min_weight;           /* a cell counts when its 8 weights are >= this */
} dgr_raycast_params;
size_t dgr_tsdf_brick_bytes(const dgr_tsdf_grid* grid);
int dgr_tsdf_bricks(void* stream, const dgr_tsdf_grid* grid, const float* volume, float min_weight, unsigned char* bricks);
int dgr_tsdf_raycast(void* stream, const dgr_tsdf_grid* grid, const float* volume, const float* color /* or NULL */,
                     const unsigned char* bricks /* or NULL */, int n_views, int width, int height, const float* viewmatrices,
                     const dgr_raycast_params* params, float* depth /* or NULL */, float* vnmap /* or NULL */,
                     float* color_out /* or NULL */, unsigned char* flags /* or NULL */);

/* Exact k-nearest-neighbour search: which points lie next to this one (simple-knn's distCUDA2 is self mode with k = 3,
 * exclude_self and the mean_dist2 output; per-point neighbourhoods for G-ICP covariances, outlier removal and duplicate
 * suppression use the indices, the radius and queries of their own).
 * THE RULE (normative: the index below only finds this answer faster, it cannot change a bit of it).
 *   points [P,3] float32, contiguous.  A point with a non-finite coordinate is INVALID: it is never indexed and never returned.
 *   queries [Q,3] float32, or NULL = SELF MODE: the queries are the indexed points, query i is point i (n_queries = n_points).
 *   distance, in fp32, every operation rounded once (to nearest even) and nothing contracted:
 *       dx = px - qx, dy = py - qy, dz = pz - qz;   d2 = ((dx dx) + (dy dy)) + (dz dz)
 *     (__fsub_rn, __fmul_rn, __fadd_rn), so that a float32 numpy twin reproduces d2 bit for bit.  d2 may be +inf for huge
 *     coordinates; it is never NaN for finite inputs.
 *   candidates are totally ordered by (d2, index): d2 as a float compare, then the index ascending.
 *   a candidate is admitted iff d2 <= max_dist2 (default +inf, which admits d2 = +inf) and, in self mode with exclude_self,
 *     its index differs from the query's (other coincident points stay, with d2 = 0).
 *   the result of a query is the first k admitted candidates in that order, ascending; 1 <= k <= DGR_KNN_MAX_K.
 *   outputs, each optional (NULL): dist2 [Q,k] float32; idx [Q,k] int32, indices into the caller's points; count [Q] int32, the
 *     number of neighbours found; mean_dist2 [Q] float32 = the k distances added left to right in ascending order (__fadd_rn),
 *     then one division (__fdiv_rn) by (float)k.  Slots beyond count hold idx = -1 and dist2 = +inf, and mean_dist2 is then
 *     +inf.  A query with a non-finite coordinate gets count = 0 (in self mode an invalid point is such a query).  Nothing else
 *     is written.
 *   distCUDA2(points) = self mode, k = 3, exclude_self, mean_dist2.  With fewer than four valid points it is +inf here
 *     (simple-knn returns a FLT_MAX-derived value there); the yardstick is the brute-force model of the rule (tests/knn_model.py),
 *     no bit parity with simple-knn is claimed.
 * dgr_knn_build writes the opaque `index` (dgr_knn_index_bytes(n_points) bytes, 16-byte aligned) from `points`: the box of the
 *   valid points, a 30-bit Morton key per point on it (an axis of zero or non-finite extent quantises to 0), a stable radix sort of
 *   (key, index), the sorted (x, y, z, index) records and, per leaf of 256 consecutive records, its exact fp32 box.  The index
 *   holds a copy of the coordinates: a search answers for the points as they were when the index was built.  dgr_knn_search's
 *   `points` is therefore not read by the launch: it is reserved (the tensor the indices refer to), and only checked for NULL.
 * dgr_knn_search: one lane per query, 64 queries that are consecutive in Morton order per wave (cross mode: the queries are keyed
 *   on the index's box and sorted by the same sort, and the results go back to the caller's rows).  A wave starts at its own leaf
 *   and sweeps the leaves outwards; a leaf is skipped only when bound > limit, where bound is the SAME rounded formula at the
 *   box's nearest point (per-axis gap max(0, lo - q, q - hi) by one rounded subtraction; rounding is monotone, so the bound never
 *   exceeds the fp32 d2 of a point inside) and limit is the smaller of max_dist2 and the lane's current k-th d2.
 * `scratch`: dgr_knn_scratch_bytes(n_points, n_queries) bytes, 16-byte aligned; nothing in it is kept between calls (a build
 *   needs no more than dgr_knn_scratch_bytes(n_points, 1)).  Both size functions return 0 for a shape they refuse.
 * Launch properties: nothing read on the host, every size known from n_points, n_queries and k, integer atomics only, no
 *   spin-wait and no grid barrier (the phases are separate launches), every loop bounded by the number of leaves or a leaf's
 *   count, the same bits on every run, capturable into a hipGraph (`points` and `queries` are read at replay).
 * Limits: n_points, n_queries <= 2^24.  The worst case per query is O(n_points) -- an outlier that stretches the box, all points
 *   coincident, or d2 = +inf neighbours, which no bound can prune: slow, and still the exact answer.
 * Refused with DGR_ERR_BAD_ARGUMENT and a message before any device call: n_points or n_queries outside 1 .. 2^24 (self mode:
 *   n_queries != n_points); k outside 1 .. 16; a NULL index, points, params or scratch; an index or scratch that is not 16-byte
 *   aligned; all four outputs NULL; a NaN or negative max_dist2; exclude_self with queries given. */
#define DGR_KNN_MAX_K 16
typedef struct dgr_knn_params {
    int k;            /* 1 .. DGR_KNN_MAX_K */
    int exclude_self; /* self mode only: the query's own index is not a candidate */
    float max_dist2;  /* admitted: d2 <= max_dist2; +inf admits everything */
} dgr_knn_params;
size_t dgr_knn_index_bytes(int n_points);
size_t dgr_knn_scratch_bytes(int n_points, int n_queries);
int dgr_knn_build(void* stream, int n_points, const float* points, void* index, void* scratch);
int dgr_knn_search(void* stream, const void* index, int n_points, const float* points, int n_queries,
                   const float* queries /* NULL: self mode */, const dgr_knn_params* params, void* scratch,
                   float* dist2 /* or NULL */, int* idx /* or NULL */, int* count /* or NULL */, float* mean_dist2 /* or NULL */);

/* ---- generalized ICP over the kNN index: neighbourhood covariances and a fused Gauss-Newton step (csrc/gicp.hip) ----
 * Segal's Generalized ICP: nearest-neighbour association in 3-D, a covariance per point, and the 6 x 6 step over
 * sum e^T (C_B + R C_A R^T)^-1 e.  It aligns two clouds that need not overlap pixel for pixel: the loop edges that
 * dgr_pgo_solve is fed, and GS-ICP SLAM's scan-to-map tracker (a map's own Sigma = R S S^T R^T as the target side).  No host
 * read, no float atomics, no spin-wait, the same bits on every run, capturable into a hipGraph.
 *
 * dgr_point_covariances: ONE launch, one thread per point.  points [n_points,3] float32; idx [n_points,k] int32 as
 * dgr_knn_search writes it, 1 <= k <= DGR_KNN_MAX_K.  A row's NEIGHBOURHOOD is its leading entries in [0, n_points): the first
 * entry outside that range (-1 among them) ends the list, and nothing is read out of bounds.  Whether the point itself is among
 * them is the caller's choice (self mode with or without exclude_self).  With n the neighbourhood's size, in double from the
 * first operation (the fp32 coordinates widened), nothing contracted:
 *   mu = (1/n) sum p_j, j in the row's order;   C = (1/n) sum (p_j - mu)(p_j - mu)^T in the same order
 *   eigenpairs of C by cyclic Jacobi: V = I, then sweeps over the pairs (0,1), (0,2), (1,2) in that order.  A pair with
 *     a_pq == 0 is skipped; otherwise theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) with
 *     sgn(0) = +1, c = 1 / sqrt(t^2 + 1), s = t c;  a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0;  with r the third index
 *     a_rp' = c a_rp - s a_rq, a_rq' = s a_rp + c a_rq;  V's columns p, q likewise.  The sweeps end when the three off-diagonal
 *     entries are exactly zero, or after 16 sweeps (quadratic convergence reaches exact zeros in 6 to 10 on a covariance whose
 *     entries are not denormal; 16 is the fixed bound).
 *   the eigenvalues (A's diagonal) are clamped at 0 and sorted ascending with their columns, ties keeping column order:
 *     lambda_0 <= lambda_1 <= lambda_2, v_0 the normal's axis.
 * A row is INVALID when its own point or a point of its neighbourhood has a non-finite coordinate, n < min_neighbours, or
 * lambda_2 is 0 (or not finite): all its outputs are +0 and its flag 0.  Outputs, each optional (NULL):
 *   cov [n_points,8] float32, 16-byte aligned rows (c00, c01, c02, c11, c12, c22, sigma, n): sigma = lambda_0 / (lambda_0 +
 *     lambda_1 + lambda_2) (the surface variation), n the neighbourhood's size as a float, 0 = invalid.  mode DGR_COV_RAW: C
 *     rounded once; DGR_COV_PLANE (GICP's (epsilon, 1, 1) replacement): I - (1 - epsilon) v_0 v_0^T, rounded once.
 *   normals [n_points,4] = (v_0, sigma): v_0 turned so that v_0 . (viewpoint - p) >= 0 with has_viewpoint (with the viewpoint
 *     at the origin of a camera-frame cloud: dgr_depth_normals' facing convention), otherwise so that its largest-magnitude
 *     component (the first such) is positive.
 *   log_scales [n_points,3] = 0.5 log(max(lambda, scale_floor^2)), largest first, and quats [n_points,4] (r, x, y, z; unit,
 *     r >= 0) of the frame (v_2, +-v_1, the oriented v_0), v_1's sign chosen for det +1: the anisotropic Gaussian the
 *     neighbourhood spans (GS-ICP SLAM's seeds; dgr_knn_search's mean_dist2 gives only an isotropic scale).
 *   flags [n_points] bytes: bit 0 valid.
 * Refused with DGR_ERR_BAD_ARGUMENT and a message before any device call: n_points outside 1 .. 2^24; k outside 1 .. 16; a NULL
 * points, idx or params; all five outputs NULL; cov not 16-byte aligned; an unknown mode; epsilon not in (0, 1];
 * min_neighbours < 3 or > k; a NaN scale_floor; with has_viewpoint a NaN in viewpoint. */
#define DGR_COV_RAW 0
#define DGR_COV_PLANE 1
typedef struct dgr_covariance_params {
    int mode;            /* DGR_COV_RAW or DGR_COV_PLANE */
    float epsilon;       /* (0, 1]: the variance along the normal in PLANE mode (GICP: 1e-3) */
    int min_neighbours;  /* 3 .. k */
    float scale_floor;   /* the smallest standard deviation log_scales reports (its square is the floor on lambda) */
    float viewpoint[3];
    int has_viewpoint;   /* 0: viewpoint is not read */
} dgr_covariance_params;
int dgr_point_covariances(void* stream, int n_points, const float* points, int k, const int* idx,
                          const dgr_covariance_params* params, float* cov /* or NULL */, float* normals /* or NULL */,
                          float* log_scales /* or NULL */, float* quats /* or NULL */, unsigned char* flags /* or NULL */);

/* dgr_gicp_step: one Gauss-Newton iteration in one C call.  Inputs: target_index, what dgr_knn_build made of target
 * [n_target,3]; target_cov [n_target,8] or NULL and source_cov [n_source,8] or NULL, rows as dgr_point_covariances packs them
 * (any symmetric positive C with n > 0 will do: a Gaussian map's own covariances); source [n_source,3]; transform_in[16], which
 * maps source to target coordinates, stored transposed with the translation at [12..14] (R[j][c] at [4 c + j]): dgr_pgo_solve's
 * measurement layout, so that with the source a cloud in camera j's frame and the target one in camera i's the result is Z_ij.
 * Launches, no host read between them:
 *   1. gicp_transform_kernel: q_i = R a_i + t into the scratch, in fp32 with every operation rounded once (__fmul_rn,
 *      __fadd_rn): q_i0 = ((R00 a0 + R01 a1) + R02 a2) + t0 and likewise; R and t are transform_in's bits.  A non-finite
 *      source row stays non-finite.
 *   2. dgr_knn_search's launches in cross mode with queries q, k = 1 and max_dist2 = the fp32 product dist_max * dist_max,
 *      writing idx to the scratch (or idx_out [n_source] when given): the association is the kNN rule's answer bit for bit.
 *   3. gicp_step_kernel, of dgr_icp_step's shape: a workgroup of 256 threads per block of 2048 sources, a thread's sources
 *      ascending, the workgroup's threads by the block sum, one 256-byte row per block, the blocks in block order.
 * A source i is VALID when q_i is finite and, with source_cov, its own row has n > 0; ASSOCIATED when valid, j = idx[i] >= 0
 * and, with target_cov, the target's row j has n > 0.  Per associated pair, in double from the widened fp32 inputs:
 *   e = q - b_j;  C = C_B + R C_A R^T (a NULL side contributes nothing; both NULL: C = I, point-to-point ICP)
 *   M = adj(C) / det(C); det <= 0 or not finite: the pair is SINGULAR and dropped
 *   s^2 = max(e^T M e, 0), s = sqrt(s^2);  w = 1 for s <= huber_delta, else huber_delta / s
 *   J = [-[q]x | I]: the left perturbation T <- exp(xi) T, the rotation part first
 * Sums in dgr_icp_step's layout and double accumulation: the 21 upper-triangle entries of A = sum w J^T M J (row-major), the
 * 6 of b = sum w J^T M e, sum w s^2, the count.  Solve, one thread in double: dgr_icp_step's -- M xi = -b by LDL^T on A + damping
 * diag(max(A_ii, 1e-3 max A_ii)); refused when count < min_points, a pivot <= rcond max A_ii, or anything is not finite.
 * T_out = exp(xi) T_in, its rotation re-orthonormalised through its unit quaternion.
 * Outputs: transform_out[16] (may be transform_in: the finishing workgroup reads before it writes); quat_out[4] (r, x, y, z;
 * unit, r >= 0) and trans_out[3] or NULL; stats, 32 doubles in dgr_icp_step's order: A (21), b (6), sum w s^2 [27], count [28],
 * ok [29], |omega| [30], |v| [31]; flags [n_source] bytes or NULL: bit 0 valid, bit 1 associated, bit 2 singular.  A refused
 * step writes the input's bits to every pose output (quat_out derived from the input matrix).
 * `scratch`: dgr_gicp_scratch_bytes(n_target, n_source) bytes (0 for a shape it refuses), 16-byte aligned.  Its first 16 bytes
 * hold the ticket and MUST BE ZERO before the first call that uses it; every call leaves them zero, so one zero-filled
 * allocation of the largest shape serves any number of calls in stream order, and a recorded graph replays.  The scratch belongs
 * to the call while it is in flight, as dgr_knn_search's does: the search sorts the queries' rows through it and reads them back
 * as indices, so nothing else may write it (a zero-fill still pending on another stream included) until the call has finished.
 * Refused with a message before any device call: n_target or n_source outside 1 .. 2^24; a NULL target_index, target, source,
 * transform_in, params, scratch, transform_out or stats; target_index, target_cov, source_cov or scratch not 16-byte aligned,
 * stats not 8-byte aligned; dist_max, huber_delta, damping or rcond NaN or negative; min_points < 1. */
typedef struct dgr_gicp_params {
    float dist_max;     /* >= 0: largest |q - b| of an association (INFINITY: the nearest target point whatever its distance) */
    float huber_delta;  /* >= 0 on s, the Mahalanobis length; INFINITY = least squares */
    float damping;      /* >= 0; 0 = Gauss-Newton */
    float rcond;        /* >= 0: smallest pivot accepted, relative to the largest diagonal entry of A */
    int min_points;     /* >= 1 */
} dgr_gicp_params;
size_t dgr_gicp_scratch_bytes(int n_target, int n_source);
int dgr_gicp_step(void* stream, const void* target_index, int n_target, const float* target, const float* target_cov /* or NULL */,
                  int n_source, const float* source, const float* source_cov /* or NULL */, const float* transform_in,
                  const dgr_gicp_params* params, void* scratch, float* transform_out, float* quat_out /* or NULL */,
                  float* trans_out /* or NULL */, double* stats, int* idx_out /* or NULL */, unsigned char* flags /* or NULL */);

/* Process-wide options (default 0 unless stated).
 *  "alpha_mode": how the blend kernels evaluate alpha = min(0.99, o exp(power)) and T / (1 - alpha).  0 (default) = the
 *     reference's expression in the reference's association (forward.cu:354-364, backward.cu:561-570) with an expf and a
 *     division whose bits the CPU restatement reproduces on any host (csrc/exact_math.h: an fp32-only polynomial expf,
 *     <= 0.9 ulp -- as faithful to nvcc's <= 2-ulp expf as any other; the correctly rounded quotient): the alpha image,
 *     n_contrib and the median depth are bit-identical to the restatement and the gradients agree with it to 1e-5 abs
 *     (BASELINE's loss scaling).
 *     1 = log2(e)-scaled conic, v_exp_f32, v_rcp_f32: each operation good to an ulp and the blend kernels faster, but
 *     the light backward's T_final = 1 - alpha image and its divisions by (1 - alpha) amplify last-bit differences: up to
 *     6e-5 abs on the pose gradient at BASELINE config 3.
 *     2 = as 0 with glibc's expf algorithm evaluated in the double pipe (rounds 5-7's default; slower), kept for A/B.
 *     Forward and backward of a view must run in the same mode.
 *  "fast_alpha": the older name of alpha_mode 0 / 1 (get: 1 iff alpha_mode == 1).
 *  "deterministic_grads": 1 = the light backward (one-view entry point, alpha_mode 0) forms its gradients without order-dependent
 *     float atomics: every quadrant wave of a tile keeps its own accumulators (added in wave order), every (tile, Gaussian) pair
 *     stores its finished row into an instance-major buffer (zero-filled first) and a Gaussian's rows are added in ascending tile
 *     order; the pose gradient's block partials are stored per block and added in block order.  Two runs give the same bits; the
 *     reference's own result, float atomics in arrival order (L/cuda_rasterizer/backward.cu:593-596, 666-680), lies within its
 *     run-to-run spread of it.  Costs about a quarter of the backward at config 3 (profiles/r8/deterministic.txt).  Needs
 *     dgr_light_backward_scratch_bytes_r() of scratch.  The full variant and the batched entry points (both variants) use the
 *     same scheme per view.
 *  "pose_grad" (default 0; DGR_POSE_GRAD = 0 / 1 in the environment sets the initial value): 0 = the reference's pose gradient
 *     (dL_dview from the mean2D path and the depth sum only); 1 = the complete pose gradient: dL_dview is the view-matrix
 *     counterpart of the dL_dmeans3D the same backward returns -- the ndc terms from its mean2D sums, the z path from its depth
 *     sums (light: depth, variance and median; full: the depth term of computeCov2DCUDA), the 2D covariance through Rcam in
 *     A = Ju Rcam and through t_cam in Ju, and the SH colour through campos.  It keeps the variant's quirks (straight-through
 *     alpha clamp, the clamp of t.x/t.z and t.y/t.z, the light median criterion, the full variant's uncertainty consumed as a
 *     variance), so for a rigid view dL_dview[12..14] = Rcam sum_g dL_dmeans3D[g] to float rounding.  Entries 3, 7, 11, 15 stay
 *     0; the per-Gaussian outputs are unchanged; track_off = 1 makes it a no-op.  The library differentiates campos as
 *     -Rcam^T t of the view matrix while using the campos passed to the forward: the derivative is exact for callers that pass a
 *     consistent campos.  A light map_off backward then runs the mapping blend backward and drops its per-Gaussian outputs.
 *     The ndc rows take their full derivative, m_w perspec[4 j + r] - m_hom.r m_w^2 perspec[4 j + 3], so an off-centre
 *     principal point (perspec[8], perspec[9]) is exact too.  The default mode keeps the reference's symmetric-frustum Jacobian
 *     (perspec[0] and perspec[5] only, L/cuda_rasterizer/backward.cu:725-739): its pose gradient is not exact for an
 *     off-centre projection, and pose_grad = 1 is.  Other values: DGR_ERR_BAD_ARGUMENT.
 *  "silhouette_grad" (default 0; DGR_SILHOUETTE_GRAD = 0 / 1 sets the initial value): the BINDINGS' switch for the exact gradient
 *     of the silhouette A = sum_k alpha_k T_k (light: opacity_map; full: the uncertainty output).  No entry point reads it; it
 *     lives here, per process and per thread and in the options word, so that both bindings and a tracker and a mapper thread
 *     share one value and a backward runs under its forward's snapshot.  1: the bindings call the dgr_*_backward*_silhouette
 *     entry points below with that output's gradient as the silhouette image (full: and NULL as dL_duncertainties).  0: they pass
 *     no image (light: the opacity_map gradient is dropped, as the reference does; full: it goes to dL_duncertainties, the
 *     reference's variance form).  Other values: DGR_ERR_BAD_ARGUMENT.
 *  "tight_cull": 1 = alpha-aware tile rectangles.  The reference gives a Gaussian every tile its
 *     3-sigma_max circle touches (cuda_rasterizer/forward.cu:229-237, auxiliary.h:46-56); with this option the rectangle
 *     is cut down to the box where alpha can reach 15/255.  Images and gradients are unchanged, but num_rendered, the
 *     tile lists and n_contrib are NOT the reference's any more -- hence opt-in.
 *  "tile_schedule" (default 2): whether the forward builds the blend kernels' tile schedule (classes of long lists first, so that
 *     a cluster's long lists start first and every XCD gets its share of them: 2x on the blend kernels of a clustered frame).
 *     1 = always, 0 = never (static map: every XCD a contiguous band of the image), 2 = by the frame: a forward whose status
 *     came back through dgr_status_arm also reports its longest tile list, and the next forward of that shape (device, P, width,
 *     height) skips the schedule kernel when that list was within twice the mean + 32 -- on an even frame the schedule is a
 *     launch and 11 us in front of the blend for nothing.  Forwards that report nothing keep it.  Results never depend on it.
 *  "lane_lists" (default 2): the lists the LIGHT blend kernels walk.  1 = one list per half of a quadrant wave (forward, tracking
 *     backward) and paired lists (mapping backward); 0 = one list per quadrant wave (rounds 1-7); 2 = by the FRAME, on the device:
 *     the binning kernels flag a frame of big splats (more than ten tiles per Gaussian on screen, profiles/r9/lists_sweep.txt), where
 *     nearly every entry lives in both halves of its quadrant and the finer lists cost 3 % for nothing, in the frame's state;
 *     forward and backward branch on that word.  Images never depend on it; gradients differ by summation order only.
 *     (DGR_FWD_HALVES = 0 / 1 in the environment sets the initial value.)
 *  "lds_count" (default 1): how the forward bins a frame's tile instances.  1 = the two-level segment binning
 *     (csrc/segment_binning.hip: pairs per 16-, 8- or 4-tile row segment, tile lists built and sorted in LDS; no global
 *     atomics, no cleared counters) whenever the frame's segment tables fit LDS (up to 8 192 four-tile segments, i.e.
 *     3840x2160 and a little beyond); 0 = returning global atomics on per-tile counters (csrc/binning.hip, round 2's path),
 *     which also serves larger frames.  Results are identical bit for bit.  dgr_binning_bytes() includes the segment
 *     binning's forward-only tables.
 *  "blend_wgs_per_cu" (default 0 = no cap; 3..7): at most this many blend workgroups per CU (they are padded with unused
 *     LDS), which leaves wave slots, registers and LDS for kernels of other streams -- collectives, other views' bandwidth-
 *     bound kernels -- that otherwise enter a CU only as blend workgroups drain.  Costs the blend kernels 3-7 % at 7.
 *  "profile_every": n >= 1 = dgr_profile_* brackets every n-th launch of the selected stage only (default 1).
 *  "batch_streams" (default 2): streams the batched entry points spread the per-view stages of a batch over (1..8).
 *  "batch_order" (default 0): 0 = view v's binning + blend chain on stream v mod batch_streams; 1 = all binning stages on a
 *     helper stream and all blend stages on the caller's, joined per view by events (measured slower: csrc/api.hip).
 * (csrc/options.h holds the table of these options: a new one is a row there and a line here.) */
int dgr_set_option(const char* name, int value);
int dgr_get_option(const char* name);

/* Per-THREAD values of the options that change what a call computes -- "alpha_mode" (and its older name "fast_alpha"),
 * "tight_cull", "deterministic_grads", "pose_grad", "silhouette_grad" -- overriding the process-wide ones above for the calling thread's next calls (value < 0:
 * inherit again).  A tracker and a mapper thread of one process hold different settings this way, and nothing a thread sets
 * reaches launches that are already queued: every entry point reads its options once, when it is called.  (The reference has
 * no options; its one compile-time choice is the variant.)  dgr_get_thread_option = the value the calling thread's next call
 * uses.  dgr_thread_options_effective() packs the five (each field value + 1: bits 0-3 alpha_mode, 4-7 tight_cull, 8-11
 * deterministic_grads, 12-15 pose_grad, 16-19 silhouette_grad) and dgr_thread_options_swap(word) installs such a word as the thread's overrides (field 0 = inherit;
 * word < 0: only read) and returns the previous one -- what an autograd binding uses to run a backward, on whatever thread the
 * engine picks, under its forward's options.  DGR_OPT_SHIFT_*: the fields' first bits. */
#define DGR_OPT_SHIFT_ALPHA_MODE 0
#define DGR_OPT_SHIFT_TIGHT_CULL 4
#define DGR_OPT_SHIFT_DETERMINISTIC_GRADS 8
#define DGR_OPT_SHIFT_POSE_GRAD 12
#define DGR_OPT_SHIFT_SILHOUETTE_GRAD 16
int dgr_set_thread_option(const char* name, int value);
int dgr_get_thread_option(const char* name);
int dgr_thread_options_effective(void);
int dgr_thread_options_swap(int word);

/* ---- work shared by the views of a batch ----
 * The 3D covariance depends on scale and rotation only.  dgr_cov3d_forward evaluates computeCov3D (cr/forward.cu:118-152)
 * once -- bit-identical to what the forward would compute per view -- for use as `cov3D_precomp` of every view of the batch;
 * dgr_cov3d_backward is its backward (L/cr/backward.cu:280-343), linear in dL_dcov3D: sum the views' dL_dcov3D first, convert
 * once.  scales [P,3], rotations [P,4] (r,x,y,z; not normalised), cov3D / dL_dcov3D [P,6], dL_dscales [P,3], dL_drotations [P,4]. */
int dgr_cov3d_forward(void* stream, int P, const float* scales, const float* rotations, float scale_modifier, float* cov3D);
int dgr_cov3d_backward(void* stream, int P, const float* scales, const float* rotations, float scale_modifier,
                       const float* dL_dcov3D, float* dL_dscales, float* dL_drotations);

/* ---- batched multi-view entry points (BASELINE configs 4 and 5: several cameras over ONE set of Gaussians) ----
 * The reference renders a keyframe batch as V independent Rasterizer::forward / backward calls (L/cr/rasterizer.h:40-104) and
 * lets autograd add the V dense gradient sets.  Here one call takes the V cameras; per view it does exactly what
 * dgr_light_forward_presized / dgr_light_backward do (every view's outputs and state buffers are bit-identical to a one-view
 * call, and usable by one), but the work that does not depend on the camera is shared:
 *  - forward: ONE per-Gaussian launch for all views -- position, opacity, 3D covariance formed once, the 192-byte SH row
 *    fetched once and evaluated for every camera that sees the Gaussian;
 *  - backward: ONE per-Gaussian launch that sums the views' gradients of the shared Gaussians in registers and writes each
 *    dense row (248 bytes per Gaussian at SH degree 3) once instead of V times plus V - 1 accumulation passes; the covariance
 *    backward (linear in dL_dcov3D) runs once on the sum.  Given the same per-view accumulator rows, dL_dopacity / dL_dmean3D /
 *    dL_dsh / dL_dcov3D are the one-view outputs accumulated in view order, operation for operation; dL_dscale / dL_drot agree
 *    to rounding (converted once, not V times).  (Two runs of the blend backward -- batched or not -- leave accumulator rows
 *    that differ by the arrival order of their float atomics, so two runs agree to ~1e-6 of a tensor's scale, not bitwise);
 *  - the per-view stages in between (binning and blend) are issued on internal streams forked from and joined to `stream`
 *    with events (option "batch_streams", 1..8, default 2: one view's binning runs under another view's blend);
 *  - no host synchronisation (hipGraph-capturable after one warm-up call, which creates the internal streams).
 * All views share the image size, tan_fovx / tan_fovy, background and the Gaussians; `views` is a HOST array of n_views
 * (1 .. DGR_MAX_BATCH_VIEWS) structs of DEVICE pointers, read during the call only.  Light variant (the full variant's
 * entry points follow below). */
#define DGR_MAX_BATCH_VIEWS 8
typedef struct dgr_light_view {        /* the per-camera arguments of dgr_light_forward_presized, same meaning */
    char* geometry_buffer;
    char* binning_buffer;
    int binning_capacity;
    char* image_buffer;
    int* status;                        /* device int[4] or NULL */
    const float* viewmatrix;
    const float* projmatrix;
    const float* cam_pos;
    float* out_color;
    float* out_depth;
    float* out_median_depth;
    float* out_alpha;
    const float* gt_depth;
    float* out_depth_var;
    float* gau_uncertainty;
    int* gau_related_pixels;
    int* radii;                         /* may be NULL */
} dgr_light_view;
int dgr_light_forward_batch(void* stream, int n_views, const dgr_light_view* views, int P, int D, int M,
                            const float* background, int width, int height, const float* means3D, const float* shs,
                            const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                            const float* rotations, const float* cov3D_precomp, float tan_fovx, float tan_fovy, int prefiltered);

typedef struct dgr_light_view_grad {   /* the per-camera arguments of dgr_light_backward, same meaning */
    char* geometry_buffer;
    char* binning_buffer;
    char* image_buffer;
    const float* viewmatrix;
    const float* projmatrix;
    const float* cam_pos;
    const float* perspec_matrix;
    const float* alphas;
    const float* gt_depth;
    const int* radii;                   /* may be NULL (internal copy is used) */
    const float* dL_dpix;
    const float* dL_dpix_depth;
    const float* dL_dpix_median_depth;
    const float* dL_dpix_depth_var;
    float* dL_dmean2D;                  /* [P,3] of THIS view (densification statistics are per view); may be NULL */
    float* dL_dview;                    /* [16] of this view */
    char* scratch;                      /* dgr_light_backward_scratch_bytes(), one per view (deterministic_grads:
                                           dgr_light_backward_scratch_bytes_r(P, width, height, num_rendered)) */
    size_t scratch_bytes;
    int num_rendered;                   /* this view's R as passed to dgr_light_backward (>= its num_rendered); read only with
                                           deterministic_grads, where it sizes the view's instance-major row buffer */
} dgr_light_view_grad;
/* dL_dopacity [P], dL_dcolor [P,3] (may be NULL), dL_dmean3D [P,3], dL_dcov3D [P,6] (may be NULL), dL_dsh [P,M,3] (NULL when
 * M == 0), dL_dscale [P,3], dL_drot [P,4]: the SUM over the views.  Every one of them may be NULL (tracking: map_off = 1). */
int dgr_light_backward_batch(void* stream, int n_views, const dgr_light_view_grad* views, int P, int D, int M,
                             const float* background, int width, int height, const float* means3D, const float* shs,
                             const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                             const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity, float* dL_dcolor,
                             float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                             int track_off, int map_off);

/* ---- the same for the -full variant: dgr_full_forward_presized / dgr_full_backward per view, the contract above ----
 * Every view's outputs and state buffers are bit-identical to a one-view dgr_full_forward_presized call; the per-Gaussian
 * backward sums the full variant's per-view terms (computeCov2DCUDA with its depth term, the campos colour term of the pose
 * gradient) in view order in one launch.  status (device int[4] or NULL): {num_rendered, overflow, prefiltered violation,
 * num_related_primitives}.  "deterministic_grads" is supported (alpha_mode 0; per view num_rendered sizes the row buffer). */
typedef struct dgr_full_view {         /* the per-camera arguments of dgr_full_forward_presized, same meaning */
    char* geometry_buffer;
    char* binning_buffer;
    int binning_capacity;
    char* image_buffer;
    int* status;                        /* device int[4] or NULL */
    const float* viewmatrix;
    const float* projmatrix;
    const float* cam_pos;
    float* out_color;
    float* out_depth;
    const float* gt_depth;              /* accepted and unused by the forward, as there */
    float* out_uncertainty;
    int* radii;                         /* may be NULL */
} dgr_full_view;
int dgr_full_forward_batch(void* stream, int n_views, const dgr_full_view* views, int P, int D, int M,
                           const float* background, int width, int height, const float* means3D, const float* shs,
                           const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                           const float* rotations, const float* cov3D_precomp, float tan_fovx, float tan_fovy, int prefiltered);

typedef struct dgr_full_view_grad {    /* the per-camera arguments of dgr_full_backward, same meaning */
    char* geometry_buffer;
    char* binning_buffer;
    char* image_buffer;
    const float* viewmatrix;
    const float* projmatrix;
    const float* cam_pos;
    const float* perspec_matrix;
    const float* gt_depth;
    const int* radii;                   /* may be NULL (internal copy is used) */
    const float* dL_dpix;
    const float* dL_depths;
    const float* dL_duncertainties;     /* may be NULL: this view takes the lean blend backward (as dgr_full_backward) */
    float* dL_dmean2D;                  /* [P,3] of THIS view; may be NULL */
    float* dL_dview;                    /* [16] of this view */
    char* scratch;                      /* dgr_light_backward_scratch_bytes_r(P, width, height, num_rendered), one per view */
    size_t scratch_bytes;
    int num_rendered;                   /* this view's R as passed to dgr_full_backward; read only with deterministic_grads */
} dgr_full_view_grad;
/* dL_dopacity [P], dL_dcolor [P,3], dL_dmean3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3] (NULL when M == 0), dL_dscale [P,3],
 * dL_drot [P,4]: the SUM over the views; each may be NULL. */
int dgr_full_backward_batch(void* stream, int n_views, const dgr_full_view_grad* views, int P, int D, int M,
                            const float* background, int width, int height, const float* means3D, const float* shs,
                            const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                            const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity, float* dL_dcolor,
                            float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot);

/* ---- absgrad: the absolute screen-space gradient of AbsGS ("homodirectional" gradient; gsplat's absgrad) ----
 * Each function takes its namesake's arguments, in the same order, plus the absgrad output, and otherwise does exactly what its
 * namesake does.  For a Gaussian g, with v_p(g) the contribution of pixel p to g's dL_dmean2D[:2] (every term that reaches it
 * through alpha at p, the ndc scale W/2, H/2 included -- so sum_p v_p(g) is dL_dmean2D[g, :2]):
 *     dL_dmean2D_abs[g] = ( sum_p |v_p(g).x|, sum_p |v_p(g).y|, 0 )        float [P,3], written densely: rows the view did not
 * render and every z are 0.  It is a per-view quantity: the batch forms give one [P,3] per view and never sum them.
 * A NULL dL_dmean2D_abs (batch: a NULL array, or a NULL entry for that view) is exactly the namesake's behaviour.
 * DGR_ERR_BAD_ARGUMENT (before any device call) for a non-NULL absgrad output with map_off = 1 (tracking computes no per-Gaussian
 * gradients), with dgr_set_option("deterministic_grads", 1) (no deterministic form) or with alpha_mode 2 (the glibc A/B form).
 * Same contract as the namesakes: no host synchronisation, capturable into a hipGraph, P == 0 handled, helper streams rejoined. */
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
                               const float* gt_depth, int track_off, int map_off, char* scratch, size_t scratch_bytes,
                               float* dL_dmean2D_abs);
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
                              size_t scratch_bytes, float* dL_dmean2D_abs);
/* dL_dmean2D_abs: a HOST array of n_views device pointers (view v's [P,3] absgrad; each may be NULL), or NULL. */
int dgr_light_backward_batch_absgrad(void* stream, int n_views, const dgr_light_view_grad* views, int P, int D, int M,
                                     const float* background, int width, int height, const float* means3D, const float* shs,
                                     const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                                     const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity, float* dL_dcolor,
                                     float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                     int track_off, int map_off, float* const* dL_dmean2D_abs);
int dgr_full_backward_batch_absgrad(void* stream, int n_views, const dgr_full_view_grad* views, int P, int D, int M,
                                    const float* background, int width, int height, const float* means3D, const float* shs,
                                    const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                                    const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity, float* dL_dcolor,
                                    float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                    float* const* dL_dmean2D_abs);

/* ---- the exact silhouette gradient ----
 * Each function takes its _absgrad namesake's arguments, in the same order, plus dL_dpix_silhouette, and otherwise does exactly
 * what the namesake does.  dL_dpix_silhouette is an [H,W] device image dL/dA (one-view forms) or a HOST array of n_views such
 * device pointers (batch forms); the array may be NULL, and so may any entry.  A = sum_k alpha_k T_k is the pixel's silhouette
 * (light: the opacity_map output, 1 - T_final; full: the uncertainty output), and dA/dalpha_k = T_final / (1 - alpha_k) -- the
 * shape of the background term, so the blend backwards take it into that term's per-pixel constant:
 *     dL/dalpha_k += T_final (dL/dA - <bg, dL/dC>) / (1 - alpha_k)
 * and every gradient downstream of dL/dalpha carries it (means2D, conics, opacities, means3D, scales, rotations, the pose gradient,
 * absgrad).  A NULL image gives bit for bit what the namesake gives.  In the full variant dL_duncertainties keeps the reference's
 * meaning (the depth-variance form): a caller that wants the exact gradient passes NULL there and the image here; given both,
 * the two terms add.  Full-variant pose caveat: with pose_grad = 0 its dL_dview comes from the reference's colour-only and
 * front-most-depth sums, which no background share reaches -- so the silhouette term does not reach it either, and dL_dview is
 * the same with and without the image; with pose_grad = 1 it comes from the mean2D sums and carries the term.
 * Same contract as the namesakes: no host synchronisation, capturable into a hipGraph, P == 0 handled; absgrad's refusals only
 * when an absgrad output is given. */
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
                                  const float* gt_depth, int track_off, int map_off, char* scratch, size_t scratch_bytes,
                                  float* dL_dmean2D_abs, const float* dL_dpix_silhouette);
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
                                 size_t scratch_bytes, float* dL_dmean2D_abs, const float* dL_dpix_silhouette);
int dgr_light_backward_batch_silhouette(void* stream, int n_views, const dgr_light_view_grad* views, int P, int D, int M,
                                        const float* background, int width, int height, const float* means3D, const float* shs,
                                        const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                                        const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity,
                                        float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                                        float* dL_drot, int track_off, int map_off, float* const* dL_dmean2D_abs,
                                        const float* const* dL_dpix_silhouette);
int dgr_full_backward_batch_silhouette(void* stream, int n_views, const dgr_full_view_grad* views, int P, int D, int M,
                                       const float* background, int width, int height, const float* means3D, const float* shs,
                                       const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                                       const float* cov3D_precomp, float tan_fovx, float tan_fovy, float* dL_dopacity,
                                       float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                                       float* dL_drot, float* const* dL_dmean2D_abs, const float* const* dL_dpix_silhouette);

/* Debug: while `device_words` (8 x uint64 per bin_tiles workgroup, caller-owned device memory) is non-NULL, every bin_tiles
 * workgroup stores phase time stamps (100 MHz wall clock) and its segment's sizes there: profiles/r9/bin_tiles_trace.py. */
int dgr_debug_bin_tiles_trace(unsigned long long* device_words);

/* Self-test of the wave64 multi-value butterfly reductions the backward blend relies on (csrc/wave_reduce.h: within-row DPP
 * stages first, then v_permlane16/32_swap as inline asm).  `in` holds 16 values per lane as in[c * 64 + lane]; out16 /
 * out12 / out4 [lane] receive what each lane holds after the 16- / 12- / 4-value network (the 12- and 4-value ones read the
 * first 12 / 4 values), comp16 / comp12 / comp4 [lane] the index of the value that lane's total belongs to.  64 entries each. */
int dgr_debug_wave_reduce(void* stream, const float* in, float* out16, float* out12, float* out4, int* comp16, int* comp12,
                          int* comp4);
/* Self-test of the reductions per HALF of a wave (csrc/wave_reduce.h), which the blend backward uses where a loop step serves one
 * list entry on lanes 0-31 and another on lanes 32-63.  `in` holds 12 values per lane as in[c * 64 + lane].  r0 / r1 [lane]: what
 * the lane holds after the twelve-value network stopped before its cross-half stage, slot0 / slot1 [lane] the index of the value
 * that total belongs to (-1: none); h3 [lane]: after the three-value network of the tracking backward (the first three values),
 * comp3 [lane] the value index (-1: none).  64 entries each. */
int dgr_debug_half_reduce(void* stream, const float* in, float* r0, float* r1, float* h3, int* slot0, int* slot1, int* comp3);
/* ... and of the SIXTEEN-value network stopped before its cross-half stage (the paired step of the full variant's backward): `in`
 * holds 16 values per lane as in[c * 64 + lane]; r0 / r1 [lane] what the lane holds, slot0 / slot1 [lane] the value index. */
int dgr_debug_half_reduce16(void* stream, const float* in, float* r0, float* r1, int* slot0, int* slot1);
/* Self-test of the per-wave list builders of the blend kernels (csrc/render_common.h: build_paired_lists, build_half_lists) on one
 * batch of 128 staged slots.  codes[slot] (128 device bytes): bit 2 w + h set <=> half h (lanes 32 h ..) of quadrant wave w takes
 * the slot.  paired / halves (4 x 280 device words, one block per wave): {steps or length, split mask 0 lo, hi, split mask 1 lo,
 * hi, list 2 w [136], list 2 w + 1 [136]}; list entries are record offsets (32 x slot), 32 x 128 = the sentinel. */
int dgr_debug_lane_lists(void* stream, const unsigned char* codes, unsigned* paired, unsigned* halves);
/* Self-test of csrc/exact_math.h, the arithmetic behind the default alpha path: out_exp[i] = the current alpha mode's expf of
 * x[i] (mode 0: exp_p32, mode 2: exp_glibc; x <= 0, clamped at -104) and out_div[i] = div_ref(a[i], b[i]) -- correctly rounded
 * a / b for normal operands.  n device floats each.  tests/test_hip_exact_math.py compares both with the CPU restatement's
 * functions bit for bit. */
int dgr_debug_exact_math(void* stream, int n, const float* x, const float* a, const float* b, float* out_exp, float* out_div);
/* Self-test of csrc/tile_sort.h, the sorting routines of the binning kernels.  A batch of n_lists lists in ONE launch, a workgroup per
 * list: list b is keys[offsets[b] .. offsets[b + 1]) -- `keys` device memory, 64-bit (depth bits << 32 | id), unique; `offsets` a
 * HOST array of n_lists + 1 ascending ints.  Every routine runs as the binning kernels call it (bin_tiles' 512 threads with the keys
 * in LDS; the global sorts in place in device memory):
 *   DGR_TILE_SORT_WAVE        sort_tile_in_wave: one wave's register network, 1 .. 1024 keys; out_ids[offsets[b] + i] = the id (low
 *                             word) of the list's i-th smallest key.  (It picks sort_wave_trunc<NCH, true> with n > 32 NCH for every
 *                             NCH > 1, which that form's transposition of the ids through the list's own LDS bytes REQUIRES: never call
 *                             the ids form of a wider network on a shorter list.)
 *   DGR_TILE_SORT_PART        sort_list_part = sort_wave_trunc<8, false>: 1 .. 512 keys sorted in place; out_keys receives the list;
 *   DGR_TILE_SORT_MERGE       the long-list sequence: 512-key parts dealt to the waves, barrier, merge_list_parts<512>; 1025 .. 6144
 *                             keys; out_ids as above;
 *   DGR_TILE_SORT_GLOBAL      wg_sort_global<512> (bin_tiles' lists above its LDS budget), any length >= 1: out_keys receives a
 *                             copy of the list and is sorted in place;
 *   DGR_TILE_SORT_GLOBAL_256  the same with sort_tiles' 256 threads.
 * The output a mode does not write may be NULL.  A length outside a mode's range is refused (DGR_ERR_BAD_ARGUMENT).  The call
 * returns after the sort has finished.  tests/test_hip_tile_sort.py compares with a sort of the keys on the host. */
#define DGR_TILE_SORT_WAVE 0
#define DGR_TILE_SORT_PART 1
#define DGR_TILE_SORT_MERGE 2
#define DGR_TILE_SORT_GLOBAL 3
#define DGR_TILE_SORT_GLOBAL_256 4
int dgr_debug_tile_sort(void* stream, int mode, int n_lists, const unsigned long long* keys, const int* offsets, unsigned* out_ids,
                        unsigned long long* out_keys);

/* ---- per-stage timing (bench.py's roofline object) ----
 * dgr_profile_select("") disables timing (default), "all" brackets every stage, a stage name brackets that
 * stage only with two HIP events recorded on the launching stream.  Stage names: dgr_profile_stage_name(i),
 * i < dgr_profile_stage_count().  dgr_profile_read waits for the recorded events, returns their summed
 * duration and the number of launches since the previous read, and clears them. */
int dgr_profile_select(const char* stage);
int dgr_profile_stage_count(void);
const char* dgr_profile_stage_name(int i);
int dgr_profile_read(const char* stage, double* total_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* DGR_HIP_H */
