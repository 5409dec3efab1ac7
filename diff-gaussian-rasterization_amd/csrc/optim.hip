// optim.hip -- fused sparse Adam step for the Gaussian parameters, the densification statistics,
// and the step that consumes them: fused densify-and-prune (second half of this file).
//
// A mapping iteration ends with an optimiser step over the per-Gaussian tensors whose gradients the backward just
// wrote (for all views: after the all-reduce).  Only Gaussians some view saw have a gradient; as in 3DGS's sparse Adam
// the rows of the others are left alone: parameter AND both moments untouched.  One launch per tensor, element-
// parallel (row = element / k), so consecutive lanes touch consecutive addresses of all four streams.
// Traffic per updated element: param, grad, exp_avg, exp_avg_sq in; param, exp_avg, exp_avg_sq out = 28 bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "philox.h"
#include "plan.h"

namespace dgr {
namespace {

__global__ void __launch_bounds__(256) sparse_adam_kernel(size_t n, int k, float* __restrict__ param,
                                                          const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                          float* __restrict__ exp_avg_sq, const int* __restrict__ visible,
                                                          float step_size, float beta1, float beta2, float eps,
                                                          float inv_sqrt_bias2, float lr, const int* __restrict__ step_dev) {
    if (step_dev) {  // capturable form: the step count lives on the device, the bias corrections are formed here
        const float st = (float)*step_dev;
        step_size = lr / (1.0f - powf(beta1, st));
        inv_sqrt_bias2 = 1.0f / sqrtf(1.0f - powf(beta2, st));
    }
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        if (visible && visible[e / (size_t)k] <= 0) continue;
        const float g = grad[e];
        const float m = beta1 * exp_avg[e] + (1.0f - beta1) * g;
        const float v = beta2 * exp_avg_sq[e] + (1.0f - beta2) * g * g;
        exp_avg[e] = m;
        exp_avg_sq[e] = v;
        // torch.optim.Adam: p -= lr / bias1 * m / (sqrt(v) / sqrt(bias2) + eps)
        param[e] -= step_size * m / (sqrtf(v) * inv_sqrt_bias2 + eps);
    }
}

// 3DGS's densification bookkeeping after a view's backward (GaussianModel.add_densification_stats and the
// max_radii2D update of the training loop), for the rows the view saw: one pass instead of five indexed torch ops.
__global__ void __launch_bounds__(256) densification_stats_kernel(int rows, const float* __restrict__ dmeans2D,
                                                                  const int* __restrict__ radii,
                                                                  float* __restrict__ grad_accum, float* __restrict__ denom,
                                                                  float* __restrict__ max_radii2D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int r = radii[i];
    if (r <= 0) return;
    if (grad_accum) {
        const float gx = dmeans2D[3 * (size_t)i], gy = dmeans2D[3 * (size_t)i + 1];
        grad_accum[i] += sqrtf(gx * gx + gy * gy);
    }
    if (denom) denom[i] += 1.0f;
    if (max_radii2D) max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
}

}  // namespace

hipError_t launch_densification_stats(int rows, const float* dmeans2D, const int* radii, float* grad_accum, float* denom,
                                      float* max_radii2D, hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    launch(densification_stats_kernel, dim3((rows + 255) / 256), dim3(256), stream, rows, dmeans2D, radii, grad_accum, denom,
           max_radii2D);
    return hipGetLastError();
}

hipError_t launch_sparse_adam(size_t rows, int k, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                              const int* visible, float lr, float beta1, float beta2, float eps, int step,
                              const int* step_dev, hipStream_t stream) {
    const size_t n = rows * (size_t)k;
    if (n == 0) return hipSuccess;
    if (step < 1) step = 1;  // (unused with step_dev)
    const double bias1 = 1.0 - pow((double)beta1, (double)step), bias2 = 1.0 - pow((double)beta2, (double)step);
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 256 * 32);
    launch(sparse_adam_kernel, dim3(blocks), dim3(256), stream, n, k, param, grad, exp_avg, exp_avg_sq, visible,
           (float)((double)lr / bias1), beta1, beta2, eps, (float)(1.0 / sqrt(bias2)), lr, step_dev);
    return hipGetLastError();
}


// ---- fused densify-and-prune (3DGS's densify_and_clone, densify_and_split and prune_points as one step) ----
//
// Three launches.  decide: one thread per row -> an action byte (which of survivor / clone / child pair the row emits) and
// per-256-row block totals of the emit counts.  scan: one workgroup turns the block totals into exclusive offsets and the
// totals into counts[8].  apply: one launch moves every tensor of the model; a workgroup takes one 256-row block of one
// tensor, recomputes the rows' in-block ranks from the action bytes (ballot + mbcnt), then streams the block's elements.
// Positions come from the scan alone: no atomics, the output order is survivors, clones, children sample 0, children
// sample 1, each in row order.
//
// plan buffer (plan.h): one action byte per row.
namespace {

constexpr unsigned ACT_SURVIVE = 1u, ACT_CLONE = 2u, ACT_CHILDREN = 4u, ACT_SPLIT = 8u;
constexpr float LOG_1P6 = 0x1.e148a2p-2f;  // logf(1.6f)

// The per-row table, derived from the sequence clone -> split -> remove the split originals -> prune everything:
//   the original survives unless it is split or prunable (its own opacity, its carried max_radii2D, its own scale);
//   a clone carries max_radii2D = 0, so only opacity, the scale rule and 0 > max_screen_size can prune it;
//   both children carry the parent's opacity, max_radii2D = 0 and the scale m - log 1.6 (rounding is monotone: the
//   largest shifted component is the shifted largest component), so they share their fate.
// Every comparison is false on a NaN: a NaN accumulator is not hot, a NaN opacity is not pruned.
__global__ void __launch_bounds__(256) densify_decide_kernel(size_t rows, const float* __restrict__ grad_accum,
                                                             const float* __restrict__ denom,
                                                             const float* __restrict__ max_radii2D,
                                                             const float* __restrict__ opacity_raw,
                                                             const float* __restrict__ scaling_raw, float grad_threshold,
                                                             float opacity_raw_min, float log_scale_split,
                                                             float log_scale_prune, float max_screen_size, void* plan) {
    __shared__ int wave_tot[4][4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned act = 0;
    if (i < rows) {
        const float a = grad_accum[i], d = denom[i], op = opacity_raw[i];
        const float m = fmaxf(fmaxf(scaling_raw[3 * i], scaling_raw[3 * i + 1]), scaling_raw[3 * i + 2]);
        const float r = max_radii2D ? max_radii2D[i] : 0.0f;
        const bool hot = d > 0.0f && a >= __fmul_rn(grad_threshold, d);  // one rounded multiply, never an fma
        const bool split = hot && m > log_scale_split;
        const bool clone = hot && !split;
        const bool op_bad = op < opacity_raw_min;
        const bool new_bad = op_bad || 0.0f > max_screen_size;  // what a row with max_radii2D = 0 can be pruned for
        if (!split && !(op_bad || r > max_screen_size || m > log_scale_prune)) act |= ACT_SURVIVE;
        if (clone && !(new_bad || m > log_scale_prune)) act |= ACT_CLONE;
        if (split) {
            act |= ACT_SPLIT;
            if (!(new_bad || __fsub_rn(m, LOG_1P6) > log_scale_prune)) act |= ACT_CHILDREN;
        }
        plan_flags(plan, rows)[i] = (unsigned char)act;
    }
    const int4 t = block_flag_totals(act, wave_tot);
    if (threadIdx.x == 0) plan_block_table(plan)[blockIdx.x] = t;
}

// One workgroup: exclusive scan of the block totals in place (plan.h); then the counts.
__global__ void __launch_bounds__(256) densify_scan_kernel(size_t blocks, void* plan, int* __restrict__ counts) {
    __shared__ int4 wave_sum[4];
    const int4 carry = scan_block_totals(plan_block_table(plan), blocks, wave_sum);
    write_counts8(carry.x + carry.y + 2 * carry.z, carry.x, carry.y, 2 * carry.z, carry.w, plan, counts);
}

// The children's noise: philox_normal (philox.h), counter = (row, sample), components 0..2: the draw of a (row, sample) does not
// depend on the grid, the launch order or on which rows are split.

// component c of R(q / |q|) (exp(s) * n): 3DGS's build_rotation, q = (r, x, y, z)
__device__ inline float child_offset(const float* __restrict__ q4, const float* __restrict__ s3, float n0, float n1, float n2,
                                     int c) {
    float r = q4[0], x = q4[1], y = q4[2], z = q4[3];
    const float inv = 1.0f / sqrtf(r * r + x * x + y * y + z * z);
    r *= inv, x *= inv, y *= inv, z *= inv;
    const float v0 = expf(s3[0]) * n0, v1 = expf(s3[1]) * n1, v2 = expf(s3[2]) * n2;
    if (c == 0) return (1.0f - 2.0f * (y * y + z * z)) * v0 + 2.0f * (x * y - r * z) * v1 + 2.0f * (x * z + r * y) * v2;
    if (c == 1) return 2.0f * (x * y + r * z) * v0 + (1.0f - 2.0f * (x * x + z * z)) * v1 + 2.0f * (y * z - r * x) * v2;
    return 2.0f * (x * z - r * y) * v0 + 2.0f * (y * z + r * x) * v1 + (1.0f - 2.0f * (x * x + y * y)) * v2;
}

using DensifyTable = TensorTable<dgr_densify_tensor, DGR_DENSIFY_MAX_TENSORS>;  // (plan.h; a tensor's cost: elements per thread)

__device__ inline float shifted(float v) { return __fsub_rn(v, LOG_1P6); }
__device__ inline float4 shifted(float4 v) { return make_float4(shifted(v.x), shifted(v.y), shifted(v.z), shifted(v.w)); }
__device__ inline void set_zero(float& v) { v = 0.0f; }
__device__ inline void set_zero(float4& v) { v = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// What a block needs to place its rows: where its survivors, clones and children start, and how many of each fit below
// rows_out (the caller's allocation: nothing is written past it, whatever the plan says).
struct BlockPlace {
    size_t first[3], n_pairs;
    unsigned fit[3], fit_second;
};
__device__ inline unsigned rows_that_fit(size_t first, size_t rows_out) {
    return first >= rows_out ? 0u : (unsigned)(rows_out - first < 256 ? rows_out - first : 256);
}

// One 256-row block of one tensor, as elements of T (float, or float4 when k is a multiple of 4 and the tensors are
// 16-byte aligned: a row's destination is then aligned too).  A thread takes the block's elements e = thread, thread + 256,
// ... with (row, column) kept incrementally: consecutive lanes read consecutive source addresses and write runs of
// consecutive destination addresses (the emitted rows of a block are compacted in row order).  Four loads are issued
// before their stores.
template <typename T>
__device__ inline void apply_block(const unsigned* row_word, const BlockPlace& place, size_t base, unsigned block_rows,
                                   const dgr_densify_tensor& d, unsigned k, const float* __restrict__ scaling_raw,
                                   const float* __restrict__ rotation_raw, const float* __restrict__ noise,
                                   unsigned long long seed) {
    constexpr int U = 4;
    const int mode = d.mode;
    const T* __restrict__ src = reinterpret_cast<const T*>(d.src) + base * k;
    T* __restrict__ dst = reinterpret_cast<T*>(d.dst);
    T* __restrict__ dst_survivor = dst + place.first[0] * k;
    T* __restrict__ dst_clone = dst + place.first[1] * k;
    T* __restrict__ dst_child0 = dst + place.first[2] * k;
    T* __restrict__ dst_child1 = dst_child0 + place.n_pairs * k;
    const bool fresh_zero = mode == DGR_DENSIFY_ZERO_NEW || mode == DGR_DENSIFY_ZERO;
    const unsigned n = block_rows * k;
    const unsigned row_step = 256u / k, col_step = 256u % k;
    unsigned r = threadIdx.x / k, c = threadIdx.x % k;
    for (unsigned e0 = threadIdx.x; e0 < n; e0 += 256u * U) {
        T v[U];
        unsigned w[U], row[U], col[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned e = e0 + 256u * u;
            w[u] = e < n ? row_word[r] : 0u;
            row[u] = r;
            col[u] = c;
            // (moments are read for survivors only, accumulators never)
            const bool reads = mode == DGR_DENSIFY_ZERO_NEW ? (w[u] & ACT_SURVIVE) != 0u : mode != DGR_DENSIFY_ZERO && (w[u] & 7u);
            set_zero(v[u]);
            if (reads) v[u] = src[e];
            r += row_step;
            c += col_step;
            if (c >= k) {
                c -= k;
                ++r;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned rank_s = (w[u] >> 8) & 255u, rank_c = (w[u] >> 16) & 255u, rank_k = w[u] >> 24;
            if ((w[u] & ACT_SURVIVE) && rank_s < place.fit[0]) dst_survivor[rank_s * k + col[u]] = v[u];
            T fresh = v[u];
            if (fresh_zero) set_zero(fresh);
            if ((w[u] & ACT_CLONE) && rank_c < place.fit[1]) dst_clone[rank_c * k + col[u]] = fresh;
            if (w[u] & ACT_CHILDREN) {
                T child0 = fresh, child1 = fresh;
                if (mode == DGR_DENSIFY_LOG_SCALE) child0 = child1 = shifted(v[u]);
                if constexpr (sizeof(T) == sizeof(float)) {
                    if (mode == DGR_DENSIFY_XYZ) {
                        const size_t g = base + row[u];
                        float z[2][3];
#pragma unroll
                        for (int s = 0; s < 2; ++s)
#pragma unroll
                            for (int j = 0; j < 3; ++j)
                                z[s][j] = noise ? noise[g * 6 + s * 3 + j] : philox_normal(seed, g, (unsigned)s, j);
                        const float *q = rotation_raw + 4 * g, *sc = scaling_raw + 3 * g;
                        child0 = v[u] + child_offset(q, sc, z[0][0], z[0][1], z[0][2], (int)col[u]);
                        child1 = v[u] + child_offset(q, sc, z[1][0], z[1][1], z[1][2], (int)col[u]);
                    }
                }
                if (rank_k < place.fit[2]) dst_child0[rank_k * k + col[u]] = child0;
                if (rank_k < place.fit_second) dst_child1[rank_k * k + col[u]] = child1;
            }
        }
    }
}

// grid (row blocks, tensor groups): a workgroup recomputes the ranks of its 256 rows from their action bytes, then moves the
// block's rows of its tensors.
__global__ void __launch_bounds__(256) densify_apply_kernel(size_t rows, size_t rows_out, const void* __restrict__ plan,
                                                            DensifyTable table, const float* __restrict__ scaling_raw,
                                                            const float* __restrict__ rotation_raw,
                                                            const float* __restrict__ noise, unsigned long long seed) {
    __shared__ unsigned row_word[256];  // action bits | rank among survivors << 8 | among clones << 16 | among children << 24
    __shared__ int wave_tot[4][3];
    const size_t base = (size_t)blockIdx.x * 256;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned act = base + threadIdx.x < rows ? plan_flags(plan, rows)[base + threadIdx.x] : 0u;
    int rank[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        const unsigned long long m = __ballot((act >> f) & 1u);
        rank[f] = lane_rank(m);
        if (lane == 0) wave_tot[wave][f] = __popcll(m);
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < 3; ++f)
        for (int w = 0; w < wave; ++w) rank[f] += wave_tot[w][f];
    row_word[threadIdx.x] = (act & 7u) | (unsigned)rank[0] << 8 | (unsigned)rank[1] << 16 | (unsigned)rank[2] << 24;
    __syncthreads();

    const int* head = static_cast<const int*>(plan);
    const int4 off = plan_block_table(plan)[blockIdx.x];
    const size_t n_survive = (size_t)head[1], n_clone = (size_t)head[2];
    BlockPlace place;
    place.n_pairs = (size_t)head[3] / 2;
    place.first[0] = (size_t)off.x;
    place.first[1] = n_survive + (size_t)off.y;
    place.first[2] = n_survive + n_clone + (size_t)off.z;
#pragma unroll
    for (int f = 0; f < 3; ++f) place.fit[f] = rows_that_fit(place.first[f], rows_out);
    place.fit_second = rows_that_fit(place.first[2] + place.n_pairs, rows_out);

    const unsigned block_rows = (unsigned)(rows - base < 256 ? rows - base : 256);
    for (int t = table.begin[blockIdx.y]; t < table.begin[blockIdx.y + 1]; ++t) {
        const dgr_densify_tensor d = table.t[t];
        const unsigned k = (unsigned)d.k;
        const bool wide = (k & 3u) == 0u && ((reinterpret_cast<uintptr_t>(d.src) | reinterpret_cast<uintptr_t>(d.dst)) & 15u) == 0u;
        if (wide)
            apply_block<float4>(row_word, place, base, block_rows, d, k / 4, scaling_raw, rotation_raw, noise, seed);
        else
            apply_block<float>(row_word, place, base, block_rows, d, k, scaling_raw, rotation_raw, noise, seed);
    }
}

}  // namespace

size_t densify_plan_bytes(size_t rows) { return plan_bytes(rows); }

hipError_t launch_densify_plan(size_t rows, const float* grad_accum, const float* denom, const float* max_radii2D,
                               const float* opacity_raw, const float* scaling_raw, float grad_threshold,
                               float opacity_raw_min, float log_scale_split, float log_scale_prune, float max_screen_size,
                               void* plan, int* counts, hipStream_t stream) {
    const size_t blocks = plan_blocks(rows);
    if (blocks) {
        launch(densify_decide_kernel, dim3((unsigned)blocks), dim3(256), stream, rows, grad_accum, denom, max_radii2D,
               opacity_raw, scaling_raw, grad_threshold, opacity_raw_min, log_scale_split, log_scale_prune, max_screen_size,
               plan);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    launch(densify_scan_kernel, dim3(1), dim3(256), stream, blocks, plan, counts);  // (no blocks: it writes zero counts)
    return hipGetLastError();
}

hipError_t launch_densify_apply(size_t rows, size_t rows_out, const void* plan, int n, const dgr_densify_tensor* tensors,
                                const float* scaling_raw, const float* rotation_raw, const float* noise,
                                unsigned long long seed, hipStream_t stream) {
    if (rows == 0 || rows_out == 0) return hipSuccess;
    DensifyTable table = {};
    const int groups = deal_tensors(table, tensors, n, [](const dgr_densify_tensor& t) { return t.k % 4 == 0 ? t.k / 4 : t.k; });
    launch(densify_apply_kernel, dim3((unsigned)plan_blocks(rows), (unsigned)groups), dim3(256), stream, rows, rows_out, plan,
           table, scaling_raw, rotation_raw, noise, seed);
    return hipGetLastError();
}

}  // namespace dgr
