// seed.hip -- fused map expansion: new Gaussians from an RGB-D keyframe (include/dgr_hip.h: dgr_seed_plan / dgr_seed_apply).
//
// The sibling of densify-and-prune (optim.hip) and built the same way, three launches.  decide: one thread per candidate pixel
// (every stride-th pixel of every stride-th row) -> a flag byte and per-256-candidate block totals.  scan: one workgroup turns the
// block totals into exclusive offsets and the totals into counts[8].  apply: one launch over a table of tensors; the first
// workgroups of the grid copy the old rows, the others take 256 candidates each, recompute the selected ones' in-block ranks from
// the flag bytes (ballot + mbcnt) and write their rows behind the old ones.  Positions come from the scan alone: no atomics,
// new rows in row-major pixel order.
//
// plan buffer (plan.h): one flag byte per candidate (candidate_grid.h).
#include <hip/hip_runtime.h>

#include "candidate_grid.h"
#include "kernels.h"
#include "plan.h"

namespace dgr {
namespace {

constexpr unsigned SEED_SELECT = 1u, SEED_VALID = 2u, SEED_UNSEEN = 4u, SEED_INFRONT = 8u;
constexpr float INV_C0 = (float)(1.0 / 0.28209479177387814);  // 1 / SH_C0, rounded once

// Every comparison is false on a NaN: a NaN depth_obs is not valid, a NaN opacity_map is not unseen, a NaN depth is not in front.
__global__ void __launch_bounds__(256) seed_decide_kernel(CandidateGrid g, const float* __restrict__ depth_obs,
                                                          const float* __restrict__ opacity_map,
                                                          const float* __restrict__ depth, float depth_min, float depth_max,
                                                          float silhouette_threshold, float depth_error_min,
                                                          const float* __restrict__ depth_error_min_dev, void* plan) {
    __shared__ int wave_tot[4][4];
    const size_t n = g.candidates();
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (depth_error_min_dev) depth_error_min = *depth_error_min_dev;
    unsigned flags = 0;
    if (c < n) {
        unsigned cx, cy;
        candidate_cell(c, g.wc, cx, cy);
        const size_t pix = (size_t)cy * (unsigned)g.stride * (unsigned)g.W + (size_t)cx * (unsigned)g.stride;
        const float d_obs = depth_obs[pix];
        const bool valid = d_obs > depth_min && d_obs < depth_max;
        bool unseen = false, infront = false;
        if (opacity_map) unseen = opacity_map[pix] < silhouette_threshold;
        if (depth) {
            const float d = depth[pix];
            infront = d > d_obs && __fsub_rn(d, d_obs) > depth_error_min;  // one rounded subtraction
        }
        const bool select = valid && (unseen || infront || (!opacity_map && !depth));
        flags = (select ? SEED_SELECT : 0u) | (valid ? SEED_VALID : 0u) | (valid && unseen ? SEED_UNSEEN : 0u) |
                (valid && infront ? SEED_INFRONT : 0u);
        plan_flags(plan, n)[c] = (unsigned char)flags;
    }
    const int4 t = block_flag_totals(flags, wave_tot);
    if (threadIdx.x == 0) plan_block_table(plan)[blockIdx.x] = t;
}

// One workgroup: exclusive scan of the block totals in place (plan.h); then the counts.
__global__ void __launch_bounds__(256) seed_scan_kernel(size_t blocks, int rows, void* plan, int* __restrict__ counts) {
    __shared__ int4 wave_sum[4];
    const int4 carry = scan_block_totals(plan_block_table(plan), blocks, wave_sum);
    write_counts8(rows + carry.x, carry.x, carry.y, carry.z, carry.w, plan, counts);
}

using SeedTable = TensorTable<dgr_seed_tensor, DGR_SEED_MAX_TENSORS>;  // (plan.h; a tensor's cost: float4 per thread in the copy)

struct SeedCamera {  // what XYZ, LOG_SCALE and RGB_DC read
    const float* color_obs;
    const float* depth_obs;
    const float* viewmatrix;
    float inv_fx, inv_fy, cx, cy, pix;
};

// The old rows of one 256-row block of one tensor: a contiguous run of block_rows * k floats, whose start (1024 k bytes into the
// tensor) is 16-byte aligned when the tensor is, so it moves as float4 whatever k is (the last block's odd floats one by one).
// Four loads are issued before their stores.
__device__ inline void copy_block(const float* __restrict__ src, float* __restrict__ dst, unsigned n, bool wide) {
    constexpr int U = 4;
    unsigned done = 0;
    if (wide) {
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
        float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
        const unsigned n4 = n / 4;
        for (unsigned e0 = threadIdx.x; e0 < n4; e0 += 256u * U) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (e0 + 256u * u < n4) v[u] = s4[e0 + 256u * u];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (e0 + 256u * u < n4) d4[e0 + 256u * u] = v[u];
        }
        done = n4 * 4;
    }
    for (unsigned e = done + threadIdx.x; e < n; e += 256u) dst[e] = src[e];
}

// The new rows of one block of candidates in one tensor: n_rows rows of k floats behind `dst` (the block's first new row),
// element e = row * k + column written by thread e % 256: runs of consecutive addresses.  sel_*: the block's selected
// candidates in rank order (pixel x, y and the observed depth).
__device__ inline void fill_block(float* __restrict__ dst, unsigned n_rows, const dgr_seed_tensor& d, const SeedCamera& cam,
                                  const CandidateGrid& g, const int* sel_x, const int* sel_y, const float* sel_d) {
    const unsigned k = (unsigned)d.k, n = n_rows * k;
    const int mode = d.mode;
    if (mode == DGR_SEED_CONST) {  // one value over a contiguous run: aligned float4 stores between a scalar head and tail
        const unsigned to_aligned = (unsigned)((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / 4u;
        const unsigned head = to_aligned < n ? to_aligned : n, n4 = (n - head) / 4u;
        if (threadIdx.x < head) dst[threadIdx.x] = d.value;
        float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + head);
        const float4 v = make_float4(d.value, d.value, d.value, d.value);
        for (unsigned e = threadIdx.x; e < n4; e += 256u) d4[e] = v;
        for (unsigned e = head + 4u * n4 + threadIdx.x; e < n; e += 256u) dst[e] = d.value;
        return;
    }
    if (mode == DGR_SEED_QUAT_IDENTITY && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0u) {  // (k = 4: a float4 per row)
        float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
        for (unsigned e = threadIdx.x; e < n_rows; e += 256u) d4[e] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const unsigned row_step = 256u / k, col_step = 256u % k;
    unsigned r = threadIdx.x / k, c = threadIdx.x % k;
    for (unsigned e = threadIdx.x; e < n; e += 256u) {
        float v = 0.0f;
        if (mode == DGR_SEED_QUAT_IDENTITY) {
            v = c == 0u ? 1.0f : 0.0f;
        } else if (mode == DGR_SEED_LOG_SCALE) {
            v = logf(__fmul_rn(sel_d[r], cam.pix));
        } else if (mode == DGR_SEED_RGB_DC) {
            const size_t plane = (size_t)g.W * (size_t)g.H;
            const float rgb = cam.color_obs[c * plane + (size_t)sel_y[r] * (unsigned)g.W + (unsigned)sel_x[r]];
            v = __fmul_rn(__fsub_rn(rgb, 0.5f), INV_C0);
        } else if (mode == DGR_SEED_XYZ) {
            const float depth = sel_d[r];
            const float* __restrict__ vm = cam.viewmatrix;  // W2C^T: row c of its rotation block gives component c, row 3 is W2C's translation
            const float p0 = ((float)sel_x[r] - cam.cx) * cam.inv_fx * depth - vm[12];
            const float p1 = ((float)sel_y[r] - cam.cy) * cam.inv_fy * depth - vm[13];
            const float p2 = depth - vm[14];
            const float v0 = vm[4 * c], v1 = vm[4 * c + 1], v2 = vm[4 * c + 2];
            v = v0 * p0 + v1 * p1 + v2 * p2;
        }
        dst[e] = v;
        r += row_step;
        c += col_step;
        if (c >= k) {
            c -= k;
            ++r;
        }
    }
}

// grid (copy blocks + candidate blocks, tensor groups).  Nothing is written past rows_out (the caller's allocation), whatever
// the plan says.
__global__ void __launch_bounds__(256) seed_apply_kernel(CandidateGrid g, size_t rows, size_t rows_out, const void* __restrict__ plan,
                                                         SeedTable table, SeedCamera cam) {
    __shared__ int sel_x[256], sel_y[256];
    __shared__ float sel_d[256];
    __shared__ int wave_tot[4][1];
    const size_t copy_blocks = plan_blocks(rows);
    if (blockIdx.x < copy_blocks) {  // (uniform over the workgroup)
        const size_t base = (size_t)blockIdx.x * 256;
        size_t block_rows = rows - base < 256 ? rows - base : 256;
        if (base + block_rows > rows_out) block_rows = base < rows_out ? rows_out - base : 0;
        for (int t = table.begin[blockIdx.y]; t < table.begin[blockIdx.y + 1]; ++t) {
            const dgr_seed_tensor d = table.t[t];
            const bool wide = ((reinterpret_cast<uintptr_t>(d.src) | reinterpret_cast<uintptr_t>(d.dst)) & 15u) == 0u;
            copy_block(d.src + base * (unsigned)d.k, d.dst + base * (unsigned)d.k, (unsigned)block_rows * (unsigned)d.k, wide);
        }
        return;
    }
    const size_t block = blockIdx.x - copy_blocks, n = g.candidates();
    const size_t cand = block * 256 + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool select = cand < n && (plan_flags(plan, n)[cand] & SEED_SELECT) != 0u;
    const unsigned long long m = __ballot(select);
    int rank = lane_rank(m);
    if (lane == 0) wave_tot[wave][0] = __popcll(m);
    __syncthreads();
    for (int w = 0; w < wave; ++w) rank += wave_tot[w][0];
    const unsigned n_sel = (unsigned)wave_total(wave_tot, 0);
    if (select) {
        unsigned ux, uy;
        candidate_pixel(cand, g.wc, g.stride, ux, uy);
        const int x = (int)ux, y = (int)uy;
        sel_x[rank] = x;
        sel_y[rank] = y;
        sel_d[rank] = cam.depth_obs[(size_t)y * (unsigned)g.W + (unsigned)x];
    }
    __syncthreads();
    const size_t first = rows + (size_t)plan_block_table(plan)[block].x;
    const unsigned n_rows = first >= rows_out ? 0u : (unsigned)(rows_out - first < n_sel ? rows_out - first : n_sel);
    if (n_rows == 0u) return;
    for (int t = table.begin[blockIdx.y]; t < table.begin[blockIdx.y + 1]; ++t) {
        const dgr_seed_tensor d = table.t[t];
        fill_block(d.dst + first * (unsigned)d.k, n_rows, d, cam, g, sel_x, sel_y, sel_d);
    }
}

}  // namespace

size_t seed_plan_bytes(int W, int H, int stride) {
    return plan_bytes(candidate_grid(W, H, stride).candidates());
}

size_t seed_candidates(int W, int H, int stride) { return candidate_grid(W, H, stride).candidates(); }

hipError_t launch_seed_plan(int W, int H, int stride, const float* depth_obs, const float* opacity_map, const float* depth,
                            float depth_min, float depth_max, float silhouette_threshold, float depth_error_min,
                            const float* depth_error_min_dev, size_t rows, void* plan, int* counts, hipStream_t stream) {
    const CandidateGrid g = candidate_grid(W, H, stride);
    const size_t blocks = plan_blocks(g.candidates());
    launch(seed_decide_kernel, dim3((unsigned)blocks), dim3(256), stream, g, depth_obs, opacity_map, depth, depth_min, depth_max,
           silhouette_threshold, depth_error_min, depth_error_min_dev, plan);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    launch(seed_scan_kernel, dim3(1), dim3(256), stream, blocks, (int)rows, plan, counts);
    return hipGetLastError();
}

hipError_t launch_seed_apply(int W, int H, int stride, size_t rows, size_t rows_out, const void* plan, int n,
                             const dgr_seed_tensor* tensors, const float* color_obs, const float* depth_obs,
                             const float* viewmatrix, float inv_fx, float inv_fy, float cx, float cy, float pix,
                             hipStream_t stream) {
    if (rows_out == 0) return hipSuccess;
    const CandidateGrid g = candidate_grid(W, H, stride);
    SeedTable table = {};
    const int groups = deal_tensors(table, tensors, n, [](const dgr_seed_tensor& t) { return (t.k + 3) / 4; });
    const size_t blocks = plan_blocks(rows) + (rows_out > rows ? plan_blocks(g.candidates()) : 0);
    const SeedCamera cam = {color_obs, depth_obs, viewmatrix, inv_fx, inv_fy, cx, cy, pix};
    launch(seed_apply_kernel, dim3((unsigned)blocks, (unsigned)groups), dim3(256), stream, g, rows, rows_out, plan, table, cam);
    return hipGetLastError();
}

}  // namespace dgr
