// keyframe_overlap.hip -- keyframe overlap scores for covisibility selection (include/dgr_hip.h: dgr_keyframe_overlap): the
// candidate pixels of the current frame (the stride grid of candidate_grid.h, seed.hip's) are unprojected with the measured depth, taken into every stored
// keyframe and counted where they land inside its image (and, with the keyframes' depths, where that depth agrees).
//
// count : one workgroup per (keyframe, block of 2048 candidates).  Threads 0..11 form the relative transform current camera ->
//         keyframe from the two W2C^T matrices in double (the rigid inverse of the current pose never exists on its own) and
//         round it once; every thread then takes a candidate per trip.  Counts: ballot + popcount per wave and trip, the four
//         waves' totals added through LDS.  With one block per keyframe this launch writes the outputs itself.
// finish: only with several blocks per keyframe: a wave per keyframe adds the blocks' totals (integers: any order gives the same
//         bits) and forms the score.
// No atomics, nothing read on the host.
#include <hip/hip_runtime.h>

#include "block_sum.h"
#include "candidate_grid.h"
#include "kernels.h"
#include "plan.h"

namespace dgr {
namespace {

constexpr int THREADS = 256;
constexpr int BLOCK_CANDIDATES = 2048;  // eight trips of a workgroup
constexpr unsigned OVERLAP_VALID = 1u, OVERLAP_INSIDE = 2u, OVERLAP_VISIBLE = 4u;

__host__ __device__ inline unsigned overlap_blocks(size_t candidates) {
    return (unsigned)((candidates + BLOCK_CANDIDATES - 1) / BLOCK_CANDIDATES);
}

__device__ inline float overlap_score(int visible, int valid) { return valid > 0 ? (float)visible / (float)valid : 0.0f; }

// grid: n_keyframes * blocks workgroups, keyframe-major.  `slots`: int4 per workgroup (valid, inside, visible, 0) when blocks > 1.
__global__ void __launch_bounds__(THREADS) overlap_count_kernel(KeyframeOverlapArgs a, unsigned blocks, int4* __restrict__ slots) {
    __shared__ float rel[12];  // camera point p -> keyframe point: X_j = rel[3 j] p_0 + rel[3 j + 1] p_1 + rel[3 j + 2] p_2 + rel[9 + j]
    __shared__ int wave_tot[THREADS / 64][3];
    const unsigned k = blockIdx.x / blocks, b = blockIdx.x - k * blocks;
    if (threadIdx.x < 12) {
        // both matrices hold W2C^T: W2C's rotation entry R[j][i] at [4 i + j], its translation t[j] at [12 + j].
        // X = R_k R_c^T (p - t_c) + t_k
        const float* __restrict__ vc = a.viewmatrix;
        const float* __restrict__ vk = a.keyframe_viewmatrices + (size_t)k * 16;
        const int j = threadIdx.x < 9 ? threadIdx.x / 3 : threadIdx.x - 9;
        double r[3];
#pragma unroll
        for (int m = 0; m < 3; ++m)
            r[m] = (double)vk[j] * (double)vc[m] + (double)vk[4 + j] * (double)vc[4 + m] + (double)vk[8 + j] * (double)vc[8 + m];
        const int m = threadIdx.x - 3 * j;
        if (threadIdx.x < 9) rel[threadIdx.x] = (float)(m == 0 ? r[0] : m == 1 ? r[1] : r[2]);
        else rel[threadIdx.x] = (float)((double)vk[12 + j] - (r[0] * (double)vc[12] + r[1] * (double)vc[13] + r[2] * (double)vc[14]));
    }
    __syncthreads();
    const float r00 = rel[0], r01 = rel[1], r02 = rel[2], r10 = rel[3], r11 = rel[4], r12 = rel[5], r20 = rel[6], r21 = rel[7],
                r22 = rel[8], t0 = rel[9], t1 = rel[10], t2 = rel[11];
    const float u_max = (float)a.W - a.edge, v_max = (float)a.H - a.edge;
    const float* __restrict__ kf_depth = a.keyframe_depths ? a.keyframe_depths + (size_t)k * (size_t)a.W * (size_t)a.H : nullptr;
    unsigned char* __restrict__ flags_out = a.flags ? a.flags + (size_t)k * a.candidates : nullptr;
    const size_t begin = (size_t)b * BLOCK_CANDIDATES;
    const size_t end = begin + BLOCK_CANDIDATES < a.candidates ? begin + BLOCK_CANDIDATES : a.candidates;
    int n_valid = 0, n_inside = 0, n_visible = 0;  // this wave's (the same in every lane)
    for (size_t c0 = begin; c0 < end; c0 += THREADS) {  // (every lane takes every trip: the ballots need them)
        const size_t c = c0 + threadIdx.x;
        bool valid = false, inside = false, visible = false;
        if (c < end) {
            unsigned x, y;
            candidate_pixel(c, a.wc, a.stride, x, y);
            const float d = a.depth_obs[(size_t)y * (unsigned)a.W + x];
            valid = d > a.depth_min && d < a.depth_max;  // (false on a NaN)
            const float p0 = ((float)x - a.cx) * a.inv_fx * d, p1 = ((float)y - a.cy) * a.inv_fy * d;
            const float X = r00 * p0 + r01 * p1 + r02 * d + t0;
            const float Y = r10 * p0 + r11 * p1 + r12 * d + t1;
            const float Z = r20 * p0 + r21 * p1 + r22 * d + t2;
            const float u = a.fx * X / Z + a.cx, v = a.fy * Y / Z + a.cy;
            inside = valid && Z > a.near_z && u > a.edge && u < u_max && v > a.edge && v < v_max;
            visible = inside;
            if (kf_depth && inside) {  // (inside: u in (edge, W - edge), v likewise, edge >= 0: the rounded pixel is 0 .. W, 0 .. H)
                const int px = (int)floorf(u + 0.5f), py = (int)floorf(v + 0.5f);
                visible = false;
                if (px < a.W && py < a.H) {
                    const float dk = kf_depth[(size_t)py * (unsigned)a.W + (unsigned)px];
                    visible = dk > a.depth_min && dk < a.depth_max && fabsf(Z - dk) <= a.depth_tolerance * dk;
                }
            }
            if (flags_out)
                flags_out[c] = (unsigned char)((valid ? OVERLAP_VALID : 0u) | (inside ? OVERLAP_INSIDE : 0u) |
                                               (visible ? OVERLAP_VISIBLE : 0u));
        }
        n_valid += __popcll(__ballot(valid));
        n_inside += __popcll(__ballot(inside));
        n_visible += __popcll(__ballot(visible));
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        wave_tot[wave][0] = n_valid;
        wave_tot[wave][1] = n_inside;
        wave_tot[wave][2] = n_visible;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot[3];
#pragma unroll
        for (int f = 0; f < 3; ++f) tot[f] = wave_total(wave_tot, f);
        if (blocks > 1) {
            slots[blockIdx.x] = make_int4(tot[0], tot[1], tot[2], 0);
        } else {
            a.inside[k] = tot[1];
            a.visible[k] = tot[2];
            a.score[k] = overlap_score(tot[2], tot[0]);
            if (k == 0) a.valid[0] = tot[0];
        }
    }
}

// a wave per keyframe: lane l adds blocks l, l + 64, ..., then the lanes
__global__ void __launch_bounds__(THREADS) overlap_finish_kernel(KeyframeOverlapArgs a, unsigned blocks,
                                                                  const int4* __restrict__ slots) {
    const unsigned k = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= (unsigned)a.K) return;  // (a whole wave)
    int n_valid = 0, n_inside = 0, n_visible = 0;
    for (unsigned b = lane; b < blocks; b += 64) {
        const int4 s = slots[(size_t)k * blocks + b];
        n_valid += s.x;
        n_inside += s.y;
        n_visible += s.z;
    }
    n_valid = wave_sum(n_valid);
    n_inside = wave_sum(n_inside);
    n_visible = wave_sum(n_visible);
    if (lane == 0) {
        a.inside[k] = n_inside;
        a.visible[k] = n_visible;
        a.score[k] = overlap_score(n_visible, n_valid);
        if (k == 0) a.valid[0] = n_valid;
    }
}

}  // namespace

size_t keyframe_overlap_scratch_bytes(int W, int H, int stride, int K) {
    const unsigned blocks = overlap_blocks(seed_candidates(W, H, stride));
    return 16 + (blocks > 1 ? (size_t)K * blocks * sizeof(int4) : 0);
}

hipError_t launch_keyframe_overlap(const KeyframeOverlapArgs& args, void* scratch, hipStream_t stream) {
    KeyframeOverlapArgs a = args;
    const CandidateGrid g = candidate_grid(a.W, a.H, a.stride);
    a.candidates = g.candidates();
    a.wc = g.wc;
    const unsigned blocks = overlap_blocks(a.candidates);
    int4* slots = static_cast<int4*>(scratch);
    launch(overlap_count_kernel, dim3((unsigned)a.K * blocks), dim3(THREADS), stream, a, blocks, slots);
    if (blocks > 1) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        launch(overlap_finish_kernel, dim3(((unsigned)a.K + THREADS / 64 - 1) / (THREADS / 64)), dim3(THREADS), stream, a, blocks,
               (const int4*)slots);
    }
    return hipGetLastError();
}

}  // namespace dgr
