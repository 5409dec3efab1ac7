// pose_reduce.h -- the pose gradient's reduction over the Gaussians and its delivery to dL_dview, for the one-view and the
// batched per-Gaussian backward (preprocess_bwd.hip), each in its atomic and its deterministic form.
#pragma once
#include "dgr_common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace dgr {

// Block reduction of the 12 pose terms and their delivery.  The sum over 4e5 Gaussians cancels to ~1e-3 of its terms, so
// everything beyond a 16-lane row is accumulated in double.
// The block's partial goes into one of 64 bucket rows with double atomics performed at L2 (agent scope: no
// cache to keep coherent), then the block takes a ticket; the block that draws the last ticket finds every
// partial delivered and finishes the sum -- no separate reduction kernel, no fence that writes back an L2.
template <int CTRL>
__device__ __forceinline__ float dpp_row_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// Step 1 (every wave): the 16 lanes of a DPP row are summed in float on the vector pipe (quad_perm ^1, ^2, row_half_mirror,
// row_mirror: four adds per value, every lane of the row ends up with the row's sum) and the row sums go to LDS as doubles.
// Sixteen float terms add nothing to the rounding the float terms already carry (each is a float product), and the 144
// ds_bpermute + 72 double adds per wave of the all-double 64-lane butterfly this replaces were 11 of the one-view kernel's
// 52 us (measured with the reduction compiled out).
__device__ __forceinline__ void pose_rows_to_lds(const float (&pose)[12], double (*red)[12]) {
    const int row = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        float v = pose[i];
        v += dpp_row_mov<0xB1>(v);   // quad_perm [1,0,3,2]
        v += dpp_row_mov<0x4E>(v);   // quad_perm [2,3,0,1]
        v += dpp_row_mov<0x141>(v);  // row_half_mirror
        v += dpp_row_mov<0x140>(v);  // row_mirror
        if ((threadIdx.x & 15) == 0) red[row][i] = (double)v;
    }
}
// The block's partial of component c: its 16 row sums, in double, rows ascending
__device__ __forceinline__ double pose_block_partial(const double (*red)[12], int c) {
    double part = 0.0;
#pragma unroll
    for (int r = 0; r < 16; r++) part += red[r][c];
    return part;
}
// The 12 sums (lanes 0..11 of the calling wave hold one each) as the [4,4] dL_dview: slot order v0,v1,v2,v4,v5,v6,v8,v9,v10,
// v12,v13,v14 (L/cuda_rasterizer/backward.cu:723), the last row zero
__device__ __forceinline__ void pose_write_view(float* dL_dview, float out) {
    if (threadIdx.x < 12) dL_dview[(threadIdx.x / 3) * 4 + threadIdx.x % 3] = out;
    if (threadIdx.x < 4) dL_dview[threadIdx.x * 4 + 3] = 0.0f;
}
// No pose gradient asked for (track_off): zeros (L/rasterize_points.cu:186)
__device__ __forceinline__ void pose_zero(float* dL_dview) {
    if (blockIdx.x == 0 && threadIdx.x < 16) dL_dview[threadIdx.x] = 0.0f;
}
// Step 2 (wave 0, after a workgroup barrier): the 16 row sums of the block in double, added to one of 64 bucket rows with
// double atomics performed at L2 (agent scope: no cache to keep coherent).
__device__ __forceinline__ void pose_add_partial(double (*red)[12], double* pose_part) {
    if (threadIdx.x < 12) {
        const double part = pose_block_partial(red, threadIdx.x);
        double* slot = pose_part + (size_t)(blockIdx.x % DGR_POSE_BUCKETS) * 12 + threadIdx.x;
        __hip_atomic_fetch_add(slot, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// Step 3 (wave 0, once its adds are acknowledged and it has drawn ticket `t`): the block that draws the last ticket finds
// every partial delivered and finishes the sum -- no separate reduction kernel, no fence that writes back an L2.
// `clear` (resident scratch, dgr_backward_scratch_clean_arm): the finisher leaves buckets and ticket as it found them at the start
// of the call -- zero -- for the next backward that uses this scratch.
__device__ __forceinline__ void pose_finish_if_last(uint32_t t, double* pose_part, float* dL_dview, uint32_t* ticket = nullptr,
                                                    bool clear = false) {
    if (t != gridDim.x - 1) return;
    if (threadIdx.x < 16) {
        float out = 0.0f;
        if (threadIdx.x < 12) {
            double tot = 0.0;
            for (int g = 0; g < DGR_POSE_BUCKETS; g++)  // (agent-scope loads: served by L2, where the adds were performed)
                tot += __hip_atomic_load(pose_part + (size_t)g * 12 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            out = (float)tot;
            // (the clearing stores in a loop of their own, behind ALL the loads: a store right behind each load of the same
            //  address made the 64 round trips of this one wave dependent -- +25 us at the kernel's tail, whatever its size)
            if (clear)
                for (int g = 0; g < DGR_POSE_BUCKETS; g++)
                    __hip_atomic_store(pose_part + (size_t)g * 12 + threadIdx.x, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (clear && threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pose_write_view(dL_dview, out);
    }
}
// One view: the delivery is wave 0's alone (no workgroup barrier after the first): two L2 round trips -- the bucket adds,
// then the ticket -- during which the other three waves would only hold their registers.
__device__ __forceinline__ void pose_block_reduce(const float (&pose)[12], double* pose_part, uint32_t* ticket, float* dL_dview,
                                                  double (*red)[12], bool clear = false) {
    pose_rows_to_lds(pose, red);
    __syncthreads();
    if (threadIdx.x >= 64) return;
    pose_add_partial(red, pose_part);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the adds are acknowledged before the ticket is taken
    uint32_t t = 0u;
    if (threadIdx.x == 0) t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pose_finish_if_last((uint32_t)__builtin_amdgcn_readfirstlane((int)t), pose_part, dL_dview, ticket, clear);
}

// Deterministic step 2 (wave 0, after a workgroup barrier): the block's partial STORED to the block's own row of `det_pose`
__device__ __forceinline__ void pose_store_partial(double (*red)[12], double* det_pose) {
    if (threadIdx.x < 12) {
        const double part = pose_block_partial(red, threadIdx.x);
        __hip_atomic_store(det_pose + (size_t)blockIdx.x * 12 + threadIdx.x, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// the block that drew a view's last ticket adds the per-block partials in a fixed order (wave 0 only)
__device__ __forceinline__ void pose_finish_det(const double* det_pose, uint32_t* ticket, float* dL_dview, double (*lane_sum)[12], bool clear) {
    {   // (a row's twelve loads in flight together, two rows per trip: one memory round trip per 128 rows, not per value)
        double acc[12];
#pragma unroll
        for (int c = 0; c < 12; c++) acc[c] = 0.0;
        for (uint32_t b = threadIdx.x; b < gridDim.x; b += 128) {
            double v[2][12];
            const bool two = b + 64 < gridDim.x;
#pragma unroll
            for (int c = 0; c < 12; c++) {
                v[0][c] = __hip_atomic_load(det_pose + (size_t)b * 12 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v[1][c] = two ? __hip_atomic_load(det_pose + (size_t)(b + 64) * 12 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
            }
#pragma unroll
            for (int c = 0; c < 12; c++) acc[c] = (acc[c] + v[0][c]) + v[1][c];  // rows l, l + 64, l + 128, ... ascending
        }
#pragma unroll
        for (int c = 0; c < 12; c++) lane_sum[threadIdx.x][c] = acc[c];
    }
    // (one wave: LDS writes and reads of a wave are in program order)
    if (threadIdx.x < 16) {
        float out = 0.0f;
        if (threadIdx.x < 12) {
            double tot = 0.0;
            for (int l = 0; l < 64; l++) tot += lane_sum[l][threadIdx.x];
            out = (float)tot;
        }
        if (clear && threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pose_write_view(dL_dview, out);
    }
}

// Deterministic form (dgr_set_option("deterministic_grads", 1)): double atomics on the 64 bucket rows arrive in any order, and a
// double sum depends on its order in the last bit.  Here every block STORES its partial to its own row of `det_pose` and the block
// that draws the last ticket adds the rows in a fixed order: lane l of wave 0 the rows l, l + 64, ... ascending, then lanes 0..11
// the 64 lane sums ascending.
__device__ __forceinline__ void pose_block_reduce_det(const float (&pose)[12], double* det_pose, uint32_t* ticket, float* dL_dview,
                                                      double (*red)[12], bool clear) {
    __shared__ double lane_sum[64][12];
    pose_rows_to_lds(pose, red);
    __syncthreads();
    if (threadIdx.x >= 64) return;
    pose_store_partial(red, det_pose);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores are acknowledged before the ticket is taken
    uint32_t t = 0u;
    if (threadIdx.x == 0) t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((uint32_t)__builtin_amdgcn_readfirstlane((int)t) != gridDim.x - 1) return;
    pose_finish_det(det_pose, ticket, dL_dview, lane_sum, clear);
}

// The V views of a batch (preprocess_bwd_batch_kernel, whose waves left every view's row sums in red[v] without a barrier): one
// barrier, then wave 0 adds every view's partial, waits once, draws every view's ticket (issued back to back: one L2 round
// trip for the batch) and finishes the views whose last block this is.
// Deterministic gradients: every view's partial of this block STORED to the view's own [blocks, 12] array, the views' tickets
// drawn together, and whoever drew a view's last one adds its rows in a fixed order (pose_block_reduce_det).
__device__ __forceinline__ void pose_batch_reduce(const PreprocessBwdBatchArgs& b, double (*red)[16][12]) {
    if (b.base.track_off) return;  // (the view loop wrote the zeros)
    const int V = b.V;
    __syncthreads();
    if (threadIdx.x >= 64) return;
    if (b.v[0].det_pose) {
        __shared__ double lane_sum[64][12];
#pragma unroll 1
        for (int v = 0; v < V; v++) pose_store_partial(red[v], b.v[v].det_pose);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t td = 0u;
#pragma unroll 1
        for (int v = 0; v < V; v++)
            if ((int)threadIdx.x == v) td = __hip_atomic_fetch_add(b.v[v].ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll 1
        for (int v = 0; v < V; v++)
            if ((uint32_t)__builtin_amdgcn_readlane((int)td, v) == gridDim.x - 1) pose_finish_det(b.v[v].det_pose, b.v[v].ticket, b.v[v].dL_dview, lane_sum, false);
        return;
    }
#pragma unroll 1
    for (int v = 0; v < V; v++) pose_add_partial(red[v], b.v[v].pose_part);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t t = 0u;
#pragma unroll 1
    for (int v = 0; v < V; v++)
        if ((int)threadIdx.x == v) t = __hip_atomic_fetch_add(b.v[v].ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll 1
    for (int v = 0; v < V; v++)
        pose_finish_if_last((uint32_t)__builtin_amdgcn_readlane((int)t, v), b.v[v].pose_part, b.v[v].dL_dview);
}

}  // namespace dgr
