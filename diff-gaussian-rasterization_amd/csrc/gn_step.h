// gn_step.h -- the tail the fused Gauss-Newton pose steps share (icp.hip: dgr_icp_step, dgr_rgbd_step; gicp.hip: dgr_gicp_step).
// A step is one workgroup of 256 threads per block of 2048 items (candidates, sources), every thread with N double accumulators:
// A's upper triangle (21), b (6), sum w r^2, count (N = 29), and the hybrid step's two more (31).  Behind the accumulation:
// reduce: block_sums; the block's partial to its own 256-byte row of the scratch; a ticket (pose_reduce.h's deterministic form).
//         The block that draws the last ticket adds the rows in block order and leaves the ticket at zero: a recorded graph
//         replays the step.
// solve : one thread: the totals -> (ok, xi): the damped 6 x 6 system by LDL^T in double (se3.h), the refusals.
// write : that thread: the new pose re-orthonormalised through its quaternion, or the input's bits on a refusal; the stats row.
// What a step keeps to itself is its loop body and its update rule from xi to (R, t).
// No contraction mode of its own: compiled in the includer's mode (gicp.hip includes it below its contract(off) pragma, icp.hip
// with the compiler's default), so the damping line and the three norms below fuse in the one file and not in the other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_sum.h"
#include "se3.h"

namespace dgr {

constexpr int GN_THREADS = 256;
constexpr int GN_BLOCK_ITEMS = 2048;       // eight trips of a workgroup
constexpr int GN_ROW = 32;                 // doubles per block in the scratch: a 256-byte row
constexpr int GN_CHUNK = 64;               // rows the finisher stages in LDS per trip
constexpr size_t GN_HEADER_BYTES = 256;    // the ticket (a uint32 at byte 0; zero between calls)
// A diagonal entry below this share of the largest is damped as if it were that large: a direction the data does not constrain
// at all (an exactly zero row of A: the fronto-parallel plane) then has a positive pivot under damping > 0 and does not move.
constexpr double GN_DAMPING_FLOOR = 1e-3;

__host__ __device__ inline unsigned gn_blocks(size_t items) { return (unsigned)((items + GN_BLOCK_ITEMS - 1) / GN_BLOCK_ITEMS); }
// the scratch of a step: the header, then a row per block
inline size_t gn_scratch_bytes(size_t items) { return GN_HEADER_BYTES + (size_t)gn_blocks(items) * GN_ROW * sizeof(double); }
inline uint32_t* gn_ticket(void* scratch) { return static_cast<uint32_t*>(scratch); }
inline double* gn_rows(void* scratch) { return reinterpret_cast<double*>(static_cast<char*>(scratch) + GN_HEADER_BYTES); }

// Every thread of every workgroup calls it with its sums.  `ticket`: zero on entry, left at zero; `part`: a row of GN_ROW doubles
// per workgroup.  Thread 0 of the block that drew the last ticket, the finisher, calls finish(the N totals, in LDS), once the
// ticket is back at zero; every other thread returns.  (The finisher as a callable, not as a flag handed back: a flag that differs
// from thread to thread would make everything the finisher loads through it divergent, and its branches vector branches.)
template <int N, class Finish>
static __device__ __forceinline__ void gn_reduce(double (&acc)[N], uint32_t* __restrict__ ticket, double* __restrict__ part, Finish finish) {
    __shared__ int last;
    __shared__ double rows[GN_CHUNK * GN_ROW];
    __shared__ double totals[GN_ROW];
    block_sums(acc);
    if (threadIdx.x == 0) {
        double* row = part + (size_t)blockIdx.x * GN_ROW;
#pragma unroll
        for (int i = 0; i < N; i++) __hip_atomic_store(row + i, acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores are acknowledged before the ticket is taken
        const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    // the last block: every row is delivered.  Rows staged in LDS GN_CHUNK at a time (all loads of a chunk in flight together),
    // then thread s < N adds sum s over the rows in block order.
    double tot = 0.0;
    for (unsigned base = 0; base < gridDim.x; base += GN_CHUNK) {
        const unsigned n = gridDim.x - base < GN_CHUNK ? gridDim.x - base : GN_CHUNK;
        for (unsigned i = threadIdx.x; i < n * GN_ROW; i += GN_THREADS)
            if ((i & (GN_ROW - 1)) < N)
                rows[i] = __hip_atomic_load(part + (size_t)base * GN_ROW + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (threadIdx.x < N)
            for (unsigned r = 0; r < n; r++) tot += rows[r * GN_ROW + threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < N) totals[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (back to zero, then the finish)
        finish(totals);
    }
}

// The totals -> xi with M xi = -b, M = A damped.  False (a refusal) on fewer than min_points pairs in `count`, a total among
// 0 .. 27 that is not finite, `rest_finite` false (the caller's word on its totals past 27), a pivot not above rcond times the
// largest diagonal entry, or an xi that is not finite.  `count` by reference: read where it is compared, behind the unpack.
__device__ __forceinline__ bool gn_solve(const double* tot, const double& count, bool rest_finite, int min_points, double damping,
                                         double rcond, double (&xi)[6]) {
    double M[6][6], b[6];
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) M[i][j] = M[j][i] = tot[k++];
#pragma unroll
        for (int i = 0; i < 6; i++) b[i] = tot[21 + i];
    }
    bool ok = count >= (double)min_points;
#pragma unroll
    for (int i = 0; i < 28; i++) ok = ok & isfinite(tot[i]);  // (&: 28 tests of values already loaded, no branch to keep)
    ok = ok && rest_finite;
    double max_diag = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) max_diag = fmax(max_diag, M[i][i]);
#pragma unroll
    for (int i = 0; i < 6; i++) M[i][i] += damping * fmax(M[i][i], GN_DAMPING_FLOOR * max_diag);
    const double pivot_min = rcond * max_diag;
    double D[6];
    ok = ldlt6_factor(M, D, pivot_min) && ok;  // (se3.h: M = L D L^T, no pivoting)
    const double nb[6] = {-b[0], -b[1], -b[2], -b[3], -b[4], -b[5]};
    ldlt6_solve(M, D, nb, xi);  // M xi = -b
#pragma unroll
    for (int i = 0; i < 6; i++) ok = ok && isfinite(xi[i]);
    return ok;
}

// The input pose (16 floats, se3.h's layout), read in full before anything is written -- the output may be the same address:
// its (R, t) for the update, its bits for a refusal.
struct GnPoseIn {
    double R[3][3], t[3];
    uint32_t bits[16];
};
__device__ __forceinline__ void gn_read_pose(const float* in, GnPoseIn& p) {
    pose_of(in, p.R, p.t);
#pragma unroll
    for (int i = 0; i < 16; i++) p.bits[i] = reinterpret_cast<const uint32_t*>(in)[i];
}

// The step's outputs.  ok: (Ro, to) is the updated pose, stored with its rotation re-orthonormalised through its unit quaternion
// (a refusal after all if that is not finite).  A refusal: the input's bits to `out` and to trans_out, the quaternion of the
// input's rotation.  quat_out, trans_out: NULL = not stored.  stats: the N totals, ok, |omega|, |v|, zeros up to STATS.
template <int N, int STATS>
__device__ __forceinline__ void gn_write(bool ok, double (&Ro)[3][3], const double (&to)[3], const GnPoseIn& in, const double (&xi)[6],
                                         const double* tot, float* out, float* quat_out, float* trans_out, double* stats) {
    const uint32_t(&in_bits)[16] = in.bits;
    double q[4];
    if (ok) {
        rotation_to_quat(Ro, q);
        quat_to_rotation(q, Ro);
#pragma unroll
        for (int i = 0; i < 4; i++) ok = ok && isfinite(q[i]);
#pragma unroll
        for (int i = 0; i < 3; i++) ok = ok && isfinite(to[i]);
    }
    if (!ok) rotation_to_quat(in.R, q);
    if (ok) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) out[4 * i + j] = (float)Ro[j][i];
            out[4 * i + 3] = 0.f;
            out[12 + i] = (float)to[i];
        }
        out[15] = 1.f;
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) reinterpret_cast<uint32_t*>(out)[i] = in_bits[i];
    }
    if (quat_out)
#pragma unroll
        for (int i = 0; i < 4; i++) quat_out[i] = (float)q[i];
    if (trans_out)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (ok) trans_out[i] = (float)to[i];
            else reinterpret_cast<uint32_t*>(trans_out)[i] = in_bits[12 + i];
        }
#pragma unroll
    for (int i = 0; i < N; i++) stats[i] = tot[i];
    stats[N] = ok ? 1.0 : 0.0;
    stats[N + 1] = ok ? sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]) : 0.0;
    stats[N + 2] = ok ? sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]) : 0.0;
#pragma unroll
    for (int i = N + 3; i < STATS; i++) stats[i] = 0.0;
}

}  // namespace dgr
