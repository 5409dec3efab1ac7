// plan_scan.h -- what the two plan-then-apply steps (densify-and-prune in optim.hip, map expansion in seed.hip) share: a lane's
// rank in a ballot, and the one-workgroup exclusive scan of the per-256-element block totals (gfx950, wave64).
#pragma once
#include <hip/hip_runtime.h>

namespace dgr {

__device__ inline int lane_rank(unsigned long long m) {  // set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ inline int4 add4(int4 a, int4 b) { return make_int4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// One workgroup of 256 threads: exclusive scan of table[0 .. blocks) in place, 256 records per pass with the running totals
// carried from pass to pass; returns the totals (in every thread).  `wave_sum`: int4[4] of LDS.
__device__ inline int4 scan_block_totals(int4* table, size_t blocks, int4* wave_sum) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int4 carry = make_int4(0, 0, 0, 0);
    for (size_t base = 0; base < blocks; base += 256) {
        const size_t b = base + threadIdx.x;
        const int4 own = b < blocks ? table[b] : make_int4(0, 0, 0, 0);
        int4 inc = own;  // inclusive scan within the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            int4 up;
            up.x = __shfl_up(inc.x, d);
            up.y = __shfl_up(inc.y, d);
            up.z = __shfl_up(inc.z, d);
            up.w = __shfl_up(inc.w, d);
            if (lane >= d) inc = add4(inc, up);
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        int4 before = carry;
        for (int w = 0; w < wave; ++w) before = add4(before, wave_sum[w]);
        if (b < blocks) table[b] = make_int4(before.x + inc.x - own.x, before.y + inc.y - own.y, before.z + inc.z - own.z,
                                             before.w + inc.w - own.w);
        carry = add4(add4(add4(add4(carry, wave_sum[0]), wave_sum[1]), wave_sum[2]), wave_sum[3]);
        __syncthreads();  // wave_sum is rewritten by the next pass
    }
    return carry;
}

// threads 0 .. 7 of the workgroup write counts[8] = {c0 .. c4, 0, 0, 0}, to `counts` and to the plan's header
__device__ inline void write_counts8(int c0, int c1, int c2, int c3, int c4, void* plan, int* __restrict__ counts) {
    if (threadIdx.x < 8) {
        const int t = (int)threadIdx.x;
        const int v = t == 0 ? c0 : t == 1 ? c1 : t == 2 ? c2 : t == 3 ? c3 : t == 4 ? c4 : 0;
        counts[t] = v;
        static_cast<int*>(plan)[t] = v;
    }
}

}  // namespace dgr
