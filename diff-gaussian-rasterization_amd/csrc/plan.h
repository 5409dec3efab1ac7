// plan.h -- what the plan-then-apply steps share (gfx950, wave64): densify-and-prune in optim.hip, map expansion in seed.hip,
// relocation in relocate.hip (and, for its tensor table, the map correction in transform.hip).  For all three: 256-row blocks, a
// lane's rank in a ballot, the one-workgroup exclusive scan of the
// block totals (over the step's own record) and the table that deals an apply launch's tensors to workgroups.  For the two that
// change P: the plan buffer's layout and the decide kernels' block totals.
// plan buffer: int[16] header (0..7: the counts), int4 per 256-element block (totals, then exclusive offsets), a flag byte per element.
#pragma once
#include <hip/hip_runtime.h>

namespace dgr {

constexpr int PLAN_HEADER_INTS = 16;
__host__ __device__ inline size_t plan_blocks(size_t n) { return (n + 255) / 256; }
__device__ inline int4* plan_block_table(void* plan) { return reinterpret_cast<int4*>(static_cast<int*>(plan) + PLAN_HEADER_INTS); }
__device__ inline const int4* plan_block_table(const void* plan) {
    return reinterpret_cast<const int4*>(static_cast<const int*>(plan) + PLAN_HEADER_INTS);
}
__device__ inline unsigned char* plan_flags(void* plan, size_t n) {
    return static_cast<unsigned char*>(plan) + PLAN_HEADER_INTS * 4 + plan_blocks(n) * 16;
}
__device__ inline const unsigned char* plan_flags(const void* plan, size_t n) {
    return static_cast<const unsigned char*>(plan) + PLAN_HEADER_INTS * 4 + plan_blocks(n) * 16;
}
inline size_t plan_bytes(size_t n) { return PLAN_HEADER_INTS * 4 + plan_blocks(n) * 16 + ((n + 15) & ~(size_t)15); }

__device__ inline int lane_rank(unsigned long long m) {  // set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
// the four waves' entries of column f of `wave_tot` (int[4][F] of LDS, one row per wave), added
template <int F>
__device__ inline int wave_total(const int (*wave_tot)[F], int f) {
    return wave_tot[0][f] + wave_tot[1][f] + wave_tot[2][f] + wave_tot[3][f];
}

// The decide kernels' epilogue: every thread of the 256 brings four flag bits, thread 0 returns how many threads set each (the
// others zeros).  `wave_tot`: int[4][4] of LDS.  (`flags` by reference: by value the compiler carries the caller's value range
// into this function and compiles seed_decide_kernel's last ballot differently, profiles/plan_apply/README.md.)
__device__ inline int4 block_flag_totals(const unsigned& flags, int (*wave_tot)[4]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const int n = __popcll(__ballot((flags >> f) & 1u));
        if (lane == 0) wave_tot[wave][f] = n;
    }
    __syncthreads();
    int4 t = make_int4(0, 0, 0, 0);
    if (threadIdx.x == 0) {
        t.x = wave_total(wave_tot, 0);
        t.y = wave_total(wave_tot, 1);
        t.z = wave_total(wave_tot, 2);
        t.w = wave_total(wave_tot, 3);
    }
    return t;
}

// what scan_block_totals needs of a block record: totals_zero (of a table of them), totals_add, totals_sub, totals_shfl_up (the
// value d lanes below)
__device__ inline int4 totals_zero(const int4*) { return make_int4(0, 0, 0, 0); }
__device__ inline int4 totals_add(int4 a, int4 b) { return make_int4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline int4 totals_sub(int4 a, int4 b) { return make_int4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ inline int4 totals_shfl_up(int4 v, int d) {
    return make_int4(__shfl_up(v.x, d), __shfl_up(v.y, d), __shfl_up(v.z, d), __shfl_up(v.w, d));
}

// One workgroup of 256 threads: exclusive scan of table[0 .. blocks) in place, 256 records per pass with the running totals
// carried from pass to pass; returns the totals (in every thread).  `wave_sum`: R[4] of LDS.
template <typename R>
__device__ inline R scan_block_totals(R* table, size_t blocks, R* wave_sum) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    R carry = totals_zero(table);
    for (size_t base = 0; base < blocks; base += 256) {
        const size_t b = base + threadIdx.x;
        const R own = b < blocks ? table[b] : totals_zero(table);
        R inc = own;  // inclusive scan within the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const R up = totals_shfl_up(inc, d);
            if (lane >= d) inc = totals_add(inc, up);
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        R before = carry;
        for (int w = 0; w < wave; ++w) before = totals_add(before, wave_sum[w]);
        if (b < blocks) table[b] = totals_sub(totals_add(before, inc), own);
        carry = totals_add(totals_add(totals_add(totals_add(carry, wave_sum[0]), wave_sum[1]), wave_sum[2]), wave_sum[3]);
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

// The tensors of one apply launch (a kernel argument), and how they are dealt to workgroups: group g (blockIdx.y) moves
// tensors begin[g] .. begin[g + 1] - 1 of its block.  A wide tensor is a group of its own; narrow ones (a [P, 1] opacity, the
// accumulators) share one, so that the ranks are recomputed once for all of them and no workgroup is launched for 256 floats.
template <typename Desc, int N>
struct TensorTable {
    Desc t[N];
    unsigned char begin[N + 1];
};
constexpr int GROUP_STEPS = 12;  // a group's cost at most, in the step's own unit (a [P, 48] tensor as float4 per thread: 12)
// fills `table` from tensors[0 .. n) and returns the number of groups; cost(tensor): what it adds to its group
template <typename Desc, int N, typename Cost>
inline int deal_tensors(TensorTable<Desc, N>& table, const Desc* tensors, int n, Cost cost) {
    int groups = 0, steps = 0;
    for (int i = 0; i < n; ++i) {
        table.t[i] = tensors[i];
        const int c = cost(tensors[i]);
        if (i == 0 || steps + c > GROUP_STEPS) {
            table.begin[groups++] = (unsigned char)i;
            steps = 0;
        }
        steps += c;
    }
    table.begin[groups] = (unsigned char)n;
    return groups;
}

}  // namespace dgr
