// block_scan.h -- the prefix sums of the binning front end (gfx950, wave64): one shuffle scan inside a wave and the two workgroup
// forms built on it with the wave totals through LDS (one value per thread; an array in LDS, a chunk per thread).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgr {

// Inclusive scan over the first WIDTH lanes of a wave (WIDTH a power of two; lanes behind them get sums nobody reads).
template <int WIDTH = 64>
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane) {
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < WIDTH; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    return incl;
}

// Exclusive scan of one value per thread over a workgroup of NT threads: returns the sum of the threads in front of this one,
// *total = the workgroup's sum.  `wsum`: NT / 64 words of LDS.  One barrier; all threads call it.
template <int NT>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t n, uint32_t* wsum, int tid, uint32_t* total) {
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t incl = wave_inclusive_scan(n, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int ww = 0; ww < NT / 64; ww++) {
        const uint32_t v = wsum[ww];
        if (ww < wave) before += v;
        all += v;
    }
    *total = all;
    return before + incl - n;
}

// Exclusive (inclusive) scan of a[0..n) in place (LDS) by the whole workgroup, a chunk per thread; returns the total.  NT threads,
// all call it.  `wsum`: NT / 64 words of LDS, which may still be read from a previous call when this one starts.
template <int NT>
__device__ __forceinline__ uint32_t block_scan(uint32_t* a, int n, bool inclusive, uint32_t* wsum, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int per = (n + NT - 1) / NT;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    uint32_t s = 0;
    for (int i = lo; i < hi; i++) s += a[i];
    const uint32_t incl = wave_inclusive_scan(s, lane);
    __syncthreads();  // (wsum may still be read from a previous call)
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    // (block_exclusive_scan's totals loop a second time: with one helper for both, in any of the forms tried, bin_segments and
    //  bin_tiles place their waits elsewhere, and bin_tiles then missed the project's A/B rule on the heavy-tailed scene,
    //  profiles/binning_shared/notes.md s5)
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int ww = 0; ww < NT / 64; ww++) {
        const uint32_t v = wsum[ww];
        if (ww < wave) before += v;
        total += v;
    }
    uint32_t run = before + incl - s;
    for (int i = lo; i < hi; i++) {
        const uint32_t c = a[i];
        a[i] = inclusive ? run + c : run;
        run += c;
    }
    __syncthreads();
    return total;
}

}  // namespace dgr
