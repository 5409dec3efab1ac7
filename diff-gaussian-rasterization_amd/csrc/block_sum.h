// block_sum.h -- the fixed-order sums of the loss and keyframe steps (gfx950, wave64).  The order IS the contract: these steps
// promise the same bits on every run, and every sum over a workgroup of 256 threads is formed the same way (block_sums).  Also
// here: the (hi, lo) float pair that carries a double partial sum through a float scratch, and torch.sign.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgr {

// the sum over the wave's 64 lanes, in every lane: partners at distance 32, 16, .. 1
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

namespace block_sum_detail {
// the sums' LDS, a row per wave: one array per <T, N>
template <typename T, int N>
__shared__ T red[4][N];
// Columns I .. N - 1: lane 0 of a wave writes its row, thread 0 adds the rows.  (The variable itself with a literal column I, not
// a reference to it or a loop's counter: only then does the front end know red[w][0] of two doubles to be 16-byte aligned, and the
// row goes out as one ds_write_b128, as it did written out.)
template <int I = 0, typename T, int N>
__device__ __forceinline__ void put(const T (&v)[N]) {
    red<T, N>[threadIdx.x >> 6][I] = v[I];
    if constexpr (I + 1 < N) put<I + 1>(v);
}
template <int I = 0, typename T, int N>
__device__ __forceinline__ void total(T (&v)[N]) {
    v[I] = (red<T, N>[0][I] + red<T, N>[1][I]) + (red<T, N>[2][I] + red<T, N>[3][I]);
    if constexpr (I + 1 < N) total<I + 1>(v);
}
}  // namespace block_sum_detail

// The sums of v[0 .. N) over a workgroup of 256 threads, all of which call it (T: double, float, uint32_t): thread 0 gets the
// totals in v, the others keep their wave's sums.  The butterfly of wave_sum, lane 0 of each wave to its row of LDS, one barrier,
// thread 0 adds the rows as (0 + 1) + (2 + 3).  The LDS is block_sum_detail's, one array per <T, N>: a kernel that sums the same
// types twice puts a barrier between the calls.
template <typename T, int N>
__device__ __forceinline__ void block_sums(T (&v)[N]) {
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < N; i++) v[i] += __shfl_xor(v[i], off, 64);
    if ((threadIdx.x & 63) == 0) block_sum_detail::put(v);
    __syncthreads();
    if (threadIdx.x == 0) block_sum_detail::total(v);
}

// a double partial sum goes through a float scratch as (hi, lo) floats whose sum in double restores 48 bits; two fill a 16-byte slot
__device__ __forceinline__ float4 doubles_to_pairs(double a, double b) {
    const float ah = (float)a, bh = (float)b;
    return make_float4(ah, (float)(a - (double)ah), bh, (float)(b - (double)bh));
}
__device__ __forceinline__ double pair_to_double(float hi, float lo) { return (double)hi + (double)lo; }

__device__ __forceinline__ float sign0(float x) { return (x > 0.f) ? 1.f : (x < 0.f) ? -1.f : 0.f; }  // torch.sign

}  // namespace dgr
