// selftest.hip -- device self-tests of the shared headers (wave_reduce.h, render_common.h, exact_math.h, tile_sort.h) behind the
// dgr_debug_* entry points (api.hip); no variant's code.
#include "render_common.h"
#include "tile_sort.h"

namespace dgr {
namespace {

// self-test of the butterflies: in[c * 64 + lane] -> the three networks' results and value maps per lane (dgr_debug_wave_reduce)
__global__ void __launch_bounds__(64) wave_reduce_test_kernel(const float* in, float* out16, float* out12, float* out4,
                                                             int* comp16, int* comp12, int* comp4) {
    const int lane = threadIdx.x;
    float g16[16], g12[12], g4[4];
#pragma unroll
    for (int k = 0; k < 16; k++) g16[k] = in[k * 64 + lane];
#pragma unroll
    for (int k = 0; k < 12; k++) g12[k] = g16[k];
#pragma unroll
    for (int k = 0; k < 4; k++) g4[k] = g16[k];
    out16[lane] = wave_reduce16d(g16);
    out12[lane] = wave_reduce12d(g12);
    out4[lane] = wave_reduce4(g4);
    comp16[lane] = wave_reduce16d_comp(lane);
    comp12[lane] = wave_reduce12d_comp(lane);
    comp4[lane] = wave_reduce4_comp(lane);
}

// self-test of the reductions per HALF of the wave (wave_reduce.h): in[c * 64 + lane], twelve values for the paired step of the
// mapping backward (r0, r1 and the butterfly slot each lane holds), the first three for the tracking backward's half_reduce3
__global__ void __launch_bounds__(64) half_reduce_test_kernel(const float* in, float* r0, float* r1, float* h3, int* slot0, int* slot1,
                                                             int* comp3) {
    const int lane = threadIdx.x;
    float g[12];
#pragma unroll
    for (int k = 0; k < 12; k++) g[k] = in[k * 64 + lane];
    h3[lane] = half_reduce3(g[0], g[1], g[2]);
    float u0, u1;
    wave_reduce12d_head(g, u0, u1);
    r0[lane] = quad_sum(u0);
    r1[lane] = quad_sum(u1);
    slot0[lane] = wave_reduce12d_half_slot0(lane);
    slot1[lane] = wave_reduce12d_half_slot1(lane);
    comp3[lane] = half_reduce3_comp(lane);
}

// ... and of the sixteen-value network stopped before its cross-half stage (the paired step of the FULL backward): in[c * 64 + lane]
__global__ void __launch_bounds__(64) half_reduce16_test_kernel(const float* in, float* r0, float* r1, int* slot0, int* slot1) {
    const int lane = threadIdx.x;
    float g[16];
#pragma unroll
    for (int k = 0; k < 16; k++) g[k] = in[k * 64 + lane];
    float u0, u1;
    wave_reduce16d_head(g, u0, u1);
    r0[lane] = quad_sum(u0);
    r1[lane] = quad_sum(u1);
    slot0[lane] = wave_reduce16d_half_slot0(lane);
    slot1[lane] = wave_reduce16d_half_slot1(lane);
}

// self-test of the list builders of render_common.h on one batch of 128 staged slots: codes[slot] = the eight bits "half h of
// quadrant wave w" (bit 2 w + h).  paired[w] / halves[w] (280 words each) = {steps or length, split[0] lo, hi, split[1] lo, hi,
// list 2 w [0..135], list 2 w + 1 [0..135]} as wave w leaves them (dgr_debug_lane_lists).
__global__ void __launch_bounds__(256) lane_lists_test_kernel(const unsigned char* codes, uint32_t* paired, uint32_t* halves) {
    typedef StagedT<128, uint32_t, 8> S;
    __shared__ S s;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned code = tid < 128 ? codes[tid] : 0u;
    for (int pass = 0; pass < 2; pass++) {
        for (int i = tid; i < 8 * S::LIST_LD; i += 256) (&s.list[0][0])[i] = 0xFFFFFFFFu;
        __syncthreads();
        unsigned long long split[2] = {0ull, 0ull};
        const int n = pass == 0 ? build_paired_lists(s, code, tid, wave, lane, split) : build_half_lists(s, code, tid, wave, lane);
        uint32_t* const o = (pass == 0 ? paired : halves) + 280 * wave;
        if (lane == 0) {
            o[0] = (uint32_t)n;
            o[1] = (uint32_t)split[0]; o[2] = (uint32_t)(split[0] >> 32);
            o[3] = (uint32_t)split[1]; o[4] = (uint32_t)(split[1] >> 32);
        }
        for (int i = lane; i < S::LIST_LD; i += 64) {
            o[5 + i] = s.list[2 * wave][i];
            o[5 + S::LIST_LD + i] = s.list[2 * wave + 1][i];
        }
        __syncthreads();
    }
}

// self-test of exact_math.h: out_exp[i] = exp_p32(x[i]) (GLIBC: exp_glibc), out_div[i] = div_ref(a[i], b[i]) (dgr_debug_exact_math)
template <bool GLIBC>
__global__ void __launch_bounds__(256) exact_math_test_kernel(int n, const float* x, const float* a, const float* b, float* out_exp,
                                                             float* out_div) {
    __shared__ uint64_t tab[32];
    exp_ref_table_fill(tab, threadIdx.x);
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        // (the clamped forms: equal to the plain ones down to -104, 0 below)
        out_exp[i] = GLIBC ? exp_glibc<true>(x[i], tab) : exp_p32<true>(x[i]);
        float inv;
        out_div[i] = t_div<ALPHA_REF>(a[i], b[i], inv);
    }
}

// self-test of tile_sort.h (dgr_debug_tile_sort): workgroup b sorts list b = keys[offsets[b] .. offsets[b + 1]), each routine as
// the binning kernels call it -- bin_tiles' 512 threads and its keys in LDS (segment_binning.hip: K2_THREADS, K2_CAP) for modes
// 0 .. 2, in place in global memory for the others.  The waves take turns (list b: wave b % 8) and every second list starts
// at an odd key index, so that the 16-byte rows of the id transposition meet both alignments of a list.
constexpr int TS_THREADS = 512, TS_WAVES = TS_THREADS / 64, TS_CAP = 6144;
template <int NT>
__global__ void __launch_bounds__(NT) tile_sort_test_kernel(int mode, const uint64_t* __restrict__ keys, const int* __restrict__ offsets,
                                                            uint32_t* __restrict__ out_ids, uint64_t* out_keys) {
    const int tid = threadIdx.x;
    const int off = offsets[blockIdx.x], n = offsets[blockIdx.x + 1] - off;
    if (n <= 0) return;
    if (mode >= DGR_TILE_SORT_GLOBAL) {
        for (int i = tid; i < n; i += NT) out_keys[off + i] = keys[off + i];
        __syncthreads();
        wg_sort_global<NT>(out_keys + off, n, tid);
        return;
    }
    if constexpr (NT == TS_THREADS) {
        __shared__ uint64_t sk[TS_CAP + 1];
        const int lane = tid & 63, wave = tid >> 6;
        // (the API checked the lengths; a list the mode cannot take is left alone rather than written past the array)
        if (n > (mode == DGR_TILE_SORT_WAVE ? 1024 : mode == DGR_TILE_SORT_PART ? PART_Q : TS_CAP)) return;
        uint64_t* const list = sk + (blockIdx.x & 1);
        for (int i = tid; i < n; i += NT) list[i] = keys[off + i];
        __syncthreads();
        const int turn = (int)(blockIdx.x % TS_WAVES);
        if (mode == DGR_TILE_SORT_WAVE) {
            if (wave == turn) sort_tile_in_wave(list, n, out_ids + off, lane);
        } else if (mode == DGR_TILE_SORT_PART) {
            if (wave == turn) sort_list_part(list, n, 0, lane);
            __syncthreads();
            for (int i = tid; i < n; i += NT) out_keys[off + i] = list[i];
        } else {  // sort_lists' sequence for one long list (segment_binning.hip)
            for (int p = 0; p < list_parts(n); p++)
                if ((turn + p) % TS_WAVES == wave) sort_list_part(list, n, p, lane);
            __syncthreads();
            merge_list_parts<NT>(list, n, out_ids + off, tid);
        }
    }
}
}  // namespace

hipError_t launch_tile_sort_test(int mode, int n_lists, const uint64_t* keys, const int* offsets, uint32_t* out_ids, uint64_t* out_keys,
                                 hipStream_t stream) {
    if (n_lists <= 0) return hipSuccess;
    if (mode == DGR_TILE_SORT_GLOBAL_256)  // (sort_tiles_kernel's SORT_THREADS, binning.hip)
        launch(tile_sort_test_kernel<256>, dim3(n_lists), dim3(256), stream, mode, keys, offsets, out_ids, out_keys);
    else
        launch(tile_sort_test_kernel<TS_THREADS>, dim3(n_lists), dim3(TS_THREADS), stream, mode, keys, offsets, out_ids, out_keys);
    return hipGetLastError();
}
hipError_t launch_exact_math_test(int n, const float* x, const float* a, const float* b, float* out_exp, float* out_div,
                                  int alpha_mode, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (alpha_mode == ALPHA_GLIBC)
        launch(exact_math_test_kernel<true>, dim3(min((n + 255) / 256, 4096)), dim3(256), stream, n, x, a, b, out_exp, out_div);
    else
        launch(exact_math_test_kernel<false>, dim3(min((n + 255) / 256, 4096)), dim3(256), stream, n, x, a, b, out_exp, out_div);
    return hipGetLastError();
}
hipError_t launch_wave_reduce_test(const float* in, float* out16, float* out12, float* out4, int* comp16, int* comp12, int* comp4,
                                   hipStream_t stream) {
    launch(wave_reduce_test_kernel, dim3(1), dim3(64), stream, in, out16, out12, out4, comp16, comp12, comp4);
    return hipGetLastError();
}

hipError_t launch_half_reduce_test(const float* in, float* r0, float* r1, float* h3, int* slot0, int* slot1, int* comp3, hipStream_t stream) {
    launch(half_reduce_test_kernel, dim3(1), dim3(64), stream, in, r0, r1, h3, slot0, slot1, comp3);
    return hipGetLastError();
}
hipError_t launch_half_reduce16_test(const float* in, float* r0, float* r1, int* slot0, int* slot1, hipStream_t stream) {
    launch(half_reduce16_test_kernel, dim3(1), dim3(64), stream, in, r0, r1, slot0, slot1);
    return hipGetLastError();
}
hipError_t launch_lane_lists_test(const unsigned char* codes, uint32_t* paired, uint32_t* halves, hipStream_t stream) {
    launch(lane_lists_test_kernel, dim3(1), dim3(256), stream, codes, paired, halves);
    return hipGetLastError();
}

}  // namespace dgr
