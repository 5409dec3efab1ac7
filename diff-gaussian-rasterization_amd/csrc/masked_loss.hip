// masked_loss.hip -- the masked L1 loss of the RGB-D SLAM systems (SplaTAM's get_loss, CG-SLAM's tracking) as plain HIP launches:
//   e = |depth - depth_obs|,  B = valid sensor depth && finite e [&& silhouette above a threshold] [&& user mask],
//   K = B && e <= factor * median_v(e over B),   loss = w_d sum_K e / N_d + w_c sum |color - color_obs| / N_c
// per view v of a [V, ., H, W] stack (include/dgr_hip.h states the contract).  The median is exact and found on the device by
// a radix select over the bit patterns of e (non-negative finite floats: unsigned order is float order), three digits of
// 11 / 11 / 10 bits from the top:
//   clear   : zeroes the three histograms of every view (a kernel, as zero_floats_kernel elsewhere: no memset node in a recorded graph)
//   select 0: histogram of the top digit of every key in B          (per-workgroup LDS histogram, flushed with integer atomics)
//   select 1: scans histogram 0 for the bin holding the lower median's rank, histograms the middle digit of the keys in that bin
//   select 2: scans histograms 0 and 1, histograms the low digit of the keys that carry both digits
//   loss    : scans all three -> the median's bits; mask byte per pixel, per-workgroup sums (double, as hi/lo pairs) and counts
//   final   : adds the workgroups' slots per view and then the views in a fixed order; loss, medians, counts, gradient scales
// Every select pass derives the previous digits itself (each workgroup scans the 2048-bin histogram the pass before it
// finished), so the passes are ordered by kernel boundaries alone: no workgroup waits for or signals another inside a launch.
// Integer atomics commute and no float is ever added atomically: every output carries the same bits on every run.  Without
// rejection the forward is loss + final.  The backward is one launch that reads the mask bytes the forward left.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "block_scan.h"
#include "block_sum.h"
#include "kernels.h"

namespace dgr {
namespace {

constexpr int THREADS = 256;
constexpr int BINS = 2048;                     // 11 bits; the last pass (10 bits) leaves the upper half zero
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;       // not in B (a key is at most 0x7F7FFFFF)
// Workgroups per view: one per 1024 pixels (four trips of its 256 threads), which fills the CUs at 1080p with one view -- but no
// more than about 2048 over the whole stack (never below 256 a view): each one scans the histograms and flushes its own with
// global atomics, and at [4,1080p] 8100 of them cost more than they hid (profiles/masked_loss/measured.txt)
constexpr long PIXELS_PER_BLOCK = 1024;
constexpr int STACK_BLOCKS = 2048, MIN_BLOCKS = 256;
constexpr int HEADER_FLOATS = 16;              // [0] w_d / N_d, [1] w_c / N_c, [2] free for the caller's loss; rest reserved
constexpr int SLOT_WORDS = 8;                  // a workgroup's partials: S_d hi, lo, S_c hi, lo, |B|, |K|, 2 unused

// THE definition of the base set: the bits of e = |depth - depth_obs| for a pixel in B, NO_KEY otherwise (NaN fails every test)
__device__ __forceinline__ uint32_t base_key(const MaskedLossArgs& a, long o) {
    const float d_obs = a.depth_obs[o];
    const float e = fabsf(a.depth[o] - d_obs);
    bool ok = a.lo < d_obs && d_obs < a.hi && e <= FLT_MAX;
    if (a.opacity) ok = ok && a.opacity[o] > a.silhouette;
    if (a.mask) ok = ok && a.mask[o] != 0;
    return ok ? __float_as_uint(e) : NO_KEY;
}

struct Pick {
    uint32_t digit, rank;  // the bin that holds the rank asked for, and the rank inside that bin
};

// The bin of a 2048-bin histogram that holds the 0-based `rank` (MEDIAN: the lower median's rank (total - 1) / 2 instead).  All
// 256 threads call it; an empty histogram gives (0, 0).  `lds`: 6 words, which may still be read from a previous call.
template <bool MEDIAN>
__device__ __forceinline__ Pick find_bin(const uint32_t* __restrict__ hist, uint32_t rank, uint32_t* lds) {
    const int tid = threadIdx.x;
    const uint4 lo = reinterpret_cast<const uint4*>(hist)[2 * tid], hi = reinterpret_cast<const uint4*>(hist)[2 * tid + 1];
    const uint32_t c[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) s += c[j];
    uint32_t total;
    const uint32_t before = block_exclusive_scan<THREADS>(s, lds, tid, &total);
    if (MEDIAN) rank = total ? (total - 1) / 2 : 0;
    if (total == 0) {
        if (tid == 0) lds[4] = lds[5] = 0;
    } else if (rank >= before && rank - before < s) {
        uint32_t run = before;
        int j = 0;
        while (j < 7 && rank - run >= c[j]) run += c[j++];
        lds[4] = 8 * tid + j;
        lds[5] = rank - run;
    }
    __syncthreads();
    return Pick{lds[4], lds[5]};
}

__global__ void __launch_bounds__(THREADS) clear_kernel(uint4* __restrict__ hist, long n16) {
    const long stride = (long)gridDim.x * THREADS;
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < n16; i += stride) hist[i] = make_uint4(0, 0, 0, 0);
}

// pass PASS of the select: histogram PASS of view blockIdx.y over the pixels [blockIdx.x * chunk, + chunk) of that view
template <int PASS>
__global__ void __launch_bounds__(THREADS) select_kernel(MaskedLossArgs a, uint32_t* hist, long chunk) {
    __shared__ uint32_t h[BINS];
    __shared__ uint32_t lds[6];
    const int tid = threadIdx.x, lane = tid & 63, v = blockIdx.y;
    const long HW = (long)a.H * a.W, per_pass = (long)a.V * BINS;
    uint32_t prefix = 0;  // the digits above this pass's
    if (PASS >= 1) {
        const Pick p0 = find_bin<true>(hist + (long)v * BINS, 0, lds);
        prefix = p0.digit;
        if (PASS == 2) prefix = (prefix << 11) | find_bin<false>(hist + per_pass + (long)v * BINS, p0.rank, lds).digit;
    }
    for (int i = tid; i < BINS; i += THREADS) h[i] = 0;
    __syncthreads();
    const long begin = blockIdx.x * chunk, end = std::min(begin + chunk, HW);
    for (long p0 = begin; p0 < end; p0 += THREADS) {  // (every lane of a wave takes every trip: the ballots below need them)
        const long p = p0 + tid;
        const uint32_t key = p < end ? base_key(a, v * HW + p) : NO_KEY;
        bool take = key != NO_KEY;
        uint32_t digit = key >> 21;
        if (PASS == 1) {
            take = take && digit == prefix;
            digit = (key >> 10) & 2047u;
        } else if (PASS == 2) {
            take = take && (key >> 10) == prefix;
            digit = key & 1023u;
        }
        // a frame whose errors are (nearly) all equal would send every LDS atomic of a wave to one bin: the lanes that share the
        // first taking lane's digit go in as one add of their count
        const unsigned long long takers = __ballot(take);
        if (takers) {
            const int leader = __ffsll(takers) - 1;
            const uint32_t first = __shfl(digit, leader, 64);
            const unsigned long long same = __ballot(take && digit == first);
            if (lane == leader) atomicAdd(&h[first], (uint32_t)__popcll(same));
            else if (take && digit != first) atomicAdd(&h[digit], 1u);
        }
    }
    __syncthreads();
    uint32_t* out = hist + PASS * per_pass + (long)v * BINS;
    for (int i = tid; i < BINS; i += THREADS) {
        const uint32_t n = h[i];
        if (n) atomicAdd(&out[i], n);
    }
}

// Four sums over the workgroup in block_sum.h's order -> the workgroup's slot.  Written out: the two types share one barrier,
// and through block_sums(s, n) the compiler orders lane 0's two LDS stores differently in loss_kernel (profiles/loss_steps/README.md)
__device__ __forceinline__ void reduce_to_slot(double sd, double sc, uint32_t nb, uint32_t nk, uint32_t* slot) {
    __shared__ double red[THREADS / 64][2];
    __shared__ uint32_t cnt[THREADS / 64][2];
    for (int off = 32; off > 0; off >>= 1) {
        sd += __shfl_xor(sd, off, 64);
        sc += __shfl_xor(sc, off, 64);
        nb += __shfl_xor(nb, off, 64);
        nk += __shfl_xor(nk, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = sd;
        red[threadIdx.x >> 6][1] = sc;
        cnt[threadIdx.x >> 6][0] = nb;
        cnt[threadIdx.x >> 6][1] = nk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sd = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        sc = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
        *reinterpret_cast<float4*>(slot) = doubles_to_pairs(sd, sc);
        reinterpret_cast<uint4*>(slot)[1] = make_uint4(cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0],
                                                       cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1], 0, 0);
    }
}

// the kept set of this workgroup's pixels: mask bytes, sums and counts.  REJECT: the median from the three histograms first
template <bool REJECT>
__global__ void __launch_bounds__(THREADS) loss_kernel(MaskedLossArgs a, const uint32_t* __restrict__ hist, long chunk,
                                                        float* __restrict__ median, unsigned char* __restrict__ kept_mask,
                                                        uint32_t* __restrict__ slots) {
    __shared__ uint32_t lds[6];
    const int tid = threadIdx.x, v = blockIdx.y;
    const long HW = (long)a.H * a.W, per_pass = (long)a.V * BINS;
    float limit = 0.f;
    if (REJECT) {
        const Pick p0 = find_bin<true>(hist + (long)v * BINS, 0, lds);
        const Pick p1 = find_bin<false>(hist + per_pass + (long)v * BINS, p0.rank, lds);
        const Pick p2 = find_bin<false>(hist + 2 * per_pass + (long)v * BINS, p1.rank, lds);
        const float m = __uint_as_float((p0.digit << 21) | (p1.digit << 10) | p2.digit);
        limit = a.factor * m;
        if (blockIdx.x == 0 && tid == 0) median[v] = m;
    } else if (blockIdx.x == 0 && tid == 0) {
        median[v] = __uint_as_float(0x7FC00000u);  // no median was computed
    }
    double sd = 0.0, sc = 0.0;
    uint32_t nb = 0, nk = 0;
    const long begin = blockIdx.x * chunk, end = std::min(begin + chunk, HW);
    for (long p = begin + tid; p < end; p += THREADS) {
        const long o = v * HW + p;
        const uint32_t key = base_key(a, o);
        const float e = __uint_as_float(key);
        const bool base = key != NO_KEY, kept = base && (!REJECT || e <= limit);
        kept_mask[o] = kept ? 1 : 0;
        nb += base;
        nk += kept;
        if (kept) sd += (double)e;
        if (kept || !a.mask_color) {
            const long oc = (long)v * a.C * HW + p;
            for (int c = 0; c < a.C; c++) sc += (double)fabsf(a.color[oc + c * HW] - a.color_obs[oc + c * HW]);
        }
    }
    reduce_to_slot(sd, sc, nb, nk, slots + SLOT_WORDS * ((long)v * gridDim.x + blockIdx.x));
}

// One workgroup.  Wave w adds the slots of views w, w + 4, ... (lane l: slots l, l + 64, ...; then the lanes), which gives the
// view's counts and sums; then the views are added the same way and thread 0 forms the loss and the backward's two scales.
__global__ void __launch_bounds__(THREADS) final_kernel(int V, int blocks, const uint32_t* __restrict__ slots, double n_color_all,
                                                         int C, float w_color, float w_depth, int mask_color, int mean,
                                                         int* __restrict__ base, int* __restrict__ kept,
                                                         double* __restrict__ view_sums, float* __restrict__ header,
                                                         float* __restrict__ loss) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (int v = tid >> 6; v < V; v += THREADS / 64) {
        double s[2] = {};
        uint32_t n[2] = {};
        for (int b = lane; b < blocks; b += 64) {
            const uint4* slot = reinterpret_cast<const uint4*>(slots + SLOT_WORDS * ((long)v * blocks + b));
            const uint4 f = slot[0], c = slot[1];
            s[0] += pair_to_double(__uint_as_float(f.x), __uint_as_float(f.y));
            s[1] += pair_to_double(__uint_as_float(f.z), __uint_as_float(f.w));
            n[0] += c.x;
            n[1] += c.y;
        }
        for (int i = 0; i < 2; i++) {
            s[i] = wave_sum(s[i]);
            n[i] = wave_sum(n[i]);
        }
        if (lane == 0) {
            base[v] = (int)n[0];
            kept[v] = (int)n[1];
            view_sums[2 * v] = s[0];
            view_sums[2 * v + 1] = s[1];
        }
    }
    __syncthreads();  // (this workgroup's own global writes, read back below)
    double s[3] = {};  // S_d, S_c, |K| (a count of up to 2^16 views x 2^30 pixels: exact in a double)
    for (int v = tid; v < V; v += THREADS) {
        s[0] += view_sums[2 * v];
        s[1] += view_sums[2 * v + 1];
        s[2] += (double)kept[v];
    }
    block_sums(s);
    if (tid == 0) {
        const double sd = s[0], sc = s[1], nk = s[2];
        const double n_d = mean ? nk : 1.0, n_c = mean ? (mask_color ? (double)C * nk : n_color_all) : 1.0;
        const double term_d = n_d > 0.0 ? (double)w_depth * sd / n_d : 0.0, term_c = n_c > 0.0 ? (double)w_color * sc / n_c : 0.0;
        header[0] = n_d > 0.0 ? w_depth / (float)n_d : 0.f;
        header[1] = n_c > 0.0 ? w_color / (float)n_c : 0.f;
        *loss = (float)(term_d + term_c);
    }
}

// dL/ddepth = up w_d / N_d sign(depth - depth_obs) [K];  dL/dcolor likewise over K, or over every pixel with mask_color off
__global__ void __launch_bounds__(THREADS) backward_kernel(MaskedLossArgs a, const float* __restrict__ header,
                                                            const unsigned char* __restrict__ kept_mask,
                                                            const float* __restrict__ upstream, float* __restrict__ dcolor,
                                                            float* __restrict__ ddepth) {
    const float up = upstream ? *upstream : 1.f;
    const float u_d = up * header[0], u_c = up * header[1];
    const long HW = (long)a.H * a.W, n = (long)a.V * HW, stride = (long)gridDim.x * THREADS;
    for (long o = (long)blockIdx.x * THREADS + threadIdx.x; o < n; o += stride) {
        const bool kept = kept_mask[o] != 0;
        if (ddepth) ddepth[o] = kept ? u_d * sign0(a.depth[o] - a.depth_obs[o]) : 0.f;
        if (dcolor) {
            const long v = o / HW, oc = v * a.C * HW + (o - v * HW);
            const bool on = kept || !a.mask_color;
            for (int c = 0; c < a.C; c++)
                dcolor[oc + c * HW] = on ? u_c * sign0(a.color[oc + c * HW] - a.color_obs[oc + c * HW]) : 0.f;
        }
    }
}

inline long round16(long bytes) { return (bytes + 15) & ~15L; }

}  // namespace

bool masked_loss_shape_ok(int V, int H, int W) {
    // (a view per grid row; H * W bounded so that a histogram count fits 32 bits with room to spare)
    return V > 0 && H > 0 && W > 0 && V <= 65535 && (long)H * W <= (1L << 30);
}

MaskedLossLayout masked_loss_layout(int V, int H, int W) {
    MaskedLossLayout l{};
    if (!masked_loss_shape_ok(V, H, W)) return l;
    const long HW = (long)H * W, vpad = round16(4L * V);
    l.blocks = (int)std::min<long>((HW + PIXELS_PER_BLOCK - 1) / PIXELS_PER_BLOCK, std::max(STACK_BLOCKS / V, MIN_BLOCKS));
    l.chunk = (HW + l.blocks - 1) / l.blocks;
    l.median = 4L * HEADER_FLOATS;
    l.base = l.median + vpad;
    l.kept = l.base + vpad;
    l.view_sums = l.kept + vpad;
    l.hist = l.view_sums + 16L * V;
    l.slots = l.hist + 3L * V * BINS * 4;
    l.mask = l.slots + 4L * SLOT_WORDS * V * l.blocks;
    l.total = l.mask + round16((long)V * HW);
    return l;
}

hipError_t launch_masked_loss_forward(const MaskedLossArgs& a, void* scratch, float* loss, hipStream_t stream) {
    const MaskedLossLayout l = masked_loss_layout(a.V, a.H, a.W);
    char* s = static_cast<char*>(scratch);
    uint32_t* hist = reinterpret_cast<uint32_t*>(s + l.hist);
    float* median = reinterpret_cast<float*>(s + l.median);
    unsigned char* kept_mask = reinterpret_cast<unsigned char*>(s + l.mask);
    uint32_t* slots = reinterpret_cast<uint32_t*>(s + l.slots);
    const dim3 grid(l.blocks, a.V);
    if (a.reject) {
        const long n16 = 3L * a.V * BINS / 4;
        launch(clear_kernel, dim3((unsigned)std::min<long>((n16 + THREADS - 1) / THREADS, 1024)), dim3(THREADS), stream,
               reinterpret_cast<uint4*>(hist), n16);
        launch(select_kernel<0>, grid, dim3(THREADS), stream, a, hist, l.chunk);
        launch(select_kernel<1>, grid, dim3(THREADS), stream, a, hist, l.chunk);
        launch(select_kernel<2>, grid, dim3(THREADS), stream, a, hist, l.chunk);
        launch(loss_kernel<true>, grid, dim3(THREADS), stream, a, (const uint32_t*)hist, l.chunk, median, kept_mask, slots);
    } else {
        launch(loss_kernel<false>, grid, dim3(THREADS), stream, a, (const uint32_t*)hist, l.chunk, median, kept_mask, slots);
    }
    launch(final_kernel, dim3(1), dim3(THREADS), stream, a.V, l.blocks, (const uint32_t*)slots,
           (double)a.C * (double)a.H * (double)a.W * (double)a.V, a.C, a.w_color, a.w_depth, (int)a.mask_color, (int)a.mean,
           reinterpret_cast<int*>(s + l.base), reinterpret_cast<int*>(s + l.kept), reinterpret_cast<double*>(s + l.view_sums),
           reinterpret_cast<float*>(s), loss);
    return hipGetLastError();
}

hipError_t launch_masked_loss_backward(const MaskedLossArgs& a, const void* scratch, const float* upstream, float* dcolor,
                                       float* ddepth, hipStream_t stream) {
    const MaskedLossLayout l = masked_loss_layout(a.V, a.H, a.W);
    const char* s = static_cast<const char*>(scratch);
    const long n = (long)a.V * a.H * a.W;
    const unsigned blocks = (unsigned)std::min<long>((n + THREADS - 1) / THREADS, 2048);
    launch(backward_kernel, dim3(blocks), dim3(THREADS), stream, a, reinterpret_cast<const float*>(s),
           reinterpret_cast<const unsigned char*>(s + l.mask), upstream, dcolor, ddepth);
    return hipGetLastError();
}

}  // namespace dgr
