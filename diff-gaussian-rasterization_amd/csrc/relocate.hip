// relocate.hip -- fixed-size map upkeep (include/dgr_hip.h: dgr_relocate_*, dgr_position_noise): 3DGS-MCMC's relocation of dead
// Gaussians onto live ones drawn in proportion to their opacity, and its gated position noise.  Both work in place on P rows: no
// tensor is reallocated and nothing is read on the host, so the steps can be recorded into a hipGraph.
//
// Relocation, six launches.  weights: one thread per row -> dead / live, the integer weight w = rint(2^20 o) (o in float64), the
// row's exclusive prefix of w inside its 256-row block (block_scan.h) and the block's totals (64-bit weight, dead, live); it also
// clears `hits` and `source`.  scan: one workgroup turns the block totals into exclusive offsets (plan.h's scan_block_totals over
// this file's record), S and counts[0..2].  sample: one thread per dead
// row -> its draw's target t = (d S) >> 32, a binary search over the block offsets, then over the block's 256 prefixes, one integer
// atomic on the source's hit count.  values: one thread per hit source -> its new opacity o' and log(coeff), in float64.  apply,
// twice over the tensor table: the relocated rows (they read live rows and the saved values, they write dead rows), then the hit
// sources (each rewrites itself from the saved values): no row is read while it is rewritten.  A workgroup takes one 256-row block
// of one tensor group, compacts the block's touched rows (ballot + mbcnt) and streams only those.
// Everything that decides is integer arithmetic, everything that is written is a pure function of the source row: the result is the
// same bits on every run, whatever the grid.
//
// scratch: u64 S in a 64-byte header; {u64 weight, int dead, int live} per block (totals, then exclusive offsets); u32 prefix[P];
// int hits[P]; int source[P]; double o'[P]; double log(coeff)[P] (the last two written at hit sources only).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_scan.h"
#include "kernels.h"
#include "philox.h"
#include "plan.h"

namespace dgr {
namespace {

struct RelocateBlock {  // a block's totals, after the scan its exclusive offsets
    unsigned long long w;
    int dead, live;
};
static_assert(sizeof(RelocateBlock) == 16, "one 16-byte record per block");
// the record of plan.h's scan_block_totals (the 64-bit weight shuffled as two words)
__device__ inline RelocateBlock totals_zero(const RelocateBlock*) { return {0ull, 0, 0}; }
__device__ inline RelocateBlock totals_add(RelocateBlock a, RelocateBlock b) { return {a.w + b.w, a.dead + b.dead, a.live + b.live}; }
__device__ inline RelocateBlock totals_sub(RelocateBlock a, RelocateBlock b) { return {a.w - b.w, a.dead - b.dead, a.live - b.live}; }
__device__ inline RelocateBlock totals_shfl_up(RelocateBlock v, int d) {
    const unsigned lo = __shfl_up((unsigned)v.w, d), hi = __shfl_up((unsigned)(v.w >> 32), d);
    return {(unsigned long long)hi << 32 | lo, __shfl_up(v.dead, d), __shfl_up(v.live, d)};
}

constexpr size_t RELOCATE_HEADER_BYTES = 64;
constexpr int RELOCATE_MAX_COPIES = 51;  // N = min(hits + 1, 51): 3DGS-MCMC's binomial table ends there

struct RelocateLayout {  // byte offsets into the scratch buffer (each a multiple of 16)
    size_t table, prefix, hits, source, o_new, log_coeff, total;
};
__host__ __device__ inline RelocateLayout relocate_layout(size_t P) {
    const size_t words = ((P + 3) & ~(size_t)3) * 4, doubles = ((P + 1) & ~(size_t)1) * 8;
    RelocateLayout l;
    l.table = RELOCATE_HEADER_BYTES;
    l.prefix = l.table + plan_blocks(P) * sizeof(RelocateBlock);
    l.hits = l.prefix + words;
    l.source = l.hits + words;
    l.o_new = l.source + words;
    l.log_coeff = l.o_new + doubles;
    l.total = l.log_coeff + doubles;
    return l;
}
template <typename T, typename V>
__device__ inline T* at(V* scratch, size_t offset) {
    return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(scratch) + offset);
}

__device__ inline bool finite_f(float v) { return fabsf(v) <= 3.4028234664e38f; }  // false on NaN and +-inf
__device__ inline double sigmoid64(float raw) { return 1.0 / (1.0 + exp(-(double)raw)); }

__global__ void __launch_bounds__(256) relocate_weight_kernel(size_t P, const float* __restrict__ opacity_raw, float thr,
                                                              void* scratch, int* __restrict__ source) {
    __shared__ uint32_t wave_w[4];
    __shared__ int wave_dead[4], wave_live[4];
    const RelocateLayout l = relocate_layout(P);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t w = 0u;
    bool dead = false, live = false;
    if (i < P) {
        const float raw = opacity_raw[i];
        if (finite_f(raw)) {
            dead = raw < thr;
            live = !dead;
            if (live) w = (unsigned)rint(1048576.0 * sigmoid64(raw));
        }
        at<int>(scratch, l.hits)[i] = 0;
        at<int>(scratch, l.source)[i] = -1;
        source[i] = -1;
    }
    const int n_dead = __popcll(__ballot(dead)), n_live = __popcll(__ballot(live));
    if (lane == 0) wave_dead[wave] = n_dead, wave_live[wave] = n_live;
    uint32_t total;  // (a block's total is at most 256 * 2^20)
    const uint32_t before = block_exclusive_scan<256>(w, wave_w, (int)threadIdx.x, &total);  // (its barrier covers the counts too)
    if (i < P) at<unsigned>(scratch, l.prefix)[i] = before;
    if (threadIdx.x == 0) {
        RelocateBlock t;
        t.w = total;
        t.dead = wave_dead[0] + wave_dead[1] + wave_dead[2] + wave_dead[3];
        t.live = wave_live[0] + wave_live[1] + wave_live[2] + wave_live[3];
        at<RelocateBlock>(scratch, l.table)[blockIdx.x] = t;
    }
}

// One workgroup: exclusive scan of the block totals in place (plan.h); then S and counts[0..7] = {dead, live, relocated, 0, 0, 0,
// 0, 0} (the sample kernel counts the hit sources and the largest hit count into [3] and [4]).
__global__ void __launch_bounds__(256) relocate_scan_kernel(size_t P, void* scratch, int* __restrict__ counts) {
    __shared__ RelocateBlock wave_sum[4];
    const RelocateBlock carry = scan_block_totals(at<RelocateBlock>(scratch, relocate_layout(P).table), plan_blocks(P), wave_sum);
    if (threadIdx.x == 0) *at<unsigned long long>(scratch, 0) = carry.w;
    if (threadIdx.x < 8) {
        const int t = (int)threadIdx.x;
        counts[t] = t == 0 ? carry.dead : t == 1 ? carry.live : t == 2 ? (carry.w > 0ull ? carry.dead : 0) : 0;
    }
}

// One thread per row; a dead row draws its source.  t < S, so the last block whose offset is <= t has a positive total and the
// last row of it whose prefix is <= t - offset a positive weight: that row is the i with C_i <= t < C_i + w_i.
__global__ void __launch_bounds__(256) relocate_sample_kernel(size_t P, const float* __restrict__ opacity_raw, float thr,
                                                              const long long* __restrict__ draws, unsigned long long seed,
                                                              int step, const int* __restrict__ step_dev, void* scratch,
                                                              int* __restrict__ counts, int* __restrict__ source) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= P) return;
    const float raw = opacity_raw[r];
    if (!(finite_f(raw) && raw < thr)) return;
    const unsigned long long S = *at<const unsigned long long>(scratch, 0);
    if (S == 0ull) return;
    const RelocateLayout l = relocate_layout(P);
    if (step_dev) step = *step_dev;
    const unsigned d = draws ? (unsigned)draws[r] : philox_words(seed, r, (unsigned)step, 1u).x;
    const unsigned long long t = __umul64hi((unsigned long long)d << 32, S);  // (d S) >> 32, exact
    const RelocateBlock* table = at<const RelocateBlock>(scratch, l.table);
    size_t lo = 0, hi = plan_blocks(P) - 1;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (table[mid].w <= t) lo = mid;
        else hi = mid - 1;
    }
    const size_t base = lo * 256;
    const unsigned rest = (unsigned)(t - table[lo].w);
    const unsigned* prefix = at<const unsigned>(scratch, l.prefix) + base;
    unsigned a = 0u, b = (unsigned)(P - base < 256 ? P - base : 256) - 1u;
    while (a < b) {
        const unsigned mid = a + (b - a + 1u) / 2u;
        if (prefix[mid] <= rest) a = mid;
        else b = mid - 1u;
    }
    const size_t i = base + a;
    at<int>(scratch, l.source)[r] = (int)i;
    source[r] = (int)i;
    const int old = atomicAdd(at<int>(scratch, l.hits) + i, 1);
    if (old == 0) atomicAdd(counts + 3, 1);
    atomicMax(counts + 4, old + 1);
}

// One thread per row; a hit source forms, in float64, the opacity o' of each of its N copies and the log of the scale factor that
// keeps the N copies' rendered sum what the one's was (3DGS-MCMC eq. 9; the sums in the header's order).
__global__ void __launch_bounds__(256) relocate_values_kernel(size_t P, const float* __restrict__ opacity_raw, void* scratch) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const RelocateLayout l = relocate_layout(P);
    const int hits = at<const int>(scratch, l.hits)[i];
    if (hits <= 0) return;
    const int N = hits + 1 < RELOCATE_MAX_COPIES ? hits + 1 : RELOCATE_MAX_COPIES;
    const double o = sigmoid64(opacity_raw[i]);
    const double o1 = 1.0 - pow(1.0 - o, 1.0 / (double)N);
    double D = 0.0;
    for (int m = 1; m <= N; ++m) {
        double binom = 1.0, p = o1;  // C(m - 1, k) (exact: below 2^53 up to C(50, 25)) and o'^(k + 1)
        for (int k = 0; k < m; ++k) {
            const double term = binom * (1.0 / sqrt((double)(k + 1))) * p;
            D += (k & 1) ? -term : term;
            binom = binom * (double)(m - 1 - k) / (double)(k + 1);
            p *= o1;
        }
    }
    at<double>(scratch, l.o_new)[i] = o1;
    at<double>(scratch, l.log_coeff)[i] = log(o / D);
}

using RelocateTable = TensorTable<dgr_relocate_tensor, DGR_RELOCATE_MAX_TENSORS>;

__device__ inline float new_opacity_raw(double o1, double min_opacity) {
    const double c = fmin(fmax(o1, min_opacity), 1.0 - 0x1p-23);
    return (float)log(c / (1.0 - c));
}
__device__ inline void set_zero(float& v) { v = 0.0f; }
__device__ inline void set_zero(float4& v) { v = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// The block's n touched rows (`list`: their indices in the block) of one tensor, as elements of T (float, or float4 for the COPY
// and ZERO modes when k is a multiple of 4 and the tensor 16-byte aligned).  take: the row whose values a touched row receives
// (pass 0: its source; pass 1: itself).
template <typename T>
__device__ inline void apply_rows(const int* list, unsigned n, size_t base, const dgr_relocate_tensor& d, unsigned k, int pass,
                                  const int* __restrict__ source, const double* __restrict__ o_new,
                                  const double* __restrict__ log_coeff, double min_opacity) {
    T* data = reinterpret_cast<T*>(d.data);
    const int mode = d.mode;
    for (unsigned e = threadIdx.x; e < n * k; e += 256u) {
        const unsigned j = e / k, c = e - j * k;
        const size_t row = base + (size_t)list[j];
        const size_t take = pass == 0 ? (size_t)source[row] : row;
        T v;
        set_zero(v);
        if (mode == DGR_RELOCATE_COPY) v = data[take * k + c];
        if constexpr (sizeof(T) == sizeof(float)) {
            if (mode == DGR_RELOCATE_OPACITY) v = new_opacity_raw(o_new[take], min_opacity);
            if (mode == DGR_RELOCATE_LOG_SCALE) v = (float)((double)data[take * k + c] + log_coeff[take]);
        }
        data[row * k + c] = v;
    }
}

// grid (row blocks, tensor groups).  pass 0: the relocated rows; pass 1: the hit sources.
__global__ void __launch_bounds__(256) relocate_apply_kernel(size_t P, const void* __restrict__ scratch, RelocateTable table,
                                                             int pass, double min_opacity) {
    __shared__ int list[256];
    __shared__ int wave_tot[4];
    const RelocateLayout l = relocate_layout(P);
    const int* source = at<const int>(scratch, l.source);
    const size_t base = (size_t)blockIdx.x * 256, i = base + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool touched = i < P && (pass == 0 ? source[i] >= 0 : at<const int>(scratch, l.hits)[i] > 0);
    const unsigned long long m = __ballot(touched);
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    int rank = lane_rank(m);
    for (int v = 0; v < wave; ++v) rank += wave_tot[v];
    const unsigned n = (unsigned)(wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3]);
    if (n == 0u) return;  // (the whole workgroup: most blocks of a healthy map)
    if (touched) list[rank] = (int)threadIdx.x;
    __syncthreads();
    const double* o_new = at<const double>(scratch, l.o_new);
    const double* log_coeff = at<const double>(scratch, l.log_coeff);
    for (int t = table.begin[blockIdx.y]; t < table.begin[blockIdx.y + 1]; ++t) {
        const dgr_relocate_tensor d = table.t[t];
        const bool moves = d.mode == DGR_RELOCATE_COPY, zeroes = d.mode == DGR_RELOCATE_ZERO_TOUCHED || d.mode == DGR_RELOCATE_ZERO_RELOCATED;
        if (pass == 1 && (moves || d.mode == DGR_RELOCATE_ZERO_RELOCATED)) continue;  // a source keeps these
        const unsigned k = (unsigned)d.k;
        if ((moves || zeroes) && (k & 3u) == 0u && (reinterpret_cast<uintptr_t>(d.data) & 15u) == 0u)
            apply_rows<float4>(list, n, base, d, k / 4, pass, source, o_new, log_coeff, min_opacity);
        else
            apply_rows<float>(list, n, base, d, k, pass, source, o_new, log_coeff, min_opacity);
    }
}

// One thread per row: xyz += g Sigma n, Sigma = R S^2 R^T (3DGS's build_rotation of q / |q|, S = diag(exp(scaling_raw))).
__global__ void __launch_bounds__(256) position_noise_kernel(size_t P, float* __restrict__ xyz, const float* __restrict__ scaling_raw,
                                                             const float* __restrict__ rotation,
                                                             const float* __restrict__ opacity_raw, const float* __restrict__ noise,
                                                             unsigned long long seed, int step, const int* __restrict__ step_dev,
                                                             float lr, const float* __restrict__ lr_dev, float scale, float gate_k,
                                                             float gate_x0) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    if (step_dev) step = *step_dev;
    if (lr_dev) lr = *lr_dev;
    const float o = 1.0f / (1.0f + expf(-opacity_raw[i]));
    const float z = gate_k * (1.0f - o - gate_x0);  // the gate 1 / (1 + exp(-z)), in the form that does not overflow
    const float ez = expf(-fabsf(z));
    const float g = scale * lr * (z >= 0.0f ? 1.0f / (1.0f + ez) : ez / (1.0f + ez));
    float n[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) n[j] = noise ? noise[3 * i + j] : philox_normal(seed, i, (unsigned)step, j);
    float r = rotation[4 * i], x = rotation[4 * i + 1], y = rotation[4 * i + 2], zq = rotation[4 * i + 3];
    const float inv = 1.0f / sqrtf(r * r + x * x + y * y + zq * zq);
    r *= inv, x *= inv, y *= inv, zq *= inv;
    const float R[3][3] = {{1.0f - 2.0f * (y * y + zq * zq), 2.0f * (x * y - r * zq), 2.0f * (x * zq + r * y)},
                           {2.0f * (x * y + r * zq), 1.0f - 2.0f * (x * x + zq * zq), 2.0f * (y * zq - r * x)},
                           {2.0f * (x * zq - r * y), 2.0f * (y * zq + r * x), 1.0f - 2.0f * (x * x + y * y)}};
    float s2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float s = expf(scaling_raw[3 * i + a]);
        s2[a] = s * s;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float cov = R[c][0] * s2[0] * R[j][0] + R[c][1] * s2[1] * R[j][1] + R[c][2] * s2[2] * R[j][2];
            acc += cov * n[j];
        }
        xyz[3 * i + c] += g * acc;
    }
}

}  // namespace

size_t relocate_scratch_bytes(size_t P) { return relocate_layout(P).total; }

hipError_t launch_relocate_plan(size_t P, const float* opacity_raw, float opacity_raw_min, const long long* draws,
                                unsigned long long seed, int step, const int* step_dev, void* scratch, int* counts, int* source,
                                hipStream_t stream) {
    const unsigned blocks = (unsigned)plan_blocks(P);
    if (blocks) {
        launch(relocate_weight_kernel, dim3(blocks), dim3(256), stream, P, opacity_raw, opacity_raw_min, scratch, source);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    launch(relocate_scan_kernel, dim3(1), dim3(256), stream, P, scratch, counts);  // (no blocks: it writes zero counts)
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !blocks) return e;
    launch(relocate_sample_kernel, dim3(blocks), dim3(256), stream, P, opacity_raw, opacity_raw_min, draws, seed, step, step_dev,
           scratch, counts, source);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    launch(relocate_values_kernel, dim3(blocks), dim3(256), stream, P, opacity_raw, scratch);
    return hipGetLastError();
}

hipError_t launch_relocate_apply(size_t P, const void* scratch, int n, const dgr_relocate_tensor* tensors, double min_opacity,
                                 hipStream_t stream) {
    if (P == 0) return hipSuccess;
    RelocateTable table = {};
    const int groups = deal_tensors(table, tensors, n, [](const dgr_relocate_tensor& t) { return t.k % 4 == 0 ? t.k / 4 : t.k; });
    for (int pass = 0; pass < 2; ++pass) {
        launch(relocate_apply_kernel, dim3((unsigned)plan_blocks(P), (unsigned)groups), dim3(256), stream, P, scratch, table, pass,
               min_opacity);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_position_noise(size_t P, float* xyz, const float* scaling_raw, const float* rotation, const float* opacity_raw,
                                 const float* noise, unsigned long long seed, int step, const int* step_dev, float lr,
                                 const float* lr_dev, float scale, float k, float x0, hipStream_t stream) {
    if (P == 0) return hipSuccess;
    launch(position_noise_kernel, dim3((unsigned)plan_blocks(P)), dim3(256), stream, P, xyz, scaling_raw, rotation, opacity_raw,
           noise, seed, step, step_dev, lr, lr_dev, scale, k, x0);
    return hipGetLastError();
}

}  // namespace dgr
