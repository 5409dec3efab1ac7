// transform.hip -- the map correction after a pose-graph update (include/dgr_hip.h: dgr_transform_*): every Gaussian moves with the
// keyframe it is anchored to, by that keyframe's Sim(3) transform.  In place on P rows, no host read: capturable.
//
// plan: one thread per transform, float64 -> one fp32 record (A, t, R, 1 / s, 1 / s^2, log s, q_R, the valid flag and the SH band
// matrices M_1, M_2, M_3, each value rounded once); then one workgroup counts the invalid transforms into counts[2] and resets the
// row counts.  M_l = Y_l(R d) Y_l^-1 over 2 l + 1 fixed directions (sh_rotation_table.h, written by gen_sh_rotation_table.py).
// apply: grid (256-row blocks, tensor groups).  A wave owns 64 consecutive rows; it reads each tensor's 64 rows as one contiguous span
// (16 bytes per lane where the span is whole and aligned) into its own LDS slab with an odd row stride, every lane rewrites its
// row there, and the span is written back the same way: the loads and stores are coalesced whatever k is, and nothing needs a
// workgroup barrier.  A wave none of whose rows is transformed touches nothing.  When all 64 rows share one anchor -- seeding
// appends a keyframe's rows together, so this is the common case -- the record's address is wave-uniform and its values are
// fetched once per wave by scalar loads; otherwise every lane reads its own record.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gaussian_math.h"
#include "kernels.h"
#include "plan.h"
#include "sh_rotation_table.h"

namespace dgr {
namespace {

// the record of one transform, in floats
constexpr int REC_A = 0, REC_T = 9, REC_R = 12, REC_INV_S = 21, REC_INV_S2 = 22, REC_LOG_S = 23, REC_Q = 24, REC_VALID = 28,
              REC_M1 = 32, REC_M2 = 41, REC_M3 = 66, REC_FLOATS = 116;
static_assert(REC_M3 + 49 <= REC_FLOATS && REC_FLOATS % 4 == 0, "a record is a whole number of 16-byte pieces");
constexpr size_t TRANSFORM_HEADER_BYTES = 64;

__device__ inline void sh_band64(int l, const double d[3], double* out) {  // gaussian_math.h's band l at d, in float64
    const double x = d[0], y = d[1], z = d[2];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    if (l == 1) {
        out[0] = -(double)SH_C1 * y, out[1] = (double)SH_C1 * z, out[2] = -(double)SH_C1 * x;
    } else if (l == 2) {
        out[0] = (double)SH_C2[0] * xy, out[1] = (double)SH_C2[1] * yz, out[2] = (double)SH_C2[2] * (2.0 * zz - xx - yy);
        out[3] = (double)SH_C2[3] * xz, out[4] = (double)SH_C2[4] * (xx - yy);
    } else {
        out[0] = (double)SH_C3[0] * y * (3.0 * xx - yy), out[1] = (double)SH_C3[1] * xy * z;
        out[2] = (double)SH_C3[2] * y * (4.0 * zz - xx - yy), out[3] = (double)SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
        out[4] = (double)SH_C3[4] * x * (4.0 * zz - xx - yy), out[5] = (double)SH_C3[5] * z * (xx - yy);
        out[6] = (double)SH_C3[6] * x * (xx - 3.0 * yy);
    }
}

// M_l = Y_l(R d) Y_l^-1, rounded once into rec[0 .. n * n)
__device__ inline void sh_band_matrix(int l, const double R[3][3], const double* yinv, float* rec) {
    const int n = 2 * l + 1;
    double Y[7][7];  // Y[i][k] = B_l,i(R d_k)
    for (int k = 0; k < n; ++k) {
        double d[3], col[7];
        for (int a = 0; a < 3; ++a) d[a] = R[a][0] * SH_ROT_DIRS[k][0] + R[a][1] * SH_ROT_DIRS[k][1] + R[a][2] * SH_ROT_DIRS[k][2];
        sh_band64(l, d, col);
        for (int i = 0; i < n; ++i) Y[i][k] = col[i];
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double m = 0.0;
            for (int k = 0; k < n; ++k) m += Y[i][k] * yinv[k * n + j];
            rec[i * n + j] = (float)m;
        }
}

__global__ void __launch_bounds__(256) transform_plan_kernel(int K, const float* __restrict__ transforms, void* scratch) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= K) return;
    float* rec = reinterpret_cast<float*>(static_cast<char*>(scratch) + TRANSFORM_HEADER_BYTES) + (size_t)k * REC_FLOATS;
    const float* T = transforms + (size_t)k * 16;
    bool finite = true;
    for (int e = 0; e < 16; ++e) finite = finite && fabsf(T[e]) <= 3.4028234664e38f;
    double A[3][3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) A[i][j] = (double)T[4 * i + j];
    }
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    bool valid = finite && det > 0.0;
    double s = 1.0;
    if (valid) {
        s = cbrt(det);
        double worst = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double g = (A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j]) / (s * s) - (i == j ? 1.0 : 0.0);
                worst = fmax(worst, fabs(g));
            }
        valid = worst <= 1e-3;
    }
    for (int e = 0; e < REC_FLOATS; ++e) rec[e] = 0.0f;  // (an invalid transform's record: all zero, the flag included)
    if (!valid) return;
    double N[3][3];  // A / s: a rotation up to the tolerance
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) N[i][j] = A[i][j] / s;
    // Shepperd: the largest of the trace and the three diagonal entries picks the component the others are divided by
    const double tr = N[0][0] + N[1][1] + N[2][2];
    double q[4];
    if (tr >= N[0][0] && tr >= N[1][1] && tr >= N[2][2]) {
        q[0] = 1.0 + tr, q[1] = N[2][1] - N[1][2], q[2] = N[0][2] - N[2][0], q[3] = N[1][0] - N[0][1];
    } else if (N[0][0] >= N[1][1] && N[0][0] >= N[2][2]) {
        q[0] = N[2][1] - N[1][2], q[1] = 1.0 + 2.0 * N[0][0] - tr, q[2] = N[0][1] + N[1][0], q[3] = N[0][2] + N[2][0];
    } else if (N[1][1] >= N[2][2]) {
        q[0] = N[0][2] - N[2][0], q[1] = N[0][1] + N[1][0], q[2] = 1.0 + 2.0 * N[1][1] - tr, q[3] = N[1][2] + N[2][1];
    } else {
        q[0] = N[1][0] - N[0][1], q[1] = N[0][2] + N[2][0], q[2] = N[1][2] + N[2][1], q[3] = 1.0 + 2.0 * N[2][2] - tr;
    }
    const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double r = q[0] * qn, x = q[1] * qn, y = q[2] * qn, z = q[3] * qn;
    const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y)},
                            {2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x)},
                            {2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y)}};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) rec[REC_A + 3 * i + j] = T[4 * i + j], rec[REC_R + 3 * i + j] = (float)R[i][j];
        rec[REC_T + i] = T[4 * i + 3];
    }
    rec[REC_INV_S] = (float)(1.0 / s), rec[REC_INV_S2] = (float)(1.0 / (s * s)), rec[REC_LOG_S] = (float)log(s);
    rec[REC_Q] = (float)r, rec[REC_Q + 1] = (float)x, rec[REC_Q + 2] = (float)y, rec[REC_Q + 3] = (float)z;
    rec[REC_VALID] = 1.0f;
    sh_band_matrix(1, R, SH_ROT_YINV1, rec + REC_M1);
    sh_band_matrix(2, R, SH_ROT_YINV2, rec + REC_M2);
    sh_band_matrix(3, R, SH_ROT_YINV3, rec + REC_M3);
}

// One workgroup: counts = {rows, 0, invalid transforms, 0}.  It runs after the plan kernel (rows = 0) and in front of every apply
// launch (rows = P), which takes the rows that stay off [0] and adds them to [1] or [3]: the counts are those of the last apply
// call, however many there were, and a map whose rows all move -- the usual one -- costs no atomic at all (one atomic per wave on
// the one address of [0] was measured at 95 us of a 190-us apply, profiles/transform/README.md).
__global__ void __launch_bounds__(256) transform_counts_kernel(int K, const void* scratch, int* __restrict__ counts, int rows) {
    __shared__ int wave_bad[4];
    const float* recs = reinterpret_cast<const float*>(static_cast<const char*>(scratch) + TRANSFORM_HEADER_BYTES);
    int bad = 0;
    for (int k = (int)threadIdx.x; k < K; k += 256) bad += recs[(size_t)k * REC_FLOATS + REC_VALID] == 0.0f;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bad += __shfl_down(bad, d);
    if ((threadIdx.x & 63) == 0) wave_bad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x < 4)
        counts[threadIdx.x] = threadIdx.x == 0 ? rows : threadIdx.x == 2 ? wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3] : 0;
}

using TransformTable = TensorTable<dgr_transform_tensor, DGR_TRANSFORM_MAX_TENSORS>;

// Pointers keep their address space across the call of the non-inlined routine below (a generic pointer would turn every access
// into a flat one): LDS for the slab, global for the tensors and the records
using lds_float = __attribute__((address_space(3))) float;
using lds_int = __attribute__((address_space(3))) int;
using g_float = __attribute__((address_space(1))) float;
// a record read through the constant address space: the plan wrote it in an earlier launch and nothing writes it here, and a
// wave-uniform address in that space is what makes the compiler use scalar loads inside a function that is not a kernel
using c_float = __attribute__((address_space(4))) const float;
typedef float v4f __attribute__((ext_vector_type(4)));
using g_v4f = __attribute__((address_space(1))) v4f;
constexpr int SLAB_LD_MAX = 49;  // the widest row (a combined shs leaf, 48 floats) at its odd stride

// A wave's `rows` consecutive rows of k floats, global <-> its slab (row stride k | 1: a lane walking its own row meets no bank
// conflict).  `whole`: all 64 rows are there and the span is 16-byte aligned.  On the way out only the rows with keep[row] >= 0
// are stored when `all` of them are not: an untouched row is not rewritten.
template <int KROW>
__device__ inline void rows_to_slab(const g_float* __restrict__ src, lds_float* slab, int rows, bool whole, int lane) {
    constexpr int LD = KROW | 1;
    if (whole) {
        const g_v4f* src4 = reinterpret_cast<const g_v4f*>(src);
#pragma unroll
        for (int e4 = 0; e4 < 16 * KROW; e4 += 64) {
            const int e = 4 * (e4 + lane);
            if (e4 + lane < 16 * KROW) {
                const v4f v = src4[e4 + lane];
                const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) slab[((e + c) / KROW) * LD + (e + c) % KROW] = f[c];
            }
        }
    } else {
        for (int e = lane; e < rows * KROW; e += 64) slab[(e / KROW) * LD + e % KROW] = src[e];
    }
}
template <int KROW>
__device__ inline void slab_to_rows(const lds_float* slab, g_float* __restrict__ dst, int rows, bool whole, bool all, const lds_int* keep,
                                    int lane) {
    constexpr int LD = KROW | 1;
    if (whole && all) {
        g_v4f* dst4 = reinterpret_cast<g_v4f*>(dst);
#pragma unroll
        for (int e4 = 0; e4 < 16 * KROW; e4 += 64) {
            const int e = 4 * (e4 + lane);
            if (e4 + lane < 16 * KROW) {
                float f[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) f[c] = slab[((e + c) / KROW) * LD + (e + c) % KROW];
                dst4[e4 + lane] = v4f{f[0], f[1], f[2], f[3]};
            }
        }
    } else {
        for (int e = lane; e < rows * KROW; e += 64) {
            const int row = e / KROW;
            if (keep[row] >= 0) dst[e] = slab[row * LD + e % KROW];
        }
    }
}

__device__ inline float sq_if(float m, bool sq) { return sq ? m * m : m; }

// out_i = sum_j W_ij in_j over j = 0 .. N - 1 in that order, W = M or (MOMENT2) its element-wise square; one channel of one band
template <int N, typename Rec>
__device__ inline void band_rotate(Rec M, bool sq, lds_float* c /* stride 3 */) {
    float in[N], out[N];
#pragma unroll
    for (int j = 0; j < N; ++j) in[j] = c[3 * j];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float acc = sq_if(M[i * N], sq) * in[0];
#pragma unroll
        for (int j = 1; j < N; ++j) acc = fmaf(sq_if(M[i * N + j], sq), in[j], acc);
        out[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) c[3 * i] = out[i];
}

// one row (k floats at `v`, in the slab) under the record `rec`
template <int KROW, typename Rec>
__device__ inline void transform_row(lds_float* v, int mode, Rec rec) {
    const int kind = mode & ~3, order = mode & 3;
    if constexpr (KROW == 3) {
        if (kind == DGR_TRANSFORM_LOG_SCALE) {
            const float ls = rec[REC_LOG_S];
            v[0] += ls, v[1] += ls, v[2] += ls;
            return;
        }
        const float x0 = v[0], x1 = v[1], x2 = v[2];
        if (order == DGR_TRANSFORM_VALUE) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                v[i] = fmaf(rec[REC_A + 3 * i + 2], x2, fmaf(rec[REC_A + 3 * i + 1], x1, fmaf(rec[REC_A + 3 * i], x0, rec[REC_T + i])));
        } else {
            const bool sq = order == DGR_TRANSFORM_MOMENT2;
            const float scale = sq ? rec[REC_INV_S2] : rec[REC_INV_S];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float a = sq_if(rec[REC_R + 3 * i], sq), b = sq_if(rec[REC_R + 3 * i + 1], sq), c = sq_if(rec[REC_R + 3 * i + 2], sq);
                v[i] = fmaf(c, x2, fmaf(b, x1, a * x0)) * scale;
            }
        }
    } else if constexpr (KROW == 4) {
        // L(q_R): the Hamilton product q_R (x) v as a matrix on v = (r, x, y, z)
        const bool sq = order == DGR_TRANSFORM_MOMENT2;
        const float a = rec[REC_Q], b = rec[REC_Q + 1], c = rec[REC_Q + 2], d = rec[REC_Q + 3];
        const float L[4][4] = {{a, -b, -c, -d}, {b, a, -d, c}, {c, d, a, -b}, {d, -c, b, a}};
        const float in[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            v[i] = fmaf(sq_if(L[i][3], sq), in[3], fmaf(sq_if(L[i][2], sq), in[2], fmaf(sq_if(L[i][1], sq), in[1], sq_if(L[i][0], sq) * in[0])));
    } else {
        const bool sq = order == DGR_TRANSFORM_MOMENT2;
        constexpr int SKIP = KROW == 12 || KROW == 27 || KROW == 48 ? 3 : 0;  // a combined shs leaf: the DC row stays
        constexpr int M = (KROW - SKIP) / 3;                                   // coefficients above the DC one: 3, 8 or 15
        lds_float* c = v + SKIP;
        // band by band, so that one band's matrix is live at a time
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) band_rotate<3>(rec + REC_M1, sq, c + ch);
        if constexpr (M >= 8) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) band_rotate<5>(rec + REC_M2, sq, c + 9 + ch);
        }
        if constexpr (M >= 15) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) band_rotate<7>(rec + REC_M3, sq, c + 24 + ch);
        }
    }
}

// One tensor's 64 rows.  Not inlined: one instance per row width, each with its own registers (inlined into the kernel's loop over
// the tensors, the eight instances' address arithmetic was hoisted out of it together and the kernel needed over 256 VGPRs).
template <int KROW>
__device__ __attribute__((noinline)) void transform_tensor(g_float* data, int mode, lds_float* slab, size_t row0, int rows, bool all,
                                                           const lds_int* keep, int a, bool uniform, const g_float* recs, int lane) {
    g_float* span = data + row0 * KROW;
    const bool whole = rows == 64 && (reinterpret_cast<uintptr_t>(data) & 15u) == 0u;
    rows_to_slab<KROW>(span, slab, rows, whole, lane);
    wave_sync();
    if (a >= 0) {
        lds_float* v = slab + lane * (KROW | 1);
        if (uniform) {  // one record for the wave: its address is made scalar, and its values come by scalar loads
            const uintptr_t p = reinterpret_cast<uintptr_t>(recs + (size_t)a * REC_FLOATS);
            const uintptr_t lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)p);
            const uintptr_t hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(p >> 32));
            transform_row<KROW>(v, mode, reinterpret_cast<c_float*>(hi << 32 | lo));
        } else {
            transform_row<KROW>(v, mode, recs + (size_t)a * REC_FLOATS);
        }
    }
    wave_sync();
    slab_to_rows<KROW>(slab, span, rows, whole, all, keep, lane);
    wave_sync();
}

// grid (row blocks, tensor groups)
__global__ void __launch_bounds__(256) transform_apply_kernel(size_t P, int K, const void* __restrict__ scratch,
                                                              const float* __restrict__ anchor, TransformTable table,
                                                              int* __restrict__ counts) {
    __shared__ float slabs[4][64 * SLAB_LD_MAX];
    __shared__ int keeps[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t row0 = (size_t)blockIdx.x * 256 + (size_t)wave * 64;
    if (row0 >= P) return;
    const int rows = P - row0 < 64 ? (int)(P - row0) : 64;
    const float* recs = reinterpret_cast<const float*>(static_cast<const char*>(scratch) + TRANSFORM_HEADER_BYTES);
    int a = -1;
    bool named = false;  // the row names a transform: an integer anchor in 0 .. K - 1
    if (lane < rows) {
        const float av = anchor ? anchor[row0 + lane] : 0.0f;
        named = av >= 0.0f && av < (float)K && av == truncf(av);  // (false on a NaN)
        if (named && recs[(size_t)(int)av * REC_FLOATS + REC_VALID] != 0.0f) a = (int)av;
    }
    const unsigned long long moved = __ballot(a >= 0);
    const int n_moved = __popcll(moved), n_named = __popcll(__ballot(named));
    if (blockIdx.y == 0 && lane == 0) {  // (integer atomics: the counts do not depend on the order)
        if (rows - n_moved) atomicSub(counts, rows - n_moved);
        if (rows - n_named) atomicAdd(counts + 1, rows - n_named);
        if (n_named - n_moved) atomicAdd(counts + 3, n_named - n_moved);
    }
    if (moved == 0ull) return;  // (the whole wave; no workgroup barrier follows)
    keeps[wave][lane] = a;
    const bool all = n_moved == rows;
    const bool uniform = all && __ballot(a == __builtin_amdgcn_readfirstlane(a)) == moved;
    lds_float* slab = (lds_float*)slabs[wave];
    const lds_int* keep = (const lds_int*)keeps[wave];
    for (int t = table.begin[blockIdx.y]; t < table.begin[blockIdx.y + 1]; ++t) {
        const dgr_transform_tensor d = table.t[t];
#define DGR_TRANSFORM_CASE(KROW)                                                                \
    case KROW:                                                                                   \
        transform_tensor<KROW>((g_float*)d.data, d.mode, slab, row0, rows, all, keep, a, uniform, (const g_float*)recs, lane); \
        break;
        switch (d.k) {
            DGR_TRANSFORM_CASE(3)
            DGR_TRANSFORM_CASE(4)
            DGR_TRANSFORM_CASE(9)
            DGR_TRANSFORM_CASE(12)
            DGR_TRANSFORM_CASE(24)
            DGR_TRANSFORM_CASE(27)
            DGR_TRANSFORM_CASE(45)
            DGR_TRANSFORM_CASE(48)
        }
#undef DGR_TRANSFORM_CASE
    }
}

}  // namespace

size_t transform_scratch_bytes(size_t K) { return TRANSFORM_HEADER_BYTES + K * REC_FLOATS * sizeof(float); }

hipError_t launch_transform_plan(int K, const float* transforms, void* scratch, int* counts, hipStream_t stream) {
    launch(transform_plan_kernel, dim3((unsigned)plan_blocks((size_t)K)), dim3(256), stream, K, transforms, scratch);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    launch(transform_counts_kernel, dim3(1), dim3(256), stream, K, (const void*)scratch, counts, 0);
    return hipGetLastError();
}

hipError_t launch_transform_apply(size_t P, int K, const void* scratch, const float* anchor, int n,
                                  const dgr_transform_tensor* tensors, int* counts, hipStream_t stream) {
    launch(transform_counts_kernel, dim3(1), dim3(256), stream, K, scratch, counts, (int)P);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || P == 0) return e;
    TransformTable table = {};
    const int groups = deal_tensors(table, tensors, n, [](const dgr_transform_tensor& t) { return (t.k + 3) / 4; });
    launch(transform_apply_kernel, dim3((unsigned)plan_blocks(P), (unsigned)groups), dim3(256), stream, P, K, scratch, anchor, table,
           counts);
    return hipGetLastError();
}

}  // namespace dgr
