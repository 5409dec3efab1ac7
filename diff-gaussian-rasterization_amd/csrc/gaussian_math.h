// gaussian_math.h -- device math of the per-Gaussian kernels (preprocess_fwd.hip, preprocess_bwd.hip): the 3x3 algebra, the
// camera transforms, the 2D / 3D covariance and its backward, the SH rows and their transposition through LDS.
//
// The arithmetic is written in the reference's association order with FMA contraction OFF: radii, tile rects and depth
// bits -- the integer path -- then agree bit for bit with the CPU oracle.  The pragma below governs everything defined
// here and, being at file scope, everything behind this header in the translation unit that includes it.
#pragma once
#include "dgr_common.h"

#pragma clang fp contract(off)

namespace dgr {
namespace {

// column-major 3x3: m[c][r]; (A*B)[c][r] = A[0][r]B[c][0] + A[1][r]B[c][1] + A[2][r]B[c][2]
struct M3 {
    float m[3][3];
};
__device__ __forceinline__ M3 mul(const M3& A, const M3& B) {
    M3 R;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) R.m[c][r] = A.m[0][r] * B.m[c][0] + A.m[1][r] * B.m[c][1] + A.m[2][r] * B.m[c][2];
    return R;
}
__device__ __forceinline__ M3 transpose(const M3& A) {
    M3 R;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) R.m[c][r] = A.m[r][c];
    return R;
}
__device__ __forceinline__ float dot3(float3 a, float3 b) {
    float tx = a.x * b.x, ty = a.y * b.y, tz = a.z * b.z;
    return tx + ty + tz;
}

__device__ __forceinline__ float3 xform4x3(float3 p, const float* m) {
    return make_float3(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]);
}
__device__ __forceinline__ float4 xform4x4(float3 p, const float* m) {
    return make_float4(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14], m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15]);
}

__device__ __forceinline__ float ndc2pix(float v, int S) { return (float)((((double)v + 1.0) * (double)S - 1.0) * 0.5); }

__device__ __forceinline__ void get_rect(float px, float py, int r, int gx, int gy, int& x0, int& y0, int& x1, int& y1) {
    x0 = min(gx, max(0, (int)((px - (float)r) / (float)DGR_BLOCK_X)));
    y0 = min(gy, max(0, (int)((py - (float)r) / (float)DGR_BLOCK_Y)));
    x1 = min(gx, max(0, (int)((px + (float)r + (float)DGR_BLOCK_X - 1.0f) / (float)DGR_BLOCK_X)));
    y1 = min(gy, max(0, (int)((py + (float)r + (float)DGR_BLOCK_Y - 1.0f) / (float)DGR_BLOCK_Y)));
}

constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
__device__ const float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                   -1.0925484305920792f, 0.5462742152960396f};
__device__ const float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                   0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                   -0.5900435899266435f};

__device__ __forceinline__ float3 operator+(float3 a, float3 b) { return make_float3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ float3 operator-(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float3 operator*(float s, float3 a) { return make_float3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float3 operator*(float3 a, float s) { return make_float3(a.x * s, a.y * s, a.z * s); }

// Loads the SH coefficients a degree needs into registers.  M == 16 rows are 192 B = 12 x 16 B, so a
// lane fetches whole 16-B pieces; consecutive lanes cover one contiguous 12 KB span per wave.
struct SHCoeffs {
    float3 c[16];
};
__device__ __forceinline__ void load_sh(const float* __restrict__ shs, int idx, int deg, int M, bool vec_ok, SHCoeffs& s) {
    const int ncoef = (deg + 1) * (deg + 1);
    if (vec_ok && M == 16) {
        const float4* p = reinterpret_cast<const float4*>(shs + (size_t)idx * 48);
        float f[48];
        const int nvec = (3 * ncoef + 3) >> 2;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            float4 v = (i < nvec) ? p[i] : make_float4(0, 0, 0, 0);
            f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
        }
#pragma unroll
        for (int k = 0; k < 16; k++) s.c[k] = make_float3(f[3 * k], f[3 * k + 1], f[3 * k + 2]);
    } else {
        const float* p = shs + (size_t)idx * M * 3;
#pragma unroll
        for (int k = 0; k < 16; k++)
            s.c[k] = (k < ncoef && k < M) ? make_float3(p[3 * k], p[3 * k + 1], p[3 * k + 2]) : make_float3(0, 0, 0);
    }
}

// */cuda_rasterizer/forward.cu:74-113 up to `cov` (before the +0.3 low-pass), shared with the backward.
struct Cov2D {
    float3 t;
    float txtz, tytz;
    M3 W, T, Vrk, cov;
};
__device__ __forceinline__ void cov2d_common(float3 mean, float fx, float fy, float tanx, float tany, const float* c3,
                                             const float* v, Cov2D& o) {
    float3 t = xform4x3(mean, v);
    const float limx = 1.3f * tanx, limy = 1.3f * tany;
    o.txtz = t.x / t.z;
    o.tytz = t.y / t.z;
    t.x = fminf(limx, fmaxf(-limx, o.txtz)) * t.z;
    t.y = fminf(limy, fmaxf(-limy, o.tytz)) * t.z;
    o.t = t;
    M3 J;
    J.m[0][0] = fx / t.z; J.m[0][1] = 0.0f; J.m[0][2] = -(fx * t.x) / (t.z * t.z);
    J.m[1][0] = 0.0f; J.m[1][1] = fy / t.z; J.m[1][2] = -(fy * t.y) / (t.z * t.z);
    J.m[2][0] = 0.0f; J.m[2][1] = 0.0f; J.m[2][2] = 0.0f;
    o.W.m[0][0] = v[0]; o.W.m[0][1] = v[4]; o.W.m[0][2] = v[8];
    o.W.m[1][0] = v[1]; o.W.m[1][1] = v[5]; o.W.m[1][2] = v[9];
    o.W.m[2][0] = v[2]; o.W.m[2][1] = v[6]; o.W.m[2][2] = v[10];
    o.T = mul(o.W, J);
    o.Vrk.m[0][0] = c3[0]; o.Vrk.m[0][1] = c3[1]; o.Vrk.m[0][2] = c3[2];
    o.Vrk.m[1][0] = c3[1]; o.Vrk.m[1][1] = c3[3]; o.Vrk.m[1][2] = c3[4];
    o.Vrk.m[2][0] = c3[2]; o.Vrk.m[2][1] = c3[4]; o.Vrk.m[2][2] = c3[5];
    o.cov = mul(mul(transpose(o.T), transpose(o.Vrk)), o.T);
}

__device__ __forceinline__ void quat_to_R(const float4 q, M3& R) {
    const float r = q.x, x = q.y, y = q.z, z = q.w;  // not normalised (forward.cu:127)
    R.m[0][0] = 1.f - 2.f * (y * y + z * z); R.m[0][1] = 2.f * (x * y - r * z); R.m[0][2] = 2.f * (x * z + r * y);
    R.m[1][0] = 2.f * (x * y + r * z); R.m[1][1] = 1.f - 2.f * (x * x + z * z); R.m[1][2] = 2.f * (y * z - r * x);
    R.m[2][0] = 2.f * (x * z - r * y); R.m[2][1] = 2.f * (y * z + r * x); R.m[2][2] = 1.f - 2.f * (x * x + y * y);
}
__device__ __forceinline__ M3 diag3(float a, float b, float c) {
    M3 S;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) S.m[i][j] = 0.0f;
    S.m[0][0] = a; S.m[1][1] = b; S.m[2][2] = c;
    return S;
}

// Row idx of a dense [P, 3] / [P, 4] float array (means, scales, colours / rotations), read ...
__device__ __forceinline__ float3 load_row3(const float* p, int idx) { return make_float3(p[3 * idx], p[3 * idx + 1], p[3 * idx + 2]); }
__device__ __forceinline__ float4 load_row4(const float* p, int idx) {
    return make_float4(p[4 * idx], p[4 * idx + 1], p[4 * idx + 2], p[4 * idx + 3]);
}
// ... and written: three floats, the six covariance terms, a 16-byte aligned float4.  (Every dense output of the backward may
// be NULL -- a tracking step needs the pose gradient only, dgr_hip.h -- the test stays with the caller: cov3d_bwd_kernel has none.)
__device__ __forceinline__ void store_row3(float* dst, int idx, float3 v) {
    dst[3 * (size_t)idx + 0] = v.x;
    dst[3 * (size_t)idx + 1] = v.y;
    dst[3 * (size_t)idx + 2] = v.z;
}
__device__ __forceinline__ void store_row6(float* dst, int idx, const float (&v)[6]) {
#pragma unroll
    for (int i = 0; i < 6; i++) dst[6 * (size_t)idx + i] = v[i];
}
__device__ __forceinline__ void store_row4(float* dst, int idx, float4 v) { reinterpret_cast<float4*>(dst)[idx] = v; }

// computeCov3D (forward.cu:118-152): M = S*R, Sigma = M^T M
__device__ __forceinline__ void compute_cov3d(const float* __restrict__ scales, const float* __restrict__ rotations, float mod, int idx,
                                              float (&c3)[6]) {
    const float3 sc = load_row3(scales, idx);
    const float4 q = load_row4(rotations, idx);
    M3 R;
    quat_to_R(q, R);
    const M3 S = diag3(mod * sc.x, mod * sc.y, mod * sc.z);
    const M3 Mm = mul(S, R);
    const M3 Sigma = mul(transpose(Mm), Mm);
    c3[0] = Sigma.m[0][0]; c3[1] = Sigma.m[0][1]; c3[2] = Sigma.m[0][2];
    c3[3] = Sigma.m[1][1]; c3[4] = Sigma.m[1][2]; c3[5] = Sigma.m[2][2];
}
// The 3D covariance of Gaussian idx for the forward and the backward alike (Args = PreprocessFwdArgs / PreprocessBwdArgs): the
// caller's, else re-formed from scale and rotation.  The forward does not keep it for the backward, which reads scale and
// rotation anyway: the same expression gives the same bits -- 24 bytes less written there and read here per Gaussian, and a
// view that culled the Gaussian never stored it.
template <class Args>
__device__ __forceinline__ void load_cov3d(const Args& a, int idx, float (&c3)[6]) {
    if (a.cov3D_precomp) {
        const float* c3p = a.cov3D_precomp + 6 * (size_t)idx;
#pragma unroll
        for (int i = 0; i < 6; i++) c3[i] = c3p[i];
    } else {
        compute_cov3d(a.scales, a.rotations, a.scale_modifier, idx, c3);
    }
}

}  // namespace

// ---- SH rows <-> lanes through LDS
// A lane that reads (or writes) its own 192-byte SH row touches 12 cache lines, one per instruction, and a wave
// instruction 64 different lines: four times the requests the data needs.  Here a wave moves the rows of 32 Gaussians
// at a time with contiguous 1-KB accesses and transposes them in LDS (row stride 52 dwords: b128-aligned, and the 64
// lanes' rows fall on all banks evenly).  Used for blocks that lie entirely inside [0, P).
constexpr int SHT_ROWS = 32, SHT_LD = 52;
// Every wave transposes through ITS OWN slab of the buffer, so the stores and the loads that follow them need no
// workgroup barrier: the LDS executes one wave's instructions in order; the fence keeps the compiler from reordering.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// A 16-byte store that is not kept in the caches: the dL_dsh rows (96 MB per view) are written once and read by nobody here.
// Left dirty in L2 / the memory-side cache they were written back under the NEXT kernel's reads: preprocess_fwd of the following
// view 45 -> 39.5 us, the view 0.513 -> 0.508 ms one at a time (profiles/r6/ab_nontemporal.txt).
__device__ __forceinline__ void store_streaming(float4* dst, float4 v) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(v4f{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f*>(dst));
}
// ... and a 16-byte load likewise: the SH rows (96 MB per view, read once by preprocess_fwd) no longer push the render records
// the same kernel writes out of the caches in front of the forward blend's gathers: one view at a time 0.510 -> 0.501 ms
// (preprocess_fwd -1 us, bin_tiles -0.7, render_fwd -2.5), several views in flight unchanged.
__device__ __forceinline__ float4 load_streaming(const float4* src) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(src));
    return make_float4(v.x, v.y, v.z, v.w);
}
// `need`: the wave's ballot of the lanes that will use their row.  Only those rows are fetched: piece e of slab r belongs to
// Gaussian 32 r + e / 12 of the wave, and a piece of a row nobody needs is not requested (its LDS cells get zeros, and its lane
// does not read them: f[] is then left as it was).  A view that culls a Gaussian so never moves its 192-byte row.
__device__ __forceinline__ void sh_rows_to_lanes(const float* __restrict__ src, size_t g_block, float* lds, uint64_t need, float (&f)[48]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* my = lds + wave * (SHT_ROWS * SHT_LD);
    const float4* base = reinterpret_cast<const float4*>(src) + (g_block + (size_t)wave * 64) * 12;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint32_t slab_need = (uint32_t)(need >> (32 * r));
        if (slab_need == 0u) continue;  // (wave-uniform)
        const float4* p = base + (size_t)r * SHT_ROWS * 12;
        float4 v[6];  // all six requests go out before the first is stored
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const int e = i * 64 + lane;  // float4 index inside the 32-row slab
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((slab_need >> (e / 12)) & 1u) v[i] = load_streaming(p + e);
        }
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const int e = i * 64 + lane;
            const int g = e / 12, c = e - 12 * g;
            *reinterpret_cast<float4*>(my + g * SHT_LD + 4 * c) = v[i];
        }
        wave_sync();
        if ((lane >> 5) == r && ((slab_need >> (lane & 31)) & 1u)) {
            const float* row = my + (lane & 31) * SHT_LD;
#pragma unroll
            for (int c = 0; c < 12; c++) {
                const float4 v = *reinterpret_cast<const float4*>(row + 4 * c);
                f[4 * c] = v.x; f[4 * c + 1] = v.y; f[4 * c + 2] = v.z; f[4 * c + 3] = v.w;
            }
        }
        wave_sync();
    }
}
__device__ __forceinline__ void lanes_to_sh_rows(const float (&f)[48], float* __restrict__ dst, size_t g_block, float* lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* my = lds + wave * (SHT_ROWS * SHT_LD);
    float4* base = reinterpret_cast<float4*>(dst) + (g_block + (size_t)wave * 64) * 12;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if ((lane >> 5) == r) {
            float* row = my + (lane & 31) * SHT_LD;
#pragma unroll
            for (int c = 0; c < 12; c++)
                *reinterpret_cast<float4*>(row + 4 * c) = make_float4(f[4 * c], f[4 * c + 1], f[4 * c + 2], f[4 * c + 3]);
        }
        wave_sync();
        float4* p = base + (size_t)r * SHT_ROWS * 12;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const int e = i * 64 + lane;
            const int g = e / 12, c = e - 12 * g;
            store_streaming(p + e, *reinterpret_cast<const float4*>(my + g * SHT_LD + 4 * c));
        }
        wave_sync();
    }
}

// The same for rows of the form coef[k] * rgb (dL_dsh: every coefficient's gradient is a scalar times the colour
// gradient): the 48 products are formed while the row is written, so that only 16 + 3 registers stay live.
__device__ __forceinline__ void lanes_to_sh_rows_scaled(const float (&coef)[16], float3 rgb, float* __restrict__ dst, size_t g_block,
                                                        float* lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* my = lds + wave * (SHT_ROWS * SHT_LD);
    float4* base = reinterpret_cast<float4*>(dst) + (g_block + (size_t)wave * 64) * 12;
    const float ch[3] = {rgb.x, rgb.y, rgb.z};
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if ((lane >> 5) == r) {
            float* row = my + (lane & 31) * SHT_LD;
#pragma unroll
            for (int c = 0; c < 12; c++)  // element e = 4 c + j of the row is coefficient e / 3, channel e % 3
                *reinterpret_cast<float4*>(row + 4 * c) =
                    make_float4(coef[(4 * c) / 3] * ch[(4 * c) % 3], coef[(4 * c + 1) / 3] * ch[(4 * c + 1) % 3],
                                coef[(4 * c + 2) / 3] * ch[(4 * c + 2) % 3], coef[(4 * c + 3) / 3] * ch[(4 * c + 3) % 3]);
        }
        wave_sync();
        float4* p = base + (size_t)r * SHT_ROWS * 12;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const int e = i * 64 + lane;
            const int g = e / 12, c = e - 12 * g;
            store_streaming(p + e, *reinterpret_cast<const float4*>(my + g * SHT_LD + 4 * c));
        }
        wave_sync();
    }
}

// d(colour)/d(unit view direction) of computeColorFromSH, term by term as the reference's backward writes it
// (L/cuda_rasterizer/backward.cu:50-133)
__device__ __forceinline__ void sh_direction_derivatives(const SHCoeffs& s, int D, float3 dir, float3& dRGBdx, float3& dRGBdy,
                                                         float3& dRGBdz) {
    const float x = dir.x, y = dir.y, z = dir.z;
    if (D > 0) {
        dRGBdx = -SH_C1 * s.c[3];
        dRGBdy = -SH_C1 * s.c[1];
        dRGBdz = SH_C1 * s.c[2];
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            dRGBdx = dRGBdx + (SH_C2[0] * y * s.c[4] + SH_C2[2] * 2.f * -x * s.c[6] + SH_C2[3] * z * s.c[7] + SH_C2[4] * 2.f * x * s.c[8]);
            dRGBdy = dRGBdy + (SH_C2[0] * x * s.c[4] + SH_C2[1] * z * s.c[5] + SH_C2[2] * 2.f * -y * s.c[6] + SH_C2[4] * 2.f * -y * s.c[8]);
            dRGBdz = dRGBdz + (SH_C2[1] * y * s.c[5] + SH_C2[2] * 2.f * 2.f * z * s.c[6] + SH_C2[3] * x * s.c[7]);
            if (D > 2) {
                dRGBdx = dRGBdx + (SH_C3[0] * s.c[9] * 3.f * 2.f * xy + SH_C3[1] * s.c[10] * yz + SH_C3[2] * s.c[11] * -2.f * xy +
                                   SH_C3[3] * s.c[12] * -3.f * 2.f * xz + SH_C3[4] * s.c[13] * (-3.f * xx + 4.f * zz - yy) +
                                   SH_C3[5] * s.c[14] * 2.f * xz + SH_C3[6] * s.c[15] * 3.f * (xx - yy));
                dRGBdy = dRGBdy + (SH_C3[0] * s.c[9] * 3.f * (xx - yy) + SH_C3[1] * s.c[10] * xz +
                                   SH_C3[2] * s.c[11] * (-3.f * yy + 4.f * zz - xx) + SH_C3[3] * s.c[12] * -3.f * 2.f * yz +
                                   SH_C3[4] * s.c[13] * -2.f * xy + SH_C3[5] * s.c[14] * -2.f * yz +
                                   SH_C3[6] * s.c[15] * -3.f * 2.f * xy);
                dRGBdz = dRGBdz + (SH_C3[1] * s.c[10] * xy + SH_C3[2] * s.c[11] * 4.f * 2.f * yz +
                                   SH_C3[3] * s.c[12] * 3.f * (2.f * zz - xx - yy) + SH_C3[4] * s.c[13] * 4.f * 2.f * xz +
                                   SH_C3[5] * s.c[14] * (xx - yy));
            }
        }
    }
}

// computeCov3D backward (L/cuda_rasterizer/backward.cu:280-343): linear in dL_dcov3D
__device__ __forceinline__ void cov3d_backward_terms(float3 sc, float4 q, float mod, const float (&dcov)[6], float3& dscale, float4& drot) {
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    M3 R;
    quat_to_R(q, R);
    const float3 s = make_float3(mod * sc.x, mod * sc.y, mod * sc.z);
    const M3 Mm = mul(diag3(s.x, s.y, s.z), R);
    M3 dSigma;
    dSigma.m[0][0] = dcov[0]; dSigma.m[0][1] = 0.5f * dcov[1]; dSigma.m[0][2] = 0.5f * dcov[2];
    dSigma.m[1][0] = 0.5f * dcov[1]; dSigma.m[1][1] = dcov[3]; dSigma.m[1][2] = 0.5f * dcov[4];
    dSigma.m[2][0] = 0.5f * dcov[2]; dSigma.m[2][1] = 0.5f * dcov[4]; dSigma.m[2][2] = dcov[5];
    M3 M2;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int rr = 0; rr < 3; rr++) M2.m[c][rr] = Mm.m[c][rr] * 2.0f;
    const M3 dL_dM = mul(M2, dSigma);
    const M3 Rt = transpose(R);
    M3 dMt = transpose(dL_dM);
    dscale.x = dot3(make_float3(Rt.m[0][0], Rt.m[0][1], Rt.m[0][2]), make_float3(dMt.m[0][0], dMt.m[0][1], dMt.m[0][2]));
    dscale.y = dot3(make_float3(Rt.m[1][0], Rt.m[1][1], Rt.m[1][2]), make_float3(dMt.m[1][0], dMt.m[1][1], dMt.m[1][2]));
    dscale.z = dot3(make_float3(Rt.m[2][0], Rt.m[2][1], Rt.m[2][2]), make_float3(dMt.m[2][0], dMt.m[2][1], dMt.m[2][2]));
#pragma unroll
    for (int k = 0; k < 3; k++) { dMt.m[0][k] *= s.x; dMt.m[1][k] *= s.y; dMt.m[2][k] *= s.z; }
    drot.x = 2 * z * (dMt.m[0][1] - dMt.m[1][0]) + 2 * y * (dMt.m[2][0] - dMt.m[0][2]) + 2 * x * (dMt.m[1][2] - dMt.m[2][1]);
    drot.y = 2 * y * (dMt.m[1][0] + dMt.m[0][1]) + 2 * z * (dMt.m[2][0] + dMt.m[0][2]) + 2 * r * (dMt.m[1][2] - dMt.m[2][1]) - 4 * x * (dMt.m[2][2] + dMt.m[1][1]);
    drot.z = 2 * x * (dMt.m[1][0] + dMt.m[0][1]) + 2 * r * (dMt.m[2][0] - dMt.m[0][2]) + 2 * z * (dMt.m[1][2] + dMt.m[2][1]) - 4 * y * (dMt.m[2][2] + dMt.m[0][0]);
    drot.w = 2 * r * (dMt.m[0][1] - dMt.m[1][0]) + 2 * x * (dMt.m[2][0] + dMt.m[0][2]) + 2 * y * (dMt.m[1][2] + dMt.m[2][1]) - 4 * z * (dMt.m[1][1] + dMt.m[0][0]);
}

}  // namespace dgr
