// preprocess_fwd.hip -- per-Gaussian forward kernels for gfx950: forward preprocess (one view and batched), the frustum
// mark and the view-independent 3D covariance.
//
// Replaces, on the hot path:
//   forward : preprocessCUDA + computeCov3D + computeCov2D + computeColorFromSH
//             (*/cuda_rasterizer/forward.cu:20-256) and the per-tile histogram that stands in for
//             tiles_touched + InclusiveSum (L/cuda_rasterizer/rasterizer_impl.cu:283)
//   checkFrustum (L/cuda_rasterizer/rasterizer_impl.cu:54-66)
//
// Both kernels are HBM-bound (one thread per Gaussian, ~250-500 B of traffic each), so the
// arithmetic is written in the reference's association order with FMA contraction OFF: radii,
// tile rects and depth bits -- the integer path -- then agree bit for bit with the CPU oracle.
#include "dgr_common.h"

#include "kernels.h"
#include "count_rank.h"
#include "gaussian_math.h"

#pragma clang fp contract(off)

namespace dgr {

// ---- per-view pieces of preprocessCUDA, shared by the one-view kernel and the batched one ----
struct FwdGeom {
    int radius;
    ushort4 rect;
    bool violation, need_sh;
};
// Frustum test, covariance projection, radius, tile rectangle and the first two pieces of the render record of Gaussian
// idx for the camera in `a` (forward.cu:155-256 up to the colour).  C3_GIVEN: the 3D covariance -- it depends on scale
// and rotation only -- was formed by the caller (the batched kernel evaluates it once for all views of the batch; same
// expression, same bits) and is only stored here.
template <bool C3_GIVEN>
__device__ __forceinline__ FwdGeom fwd_view_geometry(const PreprocessFwdArgs& a, int idx, float3 p_orig, const float (&c3_in)[6]) {
    int radius = 0;
    ushort4 rect = make_ushort4(0, 0, 0, 0);
    bool violation = false, need_sh = false;
    if (a.gau_uncertainty) a.gau_uncertainty[idx] = 0.0f;
    if (a.gau_related_pixels) a.gau_related_pixels[idx] = 0;
    // in_frustum (cuda_rasterizer/auxiliary.h:139-164)
    const float4 p_hom = xform4x4(p_orig, a.proj);
    const float p_w = 1.0f / (p_hom.w + 0.0000001f);
    const float3 p_proj = make_float3(p_hom.x * p_w, p_hom.y * p_w, p_hom.z * p_w);
    const float3 p_view = xform4x3(p_orig, a.view);
    bool live = !(p_view.z <= DGR_NEAR);
    violation = !live && a.prefiltered;  // `prefiltered` promised that nothing is culled (auxiliary.h:154-160)

    if (live) {
        float c3[6];
        if (C3_GIVEN) {
#pragma unroll
            for (int i = 0; i < 6; i++) c3[i] = c3_in[i];
        } else {
            load_cov3d(a, idx, c3);
        }
        Cov2D c;
        cov2d_common(p_orig, a.focal_x, a.focal_y, a.tan_fovx, a.tan_fovy, c3, a.view, c);
        const float cx = c.cov.m[0][0] + 0.3f, cy = c.cov.m[0][1], cz = c.cov.m[1][1] + 0.3f;
        const float det = (cx * cz - cy * cy);
        if (det != 0.0f) {
            const float det_inv = 1.f / det;
            const float3 conic = make_float3(cz * det_inv, -cy * det_inv, cx * det_inv);
            const float mid = 0.5f * (cx + cz);
            const float lambda1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
            const float lambda2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
            const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
            const float pix = ndc2pix(p_proj.x, a.W), piy = ndc2pix(p_proj.y, a.H);
            int x0, y0, x1, y1;
            get_rect(pix, piy, (int)my_radius, a.grid_x, a.grid_y, x0, y0, x1, y1);
            if ((x1 - x0) * (y1 - y0) != 0) {
                float3 rgb;
                if (a.colors_precomp) {
                    rgb = make_float3(a.colors_precomp[3 * (size_t)idx], a.colors_precomp[3 * (size_t)idx + 1],
                                      a.colors_precomp[3 * (size_t)idx + 2]);
                } else {
                    need_sh = true;  // evaluated below, after the geometry: a whole block then fetches its SH rows together
                    rgb = make_float3(0.f, 0.f, 0.f);
                }
                radius = (int)my_radius;
                int tx0 = x0, ty0 = y0, tx1 = x1, ty1 = y1;  // the rectangle that is binned (radii stay the reference's)
                if (a.tight_cull) {
                    // Optional (NOT the reference's integer path): shrink the tile rectangle to the box of
                    // the region where alpha can reach 15/255, q(d) <= tau = 2 ln(255 o / 15): half extents sqrt(tau cov_xx),
                    // sqrt(tau cov_yy) <= 2.38 sigma instead of the 3 sigma_max circle, with the same safety margin the
                    // blend kernels' own culling uses.  Every dropped (tile, Gaussian) instance is one no pixel would blend,
                    // so images and gradients are unchanged; num_rendered, the tile lists and n_contrib shrink.
                    const float o = a.opacities[idx];
                    const float tau = 2.0f * __logf(o * (255.0f / 15.0f));
                    if (!(tau > 0.0f)) {
                        tx1 = tx0;  // can never contribute
                    } else {
                        const float hx = sqrtf(tau * cx) * 1.001f + 0.05f, hy = sqrtf(tau * cz) * 1.001f + 0.05f;
                        // tile t holds pixels 16 t .. 16 t + 15 (pixel centres at integer coordinates)
                        tx0 = max(x0, (int)ceilf((pix - hx - 15.0f) / 16.0f));
                        ty0 = max(y0, (int)ceilf((piy - hy - 15.0f) / 16.0f));
                        tx1 = min(x1, (int)floorf((pix + hx) / 16.0f) + 1);
                        ty1 = min(y1, (int)floorf((piy + hy) / 16.0f) + 1);
                        if (tx1 < tx0) tx1 = tx0;
                        if (ty1 < ty0) ty1 = ty0;
                    }
                }
                rect = make_ushort4((unsigned short)tx0, (unsigned short)ty0, (unsigned short)tx1, (unsigned short)ty1);
                a.geom.depths[idx] = p_view.z;
                float4* rec = a.geom.rec + DGR_REC_STRIDE * (size_t)idx;
                rec[0] = make_float4(pix, piy, p_view.z, a.opacities[idx]);
                rec[1] = make_float4(conic.x, conic.y, conic.z, 0.0f);
                if (!need_sh) rec[2] = make_float4(rgb.x, rgb.y, rgb.z, 0.0f);
            }
        }
    }
    a.geom.radii[idx] = radius;
    if (a.radii_out) a.radii_out[idx] = radius;
    a.geom.rect[idx] = rect;
    return FwdGeom{radius, rect, violation, need_sh};
}

// computeColorFromSH (forward.cu:20-71) for the camera in `a`, plus what the backward keeps of it; writes the third piece
// of the render record
__device__ __forceinline__ void fwd_view_colour(const PreprocessFwdArgs& a, int idx, float3 p_orig, const SHCoeffs& s) {
    float3 rgb;
    const float3 cam = make_float3(a.campos[0], a.campos[1], a.campos[2]);
    float3 dir = p_orig - cam;
    const float len = sqrtf(dot3(dir, dir));
    dir = make_float3(dir.x / len, dir.y / len, dir.z / len);
    float3 res = SH_C0 * s.c[0];
    if (a.D > 0) {
        const float x = dir.x, y = dir.y, z = dir.z;
        res = res - SH_C1 * y * s.c[1] + SH_C1 * z * s.c[2] - SH_C1 * x * s.c[3];
        if (a.D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            res = res + SH_C2[0] * xy * s.c[4] + SH_C2[1] * yz * s.c[5] +
                  SH_C2[2] * (2.0f * zz - xx - yy) * s.c[6] + SH_C2[3] * xz * s.c[7] +
                  SH_C2[4] * (xx - yy) * s.c[8];
            if (a.D > 2) {
                res = res + SH_C3[0] * y * (3.0f * xx - yy) * s.c[9] + SH_C3[1] * xy * z * s.c[10] +
                      SH_C3[2] * y * (4.0f * zz - xx - yy) * s.c[11] +
                      SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * s.c[12] +
                      SH_C3[4] * x * (4.0f * zz - xx - yy) * s.c[13] +
                      SH_C3[5] * z * (xx - yy) * s.c[14] + SH_C3[6] * x * (xx - 3.0f * yy) * s.c[15];
            }
        }
    }
    res.x += 0.5f; res.y += 0.5f; res.z += 0.5f;
    {
        // d(colour)/d(direction) (L/cuda_rasterizer/backward.cu:50-133), kept for the backward: it is all the
        // backward needs of the SH coefficients beyond the basis values, which depend on the direction alone
        float3 dRGBdx = make_float3(0, 0, 0), dRGBdy = make_float3(0, 0, 0), dRGBdz = make_float3(0, 0, 0);
        sh_direction_derivatives(s, a.D, dir, dRGBdx, dRGBdy, dRGBdz);
        // nine floats in 36 bytes (dgr_common.h: shd_a / shd_b / shd_c): consecutive lanes store consecutive pieces of each plane
        a.geom.shd_a[idx] = make_float4(dRGBdx.x, dRGBdx.y, dRGBdx.z, dRGBdy.x);
        a.geom.shd_b[idx] = make_float4(dRGBdy.y, dRGBdy.z, dRGBdz.x, dRGBdz.y);
        a.geom.shd_c[idx] = dRGBdz.z;
    }
    a.geom.clamped[idx] = (uint8_t)((res.x < 0 ? 1 : 0) | (res.y < 0 ? 2 : 0) | (res.z < 0 ? 4 : 0));
    rgb = make_float3(fmaxf(res.x, 0.0f), fmaxf(res.y, 0.0f), fmaxf(res.z, 0.0f));
    a.geom.rec[DGR_REC_STRIDE * (size_t)idx + 2] = make_float4(rgb.x, rgb.y, rgb.z, 0.0f);
}

// The SH row of Gaussian idx for the lanes that `need` it -- whatever the caller's "someone needs SH" predicate is -- as SHCoeffs.
// Whole block in range, 16 coefficients, 16-byte aligned rows and some lane in need: the block's rows move through LDS
// (`lds`: 4 * SHT_ROWS * SHT_LD floats; block-uniform, every lane of the block must get here); else a lane loads its own.
// Either way only the rows of lanes in need are requested (the wave's ballot goes with the transposition): the row of a
// Gaussian this view culled costs no traffic.
__device__ __forceinline__ void fetch_sh(const PreprocessFwdArgs& a, int idx, bool need, float* lds, SHCoeffs& s) {
    const bool blk_fast = a.sh_vec_ok && a.M == 16 && (size_t)blockIdx.x * 256 + 256 <= (size_t)a.P && __syncthreads_or(need);
    float shf[48];
    if (blk_fast) sh_rows_to_lanes(a.shs, (size_t)blockIdx.x * 256, lds, __builtin_amdgcn_ballot_w64(need), shf);
    if (need) {
        if (blk_fast) {
#pragma unroll
            for (int k = 0; k < 16; k++) s.c[k] = make_float3(shf[3 * k], shf[3 * k + 1], shf[3 * k + 2]);
        } else {
            load_sh(a.shs, idx, a.D, a.M, a.sh_vec_ok, s);
        }
    }
}

// The block epilogue of the callback path: instances (tiles_touched) per block, for count_rank's offsets (the reference scans
// tiles_touched over P, L/cuda_rasterizer/rasterizer_impl.cu:283).  A wave's total; bit 31 carries "some Gaussian of this
// wave violated `prefiltered`" (scan_blocks moves it into status[2]); block totals stay far below 2^31 ...
__device__ __forceinline__ uint32_t wave_tiles_word(ushort4 rect, bool violation) {
    uint32_t n = (uint32_t)(rect.z - rect.x) * (uint32_t)(rect.w - rect.y);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (__builtin_amdgcn_ballot_w64(violation) != 0ull) n |= 0x80000000u;
    return n;
}
// ... and the block's geom.block_tiles word from its four waves' words
__device__ __forceinline__ uint32_t block_tiles_word(const uint32_t* w) {
    const uint32_t flag = (w[0] | w[1] | w[2] | w[3]) & 0x80000000u;
    return ((w[0] & 0x7fffffffu) + (w[1] & 0x7fffffffu) + (w[2] & 0x7fffffffu) + (w[3] & 0x7fffffffu)) | flag;
}

// block_scan.h's block_exclusive_scan<256> in the four-wave form preprocess_fwd_kernel had before that header existed, kept for
// this kernel alone: with the shared form the kernel is 42 instructions shorter, and its stage then missed the project's A/B rule
// at config 2 of the full variant (a workload that does not even run the fused count) while passing where the count does run
// (profiles/binning_shared/notes.md s5).  With this copy the kernel is the earlier one instruction for instruction.
__device__ __forceinline__ uint32_t block_exclusive_scan4(uint32_t n, uint32_t* wtot /* 4 words of LDS */, int tid, uint32_t* total) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t incl = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (int ww = 0; ww < wave; ww++) before += wtot[ww];
    *total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    return before + incl - n;
}

// ------------------------------------------------------------------------------------------------
#ifndef DGR_PPF_WAVES
#define DGR_PPF_WAVES 5
#endif
__global__ void __launch_bounds__(256, DGR_PPF_WAVES) preprocess_fwd_kernel(PreprocessFwdArgs a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    FwdGeom g{0, make_ushort4(0, 0, 0, 0), false, false};
    float3 p_orig = make_float3(0.f, 0.f, 0.f);
    // LDS: the SH transposition buffer and, afterwards, the rank stage of the fused count share one pool
    constexpr int POOL_WORDS = (4 * SHT_ROWS * SHT_LD > COUNT_STAGE) ? 4 * SHT_ROWS * SHT_LD : COUNT_STAGE;
    __shared__ float pool[POOL_WORDS];
    // Zeroing that would otherwise be stream memsets (one launch each): the tile counters count_rank increments
    // (callback path only -- the fused count needs them cleared before this kernel starts) and the two per-Gaussian
    // median statistics the forward blend accumulates into.
    for (int i = idx; i < a.n_zero_words; i += gridDim.x * 256) a.zero_words[i] = 0u;
    if (idx < a.P) {
        p_orig = load_row3(a.means3D, idx);
        const float no_c3[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        g = fwd_view_geometry<false>(a, idx, p_orig, no_c3);
    }
    const bool need_sh = g.need_sh, violation = g.violation;
    const ushort4 rect = g.rect;

    // computeColorFromSH (forward.cu:20-71) for the Gaussians that survived
    if (a.shs && !a.colors_precomp) {  // uniform
        SHCoeffs s;
        fetch_sh(a, idx, need_sh, pool, s);
        if (need_sh) fwd_view_colour(a, idx, p_orig, s);
    }

    __shared__ uint32_t wsum[4];
    if (a.fused_count) {
        // duplicateWithKeys' first half, here: this block's instances get a contiguous run of the rank array handed out
        // by a global cursor (any unique placement will do -- the ranks are read back through goff), then every
        // instance takes its tile-counter atomic (count_rank.h).
        __shared__ uint32_t s_base;
        const bool any_violation = __syncthreads_or(violation);  // (also orders the SH phase's LDS reads before the stage)
        const uint32_t n = (uint32_t)(rect.z - rect.x) * (uint32_t)(rect.w - rect.y);
        uint32_t block_total;
        const uint32_t loc = block_exclusive_scan4(n, wsum, threadIdx.x, &block_total);
        if (threadIdx.x == 0) {
            s_base = block_total ? atomicAdd(a.cursor, block_total) : 0u;
            if (any_violation) atomicOr(a.cursor + 1, 1u);
        }
        __syncthreads();
        const uint32_t base = s_base;
        if (idx < a.P) a.geom.goff[idx] = base + loc;
        count_and_rank(rect, base + loc, base, block_total, a.tile_count, a.ranks, a.grid_x, a.capacity,
                       reinterpret_cast<uint32_t*>(pool), threadIdx.x);
        return;
    }
    // callback path: the instances of this block
    const uint32_t n = wave_tiles_word(rect, violation);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) a.geom.block_tiles[blockIdx.x] = block_tiles_word(wsum);
}

// ------------------------------------------------------------------------------------------------
// Batched forward preprocess: the V views of a batch in ONE launch.  A Gaussian's position, opacity and
// 3D covariance are fetched / formed once, its 192-byte SH row is fetched once -- when at least one view sees it -- and
// evaluated for every camera that does; per view the lane runs exactly the code of the one-view kernel
// (fwd_view_geometry / fwd_view_colour), so every view's state buffers are bit-identical to a one-view call.  Only the
// LDS-count form of the epilogue exists here (per-block instance totals in each view's geom.block_tiles).
__device__ __forceinline__ PreprocessFwdArgs batch_view_args(const PreprocessFwdBatchArgs& b, int v) {
    PreprocessFwdArgs a = b.base;
    const FwdViewPart& p = b.v[v];
    a.view = p.view; a.proj = p.proj; a.campos = p.campos; a.geom = p.geom; a.radii_out = p.radii_out;
    a.gau_uncertainty = p.gau_uncertainty; a.gau_related_pixels = p.gau_related_pixels;
    return a;
}
__global__ void __launch_bounds__(256) preprocess_fwd_batch_kernel(PreprocessFwdBatchArgs b) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int P = b.base.P, V = b.V;
    __shared__ float pool[4 * SHT_ROWS * SHT_LD];
    __shared__ uint32_t wsum[DGR_MAX_BATCH_VIEWS][4];
    float3 p_orig = make_float3(0.f, 0.f, 0.f);
    float c3[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (idx < P) {
        p_orig = load_row3(b.base.means3D, idx);
        load_cov3d(b.base, idx, c3);
    }
    uint32_t need_mask = 0u;
#pragma unroll 1
    for (int v = 0; v < V; v++) {
        const PreprocessFwdArgs a = batch_view_args(b, v);
        FwdGeom g{0, make_ushort4(0, 0, 0, 0), false, false};
        if (idx < P) g = fwd_view_geometry<true>(a, idx, p_orig, c3);
        if (g.need_sh) need_mask |= 1u << v;
        // instances (tiles_touched) of this block in view v, as the one-view kernel leaves them for count_lds / scan_table
        const uint32_t n = wave_tiles_word(g.rect, g.violation);
        if ((threadIdx.x & 63) == 0) wsum[v][threadIdx.x >> 6] = n;
    }
    __syncthreads();
    if ((int)threadIdx.x < V) b.v[threadIdx.x].geom.block_tiles[blockIdx.x] = block_tiles_word(wsum[threadIdx.x]);
    if (b.base.shs && !b.base.colors_precomp) {  // uniform
        SHCoeffs s;
        fetch_sh(b.base, idx, need_mask != 0u, pool, s);
        if (need_mask != 0u) {
#pragma unroll 1
            for (int v = 0; v < V; v++)
                if ((need_mask >> v) & 1u) fwd_view_colour(batch_view_args(b, v), idx, p_orig, s);
        }
    }
}

// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) mark_visible_kernel(int P, const float* __restrict__ means,
                                                           const float* __restrict__ view, uint8_t* present) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    const float3 p = load_row3(means, idx);
    present[idx] = !(xform4x3(p, view).z <= DGR_NEAR);
}

// ------------------------------------------------------------------------------------------------
// View-independent half of the per-Gaussian work, shared by the views of a batch: the 3D
// covariance depends on scale and rotation only.  cov3d_fwd is computeCov3D (forward.cu:118-152) exactly as
// preprocess_fwd evaluates it (same expression: the six floats are bit-identical), to be passed to every view as
// `cov3D_precomp` (its backward: cov3d_bwd_kernel, preprocess_bwd.hip).
__global__ void __launch_bounds__(256) cov3d_fwd_kernel(int P, const float* __restrict__ scales, const float* __restrict__ rotations,
                                                        float mod, float* __restrict__ cov3D) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    float c3[6];
    compute_cov3d(scales, rotations, mod, idx, c3);
    float* o = cov3D + 6 * (size_t)idx;
#pragma unroll
    for (int i = 0; i < 6; i++) o[i] = c3[i];
}

// ------------------------------------------------------------------------------------------------
hipError_t launch_cov3d_forward(int P, const float* scales, const float* rotations, float mod, float* cov3D, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    launch(cov3d_fwd_kernel, dim3((P + 255) / 256), dim3(256), stream, P, scales, rotations, mod, cov3D);
    return hipGetLastError();
}
hipError_t launch_preprocess_fwd(const PreprocessFwdArgs& a, hipStream_t stream) {
    if (a.P <= 0) return hipSuccess;
    launch(preprocess_fwd_kernel, dim3((a.P + 255) / 256), dim3(256), stream, a);
    return hipGetLastError();
}
hipError_t launch_preprocess_fwd_batch(const PreprocessFwdBatchArgs& b, hipStream_t stream) {
    if (b.base.P <= 0 || b.V <= 0) return hipSuccess;
    launch(preprocess_fwd_batch_kernel, dim3((b.base.P + 255) / 256), dim3(256), stream, b);
    return hipGetLastError();
}
hipError_t launch_mark_visible(int P, const float* means, const float* view, uint8_t* present, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    launch(mark_visible_kernel, dim3((P + 255) / 256), dim3(256), stream, P, means, view, present);
    return hipGetLastError();
}
}  // namespace dgr
