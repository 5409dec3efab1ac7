// preprocess_bwd.hip -- per-Gaussian backward kernels for gfx950: the fused backward preprocess (one view and batched) with
// the pose-gradient reduction (pose_reduce.h), the covariance backward of a batch of views and a zero fill.
//
// Replaces, on the hot path:
//   backward: computeCov2DCUDA + preprocessCUDA + computeColorFromSH + computeCov3D
//             (L/cuda_rasterizer/backward.cu:20-416) and pose_gradient_preCUDA (:701-751)
//
// Both kernels are HBM-bound (one thread per Gaussian, ~250-500 B of traffic each), so the
// arithmetic is written in the reference's association order with FMA contraction OFF: radii,
// tile rects and depth bits -- the integer path -- then agree bit for bit with the CPU oracle.
#include "dgr_common.h"
#include <algorithm>

#include "kernels.h"
#include "gaussian_math.h"
#include "pose_reduce.h"

#pragma clang fp contract(off)
#ifndef DGR_BWD_BATCH_WAVES
// waves per SIMD the batched backward is compiled for (48 dL_dsh sums live across its view loop).  3 is what its 44 KB of LDS allow
// and what every instance ran at when compiled for 2; stated, since with the packed SH direction derivatives the full instance
// compiled for 2 takes 184 registers (2 waves) and for 3 the 166 it had, without scratch.
#define DGR_BWD_BATCH_WAVES 3
#endif

namespace dgr {

// ------------------------------------------------------------------------------------------------
// ---- per-view terms of the fused per-Gaussian backward, shared by the one-view kernel and the batched one ----
// Everything that depends on the camera: the median-depth term, computeCov2DCUDA, preprocessCUDA, the SH backward up to
// the scalars coef[k] and the masked colour gradient (dL_dsh[k] = coef[k] * dRGB), the pose-gradient terms.  `acc` = the
// blend backward's sums for this Gaussian in this view (zeros when it was not visible).
// COMPLETE (dgr_set_option("pose_grad", 1)): the pose gradient is the view-matrix counterpart of dL_dmeans3D -- the reference's
// ndc terms plus the z path (the depth sums dL_dmeans3D uses), the cov2D path (A = Ju Rcam: dL/dRcam = Ju^T dL/dA and t_cam through
// Ju) and the SH path (campos = -Rcam^T t) -- while every per-Gaussian output keeps its bits.
// Under map_off the covariance and SH blocks still run (the pose needs dL/da..c and dL/dcampos) but add nothing to the outputs.
template <bool COMPLETE = false>
__device__ __forceinline__ void bwd_view_terms(const PreprocessBwdArgs& a, const bool full, float3 m, const float (&c3)[6],
                                               const float (&acc)[16], bool vis, uint8_t cl_in, float4 shd_a, float4 shd_b,
                                               float shd_c, float3& dmean_out, float (&dcov)[6], float (&coef)[16],
                                               float3& dRGB, float (&pose)[12]) {
    // light: the blend kernel's median-depth term; full: computeCov2DCUDA ASSIGNS (F/cuda_rasterizer/backward.cu:383)
    float3 dmean = make_float3(0.f, 0.f, 0.f);
    if (!full) {
        // light: the blend kernel's median-depth term (L/cuda_rasterizer/backward.cu:654-664), whose pixel sum of
        // dL/dmedian arrives in acc[10]; the per-Gaussian factors are applied here
        // (COMPLETE under map_off: the mapping blend ran and acc[10] holds a sum, but the output stays what the tracking
        //  blend's zero row gives)
        const float* v = a.view;
        const float mul3 = v[2] * m.x + v[6] * m.y + v[10] * m.z + v[14];
        const float med = (COMPLETE && a.map_off) ? 0.0f : acc[10];
        dmean = make_float3((v[2] - v[3] * mul3) * med, (v[6] - v[7] * mul3) * med, (v[10] - v[11] * mul3) * med);
    }
    float3 s_cam = make_float3(0.f, 0.f, 0.f);  // full: sum_ch dL_dcolor[ch] * d(rgb[ch])/d(campos.{x,y,z})
    const bool do_map = vis && !a.map_off;
    const bool do_terms = COMPLETE ? vis : do_map;  // the blocks below run (COMPLETE: for the pose too)
    float px[12];  // COMPLETE: the cov2D and SH paths' pose terms, [3 k + j] = dL/dv[4 k + j]
    float3 g_cam = make_float3(0.f, 0.f, 0.f);  // COMPLETE: dL/dcampos of the masked colour gradient
#pragma unroll
    for (int i = 0; i < 12; i++) px[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 6; i++) dcov[i] = 0.0f;
    if (do_terms) {
        // ---------------- computeCov2DCUDA (L/cuda_rasterizer/backward.cu:144-276)
        const float3 dconic = make_float3(acc[6], acc[7], acc[8]);
        Cov2D c;
        cov2d_common(m, a.focal_x, a.focal_y, a.tan_fovx, a.tan_fovy, c3, a.view, c);
        const float limx = 1.3f * a.tan_fovx, limy = 1.3f * a.tan_fovy;
        const float x_grad_mul = (c.txtz < -limx || c.txtz > limx) ? 0.f : 1.f;
        const float y_grad_mul = (c.tytz < -limy || c.tytz > limy) ? 0.f : 1.f;
        const float h_x = a.focal_x, h_y = a.focal_y;
        const M3& T = c.T; const M3& Vrk = c.Vrk; const M3& W = c.W; const float3 t = c.t;
        const float ca = c.cov.m[0][0] + 0.3f, cb = c.cov.m[0][1], cc = c.cov.m[1][1] + 0.3f;
        const float denom = ca * cc - cb * cb;
        float dL_da = 0, dL_db = 0, dL_dc = 0;
        const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
        if (denom2inv != 0) {
            dL_da = denom2inv * (-cc * cc * dconic.x + 2 * cb * cc * dconic.y + (denom - ca * cc) * dconic.z);
            dL_dc = denom2inv * (-ca * ca * dconic.z + 2 * ca * cb * dconic.y + (denom - ca * cc) * dconic.x);
            dL_db = denom2inv * 2 * (cb * cc * dconic.x - (denom + 2 * cb * cb) * dconic.y + ca * cb * dconic.z);
            if (!COMPLETE || do_map) {  // (COMPLETE under map_off: no dL_dcov3D)
            dcov[0] = (T.m[0][0] * T.m[0][0] * dL_da + T.m[0][0] * T.m[1][0] * dL_db + T.m[1][0] * T.m[1][0] * dL_dc);
            dcov[3] = (T.m[0][1] * T.m[0][1] * dL_da + T.m[0][1] * T.m[1][1] * dL_db + T.m[1][1] * T.m[1][1] * dL_dc);
            dcov[5] = (T.m[0][2] * T.m[0][2] * dL_da + T.m[0][2] * T.m[1][2] * dL_db + T.m[1][2] * T.m[1][2] * dL_dc);
            dcov[1] = 2 * T.m[0][0] * T.m[0][1] * dL_da + (T.m[0][0] * T.m[1][1] + T.m[0][1] * T.m[1][0]) * dL_db + 2 * T.m[1][0] * T.m[1][1] * dL_dc;
            dcov[2] = 2 * T.m[0][0] * T.m[0][2] * dL_da + (T.m[0][0] * T.m[1][2] + T.m[0][2] * T.m[1][0]) * dL_db + 2 * T.m[1][0] * T.m[1][2] * dL_dc;
            dcov[4] = 2 * T.m[0][2] * T.m[0][1] * dL_da + (T.m[0][1] * T.m[1][2] + T.m[0][2] * T.m[1][1]) * dL_db + 2 * T.m[1][1] * T.m[1][2] * dL_dc;
            }
        }
        const float dL_dT00 = 2 * (T.m[0][0] * Vrk.m[0][0] + T.m[0][1] * Vrk.m[0][1] + T.m[0][2] * Vrk.m[0][2]) * dL_da +
                              (T.m[1][0] * Vrk.m[0][0] + T.m[1][1] * Vrk.m[0][1] + T.m[1][2] * Vrk.m[0][2]) * dL_db;
        const float dL_dT01 = 2 * (T.m[0][0] * Vrk.m[1][0] + T.m[0][1] * Vrk.m[1][1] + T.m[0][2] * Vrk.m[1][2]) * dL_da +
                              (T.m[1][0] * Vrk.m[1][0] + T.m[1][1] * Vrk.m[1][1] + T.m[1][2] * Vrk.m[1][2]) * dL_db;
        const float dL_dT02 = 2 * (T.m[0][0] * Vrk.m[2][0] + T.m[0][1] * Vrk.m[2][1] + T.m[0][2] * Vrk.m[2][2]) * dL_da +
                              (T.m[1][0] * Vrk.m[2][0] + T.m[1][1] * Vrk.m[2][1] + T.m[1][2] * Vrk.m[2][2]) * dL_db;
        const float dL_dT10 = 2 * (T.m[1][0] * Vrk.m[0][0] + T.m[1][1] * Vrk.m[0][1] + T.m[1][2] * Vrk.m[0][2]) * dL_dc +
                              (T.m[0][0] * Vrk.m[0][0] + T.m[0][1] * Vrk.m[0][1] + T.m[0][2] * Vrk.m[0][2]) * dL_db;
        const float dL_dT11 = 2 * (T.m[1][0] * Vrk.m[1][0] + T.m[1][1] * Vrk.m[1][1] + T.m[1][2] * Vrk.m[1][2]) * dL_dc +
                              (T.m[0][0] * Vrk.m[1][0] + T.m[0][1] * Vrk.m[1][1] + T.m[0][2] * Vrk.m[1][2]) * dL_db;
        const float dL_dT12 = 2 * (T.m[1][0] * Vrk.m[2][0] + T.m[1][1] * Vrk.m[2][1] + T.m[1][2] * Vrk.m[2][2]) * dL_dc +
                              (T.m[0][0] * Vrk.m[2][0] + T.m[0][1] * Vrk.m[2][1] + T.m[0][2] * Vrk.m[2][2]) * dL_db;
        const float dL_dJ00 = W.m[0][0] * dL_dT00 + W.m[0][1] * dL_dT01 + W.m[0][2] * dL_dT02;
        const float dL_dJ02 = W.m[2][0] * dL_dT00 + W.m[2][1] * dL_dT01 + W.m[2][2] * dL_dT02;
        const float dL_dJ11 = W.m[1][0] * dL_dT10 + W.m[1][1] * dL_dT11 + W.m[1][2] * dL_dT12;
        const float dL_dJ12 = W.m[2][0] * dL_dT10 + W.m[2][1] * dL_dT11 + W.m[2][2] * dL_dT12;
        const float tz = 1.f / t.z;
        const float tz2 = tz * tz;
        const float tz3 = tz2 * tz;
        const float dL_dtx = x_grad_mul * -h_x * tz2 * dL_dJ02;
        const float dL_dty = y_grad_mul * -h_y * tz2 * dL_dJ12;
        const float dL_dtz = -h_x * tz2 * dL_dJ00 - h_y * tz2 * dL_dJ11 + (2 * h_x * t.x) * tz3 * dL_dJ02 + (2 * h_y * t.y) * tz3 * dL_dJ12;
        const float* v = a.view;
        if (COMPLETE) {
            // dL/dA = 2 G A Sigma, G = [[dL_da, dL_db/2], [dL_db/2, dL_dc]]: dL_dT{i}{k} above (T.m[i][k] = A[i][k]).
            // A = Ju Rcam: dL/dRcam[j][k] = sum_i Ju[i][j] dL/dA[i][k]; t_cam = Rcam m + t reaches Ju: mm_k dL/dt_cam,j.
            const float J00 = h_x * tz, J02 = -(h_x * t.x) * tz2, J11 = h_y * tz, J12 = -(h_y * t.y) * tz2;
            const float dA0[3] = {dL_dT00, dL_dT01, dL_dT02}, dA1[3] = {dL_dT10, dL_dT11, dL_dT12};
            const float mm[4] = {m.x, m.y, m.z, 1.0f};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                px[3 * k + 0] += mm[k] * dL_dtx;
                px[3 * k + 1] += mm[k] * dL_dty;
                px[3 * k + 2] += mm[k] * dL_dtz;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                px[3 * k + 0] += J00 * dA0[k];
                px[3 * k + 1] += J11 * dA1[k];
                px[3 * k + 2] += J02 * dA0[k] + J12 * dA1[k];
            }
        }
        if (!COMPLETE || do_map) {
            dmean.x += v[0] * dL_dtx + v[1] * dL_dty + v[2] * dL_dtz;
            dmean.y += v[4] * dL_dtx + v[5] * dL_dty + v[6] * dL_dtz;
            dmean.z += v[8] * dL_dtx + v[9] * dL_dty + v[10] * dL_dtz;
        }
        if (full) {  // depth -> mean term inside computeCov2DCUDA (F/cuda_rasterizer/backward.cu:385-386)
            const float mul3f = v[2] * m.x + v[6] * m.y + v[10] * m.z + v[14];
            dmean.x = dmean.x + acc[3] * (v[2] - v[3] * mul3f);
            dmean.y = dmean.y + acc[3] * (v[6] - v[7] * mul3f);
            dmean.z = dmean.z + acc[3] * (v[10] - v[11] * mul3f);
        }

        // ---------------- preprocessCUDA (L/cuda_rasterizer/backward.cu:348-416)
        const float* pj = a.proj;
        const float4 m_hom = xform4x4(m, pj);
        const float m_w = 1.0f / (m_hom.w + 0.0000001f);
        const float mul1 = (pj[0] * m.x + pj[4] * m.y + pj[8] * m.z + pj[12]) * m_w * m_w;
        const float mul2 = (pj[1] * m.x + pj[5] * m.y + pj[9] * m.z + pj[13]) * m_w * m_w;
        const float g2x = acc[4], g2y = acc[5];
        float3 d1;
        d1.x = (pj[0] * m_w - pj[3] * mul1) * g2x + (pj[1] * m_w - pj[3] * mul2) * g2y;
        d1.y = (pj[4] * m_w - pj[7] * mul1) * g2x + (pj[5] * m_w - pj[7] * mul2) * g2y;
        d1.z = (pj[8] * m_w - pj[11] * mul1) * g2x + (pj[9] * m_w - pj[11] * mul2) * g2y;
        if (!COMPLETE || do_map) { dmean.x += d1.x; dmean.y += d1.y; dmean.z += d1.z; }
        if (!full && (!COMPLETE || do_map)) {  // light: depth -> mean term inside preprocessCUDA (L/cuda_rasterizer/backward.cu:396-407)
            const float mul3 = v[2] * m.x + v[6] * m.y + v[10] * m.z + v[14];
            float3 d2;
            d2.x = (v[2] - v[3] * mul3) * acc[3];
            d2.y = (v[6] - v[7] * mul3) * acc[3];
            d2.z = (v[10] - v[11] * mul3) * acc[3];
            dmean.x += d2.x; dmean.y += d2.y; dmean.z += d2.z;
        }
    }
    // ---------------- SH backward (L/cuda_rasterizer/backward.cu:20-139): the scalars and the masked colour gradient
#pragma unroll
    for (int k = 0; k < 16; k++) coef[k] = 0.0f;
    dRGB = make_float3(0.f, 0.f, 0.f);
    // (COMPLETE: also without a dL_dsh output -- a tracking step -- for dL/dcampos; the outputs below only where the default runs)
    const bool sh_out = a.dL_dsh && do_map;
    if ((COMPLETE ? true : a.dL_dsh != nullptr) && a.M > 0 && do_terms && a.shs) {
        const float3 cam = make_float3(a.campos[0], a.campos[1], a.campos[2]);
        const float3 dir_orig = m - cam;
        const float len = sqrtf(dot3(dir_orig, dir_orig));
        const float3 dir = make_float3(dir_orig.x / len, dir_orig.y / len, dir_orig.z / len);
        const uint8_t cl = cl_in;
        dRGB = make_float3(acc[0], acc[1], acc[2]);
        dRGB.x *= (cl & 1) ? 0 : 1;
        dRGB.y *= (cl & 2) ? 0 : 1;
        dRGB.z *= (cl & 4) ? 0 : 1;
        // d(colour)/d(direction): the forward evaluated it from the SH row it had in registers (geom.shd_a/b/c, requested
        // with the other inputs above) -- the basis values below need the direction only, so the 192-byte rows are
        // not read again
        const float3 dRGBdx = make_float3(shd_a.x, shd_a.y, shd_a.z), dRGBdy = make_float3(shd_a.w, shd_b.x, shd_b.y),
                     dRGBdz = make_float3(shd_b.z, shd_b.w, shd_c);
        const float x = dir.x, y = dir.y, z = dir.z;
        coef[0] = SH_C0;
        if (a.D > 0) {
            coef[1] = -SH_C1 * y;
            coef[2] = SH_C1 * z;
            coef[3] = -SH_C1 * x;
            if (a.D > 1) {
                const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                coef[4] = SH_C2[0] * xy;
                coef[5] = SH_C2[1] * yz;
                coef[6] = SH_C2[2] * (2.f * zz - xx - yy);
                coef[7] = SH_C2[3] * xz;
                coef[8] = SH_C2[4] * (xx - yy);
                if (a.D > 2) {
                    coef[9] = SH_C3[0] * y * (3.f * xx - yy);
                    coef[10] = SH_C3[1] * xy * z;
                    coef[11] = SH_C3[2] * y * (4.f * zz - xx - yy);
                    coef[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
                    coef[13] = SH_C3[4] * x * (4.f * zz - xx - yy);
                    coef[14] = SH_C3[5] * z * (xx - yy);
                    coef[15] = SH_C3[6] * x * (xx - 3.f * yy);
                }
            }
        }
        if (full) {
            // dgc_dCampos (F/cuda_rasterizer/backward.cu:27-43,159-166; not clamp-masked) contracted with the
            // raw colour gradient: all ComputePG's part 1 needs of this Gaussian (:990-1022, 1313-1324)
            const float len3 = len * len * len;
            const float i3 = 1.0f / len3, i1 = 1.0f / len;
            const float3 o = dir_orig;
            const float3 raw = make_float3(acc[0], acc[1], acc[2]);
            const float3 cx = dRGBdx * (o.x * o.x * i3 - i1) + dRGBdy * (o.x * o.y * i3) + dRGBdz * (o.x * o.z * i3);
            const float3 cy = dRGBdx * (o.x * o.y * i3) + dRGBdy * (o.y * o.y * i3 - i1) + dRGBdz * (o.y * o.z * i3);
            const float3 cz = dRGBdx * (o.x * o.z * i3) + dRGBdy * (o.y * o.z * i3) + dRGBdz * (o.z * o.z * i3 - i1);
            s_cam = make_float3(dot3(raw, cx), dot3(raw, cy), dot3(raw, cz));
        }
        const float3 dL_ddir = make_float3(dot3(dRGBdx, dRGB), dot3(dRGBdy, dRGB), dot3(dRGBdz, dRGB));
        // dnormvdv (cuda_rasterizer/auxiliary.h:109-119)
        {
            const float3 vv = dir_orig, dv = dL_ddir;
            const float sum2 = vv.x * vv.x + vv.y * vv.y + vv.z * vv.z;
            const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
            if (!COMPLETE || sh_out) {
                dmean.x += ((+sum2 - vv.x * vv.x) * dv.x - vv.y * vv.x * dv.y - vv.z * vv.x * dv.z) * invsum32;
                dmean.y += (-vv.x * vv.y * dv.x + (sum2 - vv.y * vv.y) * dv.y - vv.z * vv.y * dv.z) * invsum32;
                dmean.z += (-vv.x * vv.z * dv.x - vv.y * vv.z * dv.y + (sum2 - vv.z * vv.z) * dv.z) * invsum32;
            }
            if (COMPLETE)  // dir = m - campos: dL/dcampos is minus the term above
                g_cam = make_float3(-(((+sum2 - vv.x * vv.x) * dv.x - vv.y * vv.x * dv.y - vv.z * vv.x * dv.z) * invsum32),
                                    -((-vv.x * vv.y * dv.x + (sum2 - vv.y * vv.y) * dv.y - vv.z * vv.y * dv.z) * invsum32),
                                    -((-vv.x * vv.z * dv.x - vv.y * vv.z * dv.y + (sum2 - vv.z * vv.z) * dv.z) * invsum32));
        }
        if (COMPLETE && !sh_out) {  // (no dL_dsh row for this view: as the default leaves it)
            dRGB = make_float3(0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < 16; k++) coef[k] = 0.0f;
        }
    }
    if (COMPLETE) {
        // campos = -Rcam^T t: dL/dRcam[j][k] = -t_j g_k, dL/dt_j = -sum_k Rcam[j][k] g_k  (Rcam[j][k] = v[4 k + j], t_j = v[12 + j])
        const float* v = a.view;
        const float g[3] = {g_cam.x, g_cam.y, g_cam.z};
#pragma unroll
        for (int j = 0; j < 3; j++) {
#pragma unroll
            for (int k = 0; k < 3; k++) px[3 * k + j] += -v[12 + j] * g[k];
            px[9 + j] += -(v[j] * g[0] + v[4 + j] * g[1] + v[8 + j] * g[2]);
        }
    }
    // ---------------- pose gradient: sum over Gaussians of Jacobian x (sum over pixels)
    // L/cuda_rasterizer/backward.cu:633-651 accumulates J_k(g) * {nx, ny, dL_ddepth} per pixel; J_k
    // depends on the Gaussian only, so the pixel sums are taken first (acc[4], acc[5], acc[13]).
    if (vis && !a.track_off) {
        const float4 m_hom = xform4x4(m, a.proj);
        const float m_w = 1.0f / (m_hom.w + 0.0000001f);
        const float mm[4] = {m.x, m.y, m.z, 1.0f};
        if (COMPLETE) {
            // the ndc terms from the mean2D sums dL_dmeans3D uses, the z path from its depth sums (light: depth and variance in
            // acc[3], median in acc[10]; full: the depth -> mean term's acc[3]), then the cov2D and SH paths.  The ndc rows get
            // their full derivative d ndc_r / d t_cam,j = m_w persp[4 j + r] - m_hom.r m_w^2 persp[4 j + 3]: the principal point
            // (persp[8], persp[9]) and any skew reach the pose as they reach dL_dmeans3D through projmatrix
            const float A = acc[4], B = acc[5], Dz = full ? acc[3] : acc[3] + acc[10];
            const float* pp = a.perspec;
            const float hx = m_hom.x * (-m_w * m_w), hy = m_hom.y * (-m_w * m_w);
            float nd[3];
#pragma unroll
            for (int j = 0; j < 3; j++)
                nd[j] = (m_w * pp[4 * j + 0] + hx * pp[4 * j + 3]) * A + (m_w * pp[4 * j + 1] + hy * pp[4 * j + 3]) * B;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                pose[3 * k + 0] = nd[0] * mm[k] + px[3 * k + 0];
                pose[3 * k + 1] = nd[1] * mm[k] + px[3 * k + 1];
                pose[3 * k + 2] = nd[2] * mm[k] + mm[k] * Dz + px[3 * k + 2];
            }
        } else if (!full) {
            const float A = acc[4], B = acc[5], Dd = acc[13];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                pose[3 * k + 0] = (m_w * a.perspec[0] * mm[k]) * A;
                pose[3 * k + 1] = (m_w * a.perspec[5] * mm[k]) * B;
                pose[3 * k + 2] = (m_hom.x * (-m_w * m_w) * mm[k]) * A + (m_hom.y * (-m_w * m_w) * mm[k]) * B + mm[k] * Dd;
            }
        } else {
            // ComputePG (F/cuda_rasterizer/backward.cu:990-1072, 1247-1289, 1313-1324) summed per Gaussian:
            // part 1 (colour -> campos -> view) + part 2-1 (ndc -> view, colour terms) + the depth terms of the
            // pixels whose front-most valid Gaussian this is.
            const float A = acc[10], B = acc[11], Dw = acc[12], Dx = acc[13], Dy = acc[14];
            const float* v = a.view;
            const float sc[3] = {s_cam.x, s_cam.y, s_cam.z};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float jx0 = m_w * a.perspec[0] * mm[k], jy1 = m_w * a.perspec[5] * mm[k];
                const float jx2 = m_hom.x * (-m_w * m_w) * mm[k], jy2 = m_hom.y * (-m_w * m_w) * mm[k];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    float p1;
                    if (k < 3) p1 = sc[k] * (-v[12 + j]);
                    else p1 = sc[0] * (-v[j]) + sc[1] * (-v[4 + j]) + sc[2] * (-v[8 + j]);
                    float p21, dpt;
                    if (j == 0) { p21 = jx0 * A; dpt = jx0 * Dx; }
                    else if (j == 1) { p21 = jy1 * B; dpt = jy1 * Dy; }
                    else { p21 = jx2 * A + jy2 * B; dpt = mm[k] * Dw + (jx2 * Dx + jy2 * Dy); }
                    pose[3 * k + j] = (p1 + p21) + dpt;
                }
            }
        }
    }
    dmean_out = dmean;
}

// The blend kernel's accumulator row of one Gaussian, as the one-view and the batched backward use it: zero when the view culled
// the Gaussian.  (The four 16-byte loads stay with the caller, which requests every input up front.)
__device__ __forceinline__ void unpack_acc_row(float4 a0, float4 a1, float4 a2, float4 a3, bool vis, float (&acc)[16]) {
    if (vis) {
        acc[0] = a0.x; acc[1] = a0.y; acc[2] = a0.z; acc[3] = a0.w; acc[4] = a1.x; acc[5] = a1.y; acc[6] = a1.z; acc[7] = a1.w;
        acc[8] = a2.x; acc[9] = a2.y; acc[10] = a2.z; acc[11] = a2.w; acc[12] = a3.x; acc[13] = a3.y; acc[14] = a3.z; acc[15] = a3.w;
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = 0.0f;
    }
}
// dL_dmean2D (nullable, per view): a plain copy of the blend kernel's sums, zero under map_off (preprocess_bwd_kernel has the reason)
__device__ __forceinline__ void write_dmean2D(const PreprocessBwdArgs& a, int idx, const float (&acc)[16]) {
    if (a.dL_dmean2D) {
        a.dL_dmean2D[3 * (size_t)idx + 0] = a.map_off ? 0.0f : acc[4];
        a.dL_dmean2D[3 * (size_t)idx + 1] = a.map_off ? 0.0f : acc[5];
        a.dL_dmean2D[3 * (size_t)idx + 2] = 0.0f;
    }
}

// Fused per-Gaussian backward.  Order of the dL_dmean3D accumulation follows the reference's kernel
// order: blend-kernel median term, computeCov2DCUDA, preprocessCUDA (2D mean, depth, SH).
// (forcing more than 4 waves/SIMD spills: 5 -> 128 us, 6 -> 163 us against 87 us)
#ifndef DGR_PPB_WAVES
#define DGR_PPB_WAVES 4
#endif
// COMPLETE: the complete pose gradient (bwd_view_terms); the default instance is the reference's terms, unchanged.
template <bool COMPLETE>
__global__ void __launch_bounds__(256, DGR_PPB_WAVES) preprocess_bwd_kernel(PreprocessBwdArgs a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    float pose[12];
#pragma unroll
    for (int i = 0; i < 12; i++) pose[i] = 0.0f;

    if (idx < a.P) {
        // Every per-Gaussian input is requested up front, unconditionally (a culled Gaussian wastes ~130 bytes): behind
        // `if (vis)` / `if (do_map)` the loads formed a chain of three dependent round trips per wave, and this kernel
        // spends 60 % of its wave-cycles waiting for memory.
        float4* ap = reinterpret_cast<float4*>(a.acc + (size_t)idx * DGR_ACC_STRIDE);
        const float4 a0 = ap[0], a1 = ap[1], a2 = ap[2], a3 = ap[3];  // (nontemporal loads here: 45 -> 49 us -- the rows sit in L2, where the blend's atomics left them)
        const int rad = a.radii[idx];

        const float3 m = load_row3(a.means3D, idx);
        // A tracking step (map_off: the pose gradient only) needs the three sums, the mean and the radius: the covariance, the
        // scale / rotation, the clamp bits and the SH direction derivatives -- 65 of the 145 bytes a Gaussian costs this kernel --
        // feed only the per-Gaussian gradients.  The test is kernel-uniform and known at launch: no load waits for another.
        // (COMPLETE: the pose's cov2D and SH paths need the covariance, the clamp bits and the SH direction derivatives too)
        const bool need_map = !a.map_off;
        const bool need_terms = COMPLETE || need_map;
        float c3[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // (load_cov3d's branch, written out: through the helper the default instance keeps its instructions but clears c3[] in
        //  another order, and a tracking step measured 0.0302 against 0.0298 ms: profiles/per_gaussian_split/notes.md)
        if (need_terms) {
            if (a.cov3D_precomp) {
                const float* c3p = a.cov3D_precomp + 6 * (size_t)idx;
#pragma unroll
                for (int i = 0; i < 6; i++) c3[i] = c3p[i];
            } else {  // re-formed from scale and rotation: the forward's expression, the forward's bits
                compute_cov3d(a.scales, a.rotations, a.scale_modifier, idx, c3);
            }
        }
        float3 sc_in = make_float3(0.f, 0.f, 0.f);
        float4 q_in = make_float4(0.f, 0.f, 0.f, 0.f);
        if (need_map && a.scales) {
            sc_in = load_row3(a.scales, idx);
            q_in = load_row4(a.rotations, idx);
        }
        uint8_t cl_in = 0;
        float4 shd_a = make_float4(0.f, 0.f, 0.f, 0.f), shd_b = shd_a;
        float shd_c = 0.f;
        if (need_terms) {
            cl_in = a.geom.clamped[idx];
            shd_a = a.geom.shd_a[idx]; shd_b = a.geom.shd_b[idx]; shd_c = a.geom.shd_c[idx];
        }
        const bool vis = rad > 0;
        float acc[16];
        unpack_acc_row(a0, a1, a2, a3, vis, acc);

        // ---- outputs that are plain copies of the blend kernel's sums
        // (with map_off the blend kernel still sums acc[4], acc[5] for the pose gradient, but the
        //  reference leaves every per-Gaussian gradient at zero: L/cuda_rasterizer/backward.cu:666)
        // (every dense output may be NULL: a tracking step needs the pose gradient only, dgr_hip.h)
        write_dmean2D(a, idx, acc);
        // (COMPLETE under map_off: the mapping blend filled these sums, the tracking blend leaves them zero -- so do the outputs)
        const bool zero_copies = COMPLETE && a.map_off;
        if (a.dL_dopacity) a.dL_dopacity[idx] = zero_copies ? 0.0f : acc[9];
        if (a.dL_dcolor) {
            a.dL_dcolor[3 * (size_t)idx + 0] = zero_copies ? 0.0f : acc[0];
            a.dL_dcolor[3 * (size_t)idx + 1] = zero_copies ? 0.0f : acc[1];
            a.dL_dcolor[3 * (size_t)idx + 2] = zero_copies ? 0.0f : acc[2];
        }
        if (a.dL_ddepth) a.dL_ddepth[idx] = zero_copies ? 0.0f : acc[3];
        if (a.dL_dconic) {
            float4* o = reinterpret_cast<float4*>(a.dL_dconic) + idx;
            *o = zero_copies ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(acc[6], acc[7], 0.0f, acc[8]);
        }

        float3 dmean;
        float dcov[6], coef[16];
        float3 dRGB;
        bwd_view_terms<COMPLETE>(a, a.full_variant != 0, m, c3, acc, vis, cl_in, shd_a, shd_b, shd_c, dmean, dcov, coef, dRGB, pose);
        float3 dscale = make_float3(0, 0, 0);
        float4 drot = make_float4(0, 0, 0, 0);
        const bool do_map = vis && !a.map_off;
        const int ncoef_out = a.M;

        // ---------------- the dense dL_dsh row: dL_dsh[k] = coef[k] * dRGB (zeros for rows this view did not map)
        if (a.dL_dsh && ncoef_out > 0) {
            float3* out = reinterpret_cast<float3*>(a.dL_dsh) + (size_t)idx * ncoef_out;
            // whole block in range, 16 coefficients, 16-byte aligned rows: SH rows move through LDS (block-uniform)
            __shared__ float sht[4 * SHT_ROWS * SHT_LD];
            const bool blk_fast = a.sh_vec_ok && ncoef_out == 16 && a.shs != nullptr && (size_t)blockIdx.x * 256 + 256 <= (size_t)a.P;
            if (do_map && a.shs) {
                if (blk_fast) {
                    // (written below, through LDS)
                } else if (a.sh_vec_ok && ncoef_out == 16) {
                    const float ch[3] = {dRGB.x, dRGB.y, dRGB.z};
                    float4* o4 = reinterpret_cast<float4*>(out);
#pragma unroll
                    for (int i = 0; i < 12; i++)
                        o4[i] = make_float4(coef[(4 * i) / 3] * ch[(4 * i) % 3], coef[(4 * i + 1) / 3] * ch[(4 * i + 1) % 3],
                                            coef[(4 * i + 2) / 3] * ch[(4 * i + 2) % 3], coef[(4 * i + 3) / 3] * ch[(4 * i + 3) % 3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 16; k++)
                        if (k < ncoef_out) out[k] = coef[k] * dRGB;
                }
            } else if (!blk_fast) {
                if (a.sh_vec_ok && ncoef_out == 16) {
                    float4* o4 = reinterpret_cast<float4*>(out);
#pragma unroll
                    for (int i = 0; i < 12; i++) o4[i] = make_float4(0, 0, 0, 0);
                } else {
                    for (int k = 0; k < ncoef_out; k++) out[k] = make_float3(0, 0, 0);
                }
            }
            if (blk_fast) lanes_to_sh_rows_scaled(coef, dRGB, a.dL_dsh, (size_t)blockIdx.x * 256, sht);
        }

        if (do_map && a.scales) cov3d_backward_terms(sc_in, q_in, a.scale_modifier, dcov, dscale, drot);

        if (a.dL_dmean3D) store_row3(a.dL_dmean3D, idx, dmean);
        if (a.dL_dcov3D) store_row6(a.dL_dcov3D, idx, dcov);
        if (a.dL_dscale) store_row3(a.dL_dscale, idx, dscale);
        if (a.dL_drot) store_row4(a.dL_drot, idx, drot);
    }
    // Resident scratch: the readers clear the rows they have read.  The 64 rows of a wave's Gaussians are 4 KB in a row, so the
    // wave clears them together with four fully coalesced 16-byte stores per lane (rows of Gaussians the view did not see are
    // zero already; writing them again costs nothing extra).  Every lane's loads of its own row have been consumed by now.
    // (Each lane clearing its own row -- four stores of 16 bytes at a 64-byte stride, 64 partial lines per instruction -- cost the
    //  kernel 30 us at config 3, 44 -> 74; right behind the loads, where it also delayed every other input's request, the same.)
    if (a.clear_scratch) {
        const size_t wave_row0 = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u);
        float4* wbase = reinterpret_cast<float4*>(a.acc + wave_row0 * DGR_ACC_STRIDE);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int piece = k * 64 + (int)(threadIdx.x & 63u);           // 16-byte piece of the wave's 4 KB
            if (wave_row0 + (size_t)(piece >> 2) < (size_t)a.P) wbase[piece] = z;
        }
    }

    if (a.track_off) {  // no pose gradient asked for: zeros (L/rasterize_points.cu:186)
        pose_zero(a.dL_dview);
        return;
    }
    __shared__ double red[16][12];
    if (a.det_pose)
        pose_block_reduce_det(pose, a.det_pose, a.ticket, a.dL_dview, red, a.clear_scratch != 0);
    else
        pose_block_reduce(pose, a.pose_part, a.ticket, a.dL_dview, red, a.clear_scratch != 0);
}

// ------------------------------------------------------------------------------------------------
// Batched per-Gaussian backward: the V views of a batch in ONE launch, the gradients of the shared
// Gaussians SUMMED OVER THE VIEWS in registers and written once.  Per view a lane reads that view's 64-byte accumulator row,
// radius, clamp bits and SH direction derivatives and runs the code of the one-view kernel (bwd_view_terms); position,
// covariance, scale and rotation are read once; the covariance backward -- linear in dL_dcov3D -- runs once on the summed
// dL_dcov3D.  A view's terms are formed exactly as the one-view kernel forms them and added in view order with FMA
// contraction off, so -- for the same accumulator rows -- dL_dmeans3D / dL_dsh / dL_dopacity / dL_dcov3D are what accumulating
// the one-view outputs view after view (autograd's `.grad +=`) gives, operation for operation, without the V dense 248-byte
// rows per Gaussian that costs.
// Pose gradients and dL_dmean2D (densification statistics) stay per view.  FULL: the full variant's view terms
// (bwd_view_terms(a, true, ...): the campos colour term and the depth-to-mean term), summed and written the same way; the
// batch writes no dL_dconic / dL_ddepth (implementation outputs that no autograd surface returns).
__device__ __forceinline__ PreprocessBwdArgs batch_view_args(const PreprocessBwdBatchArgs& b, int v) {
    PreprocessBwdArgs a = b.base;
    const BwdViewPart& p = b.v[v];
    a.view = p.view; a.proj = p.proj; a.campos = p.campos; a.perspec = p.perspec; a.radii = p.radii; a.geom = p.geom;
    a.acc = const_cast<float*>(p.acc); a.dL_dmean2D = p.dL_dmean2D; a.pose_part = p.pose_part; a.ticket = p.ticket; a.dL_dview = p.dL_dview;
    return a;
}
// (COMPLETE: held to the default instances' 3 waves per SIMD -- left to itself the light one takes 178 VGPRs, 2 waves)
template <bool FULL, bool COMPLETE = false>
__global__ void __launch_bounds__(256, COMPLETE ? 3 : DGR_BWD_BATCH_WAVES) preprocess_bwd_batch_kernel(PreprocessBwdBatchArgs b) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int P = b.base.P, V = b.V;
    const bool in = idx < P;
    __shared__ float sht[4 * SHT_ROWS * SHT_LD];
    __shared__ double red[DGR_MAX_BATCH_VIEWS][16][12];  // every view's row sums: ONE barrier behind the view loop
    float3 m = make_float3(0.f, 0.f, 0.f), sc_in = make_float3(0.f, 0.f, 0.f);
    float4 q_in = make_float4(0.f, 0.f, 0.f, 0.f);
    float c3[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (in) {
        m = load_row3(b.base.means3D, idx);
        if (b.base.cov3D_precomp || b.base.scales) load_cov3d(b.base, idx, c3);  // (neither: zeros)
        if (b.base.scales) {
            sc_in = load_row3(b.base.scales, idx);
            q_in = load_row4(b.base.rotations, idx);
        }
    }
    float3 dmean_s = make_float3(0.f, 0.f, 0.f), dcol_s = make_float3(0.f, 0.f, 0.f);
    float dcov_s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dop_s = 0.0f;
    float dsh[48];
#pragma unroll
    for (int e = 0; e < 48; e++) dsh[e] = 0.0f;
    bool any_map = false;
#pragma unroll 1
    for (int v = 0; v < V; v++) {
        const PreprocessBwdArgs a = batch_view_args(b, v);
        float pose[12];
#pragma unroll
        for (int i = 0; i < 12; i++) pose[i] = 0.0f;
        if (in) {
            const float4* ap = reinterpret_cast<const float4*>(a.acc + (size_t)idx * DGR_ACC_STRIDE);
            const float4 a0 = ap[0], a1 = ap[1], a2 = ap[2], a3 = ap[3];
            const int rad = a.radii[idx];
            const uint8_t cl_in = a.geom.clamped[idx];
            const float4 shd_a = a.geom.shd_a[idx], shd_b = a.geom.shd_b[idx];
            const float shd_c = a.geom.shd_c[idx];
            const bool vis = rad > 0;
            float acc[16];
            unpack_acc_row(a0, a1, a2, a3, vis, acc);
            write_dmean2D(a, idx, acc);
            float3 dmean, dRGB;
            float dcov[6], coef[16];
            bwd_view_terms<COMPLETE>(a, FULL, m, c3, acc, vis, cl_in, shd_a, shd_b, shd_c, dmean, dcov, coef, dRGB, pose);
            any_map |= vis && !a.map_off;
            if (!(COMPLETE && a.map_off)) {  // (COMPLETE under map_off: the mapping blend's sums reach no output, as one view)
                dop_s += acc[9];
                dcol_s.x += acc[0]; dcol_s.y += acc[1]; dcol_s.z += acc[2];
            }
            dmean_s.x += dmean.x; dmean_s.y += dmean.y; dmean_s.z += dmean.z;
#pragma unroll
            for (int i = 0; i < 6; i++) dcov_s[i] += dcov[i];
            const float ch[3] = {dRGB.x, dRGB.y, dRGB.z};
#pragma unroll
            for (int e = 0; e < 48; e++) dsh[e] += coef[e / 3] * ch[e % 3];  // (contraction is off: product, then sum)
        }
        if (a.track_off) {
            pose_zero(a.dL_dview);
        } else {
            pose_rows_to_lds(pose, red[v]);  // (no barrier inside the view loop: the waves run through it independently)
        }
    }
    const int M = b.base.M;
    const bool blk_fast = b.base.dL_dsh && b.base.sh_vec_ok && M == 16 && (size_t)blockIdx.x * 256 + 256 <= (size_t)P;
    if (in) {
        float3 dscale = make_float3(0, 0, 0);
        float4 drot = make_float4(0, 0, 0, 0);
        if (any_map && b.base.scales) cov3d_backward_terms(sc_in, q_in, b.base.scale_modifier, dcov_s, dscale, drot);
        if (b.base.dL_dopacity) b.base.dL_dopacity[idx] = dop_s;
        if (b.base.dL_dcolor) store_row3(b.base.dL_dcolor, idx, dcol_s);
        if (b.base.dL_dmean3D) store_row3(b.base.dL_dmean3D, idx, dmean_s);
        if (b.base.dL_dcov3D) store_row6(b.base.dL_dcov3D, idx, dcov_s);
        if (b.base.dL_dscale) store_row3(b.base.dL_dscale, idx, dscale);
        if (b.base.dL_drot) store_row4(b.base.dL_drot, idx, drot);
        if (b.base.dL_dsh && M > 0 && !blk_fast) {
            float* out = b.base.dL_dsh + (size_t)idx * M * 3;
#pragma unroll
            for (int e = 0; e < 48; e++)
                if (e < 3 * M) out[e] = dsh[e];
        }
    }
    if (blk_fast) lanes_to_sh_rows(dsh, b.base.dL_dsh, (size_t)blockIdx.x * 256, sht);
    pose_batch_reduce(b, red);
}

// ------------------------------------------------------------------------------------------------
// Backward of the view-independent 3D covariance of a batch of views (cov3d_fwd_kernel; L/cuda_rasterizer/backward.cu:280-343).
// It is LINEAR in dL_dcov3D, so the views' dL_dcov3D are summed first (autograd does that) and converted to dL_dscale /
// dL_drot once.
__global__ void __launch_bounds__(256) cov3d_bwd_kernel(int P, const float* __restrict__ scales, const float* __restrict__ rotations,
                                                        float mod, const float* __restrict__ dL_dcov3D, float* __restrict__ dL_dscale,
                                                        float* __restrict__ dL_drot) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    float dcov[6];
#pragma unroll
    for (int i = 0; i < 6; i++) dcov[i] = dL_dcov3D[6 * (size_t)idx + i];
    const float3 sc = load_row3(scales, idx);
    const float4 q = load_row4(rotations, idx);
    float3 dscale;
    float4 drot;
    cov3d_backward_terms(sc, q, mod, dcov, dscale, drot);
    // the reference scales dL_dscale by the modifier through `s` only (backward.cu:318-322): so does preprocess_bwd
    store_row3(dL_dscale, idx, dscale);
    store_row4(dL_drot, idx, drot);
}

hipError_t launch_cov3d_backward(int P, const float* scales, const float* rotations, float mod, const float* dL_dcov3D,
                                 float* dL_dscale, float* dL_drot, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    launch(cov3d_bwd_kernel, dim3((P + 255) / 256), dim3(256), stream, P, scales, rotations, mod, dL_dcov3D, dL_dscale, dL_drot);
    return hipGetLastError();
}
namespace {
__global__ void __launch_bounds__(256) zero_fill_kernel(float4* dst, size_t n16) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) dst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
}  // namespace
hipError_t launch_zero_fill(void* dst, size_t bytes, hipStream_t stream) {
    const size_t n16 = bytes / 16;
    if (n16 == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<size_t>((n16 + 255) / 256, 256 * 16);
    launch(zero_fill_kernel, dim3(blocks), dim3(256), stream, (float4*)dst, n16);
    return hipGetLastError();
}
hipError_t launch_preprocess_bwd(const PreprocessBwdArgs& a, hipStream_t stream, bool complete_pose) {
    const int blocks = (a.P + 255) / 256;
    if (blocks <= 0) return hipSuccess;
    if (complete_pose) launch(preprocess_bwd_kernel<true>, dim3(blocks), dim3(256), stream, a);
    else launch(preprocess_bwd_kernel<false>, dim3(blocks), dim3(256), stream, a);
    return hipGetLastError();
}
hipError_t launch_preprocess_bwd_batch(const PreprocessBwdBatchArgs& b, hipStream_t stream, bool complete_pose) {
    if (b.base.P <= 0 || b.V <= 0) return hipSuccess;
    const dim3 grid((b.base.P + 255) / 256);
    if (b.base.full_variant) {
        if (complete_pose) launch(preprocess_bwd_batch_kernel<true, true>, grid, dim3(256), stream, b);
        else launch(preprocess_bwd_batch_kernel<true>, grid, dim3(256), stream, b);
    } else {
        if (complete_pose) launch(preprocess_bwd_batch_kernel<false, true>, grid, dim3(256), stream, b);
        else launch(preprocess_bwd_batch_kernel<false>, grid, dim3(256), stream, b);
    }
    return hipGetLastError();
}
}  // namespace dgr
