// icp.hip -- frame-to-model ICP pose alignment (include/dgr_hip.h: dgr_depth_normals, dgr_icp_step): the geometric pose
// initialisation in front of the photometric tracker.  KinectFusion's projective point-to-plane ICP of the sensor depth against the
// model's rendered depth.
//
// normals: one thread per pixel: the packed vertex-normal map (nx, ny, nz, d) from a depth image by central differences of the
//          unprojected neighbours.  One 16-byte store per pixel, so that the step's gather is one 16-byte load from one line.
// step   : one Gauss-Newton iteration in ONE launch.  One workgroup per block of 2048 candidates (the stride grid of
//          candidate_grid.h), as overlap_count_kernel: threads 0..11 form rel = T_model T_in^-1 in double and round it once, every
//          thread takes a candidate per trip and adds its 29 terms (A's upper triangle, b, sum w r^2, count) to its own double
//          accumulators.  Everything behind the sums is gn_step.h's, shared with gicp.hip: the row / ticket / block-order
//          reduction, the damped LDL^T solve, the pose and stats writer.  This file's own is the update between the last two:
//          T_out = T_in T_model^-1 exp(-xi) T_model.
// Hybrid RGB-D alignment (dgr_intensity_map, dgr_frame_halve, dgr_rgbd_step): the photometric term beside the geometric one.
// intensity: one thread per pixel: the packed intensity-gradient map (I, I_x, I_y, usable), Sobel / 8, and the plain intensity plane.
// halve    : one thread per output pixel: one pyramid level of any number of mean planes and one depth plane.
// rgbd step: the step's body instantiated on RgbdStepArgs: a second 16-byte gather, the photometric pair through the same
//          accumulation, two more sums (31); everything behind the sums is the ICP step's.
// No host read, no float atomics, the same bits on every run.
#include <hip/hip_runtime.h>

#include "candidate_grid.h"
#include "gn_step.h"
#include "kernels.h"

namespace dgr {
namespace {

constexpr int THREADS = GN_THREADS;
constexpr int BLOCK_CANDIDATES = GN_BLOCK_ITEMS;
constexpr int SUMS = 29;                // A (21), b (6), sum w r^2, count
constexpr int RGBD_SUMS = 31;           // A (21), b (6), sum w r^2, count_g, sum w_p r_p^2, count_p (the hybrid step's)
constexpr int RGBD_STATS = 40;          // doubles of the hybrid step's stats
constexpr unsigned ICP_VALID = 1u, ICP_INSIDE = 2u, ICP_ASSOCIATED = 4u, ICP_PHOTOMETRIC = 8u;

// ---------------------------------------------------------------------------------------------------------------- normals
__global__ void __launch_bounds__(THREADS) depth_normals_kernel(DepthNormalsArgs a) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const size_t n = (size_t)a.W * (size_t)a.H;
    if (i >= n) return;
    const unsigned y = (unsigned)(i / (unsigned)a.W), x = (unsigned)(i - (size_t)y * (unsigned)a.W);
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x >= 1 && y >= 1 && x + 1 < (unsigned)a.W && y + 1 < (unsigned)a.H) {
        const float d = a.depth[i], dl = a.depth[i - 1], dr = a.depth[i + 1], du = a.depth[i - a.W], dd = a.depth[i + a.W];
        const float lo = a.depth_min, hi = a.depth_max;
        bool ok = d > lo && d < hi && dl > lo && dl < hi && dr > lo && dr < hi && du > lo && du < hi && dd > lo && dd < hi;
        if (a.mask) ok = ok && a.mask[i] > a.mask_threshold;
        if (ok) {  // (false on a NaN, as every test here)
            const float jump = a.max_jump * d;
            ok = fabsf(dl - d) <= jump && fabsf(dr - d) <= jump && fabsf(du - d) <= jump && fabsf(dd - d) <= jump;
        }
        if (ok) {
            const float fx_ = (float)x, fy_ = (float)y;
            const float X = (fx_ - a.cx) * a.inv_fx, Y = (fy_ - a.cy) * a.inv_fy;  // the centre's ray
            const float Xl = ((fx_ - 1.f) - a.cx) * a.inv_fx, Xr = ((fx_ + 1.f) - a.cx) * a.inv_fx;
            const float Yu = ((fy_ - 1.f) - a.cy) * a.inv_fy, Yd = ((fy_ + 1.f) - a.cy) * a.inv_fy;
            // a = V(x + 1, y) - V(x - 1, y), b = V(x, y + 1) - V(x, y - 1)
            const float a0 = Xr * dr - Xl * dl, a1 = Y * dr - Y * dl, a2 = dr - dl;
            const float b0 = X * dd - X * du, b1 = Yd * dd - Yu * du, b2 = dd - du;
            float c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
            const float len2 = c0 * c0 + c1 * c1 + c2 * c2;
            if (len2 > 0.f && len2 < INFINITY) {
                const float len = sqrtf(len2);
                c0 /= len, c1 /= len, c2 /= len;
                if (c0 * (X * d) + c1 * (Y * d) + c2 * d > 0.f) c0 = -c0, c1 = -c1, c2 = -c2;  // facing the camera
                out = make_float4(c0, c1, c2, d);
            }
        }
    }
    a.vnmap[i] = out;
}

// ---------------------------------------------------------------------------------------------------------- intensity map
// the intensity of pixel i: the single channel's bits, or (0.299 R + 0.587 G) + 0.114 B
__device__ __forceinline__ float intensity_at(const IntensityMapArgs& a, size_t i, size_t n) {
    if (a.C == 1) return a.image[i];
    return (0.299f * a.image[i] + 0.587f * a.image[n + i]) + 0.114f * a.image[2 * n + i];
}
__global__ void __launch_bounds__(THREADS) intensity_map_kernel(IntensityMapArgs a) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const size_t n = (size_t)a.W * (size_t)a.H;
    if (i >= n) return;
    const unsigned y = (unsigned)(i / (unsigned)a.W), x = (unsigned)(i - (size_t)y * (unsigned)a.W);
    const float I = intensity_at(a, i, n);
    if (a.intensity) a.intensity[i] = I;
    if (!a.imap) return;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x >= 1 && y >= 1 && x + 1 < (unsigned)a.W && y + 1 < (unsigned)a.H) {
        const size_t up = i - (size_t)a.W, dn = i + (size_t)a.W;
        const float ul = intensity_at(a, up - 1, n), uc = intensity_at(a, up, n), ur = intensity_at(a, up + 1, n);
        const float cl = intensity_at(a, i - 1, n), cr = intensity_at(a, i + 1, n);
        const float dl = intensity_at(a, dn - 1, n), dc = intensity_at(a, dn, n), dr = intensity_at(a, dn + 1, n);
        // finite: |v| < inf is false on a NaN
        bool ok = fabsf(ul) < INFINITY && fabsf(uc) < INFINITY && fabsf(ur) < INFINITY && fabsf(cl) < INFINITY &&
                  fabsf(I) < INFINITY && fabsf(cr) < INFINITY && fabsf(dl) < INFINITY && fabsf(dc) < INFINITY && fabsf(dr) < INFINITY;
        if (ok && a.mask) {
            const float t = a.mask_threshold;
            ok = a.mask[up - 1] > t && a.mask[up] > t && a.mask[up + 1] > t && a.mask[i - 1] > t && a.mask[i] > t &&
                 a.mask[i + 1] > t && a.mask[dn - 1] > t && a.mask[dn] > t && a.mask[dn + 1] > t;
        }
        if (ok) {
            const float gx = (((ur - ul) + (dr - dl)) + 2.f * (cr - cl)) * 0.125f;
            const float gy = (((dl - ul) + (dr - ur)) + 2.f * (dc - uc)) * 0.125f;
            out = make_float4(I, gx, gy, 1.f);
        }
    }
    a.imap[i] = out;
}

// ------------------------------------------------------------------------------------------------------------------ halve
__global__ void __launch_bounds__(THREADS) frame_halve_kernel(FrameHalveArgs a) {
    const unsigned Wo = (unsigned)a.W >> 1, Ho = (unsigned)a.H >> 1;
    const size_t o = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const size_t no = (size_t)Wo * Ho, n = (size_t)a.W * (size_t)a.H;
    if (o >= no) return;
    const unsigned y = (unsigned)(o / Wo), x = (unsigned)(o - (size_t)y * Wo);
    const size_t i = (size_t)(2u * y) * (unsigned)a.W + 2u * x;  // the block's first pixel; an odd last row or column is dropped
    for (int p = 0; p < a.planes; p++) {
        const float* in = a.planes_in + (size_t)p * n;
        a.planes_out[(size_t)p * no + o] = ((in[i] + in[i + 1]) + (in[i + a.W] + in[i + a.W + 1])) * 0.25f;
    }
    if (a.depth_in) {
        const float d[4] = {a.depth_in[i], a.depth_in[i + 1], a.depth_in[i + a.W], a.depth_in[i + a.W + 1]};
        float v[4], lo = INFINITY, hi = -INFINITY, count = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool ok = d[k] > a.depth_min && d[k] < a.depth_max;  // (false on a NaN)
            v[k] = ok ? d[k] : 0.f;
            if (ok) lo = fminf(lo, d[k]), hi = fmaxf(hi, d[k]), count += 1.f;
        }
        float out = 0.f;
        if (count > 0.f && hi - lo <= a.max_jump * lo) out = ((v[0] + v[1]) + (v[2] + v[3])) / count;
        a.depth_out[o] = out;
    }
}

// -------------------------------------------------------------------------------------------------------------------- step
// One thread: the totals through gn_step.h's solve, the model-frame update, its writer.  RGBD: the hybrid step's 31 totals (the
// count is both classes', the photometric sum w r^2 must be finite too) and 40 stats.
template <bool RGBD>
__device__ void icp_finish(const IcpStepArgs& a, const double* tot) {
    double xi[6];
    const bool ok = gn_solve(tot, RGBD ? tot[28] + tot[30] : tot[28], !RGBD || isfinite(tot[29]), a.min_points, a.damping, a.rcond, xi);
    GnPoseIn in;
    gn_read_pose(a.viewmatrix_in, in);
    double Ro[3][3], to[3];
    if (ok) {
        // T_out = T_in T_model^-1 exp(-xi) T_model
        double Rm[3][3], tm[3], Re[3][3], te[3], R1[3][3], t1[3], R2[3][3], t2[3];
        pose_of(a.model_viewmatrix, Rm, tm);
        const double w[3] = {-xi[0], -xi[1], -xi[2]}, v[3] = {-xi[3], -xi[4], -xi[5]};
        se3_exp(w, v, Re, te);
        compose(Re, te, Rm, tm, R1, t1);
        double Rmt[3][3], tmi[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) Rmt[i][j] = Rm[j][i];
            tmi[i] = -(Rm[0][i] * tm[0] + Rm[1][i] * tm[1] + Rm[2][i] * tm[2]);
        }
        compose(Rmt, tmi, R1, t1, R2, t2);
        compose(in.R, in.t, R2, t2, Ro, to);
    }
    gn_write<RGBD ? RGBD_SUMS : SUMS, RGBD ? RGBD_STATS : SUMS + 3>(ok, Ro, to, in, xi, tot, a.viewmatrix_out, a.quat_out, a.trans_out, a.stats);
}

// one pair's terms onto a thread's sums: A += (s J_i) J_j, b += (s J_i) r, each product rounded to fp32 before it is widened
__device__ __forceinline__ void add_pair(double* acc, const float (&J)[6], float r, float s) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const float sj = s * J[i];
#pragma unroll
        for (int j = i; j < 6; j++) acc[k++] += (double)(sj * J[j]);
        acc[21 + i] += (double)(sj * r);
    }
}

// grid: one workgroup per block of candidates.  `ticket`, `part`: gn_reduce's.
// Args: IcpStepArgs, or RgbdStepArgs for the hybrid step (dgr_rgbd_step): the photometric pair beside the geometric one, each
// scaled by its class weight, two more sums.
template <class Args>
__global__ void __launch_bounds__(THREADS) icp_step_kernel(Args a, uint32_t* __restrict__ ticket, double* __restrict__ part) {
    constexpr bool RGBD = Args::rgbd;
    constexpr int SUMS = RGBD ? RGBD_SUMS : dgr::SUMS;
    __shared__ float rel[12];  // current camera point p -> model camera point: q_j = rel[3 j] p_0 + rel[3 j + 1] p_1 + rel[3 j + 2] p_2 + rel[9 + j]
    if (threadIdx.x < 12) {
        // both matrices hold W2C^T: W2C's rotation entry R[j][i] at [4 i + j], its translation t[j] at [12 + j].
        // q = R_m R_in^T (p - t_in) + t_m
        const float* __restrict__ vc = a.viewmatrix_in;
        const float* __restrict__ vk = a.model_viewmatrix;
        const int j = threadIdx.x < 9 ? threadIdx.x / 3 : threadIdx.x - 9;
        double r[3];
#pragma unroll
        for (int m = 0; m < 3; ++m)
            r[m] = (double)vk[j] * (double)vc[m] + (double)vk[4 + j] * (double)vc[4 + m] + (double)vk[8 + j] * (double)vc[8 + m];
        const int m = threadIdx.x - 3 * j;
        if (threadIdx.x < 9) rel[threadIdx.x] = (float)(m == 0 ? r[0] : m == 1 ? r[1] : r[2]);
        else rel[threadIdx.x] = (float)((double)vk[12 + j] - (r[0] * (double)vc[12] + r[1] * (double)vc[13] + r[2] * (double)vc[14]));
    }
    __syncthreads();
    const float r00 = rel[0], r01 = rel[1], r02 = rel[2], r10 = rel[3], r11 = rel[4], r12 = rel[5], r20 = rel[6], r21 = rel[7],
                r22 = rel[8], t0 = rel[9], t1 = rel[10], t2 = rel[11];
    const float Wf = (float)a.W, Hf = (float)a.H;
    const size_t begin = (size_t)blockIdx.x * BLOCK_CANDIDATES;
    const size_t end = begin + BLOCK_CANDIDATES < a.candidates ? begin + BLOCK_CANDIDATES : a.candidates;
    double acc[SUMS];
#pragma unroll
    for (int i = 0; i < SUMS; i++) acc[i] = 0.0;
    for (size_t c = begin + threadIdx.x; c < end; c += THREADS) {  // this thread's candidates, ascending
        unsigned x, y;
        candidate_pixel(c, a.wc, a.stride, x, y);
        const size_t pix = (size_t)y * (unsigned)a.W + x;
        const float d = a.depth_obs[pix];
        bool valid = d > a.depth_min && d < a.depth_max;  // (false on a NaN)
        float4 no = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.vn_obs) {
            no = a.vn_obs[pix];
            valid = valid && no.w > 0.f;
        }
        bool inside = false, associated = false;
        [[maybe_unused]] bool photometric = false;
        if (valid) {
            const float p0 = ((float)x - a.cx) * a.inv_fx * d, p1 = ((float)y - a.cy) * a.inv_fy * d;
            const float q0 = r00 * p0 + r01 * p1 + r02 * d + t0;
            const float q1 = r10 * p0 + r11 * p1 + r12 * d + t1;
            const float q2 = r20 * p0 + r21 * p1 + r22 * d + t2;
            const float u = a.fx * q0 / q2 + a.cx, v = a.fy * q1 / q2 + a.cy;
            const float uf = floorf(u + 0.5f), vf = floorf(v + 0.5f);
            if (q2 > 0.f && uf >= 0.f && uf < Wf && vf >= 0.f && vf < Hf) {  // (false on a NaN: the casts below are in range)
                const size_t mpix = (size_t)(unsigned)(int)vf * (unsigned)a.W + (unsigned)(int)uf;
                const float4 m = a.vn_model[mpix];
                [[maybe_unused]] float4 im;
                [[maybe_unused]] float io;
                if constexpr (RGBD) im = a.imap_model[mpix], io = a.intensity_obs[pix];  // (in flight beside m)
                if (m.w > 0.f) {
                    inside = true;
                    const float e0 = q0 - (uf - a.cx) * a.inv_fx * m.w, e1 = q1 - (vf - a.cy) * a.inv_fy * m.w, e2 = q2 - m.w;
                    associated = sqrtf(e0 * e0 + e1 * e1 + e2 * e2) <= a.dist_max;
                    [[maybe_unused]] const bool near = associated;  // |e| <= dist_max: the photometric pair's occlusion test
                    if (a.vn_obs) {
                        const float n0 = r00 * no.x + r01 * no.y + r02 * no.z, n1 = r10 * no.x + r11 * no.y + r12 * no.z,
                                    n2 = r20 * no.x + r21 * no.y + r22 * no.z;
                        associated = associated && n0 * m.x + n1 * m.y + n2 * m.z >= a.normal_cos_min;
                    }
                    bool geometric = associated;
                    if constexpr (RGBD) geometric = geometric && a.geo_weight > 0.f;
                    if (geometric) {
                        const float r = m.x * e0 + m.y * e1 + m.z * e2;
                        const float J[6] = {q1 * m.z - q2 * m.y, q2 * m.x - q0 * m.z, q0 * m.y - q1 * m.x, m.x, m.y, m.z};
                        const float ar = fabsf(r);
                        const float w = ar <= a.huber_delta ? 1.f : a.huber_delta / ar;
                        if constexpr (RGBD) add_pair(acc, J, r, a.geo_weight * w);
                        else add_pair(acc, J, r, w);
                        acc[27] += (double)((w * r) * r);
                        acc[28] += 1.0;
                    }
                    if constexpr (RGBD) {
                        // the nearest model pixel's intensity with its first-order sub-pixel correction against the candidate's own
                        const float rp = ((im.x + im.y * (u - uf)) + im.z * (v - vf)) - io;
                        const float ap = fabsf(rp);
                        photometric = near && im.w == 1.f && ap <= a.photo_max && fabsf(io) < INFINITY;  // (false on a NaN)
                        if (photometric && a.photo_weight > 0.f) {
                            const float g0 = im.y * a.fx / q2, g1 = im.z * a.fy / q2, g2 = -((g0 * q0 + g1 * q1) / q2);
                            const float J[6] = {q1 * g2 - q2 * g1, q2 * g0 - q0 * g2, q0 * g1 - q1 * g0, g0, g1, g2};
                            const float w = ap <= a.photo_huber ? 1.f : a.photo_huber / ap;
                            add_pair(acc, J, rp, a.photo_weight * w);
                            acc[29] += (double)((w * rp) * rp);
                            acc[30] += 1.0;
                        }
                    }
                }
            }
        }
        if (a.flags)
            a.flags[c] = (unsigned char)((valid ? ICP_VALID : 0u) | (inside ? ICP_INSIDE : 0u) | (associated ? ICP_ASSOCIATED : 0u) |
                                         (RGBD && photometric ? ICP_PHOTOMETRIC : 0u));
    }
    gn_reduce(acc, ticket, part, [&](const double* totals) { icp_finish<RGBD>(a, totals); });
}

}  // namespace

hipError_t launch_depth_normals(const DepthNormalsArgs& a, hipStream_t stream) {
    const size_t n = (size_t)a.W * (size_t)a.H;
    launch(depth_normals_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), stream, a);
    return hipGetLastError();
}

hipError_t launch_intensity_map(const IntensityMapArgs& a, hipStream_t stream) {
    const size_t n = (size_t)a.W * (size_t)a.H;
    launch(intensity_map_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), stream, a);
    return hipGetLastError();
}

hipError_t launch_frame_halve(const FrameHalveArgs& a, hipStream_t stream) {
    const size_t n = (size_t)(a.W / 2) * (size_t)(a.H / 2);
    launch(frame_halve_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), stream, a);
    return hipGetLastError();
}

size_t icp_scratch_bytes(int W, int H, int stride) { return gn_scratch_bytes(seed_candidates(W, H, stride)); }

namespace {
template <class Args>
hipError_t launch_step(const Args& args, void* scratch, hipStream_t stream) {
    Args a = args;
    const CandidateGrid g = candidate_grid(a.W, a.H, a.stride);
    a.candidates = g.candidates();
    a.wc = g.wc;
    launch(icp_step_kernel<Args>, dim3(gn_blocks(a.candidates)), dim3(THREADS), stream, a, gn_ticket(scratch), gn_rows(scratch));
    return hipGetLastError();
}
}  // namespace

hipError_t launch_icp_step(const IcpStepArgs& args, void* scratch, hipStream_t stream) { return launch_step(args, scratch, stream); }
hipError_t launch_rgbd_step(const RgbdStepArgs& args, void* scratch, hipStream_t stream) { return launch_step(args, scratch, stream); }

}  // namespace dgr
