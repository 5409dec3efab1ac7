// gicp.hip -- generalized ICP over the kNN index (include/dgr_hip.h: dgr_point_covariances, dgr_gicp_step): the alignment of two
// point clouds that need not overlap pixel for pixel -- loop edges for the pose graph, GS-ICP SLAM's scan-to-map tracker.
//
// covariances: one thread per point: the mean and covariance of its neighbourhood (the leading in-range entries of its kNN row),
//          in double from the first operation; eigenpairs by cyclic Jacobi in a fixed order; the packed 32-byte row (c00, c01,
//          c02, c11, c12, c22, sigma, n) the step gathers with two 16-byte loads, the oriented normal, and the anisotropic
//          Gaussian (log-scales, quaternion) the neighbourhood spans.
// step   : one Gauss-Newton iteration in THREE stages with no host read between them: the source moved by the current estimate
//          (fp32, every operation rounded once: a numpy twin gives the same bits), the cross-mode kNN search with k = 1 (the
//          association IS the kNN rule's answer), and the step kernel: icp.hip's shape -- a workgroup per block of 2048 sources,
//          a thread's sources ascending, 29 double accumulators.  Everything behind the sums is gn_step.h's, shared with
//          icp.hip: the row / ticket / block-order reduction, the damped LDL^T solve, the pose and stats writer.  This file's
//          own is the update between the last two: T_out = exp(xi) T_in.
// No host read, no float atomics, no spin-wait, the same bits on every run.  Compiled with contraction off: the transform's fp32
// rule and the double rules of the header mean one thing.  se3.h above the pragma is contracted here as everywhere; gn_step.h
// below it sets no mode of its own and is not.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "se3.h"

#pragma clang fp contract(off)

#include "gn_step.h"

namespace dgr {
namespace {

constexpr int THREADS = GN_THREADS;
constexpr int BLOCK_SOURCES = GN_BLOCK_ITEMS;
constexpr int SUMS = 29;              // A (21), b (6), sum w s^2, count
constexpr int JACOBI_SWEEPS = 16;     // (dgr_hip.h: the fixed number of sweeps)
constexpr unsigned GICP_VALID = 1u, GICP_ASSOCIATED = 2u, GICP_SINGULAR = 4u;

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;  // (false on a NaN)
}

// ------------------------------------------------------------------------------------------------------------ covariances
// One Jacobi rotation of the symmetric A (upper triangle used) in the plane (P, Q), R the third index; V's columns follow.
template <int P, int Q, int R>
__device__ __forceinline__ void jacobi_rotate(double (&A)[3][3], double (&V)[3][3]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    const double arp = A[R][P], arq = A[R][Q];
    A[R][P] = A[P][R] = c * arp - s * arq;
    A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double vip = V[i][P], viq = V[i][Q];
        V[i][P] = c * vip - s * viq;
        V[i][Q] = s * vip + c * viq;
    }
}
// eigenpair a after eigenpair b in ascending order: swapped (values and V's columns) only when strictly greater -- ties keep order
template <int A_, int B_>
__device__ __forceinline__ void order_pair(double (&l)[3], double (&V)[3][3]) {
    if (l[A_] > l[B_]) {
        const double t = l[A_];
        l[A_] = l[B_], l[B_] = t;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double v = V[i][A_];
            V[i][A_] = V[i][B_], V[i][B_] = v;
        }
    }
}

__global__ void __launch_bounds__(THREADS) point_covariances_kernel(PointCovArgs a) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (size_t)a.P) return;
    const int* __restrict__ row = a.idx + i * (size_t)a.k;
    const float own0 = a.points[3 * i], own1 = a.points[3 * i + 1], own2 = a.points[3 * i + 2];
    bool valid = finite3(own0, own1, own2);
    // the neighbourhood: the leading entries in [0, P); the first one outside ends the list
    int n = 0;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    for (; n < a.k; n++) {
        const int j = row[n];
        if ((unsigned)j >= (unsigned)a.P) break;
        const float x = a.points[3 * (size_t)j], y = a.points[3 * (size_t)j + 1], z = a.points[3 * (size_t)j + 2];
        valid = valid && finite3(x, y, z);
        m0 += (double)x, m1 += (double)y, m2 += (double)z;
    }
    valid = valid && n >= a.min_neighbours;
    double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    double l[3] = {0.0, 0.0, 0.0}, C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (valid) {
        const double dn = (double)n;
        m0 /= dn, m1 /= dn, m2 /= dn;
        for (int s = 0; s < n; s++) {  // (the entries are in range: the first pass stopped at the first that is not)
            const size_t j = (size_t)row[s];
            const double d0 = (double)a.points[3 * j] - m0, d1 = (double)a.points[3 * j + 1] - m1, d2 = (double)a.points[3 * j + 2] - m2;
            C[0] += d0 * d0, C[1] += d0 * d1, C[2] += d0 * d2, C[3] += d1 * d1, C[4] += d1 * d2, C[5] += d2 * d2;
        }
#pragma unroll
        for (int c = 0; c < 6; c++) C[c] /= dn;
        A[0][0] = C[0], A[0][1] = A[1][0] = C[1], A[0][2] = A[2][0] = C[2], A[1][1] = C[3], A[1][2] = A[2][1] = C[4], A[2][2] = C[5];
        for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
            if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
            jacobi_rotate<0, 1, 2>(A, V);
            jacobi_rotate<0, 2, 1>(A, V);
            jacobi_rotate<1, 2, 0>(A, V);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) l[c] = A[c][c] > 0.0 ? A[c][c] : 0.0;  // clamped at 0 (a NaN becomes 0)
        order_pair<0, 1>(l, V);
        order_pair<1, 2>(l, V);
        order_pair<0, 1>(l, V);
        valid = l[2] > 0.0 && l[2] < (double)INFINITY;
    }
    float cov[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float4 normal = make_float4(0.f, 0.f, 0.f, 0.f), quat = make_float4(0.f, 0.f, 0.f, 0.f);
    float ls[3] = {0.f, 0.f, 0.f};
    if (valid) {
        const double sigma = l[0] / ((l[0] + l[1]) + l[2]);
        // v_0 toward the viewpoint, or its largest-magnitude component (the first such) positive
        double v0[3] = {V[0][0], V[1][0], V[2][0]};
        bool flip;
        if (a.has_viewpoint) {
            flip = (v0[0] * ((double)a.viewpoint[0] - (double)own0) + v0[1] * ((double)a.viewpoint[1] - (double)own1)) +
                       v0[2] * ((double)a.viewpoint[2] - (double)own2) < 0.0;
        } else {
            const double a0 = fabs(v0[0]), a1 = fabs(v0[1]), a2 = fabs(v0[2]);
            flip = a0 >= a1 && a0 >= a2 ? v0[0] < 0.0 : a1 >= a2 ? v0[1] < 0.0 : v0[2] < 0.0;
        }
        if (flip) v0[0] = -v0[0], v0[1] = -v0[1], v0[2] = -v0[2];
        if (a.mode == DGR_COV_PLANE) {
            const double g = 1.0 - (double)a.epsilon;
            cov[0] = (float)(1.0 - g * v0[0] * v0[0]), cov[1] = (float)(-(g * v0[0] * v0[1])), cov[2] = (float)(-(g * v0[0] * v0[2]));
            cov[3] = (float)(1.0 - g * v0[1] * v0[1]), cov[4] = (float)(-(g * v0[1] * v0[2])), cov[5] = (float)(1.0 - g * v0[2] * v0[2]);
        } else {
#pragma unroll
            for (int c = 0; c < 6; c++) cov[c] = (float)C[c];
        }
        cov[6] = (float)sigma, cov[7] = (float)n;
        normal = make_float4((float)v0[0], (float)v0[1], (float)v0[2], (float)sigma);
        // the Gaussian: scales largest first, the frame (v_2, +-v_1, the oriented v_0) with det +1
        const double floor2 = (double)a.scale_floor * (double)a.scale_floor;
#pragma unroll
        for (int c = 0; c < 3; c++) ls[c] = (float)(0.5 * log(fmax(l[2 - c], floor2)));
        double R[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++) R[r][0] = V[r][2], R[r][1] = V[r][1], R[r][2] = v0[r];
        const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                           R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
        if (det < 0.0) R[0][1] = -R[0][1], R[1][1] = -R[1][1], R[2][1] = -R[2][1];
        double q[4];
        rotation_to_quat(R, q);
        quat = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
    }
    if (a.cov) {
        a.cov[2 * i] = make_float4(cov[0], cov[1], cov[2], cov[3]);
        a.cov[2 * i + 1] = make_float4(cov[4], cov[5], cov[6], cov[7]);
    }
    if (a.normals) {
        float* o = a.normals + 4 * i;
        o[0] = normal.x, o[1] = normal.y, o[2] = normal.z, o[3] = normal.w;
    }
    if (a.log_scales) {
        float* o = a.log_scales + 3 * i;
        o[0] = ls[0], o[1] = ls[1], o[2] = ls[2];
    }
    if (a.quats) {
        float* o = a.quats + 4 * i;
        o[0] = quat.x, o[1] = quat.y, o[2] = quat.z, o[3] = quat.w;
    }
    if (a.flags) a.flags[i] = valid ? 1 : 0;
}

// -------------------------------------------------------------------------------------------------------------- transform
// q_i = R a_i + t in fp32, every operation rounded once: q_j = ((R_j0 a_0 + R_j1 a_1) + R_j2 a_2) + t_j.  T holds the transform
// transposed: R[j][c] at [4 c + j], t[j] at [12 + j].
__global__ void __launch_bounds__(THREADS) gicp_transform_kernel(int S, const float* __restrict__ source, const float* __restrict__ T,
                                                                float* __restrict__ q) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (size_t)S) return;
    const float a0 = source[3 * i], a1 = source[3 * i + 1], a2 = source[3 * i + 2];
#pragma unroll
    for (int j = 0; j < 3; j++) q[3 * i + j] = ((T[j] * a0 + T[4 + j] * a1) + T[8 + j] * a2) + T[12 + j];
}

// -------------------------------------------------------------------------------------------------------------------- step
// One thread: the totals through gn_step.h's solve, the left update T_out = exp(xi) T_in, its writer.
__device__ void gicp_finish(const GicpStepArgs& a, const double* tot) {
    double xi[6];
    const bool ok = gn_solve(tot, tot[28], true, a.min_points, a.damping, a.rcond, xi);
    GnPoseIn in;
    gn_read_pose(a.transform_in, in);
    double Ro[3][3], to[3];
    if (ok) {
        double Re[3][3], te[3];
        const double w[3] = {xi[0], xi[1], xi[2]}, v[3] = {xi[3], xi[4], xi[5]};
        se3_exp(w, v, Re, te);
        compose(Re, te, in.R, in.t, Ro, to);
    }
    gn_write<SUMS, SUMS + 3>(ok, Ro, to, in, xi, tot, a.transform_out, a.quat_out, a.trans_out, a.stats);
}

// the six entries (00, 01, 02, 11, 12, 22) and the validity of a packed covariance row: two 16-byte loads from one line
__device__ __forceinline__ bool load_cov(const float4* __restrict__ rows, size_t i, double (&c)[6]) {
    const float4 lo = rows[2 * i], hi = rows[2 * i + 1];
    c[0] = (double)lo.x, c[1] = (double)lo.y, c[2] = (double)lo.z, c[3] = (double)lo.w, c[4] = (double)hi.x, c[5] = (double)hi.y;
    return hi.w > 0.f;  // n, the neighbour count: 0 = invalid (false on a NaN)
}

// grid: one workgroup per block of sources.  `ticket`, `part`: gn_reduce's.
__global__ void __launch_bounds__(THREADS) gicp_step_kernel(GicpStepArgs a, uint32_t* __restrict__ ticket, double* __restrict__ part) {
    // R of the current estimate, widened: R[j][c] at [4 c + j]
    const float* T = a.transform_in;  // (not __restrict__: transform_out may be the same address)
    const double R00 = (double)T[0], R01 = (double)T[4], R02 = (double)T[8], R10 = (double)T[1], R11 = (double)T[5], R12 = (double)T[9],
                 R20 = (double)T[2], R21 = (double)T[6], R22 = (double)T[10];
    const size_t begin = (size_t)blockIdx.x * BLOCK_SOURCES;
    const size_t end = begin + BLOCK_SOURCES < (size_t)a.S ? begin + BLOCK_SOURCES : (size_t)a.S;
    double acc[SUMS];
#pragma unroll
    for (int i = 0; i < SUMS; i++) acc[i] = 0.0;
    for (size_t i = begin + threadIdx.x; i < end; i += THREADS) {  // this thread's sources, ascending
        const float qf0 = a.q[3 * i], qf1 = a.q[3 * i + 1], qf2 = a.q[3 * i + 2];
        const int j = a.idx[i];
        bool valid = finite3(qf0, qf1, qf2);
        double ca[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (a.source_cov) valid = load_cov(a.source_cov, i, ca) && valid;
        bool associated = valid && (unsigned)j < (unsigned)a.N;
        double cb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (associated && a.target_cov) associated = load_cov(a.target_cov, (size_t)j, cb);
        bool singular = false;
        if (associated) {
            const double q0 = (double)qf0, q1 = (double)qf1, q2 = (double)qf2;
            const double e0 = q0 - (double)a.target[3 * (size_t)j], e1 = q1 - (double)a.target[3 * (size_t)j + 1],
                         e2 = q2 - (double)a.target[3 * (size_t)j + 2];
            // C = C_B + R C_A R^T (a NULL side contributes nothing; both NULL: I)
            double c00 = cb[0], c01 = cb[1], c02 = cb[2], c11 = cb[3], c12 = cb[4], c22 = cb[5];
            if (a.source_cov) {
                // P = R C_A (rows of R against the symmetric C_A), then P R^T
                const double p00 = R00 * ca[0] + R01 * ca[1] + R02 * ca[2], p01 = R00 * ca[1] + R01 * ca[3] + R02 * ca[4],
                             p02 = R00 * ca[2] + R01 * ca[4] + R02 * ca[5];
                const double p10 = R10 * ca[0] + R11 * ca[1] + R12 * ca[2], p11 = R10 * ca[1] + R11 * ca[3] + R12 * ca[4],
                             p12 = R10 * ca[2] + R11 * ca[4] + R12 * ca[5];
                const double p20 = R20 * ca[0] + R21 * ca[1] + R22 * ca[2], p21 = R20 * ca[1] + R21 * ca[3] + R22 * ca[4],
                             p22 = R20 * ca[2] + R21 * ca[4] + R22 * ca[5];
                c00 += p00 * R00 + p01 * R01 + p02 * R02, c01 += p00 * R10 + p01 * R11 + p02 * R12;
                c02 += p00 * R20 + p01 * R21 + p02 * R22, c11 += p10 * R10 + p11 * R11 + p12 * R12;
                c12 += p10 * R20 + p11 * R21 + p12 * R22, c22 += p20 * R20 + p21 * R21 + p22 * R22;
            } else if (!a.target_cov) {
                c00 = c11 = c22 = 1.0;
            }
            // M = C^-1: adjugate over determinant
            const double a00 = c11 * c22 - c12 * c12, a01 = c02 * c12 - c01 * c22, a02 = c01 * c12 - c02 * c11;
            const double a11 = c00 * c22 - c02 * c02, a12 = c01 * c02 - c00 * c12, a22 = c00 * c11 - c01 * c01;
            const double det = (c00 * a00 + c01 * a01) + c02 * a02;
            singular = !(det > 0.0 && det < (double)INFINITY);  // (true on a NaN)
            if (!singular) {
                const double m00 = a00 / det, m01 = a01 / det, m02 = a02 / det, m11 = a11 / det, m12 = a12 / det, m22 = a22 / det;
                const double g0 = m00 * e0 + m01 * e1 + m02 * e2, g1 = m01 * e0 + m11 * e1 + m12 * e2, g2 = m02 * e0 + m12 * e1 + m22 * e2;  // M e
                const double s2r = e0 * g0 + e1 * g1 + e2 * g2;
                const double s2 = s2r > 0.0 ? s2r : 0.0;  // clamped: rounding in adj / det may leave a badly conditioned C's form just below 0
                const double s = sqrt(s2);
                const double w = s <= (double)a.huber_delta ? 1.0 : (double)a.huber_delta / s;
                // G = [q]x M: column c of G is q x (column c of M); row r of G is G[r][.]
                const double G00 = q1 * m02 - q2 * m01, G01 = q1 * m12 - q2 * m11, G02 = q1 * m22 - q2 * m12;
                const double G10 = q2 * m00 - q0 * m02, G11 = q2 * m01 - q0 * m12, G12 = q2 * m02 - q0 * m22;
                const double G20 = q0 * m01 - q1 * m00, G21 = q0 * m11 - q1 * m01, G22 = q0 * m12 - q1 * m02;
                // J^T M J = [[G [q]x^T, G], [G^T, M]], J = [-[q]x | I]; (G [q]x^T)[r][c] = (q x G[r][.])[c]
                acc[0] += w * (q1 * G02 - q2 * G01), acc[1] += w * (q2 * G00 - q0 * G02), acc[2] += w * (q0 * G01 - q1 * G00);
                acc[3] += w * G00, acc[4] += w * G01, acc[5] += w * G02;
                acc[6] += w * (q2 * G10 - q0 * G12), acc[7] += w * (q0 * G11 - q1 * G10);
                acc[8] += w * G10, acc[9] += w * G11, acc[10] += w * G12;
                acc[11] += w * (q0 * G21 - q1 * G20);
                acc[12] += w * G20, acc[13] += w * G21, acc[14] += w * G22;
                acc[15] += w * m00, acc[16] += w * m01, acc[17] += w * m02, acc[18] += w * m11, acc[19] += w * m12, acc[20] += w * m22;
                // J^T M e = (q x (M e), M e)
                acc[21] += w * (q1 * g2 - q2 * g1), acc[22] += w * (q2 * g0 - q0 * g2), acc[23] += w * (q0 * g1 - q1 * g0);
                acc[24] += w * g0, acc[25] += w * g1, acc[26] += w * g2;
                acc[27] += w * s2;
                acc[28] += 1.0;
            }
        }
        if (a.flags)
            a.flags[i] = (unsigned char)((valid ? GICP_VALID : 0u) | (associated ? GICP_ASSOCIATED : 0u) | (singular ? GICP_SINGULAR : 0u));
    }
    gn_reduce(acc, ticket, part, [&](const double* totals) { gicp_finish(a, totals); });
}

// the scratch: the header (ticket), a row per block, q [S,3], idx [S], then the search's own scratch; every part 256-byte aligned
struct GicpScratch {
    size_t q, idx, knn, total;
};
GicpScratch gicp_layout(int N, int S) {
    GicpScratch l{};
    const size_t knn = knn_scratch_bytes(N, S);
    if (!knn) return l;
    l.q = gn_scratch_bytes((size_t)S);
    l.idx = l.q + align256(12 * (size_t)S);
    l.knn = l.idx + align256(4 * (size_t)S);
    l.total = l.knn + align256(knn);
    return l;
}

}  // namespace

hipError_t launch_point_covariances(const PointCovArgs& a, hipStream_t stream) {
    launch(point_covariances_kernel, dim3((unsigned)(((size_t)a.P + THREADS - 1) / THREADS)), dim3(THREADS), stream, a);
    return hipGetLastError();
}

size_t gicp_scratch_bytes(int n_target, int n_source) { return gicp_layout(n_target, n_source).total; }

hipError_t launch_gicp_step(const GicpStepArgs& args, const void* index, float dist_max, int* idx_out, void* scratch,
                            hipStream_t stream) {
    GicpStepArgs a = args;
    const GicpScratch l = gicp_layout(a.N, a.S);
    char* base = static_cast<char*>(scratch);
    float* q = reinterpret_cast<float*>(base + l.q);
    int* idx = idx_out ? idx_out : reinterpret_cast<int*>(base + l.idx);
    launch(gicp_transform_kernel, dim3((unsigned)(((size_t)a.S + THREADS - 1) / THREADS)), dim3(THREADS), stream, a.S, a.source,
           a.transform_in, q);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    KnnSearchCall c{};
    c.index = index, c.n_points = a.N, c.n_queries = a.S, c.queries = q, c.k = 1, c.exclude_self = 0;
    c.max_dist2 = dist_max * dist_max;  // (fp32, rounded once: the file is compiled with contraction off)
    c.scratch = base + l.knn, c.idx = idx;
    if (hipError_t e = launch_knn_search(c, stream); e != hipSuccess) return e;
    a.q = q, a.idx = idx;
    launch(gicp_step_kernel, dim3(gn_blocks((size_t)a.S)), dim3(THREADS), stream, a, gn_ticket(scratch), gn_rows(scratch));
    return hipGetLastError();
}

}  // namespace dgr
