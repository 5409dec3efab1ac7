// pgo.hip -- pose-graph optimisation on the device (include/dgr_hip.h: dgr_pgo_plan, dgr_pgo_solve): the solver in front of the
// map correction.  K keyframe poses T_k (W2C) and E relative-pose constraints Z_e ~ T_i T_j^-1; minimised is
// sum_e rho(sqrt(r_e^T Omega_e r_e)), r_e = Log(Z_e^-1 T_i T_j^-1) in R^6 ordered (w, v), rho Huber's, over the free poses with
// the update T_k <- Exp(d_k) T_k.
//
// plan : ONE workgroup: every node's incidence list (entry 2 e + side, side 0 = the edge's i) in ascending entry order.  Degrees by
//        integer atomics (a count has one value), offsets by a scan, then the entries in chunks of 256 in entry order: an entry's
//        slot is its node's cursor plus the number of earlier entries of the chunk with the same node -- no atomics, so the order
//        does not depend on scheduling.
// solve: ONE launch of ONE workgroup of 256 threads runs the whole Levenberg-Marquardt loop.  A graph of a few hundred nodes is
//        bound by synchronisation, not by throughput: every step below is a pass over the edges or the nodes (thread t takes
//        t, t + 256, ..) between workgroup barriers, the state lives in the scratch (L2-resident at these sizes; per-node arrays
//        component-major, so a wave reads neighbouring addresses), and no loop waits on another workgroup.  Every loop's bound
//        is an argument.  The CG's search direction -- the one vector read across nodes -- is in LDS up to 1024 nodes, and up to
//        256 nodes (one per thread) a node's block, factor and vectors stay in registers for the whole CG solve.
//        linearise (per edge): r, J_j = -J_r^-1(r), J_i = J_r^-1(r) Ad(T_j T_i^-1) in closed form, w = min(1, delta / s), the blocks
//                   H_ii, H_ij, H_jj and g_i, g_j of J^T (w Omega) J and J^T (w Omega) r, rho.
//        gather (per node): the diagonal block and g in list order; the damped block's LDL^T; loose nodes.
//        CG: x0 = 0, block-Jacobi preconditioner; H p as a per-node gather over the list (the damped diagonal block first, then the
//                   off-diagonal blocks in list order); no atomics.
//        accept or reject on the candidate's cost.
// Every sum over edges or nodes: a thread's items ascending (a node's six components 0 .. 5), then block_sum.h's block_sums.
// All arithmetic in double.  No host read, no float atomics, the same bits on every run.
#include <hip/hip_runtime.h>

#include "block_sum.h"
#include "kernels.h"
#include "se3.h"

namespace dgr {
namespace {

constexpr int THREADS = 256;
constexpr int PGO_MAGIC = 0x50474f31;
constexpr size_t HEADER_BYTES = 256;  // ints: magic, K, E, the edges the plan skipped
constexpr int EDGE_BLOCKS = 108;      // H_ii, H_ij, H_jj, row-major
constexpr int NODE_FIXED = 1, NODE_LOOSE = 2;
constexpr int LDS_NODES = 1024;       // graphs up to this many nodes keep the CG's search direction in LDS (48 KiB)
constexpr double LAMBDA_MIN = 1e-12, LAMBDA_MAX = 1e12;
constexpr int FLAG_REFUSED = 1, FLAG_SKIPPED = 2, FLAG_LOOSE = 4, FLAG_LAMBDA_MAX = 8, FLAG_CG_CAP = 16, FLAG_NO_PLAN = 32;

// byte offsets into the scratch.  The plan's part (ints), then the solve's (doubles per node, then per edge)
struct Layout {
    size_t start, cursor, list, state, usable, nbr;
    size_t pose, backup, g, diag, fac, x, r, z, p, ap;
    size_t blocks, gvec, rho, s2, off, total;
};
__host__ __device__ inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
__host__ __device__ inline Layout pgo_layout(int K_, int E_) {
    const size_t K = (size_t)K_, E = (size_t)E_;
    Layout L;
    size_t o = HEADER_BYTES;
    L.start = o, o = up16(o + (K + 1) * 4);
    L.cursor = o, o = up16(o + K * 4);
    L.list = o, o = up16(o + 2 * E * 4);
    L.state = o, o = up16(o + K * 4);
    L.usable = o, o = up16(o + E * 4);
    L.nbr = o, o = up16(o + 2 * E * 4);  // per list entry: the node at the edge's other end, -1 for an edge not in use
    L.pose = o, o += K * 8 * 8;    // q (4), t (3), one spare
    L.backup = o, o += K * 8 * 8;
    // (from here on component-major, entry m of node k at [m K + k]: the lanes of a wave read neighbouring addresses)
    L.g = o, o += K * 6 * 8;
    L.diag = o, o += K * 36 * 8;
    L.fac = o, o += K * 36 * 8;    // L below the diagonal, D on it
    L.x = o, o += K * 6 * 8;
    L.r = o, o += K * 6 * 8;
    L.z = o, o += K * 6 * 8;
    L.p = o, o += K * 6 * 8;
    L.ap = o, o += K * 6 * 8;
    L.blocks = o, o += E * EDGE_BLOCKS * 8;
    L.gvec = o, o += E * 12 * 8;
    L.rho = o, o += E * 8;
    L.s2 = o, o += E * 8;
    L.off = o, o += 2 * E * 36 * 8;  // per list entry: the off-diagonal block as its node multiplies it (H_ij, or H_ij^T on side j)
    L.total = up16(o);
    return L;
}

// ------------------------------------------------------------------------------------------------------------------- plan
__global__ void __launch_bounds__(THREADS) pgo_plan_kernel(int K, int E, const int* __restrict__ edges, char* scratch) {
    const Layout L = pgo_layout(K, E);
    int* hdr = reinterpret_cast<int*>(scratch);
    int* start = reinterpret_cast<int*>(scratch + L.start);
    int* cursor = reinterpret_cast<int*>(scratch + L.cursor);
    int* list = reinterpret_cast<int*>(scratch + L.list);
    __shared__ int keys[THREADS];
    __shared__ int partial[THREADS];
    const int tid = threadIdx.x;
    for (int k = tid; k < K; k += THREADS) cursor[k] = 0;
    __syncthreads();
    int bad = 0;
    for (int e = tid; e < E; e += THREADS) {
        const int i = edges[2 * e], j = edges[2 * e + 1];
        if ((unsigned)i < (unsigned)K && (unsigned)j < (unsigned)K && i != j) {
            atomicAdd(&cursor[i], 1);
            atomicAdd(&cursor[j], 1);
        } else {
            bad++;
        }
    }
    __syncthreads();
    // offsets: thread t owns nodes [t seg, (t + 1) seg)
    const int seg = (K + THREADS - 1) / THREADS;
    const int k0 = tid * seg < K ? tid * seg : K, k1 = k0 + seg < K ? k0 + seg : K;
    int own = 0;
    for (int k = k0; k < k1; k++) own += cursor[k];
    partial[tid] = own;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < THREADS; t++) {
            const int v = partial[t];
            partial[t] = run;
            run += v;
        }
        start[K] = run;
    }
    __syncthreads();
    {
        int run = partial[tid];
        for (int k = k0; k < k1; k++) {
            const int d = cursor[k];
            start[k] = run, cursor[k] = run;
            run += d;
        }
    }
    __syncthreads();
    // the entries, 256 at a time in entry order
    const int entries = 2 * E;
    for (int base = 0; base < entries; base += THREADS) {
        const int n = base + tid;
        int key = -1;
        if (n < entries) {
            const int e = n >> 1, i = edges[2 * e], j = edges[2 * e + 1];
            if ((unsigned)i < (unsigned)K && (unsigned)j < (unsigned)K && i != j) key = (n & 1) ? j : i;
        }
        keys[tid] = key;
        __syncthreads();
        int slot = 0;
        bool later = false;
        if (key >= 0) {
            int rank = 0;
            for (int t = 0; t < tid; t++) rank += keys[t] == key;
            for (int t = tid + 1; t < THREADS; t++) later = later || keys[t] == key;
            slot = cursor[key] + rank;
            list[slot] = n;
        }
        __syncthreads();
        if (key >= 0 && !later) cursor[key] = slot + 1;
        __syncthreads();
    }
    int v[1] = {bad};
    // (an int sum: any order gives the same value)
    for (int off = 32; off > 0; off >>= 1) v[0] += __shfl_xor(v[0], off, 64);
    if ((tid & 63) == 0) partial[tid >> 6] = v[0];
    __syncthreads();
    if (tid == 0) hdr[0] = PGO_MAGIC, hdr[1] = K, hdr[2] = E, hdr[3] = partial[0] + partial[1] + partial[2] + partial[3];
}

// ------------------------------------------------------------------------------------------------------------------ maths
__device__ inline void mul3(const double (&A)[3][3], const double (&B)[3][3], double (&C)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i][j] = A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j];
}
__device__ inline void hat(const double (&w)[3], double (&K)[3][3]) {
    K[0][0] = 0.0, K[0][1] = -w[2], K[0][2] = w[1];
    K[1][0] = w[2], K[1][1] = 0.0, K[1][2] = -w[0];
    K[2][0] = -w[1], K[2][1] = w[0], K[2][2] = 0.0;
}
// c of J_l^-1(w) = I - 1/2 [w]x + c [w]x^2: (1 - (th / 2) cot(th / 2)) / th^2, finite up to th = pi; its series below th^2 = 1e-6
__device__ inline double so3_inv_c(double th2) {
    if (th2 < 1e-6) return 1.0 / 12.0 + th2 * (1.0 / 720.0 + th2 / 30240.0);
    const double h = 0.5 * sqrt(th2);
    return (1.0 - h * cos(h) / sin(h)) / th2;
}
// the pose (16 floats, W2C^T) as unit quaternion and translation; false unless rigid: finite, det > 0, R^T R within 1e-3 of I
__device__ inline bool load_rigid(const float* v, double (&q)[4], double (&t)[3]) {
    double R[3][3];
    pose_of(v, R, t);
    bool ok = isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) ok = ok && isfinite(R[i][j]);
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    ok = ok && det > 0.0;
    double worst = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            worst = fmax(worst, fabs(R[0][i] * R[0][j] + R[1][i] * R[1][j] + R[2][i] * R[2][j] - (i == j ? 1.0 : 0.0)));
    ok = ok && worst <= 1e-3;
    if (ok) rotation_to_quat(R, q);
    else q[0] = 1.0, q[1] = q[2] = q[3] = 0.0;
    return ok;
}
// Log of (R, t), R a rotation: through the sign-normalised unit quaternion (r >= 0), so the angle is 2 atan2(|v|, r) in [0, pi]
__device__ inline void se3_log(const double (&R)[3][3], const double (&t)[3], double (&r)[6]) {
    double q[4];
    rotation_to_quat(R, q);
    const double n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    double k;  // w = k (x, y, z)
    if (n2 < 2.5e-7) {  // th^2 < 1e-6: 2 atan(u) / |v|, u = |v| / r
        const double u2 = n2 / (q[0] * q[0]);
        k = 2.0 / q[0] * (1.0 - u2 * (1.0 / 3.0 - u2 / 5.0));
    } else {
        const double n = sqrt(n2);
        k = 2.0 * atan2(n, q[0]) / n;
    }
    const double w[3] = {k * q[1], k * q[2], k * q[3]};
    const double c = so3_inv_c(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    // v = J_l^-1(w) t = t - 1/2 w x t + c w x (w x t)
    const double a[3] = {w[1] * t[2] - w[2] * t[1], w[2] * t[0] - w[0] * t[2], w[0] * t[1] - w[1] * t[0]};
    const double b[3] = {w[1] * a[2] - w[2] * a[1], w[2] * a[0] - w[0] * a[2], w[0] * a[1] - w[1] * a[0]};
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = w[i], r[3 + i] = t[i] - 0.5 * a[i] + c * b[i];
}
// J_r^-1(r) = J_l^-1(-r) of SE(3), ordered (w, v): [[A, 0], [B, A]], A = J_l^-1 of SO(3) at -w, B = -A Q A (Barfoot's Q at -r)
__device__ inline void se3_jr_inv(const double (&r)[6], double (&A)[3][3], double (&B)[3][3]) {
    const double phi[3] = {-r[0], -r[1], -r[2]}, rho[3] = {-r[3], -r[4], -r[5]};
    const double th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    double F[3][3], P[3][3], FF[3][3];
    hat(phi, F), hat(rho, P);
    mul3(F, F, FF);
    const double c = so3_inv_c(th2);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) A[i][j] = (i == j ? 1.0 : 0.0) - 0.5 * F[i][j] + c * FF[i][j];
    double a1, a2, a3;
    if (th2 < 1e-2) {  // the closed forms cancel: (th - sin th) / th^3, (th^2 + 2 cos th - 2) / (2 th^4), (2 th - 3 sin th + th cos th) / (2 th^5)
        a1 = 1.0 / 6.0 - th2 * (1.0 / 120.0 - th2 * (1.0 / 5040.0 - th2 / 362880.0));
        a2 = 1.0 / 24.0 - th2 * (1.0 / 720.0 - th2 * (1.0 / 40320.0 - th2 / 3628800.0));
        a3 = 1.0 / 120.0 - th2 * (1.0 / 2520.0 - th2 * (1.0 / 120960.0 - th2 / 9979200.0));
    } else {
        const double th = sqrt(th2), s = sin(th), co = cos(th), th4 = th2 * th2;
        a1 = (th - s) / (th2 * th);
        a2 = (th2 + 2.0 * co - 2.0) / (2.0 * th4);
        a3 = (2.0 * th - 3.0 * s + th * co) / (2.0 * th4 * th);
    }
    double FP[3][3], PF[3][3], FPF[3][3], FFP[3][3], PFF[3][3], FPFF[3][3], FFPF[3][3], Q[3][3];
    mul3(F, P, FP), mul3(P, F, PF), mul3(FP, F, FPF), mul3(FF, P, FFP), mul3(PF, F, PFF), mul3(FPF, F, FPFF), mul3(FF, PF, FFPF);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            Q[i][j] = 0.5 * P[i][j] + a1 * (FP[i][j] + PF[i][j] + FPF[i][j]) + a2 * (FFP[i][j] + PFF[i][j] - 3.0 * FPF[i][j]) +
                      a3 * (FPFF[i][j] + FFPF[i][j]);
    double QA[3][3], AQA[3][3];
    mul3(Q, A, QA), mul3(A, QA, AQA);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) B[i][j] = -AQA[i][j];
}

// ------------------------------------------------------------------------------------------------------------------ solve
struct Solve {
    PgoArgs a;
    Layout L;
    char* s;
    __device__ int* ints(size_t off) const { return reinterpret_cast<int*>(s + off); }
    __device__ double* dbl(size_t off) const { return reinterpret_cast<double*>(s + off); }
};

__shared__ double bcast[4];

// the workgroup's sum of v in every thread: block_sums, then thread 0's total through LDS
__device__ inline double block_total(double v) {
    double a[1] = {v};
    block_sums(a);
    if (threadIdx.x == 0) bcast[0] = a[0];
    __syncthreads();
    const double t = bcast[0];
    __syncthreads();
    return t;
}
__device__ inline double block_max(double v) {
    __shared__ double red[4];
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return t;
}

// One edge at the current poses: usable or not, s^2 and rho; FULL: its blocks and gradient parts too.  Returns rho (0 when skipped).
template <bool FULL>
__device__ double edge_pass(const Solve& S, int e) {
    const PgoArgs& a = S.a;
    int* usable = S.ints(S.L.usable);
    double* rho_out = S.dbl(S.L.rho);
    double* s2_out = S.dbl(S.L.s2);
    const int i = a.edges[2 * e], j = a.edges[2 * e + 1];
    bool ok = (unsigned)i < (unsigned)a.K && (unsigned)j < (unsigned)a.K && i != j;
    double qz[4], tz[3];
    ok = load_rigid(a.measurements + (size_t)e * 16, qz, tz) && ok;
    double W[6][6];
#pragma unroll
    for (int m = 0; m < 6; m++)
#pragma unroll
        for (int n = 0; n < 6; n++) W[m][n] = m == n ? 1.0 : 0.0;
    if (a.information_kind == 2) {
        const double wr = (double)a.information[2 * (size_t)e], wt = (double)a.information[2 * (size_t)e + 1];
        ok = ok && isfinite(wr) && isfinite(wt);
#pragma unroll
        for (int m = 0; m < 3; m++) W[m][m] = wr, W[3 + m][3 + m] = wt;
    } else if (a.information_kind == 36) {
        const float* om = a.information + (size_t)e * 36;
#pragma unroll
        for (int m = 0; m < 6; m++)
#pragma unroll
            for (int n = 0; n < 6; n++) {
                ok = ok && isfinite(om[6 * m + n]);
                W[m][n] = 0.5 * ((double)om[6 * m + n] + (double)om[6 * n + m]);
            }
    }
    if (!ok) {
        usable[e] = 0, rho_out[e] = 0.0, s2_out[e] = __longlong_as_double(0x7ff8000000000000LL);
        return 0.0;
    }
    const double* pi = S.dbl(S.L.pose) + (size_t)i * 8;
    const double* pj = S.dbl(S.L.pose) + (size_t)j * 8;
    const double qi[4] = {pi[0], pi[1], pi[2], pi[3]}, qj[4] = {pj[0], pj[1], pj[2], pj[3]};
    const double ti[3] = {pi[4], pi[5], pi[6]}, tj[3] = {pj[4], pj[5], pj[6]};
    double Ri[3][3], Rj[3][3], Rz[3][3];
    quat_to_rotation(qi, Ri), quat_to_rotation(qj, Rj), quat_to_rotation(qz, Rz);
    // E = Z^-1 T_i T_j^-1 = (Rz^T Rij, Rz^T (ti - Rij tj - tz)), Rij = Ri Rj^T
    double Rij[3][3], Re[3][3], d[3], te[3];
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int n = 0; n < 3; n++) Rij[m][n] = Ri[m][0] * Rj[n][0] + Ri[m][1] * Rj[n][1] + Ri[m][2] * Rj[n][2];
#pragma unroll
    for (int m = 0; m < 3; m++) d[m] = ti[m] - (Rij[m][0] * tj[0] + Rij[m][1] * tj[1] + Rij[m][2] * tj[2]) - tz[m];
#pragma unroll
    for (int m = 0; m < 3; m++) {
#pragma unroll
        for (int n = 0; n < 3; n++) Re[m][n] = Rz[0][m] * Rij[0][n] + Rz[1][m] * Rij[1][n] + Rz[2][m] * Rij[2][n];
        te[m] = Rz[0][m] * d[0] + Rz[1][m] * d[1] + Rz[2][m] * d[2];
    }
    double r[6];
    se3_log(Re, te, r);
    double Wr[6], s2 = 0.0;
#pragma unroll
    for (int m = 0; m < 6; m++) {
        double v = 0.0;
#pragma unroll
        for (int n = 0; n < 6; n++) v += W[m][n] * r[n];
        Wr[m] = v;
    }
#pragma unroll
    for (int m = 0; m < 6; m++) s2 += r[m] * Wr[m];
    const double sd = sqrt(fmax(s2, 0.0));
    const bool inlier = sd <= a.huber_delta;
    const double wgt = inlier ? 1.0 : a.huber_delta / sd;
    const double rho = inlier ? s2 : 2.0 * a.huber_delta * sd - a.huber_delta * a.huber_delta;
    usable[e] = 1, rho_out[e] = rho, s2_out[e] = s2;
    if constexpr (FULL) {
        double A[3][3], B[3][3];
        se3_jr_inv(r, A, B);
        // Ad(T_j T_i^-1): Rji = Rij^T, tji = tj - Rji ti
        double Rji[3][3], tji[3], Sx[3][3], Sm[3][3];
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int n = 0; n < 3; n++) Rji[m][n] = Rij[n][m];
#pragma unroll
        for (int m = 0; m < 3; m++) tji[m] = tj[m] - (Rji[m][0] * ti[0] + Rji[m][1] * ti[1] + Rji[m][2] * ti[2]);
        hat(tji, Sx);
        mul3(Sx, Rji, Sm);
        double P[3][3], BR[3][3], AS[3][3];
        mul3(A, Rji, P), mul3(B, Rji, BR), mul3(A, Sm, AS);
        double Ji[6][6], Jj[6][6];
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int n = 0; n < 3; n++) {
                Ji[m][n] = P[m][n], Ji[m][3 + n] = 0.0, Ji[3 + m][n] = BR[m][n] + AS[m][n], Ji[3 + m][3 + n] = P[m][n];
                Jj[m][n] = -A[m][n], Jj[m][3 + n] = 0.0, Jj[3 + m][n] = -B[m][n], Jj[3 + m][3 + n] = -A[m][n];
            }
        double WJi[6][6], WJj[6][6];
#pragma unroll
        for (int m = 0; m < 6; m++)
#pragma unroll
            for (int n = 0; n < 6; n++) {
                double vi = 0.0, vj = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) vi += W[m][k] * Ji[k][n], vj += W[m][k] * Jj[k][n];
                WJi[m][n] = wgt * vi, WJj[m][n] = wgt * vj;
            }
        double* blk = S.dbl(S.L.blocks) + (size_t)e * EDGE_BLOCKS;
        double* gv = S.dbl(S.L.gvec) + (size_t)e * 12;
#pragma unroll
        for (int m = 0; m < 6; m++) {
#pragma unroll
            for (int n = 0; n < 6; n++) {
                double hii = 0.0, hij = 0.0, hjj = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) hii += Ji[k][m] * WJi[k][n], hij += Ji[k][m] * WJj[k][n], hjj += Jj[k][m] * WJj[k][n];
                blk[6 * m + n] = hii, blk[36 + 6 * m + n] = hij, blk[72 + 6 * m + n] = hjj;
            }
            double gi = 0.0, gj = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) gi += Ji[k][m] * (wgt * Wr[k]), gj += Jj[k][m] * (wgt * Wr[k]);
            gv[m] = gi, gv[6 + m] = gj;
        }
    }
    return rho;
}

// the cost at the current poses: every edge's pass, the thread's edges ascending, then the block sum
template <bool FULL>
__device__ double edges_cost(const Solve& S) {
    double acc = 0.0;
    for (int e = threadIdx.x; e < S.a.E; e += THREADS) acc += edge_pass<FULL>(S, e);
    __syncthreads();  // the edges' records are written before any thread gathers them
    return block_total(acc);
}

// per node in list order: the diagonal block and g; returns the largest |g| over the active nodes
__device__ double gather_nodes(const Solve& S) {
    const int* start = S.ints(S.L.start);
    const int* list = S.ints(S.L.list);
    const int* usable = S.ints(S.L.usable);
    const int* state = S.ints(S.L.state);
    int* nbr = S.ints(S.L.nbr);
    const int K = S.a.K;
    const size_t entries = 2 * (size_t)S.a.E;
    double gmax = 0.0;
    for (int k = threadIdx.x; k < K; k += THREADS) {
        double D[36], g[6];
#pragma unroll
        for (int m = 0; m < 36; m++) D[m] = 0.0;
#pragma unroll
        for (int m = 0; m < 6; m++) g[m] = 0.0;
        const int n0 = start[k], n1 = start[k + 1];
        for (int n = n0; n < n1; n++) {
            const int ent = list[n], e = ent >> 1, side = ent & 1;
            int other = -1;
            if ((unsigned)e < (unsigned)S.a.E && usable[e]) other = S.a.edges[2 * e + (side ^ 1)];
            if ((unsigned)other >= (unsigned)K) other = -1;
            nbr[n] = other;
            if (other < 0) continue;
            {
                const double* H = S.dbl(S.L.blocks) + (size_t)e * EDGE_BLOCKS + 36;  // H_ij
                double* O = S.dbl(S.L.off) + n;
#pragma unroll
                for (int m = 0; m < 6; m++)
#pragma unroll
                    for (int q = 0; q < 6; q++) O[(size_t)(6 * m + q) * entries] = side ? H[6 * q + m] : H[6 * m + q];
            }
            const double* blk = S.dbl(S.L.blocks) + (size_t)e * EDGE_BLOCKS + (side ? 72 : 0);
            const double* gv = S.dbl(S.L.gvec) + (size_t)e * 12 + (side ? 6 : 0);
#pragma unroll
            for (int m = 0; m < 36; m++) D[m] += blk[m];
#pragma unroll
            for (int m = 0; m < 6; m++) g[m] += gv[m];
        }
        double* Dk = S.dbl(S.L.diag) + k;
        double* gk = S.dbl(S.L.g) + k;
#pragma unroll
        for (int m = 0; m < 36; m++) Dk[(size_t)m * K] = D[m];
#pragma unroll
        for (int m = 0; m < 6; m++) gk[(size_t)m * K] = g[m];
        if (state[k] == 0)
#pragma unroll
            for (int m = 0; m < 6; m++) gmax = fmax(gmax, fabs(g[m]));
    }
    return block_max(gmax);
}

// the damped blocks' LDL^T; a free node with a pivot <= rcond * max diag becomes loose (and stays so).  Returns the active nodes.
__device__ double factor_nodes(const Solve& S, double lambda) {
    int* state = S.ints(S.L.state);
    double active = 0.0;
    for (int k = threadIdx.x; k < S.a.K; k += THREADS) {
        if (state[k] != 0) continue;
        const size_t K = (size_t)S.a.K;
        const double* Dk = S.dbl(S.L.diag) + k;
        double M[6][6], Dv[6], max_diag = 0.0;
#pragma unroll
        for (int m = 0; m < 6; m++)
#pragma unroll
            for (int n = 0; n < 6; n++) M[m][n] = Dk[(6 * m + n) * K];
#pragma unroll
        for (int m = 0; m < 6; m++) max_diag = fmax(max_diag, M[m][m]);
#pragma unroll
        for (int m = 0; m < 6; m++) M[m][m] += lambda * M[m][m];
        const bool ok = ldlt6_factor(M, Dv, S.a.rcond * max_diag);
        if (!ok) {
            state[k] = NODE_LOOSE;
            continue;
        }
        double* F = S.dbl(S.L.fac) + k;
#pragma unroll
        for (int m = 0; m < 6; m++)
#pragma unroll
            for (int n = 0; n <= m; n++) F[(6 * m + n) * K] = m == n ? Dv[m] : M[m][n];
        active += 1.0;
    }
    __syncthreads();
    return block_total(active);
}

// z = M^-1 r with node k's factor (F: the factors' base + k; K: the entry stride); only L's entries below the diagonal are kept
__device__ inline void precondition(const double* F, size_t K, const double (&r)[6], double (&z)[6]) {
    double M[6][6], Dv[6];
#pragma unroll
    for (int m = 0; m < 6; m++) {
#pragma unroll
        for (int n = 0; n < 6; n++) M[m][n] = n < m ? F[(6 * m + n) * K] : 0.0;
        Dv[m] = F[(7 * m) * K];
    }
    ldlt6_solve(M, Dv, r, z);
}

// (H + lambda diag H) x = -g over the active nodes by preconditioned conjugate gradients; x in the scratch.  Returns the iterations.
// P: the search direction, component-major like the scratch's vectors: in LDS when the graph is small enough, else in the scratch.
__device__ int conjugate_gradients(const Solve& S, double lambda, double* P, bool& capped) {
    const PgoArgs& a = S.a;
    const int K = a.K;
    const size_t Ks = (size_t)K, entries = 2 * (size_t)a.E;
    const int* start = S.ints(S.L.start);
    const int* nbr = S.ints(S.L.nbr);
    const int* state = S.ints(S.L.state);
    const double* OFF = S.dbl(S.L.off);
    double *X = S.dbl(S.L.x), *R = S.dbl(S.L.r), *Z = S.dbl(S.L.z), *AP = S.dbl(S.L.ap);
    double acc = 0.0;
    for (int k = threadIdx.x; k < K; k += THREADS) {
        double r[6], z[6];
        const bool act = state[k] == 0;
#pragma unroll
        for (int m = 0; m < 6; m++) r[m] = act ? -S.dbl(S.L.g)[m * Ks + k] : 0.0, z[m] = 0.0;
        if (act) precondition(S.dbl(S.L.fac) + k, Ks, r, z);
#pragma unroll
        for (int m = 0; m < 6; m++) {
            X[m * Ks + k] = 0.0, R[m * Ks + k] = r[m], Z[m * Ks + k] = z[m], P[m * Ks + k] = z[m];
            acc += r[m] * z[m];
        }
    }
    __syncthreads();
    double rz = block_total(acc);
    const double stop = a.cg_tolerance * a.cg_tolerance * rz;
    int it = 0;
    capped = false;
    for (; it < a.cg_iterations; it++) {
        if (!(rz > stop) || !(rz > 0.0)) break;  // converged (or nothing to solve, or a NaN)
        acc = 0.0;
        for (int k = threadIdx.x; k < K; k += THREADS) {
            if (state[k] != 0) continue;
            const double* Dk = S.dbl(S.L.diag) + k;
            const int n0 = start[k], n1 = start[k + 1];
            double p[6], ap[6];
#pragma unroll
            for (int m = 0; m < 6; m++) p[m] = P[m * Ks + k];
#pragma unroll
            for (int m = 0; m < 6; m++) {
                double v = 0.0;
#pragma unroll
                for (int n = 0; n < 6; n++) v += Dk[(6 * m + n) * Ks] * p[n];
                ap[m] = v + lambda * Dk[(7 * m) * Ks] * p[m];
            }
            for (int n = n0; n < n1; n++) {
                const int other = nbr[n];
                if (other < 0) continue;
                double po[6];
#pragma unroll
                for (int m = 0; m < 6; m++) po[m] = P[m * Ks + other];
#pragma unroll
                for (int m = 0; m < 6; m++) {
                    double v = 0.0;
#pragma unroll
                    for (int q = 0; q < 6; q++) v += OFF[(size_t)(6 * m + q) * entries + n] * po[q];
                    ap[m] += v;
                }
            }
#pragma unroll
            for (int m = 0; m < 6; m++) AP[m * Ks + k] = ap[m], acc += p[m] * ap[m];
        }
        const double pap = block_total(acc);
        if (!(pap > 0.0)) break;  // not positive definite along p (or a NaN): keep x
        const double alpha = rz / pap;
        acc = 0.0;
        for (int k = threadIdx.x; k < K; k += THREADS) {
            if (state[k] != 0) continue;
            double r[6], z[6];
#pragma unroll
            for (int m = 0; m < 6; m++) {
                X[m * Ks + k] += alpha * P[m * Ks + k];
                r[m] = R[m * Ks + k] - alpha * AP[m * Ks + k];
                R[m * Ks + k] = r[m];
            }
            precondition(S.dbl(S.L.fac) + k, Ks, r, z);
#pragma unroll
            for (int m = 0; m < 6; m++) Z[m * Ks + k] = z[m], acc += r[m] * z[m];
        }
        const double rz_new = block_total(acc);
        const double beta = rz_new / rz;
        rz = rz_new;
        for (int k = threadIdx.x; k < K; k += THREADS) {
            if (state[k] != 0) continue;
#pragma unroll
            for (int m = 0; m < 6; m++) P[m * Ks + k] = Z[m * Ks + k] + beta * P[m * Ks + k];
        }
        __syncthreads();  // every p is written before the next gather reads its neighbours'
    }
    if (it == a.cg_iterations && rz > stop && rz > 0.0) capped = true;
    return it;
}

// The same solve for a graph of at most one node per thread (K <= 256), the same operations in the same order: the node's
// damped block, its factor and its five vectors stay in registers for the whole solve, so an iteration reads only its neighbours'
// search directions (LDS) and off-diagonal blocks, and stores nothing but its own search direction (LDS).
__device__ int conjugate_gradients_one(const Solve& S, double lambda, double* P, bool& capped) {
    const PgoArgs& a = S.a;
    const int K = a.K, k = threadIdx.x;
    const size_t Ks = (size_t)K, entries = 2 * (size_t)a.E;
    const int* nbr = S.ints(S.L.nbr);
    const double* OFF = S.dbl(S.L.off);
    const bool act = k < K && S.ints(S.L.state)[k] == 0;
    double D[6][6], M[6][6], Dv[6], x[6], r[6], z[6], p[6], ap[6];
    int n0 = 0, n1 = 0;
#pragma unroll
    for (int m = 0; m < 6; m++) {
        x[m] = r[m] = z[m] = p[m] = ap[m] = 0.0, Dv[m] = 1.0;
#pragma unroll
        for (int n = 0; n < 6; n++) D[m][n] = M[m][n] = 0.0;
    }
    double acc = 0.0;
    if (act) {
        const double* Dk = S.dbl(S.L.diag) + k;
        const double* F = S.dbl(S.L.fac) + k;
        n0 = S.ints(S.L.start)[k], n1 = S.ints(S.L.start)[k + 1];
#pragma unroll
        for (int m = 0; m < 6; m++) {
#pragma unroll
            for (int n = 0; n < 6; n++) {
                D[m][n] = Dk[(6 * m + n) * Ks];
                if (n < m) M[m][n] = F[(6 * m + n) * Ks];
            }
            Dv[m] = F[(7 * m) * Ks];
            r[m] = -S.dbl(S.L.g)[m * Ks + k];
        }
        ldlt6_solve(M, Dv, r, z);
#pragma unroll
        for (int m = 0; m < 6; m++) p[m] = z[m], acc += r[m] * z[m];
    }
    if (k < K)
#pragma unroll
        for (int m = 0; m < 6; m++) P[m * Ks + k] = p[m];
    __syncthreads();
    double rz = block_total(acc);
    const double stop = a.cg_tolerance * a.cg_tolerance * rz;
    int it = 0;
    capped = false;
    for (; it < a.cg_iterations; it++) {
        if (!(rz > stop) || !(rz > 0.0)) break;
        acc = 0.0;
        if (act) {
#pragma unroll
            for (int m = 0; m < 6; m++) {
                double v = 0.0;
#pragma unroll
                for (int n = 0; n < 6; n++) v += D[m][n] * p[n];
                ap[m] = v + lambda * D[m][m] * p[m];
            }
            for (int n = n0; n < n1; n++) {
                const int other = nbr[n];
                if (other < 0) continue;
                double po[6];
#pragma unroll
                for (int m = 0; m < 6; m++) po[m] = P[m * Ks + other];
#pragma unroll
                for (int m = 0; m < 6; m++) {
                    double v = 0.0;
#pragma unroll
                    for (int q = 0; q < 6; q++) v += OFF[(size_t)(6 * m + q) * entries + n] * po[q];
                    ap[m] += v;
                }
            }
#pragma unroll
            for (int m = 0; m < 6; m++) acc += p[m] * ap[m];
        }
        const double pap = block_total(acc);
        if (!(pap > 0.0)) break;
        const double alpha = rz / pap;
        acc = 0.0;
        if (act) {
#pragma unroll
            for (int m = 0; m < 6; m++) x[m] += alpha * p[m], r[m] = r[m] - alpha * ap[m];
            ldlt6_solve(M, Dv, r, z);
#pragma unroll
            for (int m = 0; m < 6; m++) acc += r[m] * z[m];
        }
        const double rz_new = block_total(acc);
        const double beta = rz_new / rz;
        rz = rz_new;
        if (act)
#pragma unroll
            for (int m = 0; m < 6; m++) p[m] = z[m] + beta * p[m], P[m * Ks + k] = p[m];
        __syncthreads();
    }
    if (it == a.cg_iterations && rz > stop && rz > 0.0) capped = true;
    if (k < K)
#pragma unroll
        for (int m = 0; m < 6; m++) S.dbl(S.L.x)[m * Ks + k] = x[m];
    __syncthreads();
    return it;
}

__global__ void __launch_bounds__(THREADS) pgo_solve_kernel(PgoArgs a, char* scratch) {
    Solve S{a, pgo_layout(a.K, a.E), scratch};
    const int K = a.K, E = a.E, tid = threadIdx.x;
    const int* hdr = reinterpret_cast<const int*>(scratch);
    const bool planned = hdr[0] == PGO_MAGIC && hdr[1] == K && hdr[2] == E;
    int* state = S.ints(S.L.state);
    double* pose = S.dbl(S.L.pose);
    double* backup = S.dbl(S.L.backup);
    const double NaN = __longlong_as_double(0x7ff8000000000000LL);
    // the CG's search direction is the one vector read across nodes: in LDS while 6 K doubles fit
    __shared__ double p_lds[6 * LDS_NODES];
    double* P = K <= LDS_NODES ? p_lds : S.dbl(S.L.p);

    // the poses; one that is not rigid refuses the solve
    int bad = 0;
    for (int k = tid; k < K; k += THREADS) {
        double q[4], t[3];
        if (!load_rigid(a.poses_in + (size_t)k * 16, q, t)) bad = 1;
#pragma unroll
        for (int m = 0; m < 4; m++) pose[(size_t)k * 8 + m] = q[m];
#pragma unroll
        for (int m = 0; m < 3; m++) pose[(size_t)k * 8 + 4 + m] = t[m];
        state[k] = (a.fixed ? a.fixed[k] != 0 : k == 0) ? NODE_FIXED : 0;
    }
    const bool refused = __syncthreads_or(bad) != 0 || !planned;
    if (refused) {
        for (int k = tid; k < K; k += THREADS)
#pragma unroll
            for (int m = 0; m < 16; m++)
                reinterpret_cast<uint32_t*>(a.poses_out)[(size_t)k * 16 + m] = reinterpret_cast<const uint32_t*>(a.poses_in)[(size_t)k * 16 + m];
        if (a.chi2)
            for (int e = tid; e < E; e += THREADS) a.chi2[e] = (float)NaN;
        if (tid < 16) a.stats[tid] = 0.0;
        if (tid == 0) a.flags[0] = FLAG_REFUSED | (planned ? 0 : FLAG_NO_PLAN);
        return;
    }

    double lambda = fmin(fmax(a.damping, LAMBDA_MIN), LAMBDA_MAX);
    double cost = edges_cost<true>(S);
    const double cost_initial = cost;
    int run = 0, accepted = 0, rejected = 0, cg_total = 0, flags = 0;
    double last_w = 0.0, last_v = 0.0;
    bool converged = false, linearised = true, gathered = false;
    for (int it = 0; it < a.iterations; it++) {
        if (!linearised) edges_cost<true>(S), linearised = true, gathered = false;
        if (!gathered) {
            const double gmax = gather_nodes(S);
            gathered = true;
            if (!(gmax > 0.0)) {  // nothing to move, or already stationary
                converged = true;
                break;
            }
        }
        const double active = factor_nodes(S, lambda);
        if (!(active > 0.0)) {
            converged = true;
            break;
        }
        run++;
        bool capped;
        cg_total += K <= THREADS ? conjugate_gradients_one(S, lambda, P, capped) : conjugate_gradients(S, lambda, P, capped);
        if (capped) flags |= FLAG_CG_CAP;
        // the candidate: T_k <- Exp(x_k) T_k
        double wmax = 0.0, vmax = 0.0;
        for (int k = tid; k < K; k += THREADS) {
#pragma unroll
            for (int m = 0; m < 8; m++) backup[(size_t)k * 8 + m] = pose[(size_t)k * 8 + m];
            if (state[k] != 0) continue;
            const double* x = S.dbl(S.L.x) + k;
            const size_t Ks = (size_t)K;
            const double w[3] = {x[0], x[Ks], x[2 * Ks]}, v[3] = {x[3 * Ks], x[4 * Ks], x[5 * Ks]};
            wmax = fmax(wmax, sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]));
            vmax = fmax(vmax, sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
            const double q[4] = {pose[(size_t)k * 8], pose[(size_t)k * 8 + 1], pose[(size_t)k * 8 + 2], pose[(size_t)k * 8 + 3]};
            const double t[3] = {pose[(size_t)k * 8 + 4], pose[(size_t)k * 8 + 5], pose[(size_t)k * 8 + 6]};
            double Rk[3][3], Re[3][3], te[3], Rn[3][3], tn[3], qn[4];
            quat_to_rotation(q, Rk);
            se3_exp(w, v, Re, te);
            compose(Re, te, Rk, t, Rn, tn);
            rotation_to_quat(Rn, qn);
#pragma unroll
            for (int m = 0; m < 4; m++) pose[(size_t)k * 8 + m] = qn[m];
#pragma unroll
            for (int m = 0; m < 3; m++) pose[(size_t)k * 8 + 4 + m] = tn[m];
        }
        __syncthreads();
        wmax = block_max(wmax), vmax = block_max(vmax);
        const double cost_new = edges_cost<false>(S);
        if (cost_new < cost) {  // (false on a NaN)
            accepted++;
            last_w = wmax, last_v = vmax;
            const double decrease = (cost - cost_new) / cost;
            cost = cost_new;
            lambda = fmax(lambda / 10.0, LAMBDA_MIN);
            linearised = false;
            if (fmax(wmax, vmax) < a.step_tolerance || decrease < a.cost_tolerance) {
                converged = true;
                break;
            }
        } else {
            rejected++;
            for (int k = tid; k < K; k += THREADS)
#pragma unroll
                for (int m = 0; m < 8; m++) pose[(size_t)k * 8 + m] = backup[(size_t)k * 8 + m];
            __syncthreads();
            lambda = fmin(lambda * 10.0, LAMBDA_MAX);
            if (lambda >= LAMBDA_MAX) {
                flags |= FLAG_LAMBDA_MAX;
                break;
            }
        }
    }

    // outputs: a node that moved from its quaternion, every other the input's bits; then everything reported is taken at the
    // poses as written (fp32), so that it is the caller's own view of them
    for (int k = tid; k < K; k += THREADS) {
        float* out = a.poses_out + (size_t)k * 16;
        if (accepted > 0 && state[k] == 0) {
            const double q[4] = {pose[(size_t)k * 8], pose[(size_t)k * 8 + 1], pose[(size_t)k * 8 + 2], pose[(size_t)k * 8 + 3]};
            double Ro[3][3];
            quat_to_rotation(q, Ro);
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++) out[4 * i + j] = (float)Ro[j][i];
                out[4 * i + 3] = 0.f;
                out[12 + i] = (float)pose[(size_t)k * 8 + 4 + i];
            }
            out[15] = 1.f;
        } else {
            uint32_t bits[16];
#pragma unroll
            for (int m = 0; m < 16; m++) bits[m] = reinterpret_cast<const uint32_t*>(a.poses_in)[(size_t)k * 16 + m];
#pragma unroll
            for (int m = 0; m < 16; m++) reinterpret_cast<uint32_t*>(out)[m] = bits[m];
        }
    }
    __syncthreads();
    for (int k = tid; k < K; k += THREADS) {
        double q[4], t[3];
        load_rigid(a.poses_out + (size_t)k * 16, q, t);
#pragma unroll
        for (int m = 0; m < 4; m++) pose[(size_t)k * 8 + m] = q[m];
#pragma unroll
        for (int m = 0; m < 3; m++) pose[(size_t)k * 8 + 4 + m] = t[m];
    }
    __syncthreads();
    const double cost_final = edges_cost<true>(S);
    const double gmax = gather_nodes(S);
    const int* usable = S.ints(S.L.usable);
    double used = 0.0, loose = 0.0;
    for (int e = tid; e < E; e += THREADS) {
        used += usable[e] ? 1.0 : 0.0;
        if (a.chi2) a.chi2[e] = (float)S.dbl(S.L.s2)[e];
    }
    for (int k = tid; k < K; k += THREADS) loose += state[k] == NODE_LOOSE ? 1.0 : 0.0;
    used = block_total(used), loose = block_total(loose);
    if (tid == 0) {
        if (used < (double)E) flags |= FLAG_SKIPPED;
        if (loose > 0.0) flags |= FLAG_LOOSE;
        double* st = a.stats;
        st[0] = cost_initial, st[1] = cost_final, st[2] = 1.0, st[3] = (double)run, st[4] = (double)accepted, st[5] = (double)rejected;
        st[6] = (double)cg_total, st[7] = lambda, st[8] = last_w, st[9] = last_v, st[10] = gmax, st[11] = used;
        st[12] = (double)E - used, st[13] = loose, st[14] = converged ? 1.0 : 0.0, st[15] = 0.0;
        a.flags[0] = flags;
    }
}

}  // namespace

size_t pgo_scratch_bytes(int K, int E) { return pgo_layout(K, E).total; }

hipError_t launch_pgo_plan(int K, int E, const int* edges, void* scratch, hipStream_t stream) {
    launch(pgo_plan_kernel, dim3(1), dim3(THREADS), stream, K, E, edges, static_cast<char*>(scratch));
    return hipGetLastError();
}

hipError_t launch_pgo_solve(const PgoArgs& args, void* scratch, hipStream_t stream) {
    launch(pgo_solve_kernel, dim3(1), dim3(THREADS), stream, args, static_cast<char*>(scratch));
    return hipGetLastError();
}

}  // namespace dgr
