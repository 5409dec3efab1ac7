// se3.h -- the rigid-motion helpers the pose steps share (gn_step.h's solve and writer, the update rules of icp.hip and gicp.hip
// between them, pgo.hip), all in double on the device: a pose as (R, t) of W2C, its unit quaternion (r, x, y, z; r >= 0), the
// exponential of a twist (w, v) and the 6 x 6 LDL^T the steps solve with.  No contraction mode of its own either: every file
// includes it above any pragma of its own, so it is contracted everywhere.
#pragma once
#include <hip/hip_runtime.h>

namespace dgr {

// (r, x, y, z) of a rotation matrix, unit, r >= 0 (Shepperd's branches); R = (r^2 - |v|^2) I + 2 v v^T + 2 r [v]x, pose.hip's
__device__ inline void rotation_to_quat(const double (&R)[3][3], double (&q)[4]) {
    const double tr = R[0][0] + R[1][1] + R[2][2];
    if (tr > 0.0) {
        const double s = 2.0 * sqrt(tr + 1.0);
        q[0] = 0.25 * s, q[1] = (R[2][1] - R[1][2]) / s, q[2] = (R[0][2] - R[2][0]) / s, q[3] = (R[1][0] - R[0][1]) / s;
    } else if (R[0][0] > R[1][1] && R[0][0] > R[2][2]) {
        const double s = 2.0 * sqrt(1.0 + R[0][0] - R[1][1] - R[2][2]);
        q[0] = (R[2][1] - R[1][2]) / s, q[1] = 0.25 * s, q[2] = (R[0][1] + R[1][0]) / s, q[3] = (R[0][2] + R[2][0]) / s;
    } else if (R[1][1] > R[2][2]) {
        const double s = 2.0 * sqrt(1.0 + R[1][1] - R[0][0] - R[2][2]);
        q[0] = (R[0][2] - R[2][0]) / s, q[1] = (R[0][1] + R[1][0]) / s, q[2] = 0.25 * s, q[3] = (R[1][2] + R[2][1]) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + R[2][2] - R[0][0] - R[1][1]);
        q[0] = (R[1][0] - R[0][1]) / s, q[1] = (R[0][2] + R[2][0]) / s, q[2] = (R[1][2] + R[2][1]) / s, q[3] = 0.25 * s;
    }
    const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double sgn = q[0] < 0.0 ? -inv : inv;
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] *= sgn;
}
__device__ inline void quat_to_rotation(const double (&q)[4], double (&R)[3][3]) {
    const double r = q[0], x = q[1], y = q[2], z = q[3];
    const double d = r * r - (x * x + y * y + z * z);
    R[0][0] = d + 2.0 * x * x, R[0][1] = 2.0 * x * y - 2.0 * r * z, R[0][2] = 2.0 * x * z + 2.0 * r * y;
    R[1][0] = 2.0 * x * y + 2.0 * r * z, R[1][1] = d + 2.0 * y * y, R[1][2] = 2.0 * y * z - 2.0 * r * x;
    R[2][0] = 2.0 * x * z - 2.0 * r * y, R[2][1] = 2.0 * y * z + 2.0 * r * x, R[2][2] = d + 2.0 * z * z;
}
// (R, t) of 16 floats holding W2C^T: R[j][i] at [4 i + j], t[j] at [12 + j]
__device__ inline void pose_of(const float* v, double (&R)[3][3], double (&t)[3]) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
#pragma unroll
        for (int i = 0; i < 3; i++) R[j][i] = (double)v[4 * i + j];
        t[j] = (double)v[12 + j];
    }
}
// (Ra, ta) (Rb, tb) = (Ra Rb, Ra tb + ta)
__device__ inline void compose(const double (&Ra)[3][3], const double (&ta)[3], const double (&Rb)[3][3], const double (&tb)[3],
                        double (&R)[3][3], double (&t)[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = Ra[i][0] * Rb[0][j] + Ra[i][1] * Rb[1][j] + Ra[i][2] * Rb[2][j];
        t[i] = Ra[i][0] * tb[0] + Ra[i][1] * tb[1] + Ra[i][2] * tb[2] + ta[i];
    }
}
// exp of the twist (w, v): R = I + A [w]x + B [w]x^2, t = (I + B [w]x + C [w]x^2) v, A = sin th / th, B = (1 - cos th) / th^2,
// C = (th - sin th) / th^3, their series below th^2 = 1e-6
__device__ inline void se3_exp(const double (&w)[3], const double (&v)[3], double (&R)[3][3], double (&t)[3]) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double A, B, C;
    if (th2 < 1e-6) {
        A = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0);
        B = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0);
        C = 1.0 / 6.0 - th2 / 120.0 * (1.0 - th2 / 42.0);
    } else {
        const double th = sqrt(th2), s = sin(th), h = sin(0.5 * th);
        A = s / th, B = 2.0 * h * h / th2, C = (th - s) / (th2 * th);
    }
    const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double ti = 0.0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double K2 = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
            const double I = i == j ? 1.0 : 0.0;
            R[i][j] = I + A * K[i][j] + B * K2;
            ti += (I + B * K[i][j] + C * K2) * v[j];
        }
        t[i] = ti;
    }
}

// M = L D L^T in place, L unit lower triangular (kept in M's lower triangle), no pivoting: M is symmetric positive semi-definite.
// False when a pivot is not above pivot_min or not positive (or is a NaN); the factor is completed either way.
__device__ __forceinline__ bool ldlt6_factor(double (&M)[6][6], double (&D)[6], double pivot_min) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double dj = M[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) dj -= M[j][k] * M[j][k] * D[k];
        ok = ok && dj > pivot_min && dj > 0.0;  // (false on a NaN)
        D[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double l = M[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) l -= M[i][k] * M[j][k] * D[k];
            M[i][j] = l / dj;
        }
    }
    return ok;
}
// x = (L D L^T)^-1 b: forward, diagonal, backward
__device__ __forceinline__ void ldlt6_solve(const double (&M)[6][6], const double (&D)[6], const double (&b)[6], double (&xi)[6]) {
#pragma unroll
    for (int i = 0; i < 6; i++) {  // L z = b
        double z = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) z -= M[i][k] * xi[k];
        xi[i] = z;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) xi[i] /= D[i];
#pragma unroll
    for (int i = 5; i >= 0; i--) {  // L^T xi = y
        double z = xi[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) z -= M[k][i] * xi[k];
        xi[i] = z;
    }
}

}  // namespace dgr
