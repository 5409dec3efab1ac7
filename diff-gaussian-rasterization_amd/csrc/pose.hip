// pose.hip -- (quaternion, translation) <-> the rasterizer's camera tensors and dL/dviewmatrix, each way as ONE launch instead of
// ~40 elementwise torch kernels: a 640x480 tracking iteration is launch-bound (the rasterizer's kernels
// are 0.17 ms of a 0.43 ms hipGraph replay when pose, loss and their backward run as torch ops).
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dgr {
namespace {

// R = (r^2 - |v|^2) I + 2 v v^T + 2 r [v]x of the NORMALISED quaternion (r, x, y, z) -- dgr_amd.pose.quat_to_rotmat
__device__ void rotation(const float* q, float (&R)[3][3], float& inv_norm, float (&qh)[4]) {
    inv_norm = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) qh[i] = q[i] * inv_norm;
    const float r = qh[0], x = qh[1], y = qh[2], z = qh[3];
    const float d = r * r - (x * x + y * y + z * z);
    R[0][0] = d + 2.f * x * x;      R[0][1] = 2.f * x * y - 2.f * r * z;  R[0][2] = 2.f * x * z + 2.f * r * y;
    R[1][0] = 2.f * x * y + 2.f * r * z;  R[1][1] = d + 2.f * y * y;      R[1][2] = 2.f * y * z - 2.f * r * x;
    R[2][0] = 2.f * x * z - 2.f * r * y;  R[2][1] = 2.f * y * z + 2.f * r * x;  R[2][2] = d + 2.f * z * z;
}

// viewmatrix = W2C^T, projmatrix = W2C^T Proj^T, campos = -R^T t  (cuda_rasterizer/auxiliary.h:58-77 reads all three
// column-major, i.e. as the transposes stored row-major)
__global__ void pose_forward_kernel(const float* q, const float* t, const float* perspec, float* view, float* proj, float* campos) {
    if (threadIdx.x != 0) return;
    float R[3][3], inv_norm, qh[4];
    rotation(q, R, inv_norm, qh);
    float V[4][4];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) V[i][j] = R[j][i];
        V[i][3] = 0.f;
        V[3][i] = t[i];
    }
    V[3][3] = 1.f;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            view[4 * i + j] = V[i][j];
            float s = 0.f;
            for (int k = 0; k < 4; k++) s += V[i][k] * perspec[4 * k + j];
            proj[4 * i + j] = s;
        }
    for (int i = 0; i < 3; i++) campos[i] = -(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]);
}

// dL/dviewmatrix -> dL/dq, dL/dt.  projmatrix and campos enter the rasterizer as constants (the reference's backward adds
// their dependence on the pose inside its kernels: L/cuda_rasterizer/backward.cu:633-651, 683-751).
__global__ void pose_backward_kernel(const float* q, const float* dview, float* dq, float* dt) {
    if (threadIdx.x != 0) return;
    float R[3][3], inv_norm, qh[4];
    rotation(q, R, inv_norm, qh);
    float G[3][3];  // dL/dR[a][b] = dL/dviewmatrix[b][a]
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) G[a][b] = dview[4 * b + a];
    for (int a = 0; a < 3; a++) dt[a] = dview[12 + a];
    const float r = qh[0], v[3] = {qh[1], qh[2], qh[3]};
    const float tr = G[0][0] + G[1][1] + G[2][2];
    float g[4];
    g[0] = 2.f * r * tr + 2.f * (-v[2] * G[0][1] + v[1] * G[0][2] + v[2] * G[1][0] - v[0] * G[1][2] - v[1] * G[2][0] + v[0] * G[2][1]);
    const float skew[3] = {G[2][1] - G[1][2], G[0][2] - G[2][0], G[1][0] - G[0][1]};
    for (int k = 0; k < 3; k++) {
        float gv = 0.f;
        for (int j = 0; j < 3; j++) gv += (G[k][j] + G[j][k]) * v[j];
        g[1 + k] = -2.f * v[k] * tr + 2.f * gv + 2.f * r * skew[k];
    }
    const float along = qh[0] * g[0] + qh[1] * g[1] + qh[2] * g[2] + qh[3] * g[3];
    for (int i = 0; i < 4; i++) dq[i] = (g[i] - qh[i] * along) * inv_norm;  // through q / |q|
}

}  // namespace

hipError_t launch_pose_forward(const float* q, const float* t, const float* perspec, float* view, float* proj, float* campos,
                               hipStream_t stream) {
    launch(pose_forward_kernel, dim3(1), dim3(64), stream, q, t, perspec, view, proj, campos);
    return hipGetLastError();
}
hipError_t launch_pose_backward(const float* q, const float* dview, float* dq, float* dt, hipStream_t stream) {
    launch(pose_backward_kernel, dim3(1), dim3(64), stream, q, dview, dq, dt);
    return hipGetLastError();
}

}  // namespace dgr
