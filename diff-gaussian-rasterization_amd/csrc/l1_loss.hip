// l1_loss.hip -- the plain tracking loss w_c mean|C - C_obs| + w_d mean|D - D_obs| as ONE fused reduction (two launches) and its
// two gradient images as one more, instead of a dozen elementwise torch kernels: a 640x480 tracking iteration is launch-bound
// (SURVEY.md s8(f) item 1).  ssim.hip's depth term uses the backward too.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "block_sum.h"
#include "kernels.h"

namespace dgr {
namespace {

constexpr int LOSS_BLOCKS = 128;

// partial[b] = block b's share of  w_c / n_c * sum|C - C_obs| + w_d / n_d * sum|D - D_obs|
__global__ void __launch_bounds__(256) l1_partial_kernel(long n_c, const float* c, const float* c_obs, long n_d, const float* d,
                                                         const float* d_obs, float k_c, float k_d, float* partial) {
    float s[1] = {0.f};
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_c; i += stride) s[0] += k_c * fabsf(c[i] - c_obs[i]);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_d; i += stride) s[0] += k_d * fabsf(d[i] - d_obs[i]);
    block_sums(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s[0];
}
__global__ void __launch_bounds__(64) l1_final_kernel(const float* partial, int n, float* loss) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) s += partial[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) *loss = s;
}
__global__ void __launch_bounds__(256) l1_backward_kernel(long n_c, const float* c, const float* c_obs, long n_d, const float* d,
                                                          const float* d_obs, float k_c, float k_d, const float* upstream,
                                                          float* dc, float* dd) {
    const float up = upstream ? *upstream : 1.f;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_c; i += stride) dc[i] = (up * k_c) * sign0(c[i] - c_obs[i]);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_d; i += stride) dd[i] = (up * k_d) * sign0(d[i] - d_obs[i]);
}

}  // namespace

int l1_loss_partials() { return LOSS_BLOCKS; }
hipError_t launch_l1_loss_forward(long n_c, const float* c, const float* c_obs, long n_d, const float* d, const float* d_obs,
                                  float w_c, float w_d, float* partial, float* loss, hipStream_t stream) {
    const float k_c = n_c > 0 ? w_c / (float)n_c : 0.f, k_d = n_d > 0 ? w_d / (float)n_d : 0.f;
    launch(l1_partial_kernel, dim3(LOSS_BLOCKS), dim3(256), stream, n_c, c, c_obs, n_d, d, d_obs, k_c, k_d, partial);
    launch(l1_final_kernel, dim3(1), dim3(64), stream, (const float*)partial, LOSS_BLOCKS, loss);
    return hipGetLastError();
}
hipError_t launch_l1_loss_backward(long n_c, const float* c, const float* c_obs, long n_d, const float* d, const float* d_obs,
                                   float w_c, float w_d, const float* upstream, float* dc, float* dd, hipStream_t stream) {
    const float k_c = n_c > 0 ? w_c / (float)n_c : 0.f, k_d = n_d > 0 ? w_d / (float)n_d : 0.f;
    const long n = std::max(n_c, n_d);
    if (n <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 2048);
    launch(l1_backward_kernel, dim3(blocks), dim3(256), stream, n_c, c, c_obs, n_d, d, d_obs, k_c, k_d, upstream, dc, dd);
    return hipGetLastError();
}

}  // namespace dgr
