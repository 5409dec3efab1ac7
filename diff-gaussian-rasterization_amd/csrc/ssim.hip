// ssim.hip -- the standard 3DGS mapping loss around the rasterizer, forward and backward, as plain HIP launches:
//   loss = w_l1 mean|img - ref| + w_ssim (1 - SSIM(img, ref)) + w_depth mean|depth - depth_obs|
// SSIM is 3DGS's `ssim(img1, img2, window_size=11, size_average=True)`: an 11 x 11 Gaussian window (sigma 1.5) over the
// zero-padded image, per channel and per image of a [V, C, H, W] stack, mean of the map m over every element.
//
// Both kernels work on a 32 x 16 tile of one (image, channel) plane per 256-thread workgroup.  The halo tile (42 x 26) goes to
// LDS with predicated loads (0 outside the image), a horizontal 11-tap pass writes 26 x 32 row sums per moment back to LDS and a
// vertical pass forms two vertically adjacent outputs per thread from twelve rows (a sliding window: 12 LDS reads per moment for
// 2 pixels).  In every pass a wave's lanes walk ALONG a row -- consecutive lanes, consecutive LDS dwords -- so no access puts
// two lanes of a 32-lane ds_read_b32 group on one bank, whatever the row stride; the row sums keep the stride 32.
//   forward : five moments (x, y, xx, yy, xy) -> m, the three derivative maps dm/dmu1, dm/dsigma1^2, dm/dsigma12 (when asked
//             for), and per workgroup the sums of m and of |x - y|, reduced in double and stored as (hi, lo) float pairs in the
//             workgroup's own slot.  A one-workgroup kernel adds the slots in a fixed order.  No atomics: same bits every run.
//   backward: the same correlation of the three maps, then
//             dSSIM/dx = [w*(dm/dmu1) + 2x w*(dm/dsigma1^2) + y w*(dm/dsigma12)] / N   (the window is symmetric)
//             plus the L1 term's sign(x - y); dimg is written once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "block_sum.h"
#include "kernels.h"

namespace dgr {
namespace {

constexpr int RAD = 5, TAPS = 2 * RAD + 1;
constexpr int TW = 32, TH = 16;                      // the tile: 256 threads, two rows each
constexpr int HALO_W = TW + 2 * RAD, HALO_H = TH + 2 * RAD, HALO_N = HALO_H * HALO_W;
constexpr int THREADS = 256;
constexpr int DEPTH_BLOCKS = 128;                    // slots of the depth term's partial sums
constexpr int HEADER = 4;                            // scratch[0..3]: mean SSIM, mean|img - ref|, mean|depth - depth_obs|, maps flag
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

struct Window {
    float g[TAPS];
};

// g[i] ~ exp(-(i - 5)^2 / (2 1.5^2)), normalised in double, rounded once
Window make_window() {
    double e[TAPS], sum = 0.0;
    for (int i = 0; i < TAPS; i++) sum += e[i] = std::exp(-(double)((i - RAD) * (i - RAD)) / (2.0 * 1.5 * 1.5));
    Window w;
    for (int i = 0; i < TAPS; i++) w.g[i] = (float)(e[i] / sum);
    return w;
}

// the halo tiles of K planes (src[q] + offset of the same element) into LDS, 0 outside the image.  Every load of a thread is
// issued before the first LDS store waits for one: five steps x K loads in flight instead of one round trip to L2 / HBM per step
template <int K>
__device__ __forceinline__ void load_halos(const float* const (&src)[K], long plane, int H, int W, int x0, int y0,
                                           float (*dst)[HALO_N]) {
    constexpr int STEPS = (HALO_N + THREADS - 1) / THREADS;
    float v[STEPS][K];
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
        const int i = threadIdx.x + s * THREADS;
        const int r = i / HALO_W, c = i - r * HALO_W;
        const int gy = y0 + r, gx = x0 + c;
        const bool in = i < HALO_N && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const long o = plane + (long)gy * W + gx;
#pragma unroll
        for (int q = 0; q < K; q++) v[s][q] = in ? src[q][o] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
        const int i = threadIdx.x + s * THREADS;
        if (i < HALO_N) {
#pragma unroll
            for (int q = 0; q < K; q++) dst[q][i] = v[s][q];
        }
    }
}

// two sums in double over the workgroup (block_sum.h's order) to the workgroup's slot as (hi, lo) float pairs
__device__ __forceinline__ void reduce_to_slot(double a, double b, float* slot) {
    double s[2] = {a, b};
    block_sums(s);
    if (threadIdx.x == 0) *reinterpret_cast<float4*>(slot) = doubles_to_pairs(s[0], s[1]);
}

template <bool MAPS>
__global__ void __launch_bounds__(THREADS) ssim_forward_kernel(int H, int W, const float* __restrict__ img,
                                                               const float* __restrict__ ref, Window win, long n,
                                                               float* __restrict__ maps, float* __restrict__ partials) {
    __shared__ float sxy[2][HALO_N];
    __shared__ float rows[5][HALO_H * TW];
    const float* sx = sxy[0];
    const float* sy = sxy[1];
    const long plane = (long)blockIdx.z * H * W;
    const int bx = blockIdx.x * TW, by = blockIdx.y * TH;
    const float* const src[2] = {img, ref};
    load_halos(src, plane, H, W, bx - RAD, by - RAD, sxy);
    __syncthreads();
    // horizontal: 26 x 32 row sums of the five moments
    for (int i = threadIdx.x; i < HALO_H * TW; i += THREADS) {
        const float* px = sx + (i >> 5) * HALO_W + (i & 31);
        const float* py = sy + (i >> 5) * HALO_W + (i & 31);
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < TAPS; k++) {
            const float u = px[k], v = py[k], gu = win.g[k] * u, gv = win.g[k] * v;
            a += gu;
            b += gv;
            aa = fmaf(gu, u, aa);
            bb = fmaf(gv, v, bb);
            ab = fmaf(gu, v, ab);
        }
        rows[0][i] = a;
        rows[1][i] = b;
        rows[2][i] = aa;
        rows[3][i] = bb;
        rows[4][i] = ab;
    }
    __syncthreads();
    // vertical: outputs (tx, ty) and (tx, ty + 1) from rows ty .. ty + 11
    const int tx = threadIdx.x & 31, ty = (threadIdx.x >> 5) * 2;
    float acc[2][5] = {};
#pragma unroll
    for (int k = 0; k <= TAPS; k++)
#pragma unroll
        for (int q = 0; q < 5; q++) {
            const float v = rows[q][(ty + k) * TW + tx];
            if (k < TAPS) acc[0][q] = fmaf(win.g[k], v, acc[0][q]);
            if (k > 0) acc[1][q] = fmaf(win.g[k - 1], v, acc[1][q]);
        }
    double sum_m = 0.0, sum_l1 = 0.0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int gx = bx + tx, gy = by + ty + j;
        if (gx >= W || gy >= H) continue;
        const float mu1 = acc[j][0], mu2 = acc[j][1];
        const float s1 = acc[j][2] - mu1 * mu1, s2 = acc[j][3] - mu2 * mu2, s12 = acc[j][4] - mu1 * mu2;
        const float A = 2.f * mu1 * mu2 + C1, B = 2.f * s12 + C2;
        const float Cc = mu1 * mu1 + mu2 * mu2 + C1, D = s1 + s2 + C2;
        const float inv = 1.f / (Cc * D);
        const float m = A * B * inv;
        sum_m += (double)m;
        const int c = (ty + j + RAD) * HALO_W + tx + RAD;
        sum_l1 += (double)fabsf(sx[c] - sy[c]);
        if (MAPS) {
            const float dm_ds1 = -m / D, dm_ds12 = 2.f * A * inv;
            const float dm_dmu1 = 2.f * mu2 * B * inv - 2.f * mu1 * m / Cc - 2.f * mu1 * dm_ds1 - mu2 * dm_ds12;
            const long o = plane + (long)gy * W + gx;
            maps[o] = dm_dmu1;
            maps[n + o] = dm_ds1;
            maps[2 * n + o] = dm_ds12;
        }
    }
    const long wg = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    reduce_to_slot(sum_m, sum_l1, partials + 4 * wg);
}

// the depth term's sum|d - d_obs| in DEPTH_BLOCKS slots
__global__ void __launch_bounds__(THREADS) depth_partial_kernel(long n_d, const float* __restrict__ d, const float* __restrict__ d_obs,
                                                                float* __restrict__ partials) {
    double s = 0.0;
    const long stride = (long)gridDim.x * THREADS;
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < n_d; i += stride) s += (double)fabsf(d[i] - d_obs[i]);
    reduce_to_slot(s, 0.0, partials + 4 * (long)blockIdx.x);
}

// adds the slots in a fixed order and forms the loss: header[0..3] = mean SSIM, mean|img - ref|, mean|depth - depth_obs|, maps flag
__global__ void __launch_bounds__(THREADS) ssim_final_kernel(const float* __restrict__ partials, long n_tiles, int n_depth_slots,
                                                             double inv_n, double inv_n_d, float w_l1, float w_ssim, float w_depth,
                                                             float maps_flag, float* __restrict__ header, float* __restrict__ loss) {
    double s[3] = {};  // sums of m, of |img - ref|, of |depth - depth_obs|
    for (long i = threadIdx.x; i < n_tiles; i += THREADS) {
        const float4 p = *reinterpret_cast<const float4*>(partials + 4 * i);
        s[0] += pair_to_double(p.x, p.y);
        s[1] += pair_to_double(p.z, p.w);
    }
    for (long i = threadIdx.x; i < n_depth_slots; i += THREADS) {
        const float4 p = *reinterpret_cast<const float4*>(partials + 4 * (n_tiles + i));
        s[2] += pair_to_double(p.x, p.y);
    }
    block_sums(s);
    if (threadIdx.x == 0) {
        const double ssim = s[0] * inv_n, l1 = s[1] * inv_n, dl1 = s[2] * inv_n_d;
        header[0] = (float)ssim;
        header[1] = (float)l1;
        header[2] = (float)dl1;
        header[3] = maps_flag;
        *loss = (float)((double)w_l1 * l1 + (double)w_ssim * (1.0 - ssim) + (double)w_depth * dl1);
    }
}

// dimg = up k_l1 sign(x - y) + up k_ssim [w*(dm/dmu1) + 2x w*(dm/dsigma1^2) + y w*(dm/dsigma12)],  k_ssim = -w_ssim / N
__global__ void __launch_bounds__(THREADS) ssim_backward_kernel(int H, int W, const float* __restrict__ img,
                                                                const float* __restrict__ ref, Window win, long n,
                                                                const float* __restrict__ maps, const float* __restrict__ header,
                                                                float k_l1, float k_ssim, const float* __restrict__ upstream,
                                                                float* __restrict__ dimg) {
    __shared__ float sm[3][HALO_N];
    __shared__ float rows[3][HALO_H * TW];
    const long plane = (long)blockIdx.z * H * W;
    const int bx = blockIdx.x * TW, by = blockIdx.y * TH;
    const int tx = threadIdx.x & 31, ty = (threadIdx.x >> 5) * 2;
    // this thread's two centre pixels, asked for before the passes that hide their latency
    float cx[2], cy[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const bool in = bx + tx < W && by + ty + j < H;
        const long o = plane + (long)(by + ty + j) * W + bx + tx;
        cx[j] = in ? img[o] : 0.f;
        cy[j] = in ? ref[o] : 0.f;
    }
    const float* const src[3] = {maps, maps + n, maps + 2 * n};
    load_halos(src, plane, H, W, bx - RAD, by - RAD, sm);
    __syncthreads();
    for (int i = threadIdx.x; i < HALO_H * TW; i += THREADS) {
        const int o = (i >> 5) * HALO_W + (i & 31);
        float s[3] = {};
#pragma unroll
        for (int k = 0; k < TAPS; k++)
#pragma unroll
            for (int q = 0; q < 3; q++) s[q] = fmaf(win.g[k], sm[q][o + k], s[q]);
#pragma unroll
        for (int q = 0; q < 3; q++) rows[q][i] = s[q];
    }
    __syncthreads();
    float acc[2][3] = {};
#pragma unroll
    for (int k = 0; k <= TAPS; k++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const float v = rows[q][(ty + k) * TW + tx];
            if (k < TAPS) acc[0][q] = fmaf(win.g[k], v, acc[0][q]);
            if (k > 0) acc[1][q] = fmaf(win.g[k - 1], v, acc[1][q]);
        }
    // a forward that wrote no maps (want_maps = 0) left nothing to differentiate: say so in the result instead of reading stale maps
    const float up = header[3] != 0.f ? (upstream ? *upstream : 1.f) : __builtin_nanf("");
    const float u_l1 = up * k_l1, u_ssim = up * k_ssim;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int gx = bx + tx, gy = by + ty + j;
        if (gx >= W || gy >= H) continue;
        const long o = plane + (long)gy * W + gx;
        const float x = cx[j], y = cy[j];
        const float g = acc[j][0] + 2.f * x * acc[j][1] + y * acc[j][2];
        dimg[o] = u_l1 * sign0(x - y) + u_ssim * g;
    }
}

inline long tiles_of(int V, int C, int H, int W) { return (long)V * C * ((H + TH - 1) / TH) * ((W + TW - 1) / TW); }

}  // namespace

bool ssim_shape_ok(int V, int C, int H, int W) {
    // (V C planes ride on the grid's z dimension; H, W bounded so that the tile counts and H * W stay far inside int / long)
    return V > 0 && C > 0 && H > 0 && W > 0 && (long)V * C <= 65535 && H <= (1 << 20) && W <= (1 << 20);
}
long ssim_partial_floats(int V, int C, int H, int W) { return HEADER + 4 * (tiles_of(V, C, H, W) + DEPTH_BLOCKS); }
long ssim_scratch_floats(int V, int C, int H, int W) {
    return ssim_shape_ok(V, C, H, W) ? ssim_partial_floats(V, C, H, W) + 3 * ((long)V * C * H * W) : 0;
}

hipError_t launch_ssim_loss_forward(int V, int C, int H, int W, const float* img, const float* ref, long n_d, const float* d,
                                    const float* d_obs, float w_l1, float w_ssim, float w_depth, float* scratch, bool want_maps,
                                    float* loss, hipStream_t stream) {
    static const Window win = make_window();
    const long n = (long)V * C * H * W, n_tiles = tiles_of(V, C, H, W);
    float* partials = scratch + HEADER;
    float* maps = scratch + ssim_partial_floats(V, C, H, W);
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, V * C);
    if (want_maps) launch(ssim_forward_kernel<true>, grid, dim3(THREADS), stream, H, W, img, ref, win, n, maps, partials);
    else launch(ssim_forward_kernel<false>, grid, dim3(THREADS), stream, H, W, img, ref, win, n, maps, partials);
    if (n_d > 0) launch(depth_partial_kernel, dim3(DEPTH_BLOCKS), dim3(THREADS), stream, n_d, d, d_obs, partials + 4 * n_tiles);
    launch(ssim_final_kernel, dim3(1), dim3(THREADS), stream, (const float*)partials, n_tiles, n_d > 0 ? DEPTH_BLOCKS : 0,
           1.0 / (double)n, n_d > 0 ? 1.0 / (double)n_d : 0.0, w_l1, w_ssim, w_depth, want_maps ? 1.f : 0.f, scratch, loss);
    return hipGetLastError();
}

hipError_t launch_ssim_loss_backward(int V, int C, int H, int W, const float* img, const float* ref, long n_d, const float* d,
                                     const float* d_obs, float w_l1, float w_ssim, float w_depth, const float* scratch,
                                     const float* upstream, float* dimg, float* ddepth, hipStream_t stream) {
    static const Window win = make_window();
    const long n = (long)V * C * H * W;
    const float* maps = scratch + ssim_partial_floats(V, C, H, W);
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, V * C);
    launch(ssim_backward_kernel, grid, dim3(THREADS), stream, H, W, img, ref, win, n, maps, scratch, w_l1 / (float)n,
           -w_ssim / (float)n, upstream, dimg);
    if (n_d > 0) {  // the depth image's gradient: l1_backward_kernel with no colour part
        const hipError_t e = launch_l1_loss_backward(0, nullptr, nullptr, n_d, d, d_obs, 0.f, w_depth, upstream, nullptr, ddepth, stream);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

}  // namespace dgr
