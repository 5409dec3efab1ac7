// state_export.hip -- dgr_state_export: a forward's state arrays in the reference's layouts (tests / profiling).
#include <hip/hip_runtime.h>

#include <string>

#include "dgr_common.h"
#include "host_util.h"

namespace {

enum ExportKind { EX_MEANS2D, EX_CONIC_OPACITY, EX_RGB, EX_CLAMPED, EX_TILES_TOUCHED, EX_KEYS };

__global__ void export_geom_kernel(int kind, int P, dgr::GeometryView g, void* dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const bool vis = g.radii[i] > 0;
    switch (kind) {
        case EX_MEANS2D: {
            const float4 q = g.rec[DGR_REC_STRIDE * (size_t)i];
            ((float2*)dst)[i] = vis ? make_float2(q.x, q.y) : make_float2(0, 0);
        } break;
        case EX_CONIC_OPACITY: {
            const float4 q0 = g.rec[DGR_REC_STRIDE * (size_t)i], q1 = g.rec[DGR_REC_STRIDE * (size_t)i + 1];
            ((float4*)dst)[i] = vis ? make_float4(q1.x, q1.y, q1.z, q0.w) : make_float4(0, 0, 0, 0);
        } break;
        case EX_RGB: {
            const float4 q = g.rec[DGR_REC_STRIDE * (size_t)i + 2];
            float* d = (float*)dst + 3 * (size_t)i;
            d[0] = vis ? q.x : 0; d[1] = vis ? q.y : 0; d[2] = vis ? q.z : 0;
        } break;
        case EX_CLAMPED: {
            const uint8_t c = vis ? g.clamped[i] : 0;
            uint8_t* d = (uint8_t*)dst + 3 * (size_t)i;
            d[0] = c & 1; d[1] = (c >> 1) & 1; d[2] = (c >> 2) & 1;
        } break;
        case EX_TILES_TOUCHED: {
            const ushort4 r = g.rect[i];
            ((uint32_t*)dst)[i] = (uint32_t)(r.z - r.x) * (uint32_t)(r.w - r.y);
        } break;
    }
}
// the reference's sorted 64-bit keys: tile id << 32 | depth bits (rasterizer_impl.cu:97-100)
__global__ void export_keys_kernel(dgr::ImageView img, dgr::BinningView bin, dgr::GeometryView g, uint64_t* dst) {
    const int tile = blockIdx.x;
    const uint2 rg = img.ranges[tile];
    for (uint32_t i = rg.x + threadIdx.x; i < rg.y; i += blockDim.x)
        dst[i] = ((uint64_t)tile << 32) | __float_as_uint(g.depths[bin.point_list[i] & DGR_ID_MASK]);
}
// the sorted Gaussian ids (the mask: rounds 3-8 kept contribution tags in the top 4 bits; nothing writes them any more)
__global__ void export_point_list_kernel(const uint32_t* src, uint32_t* dst, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i] & DGR_ID_MASK;
}
// ... and the contribution tags (tests): the blend forward's tag bytes (bit 2 w + h: half h of quadrant wave w; `half` = 1: as they
// are), or folded to 4 bits, bit w = quadrant wave w
__global__ void export_tag_bytes_kernel(const uint8_t* src, uint8_t* dst, int n, int half) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t t = src[i];
    if (!half) {
        t = (t | (t >> 1)) & 0x55u;
        t = (t & 1u) | ((t >> 1) & 2u) | ((t >> 2) & 4u) | ((t >> 3) & 8u);
    }
    dst[i] = (uint8_t)t;
}

}  // namespace

extern "C" {

long dgr_state_export(void* stream, const char* name, int P, int width, int height, int num_rendered,
                      int binning_capacity, const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
                      void* dst) {
    hipStream_t st = (hipStream_t)stream;
    if (binning_capacity < num_rendered) { dgr::set_last_error("binning_capacity < num_rendered"); return -1; }
    dgr::GeometryView g = dgr::carve_geometry(const_cast<char*>(geom_buffer), P);
    dgr::ImageView img = dgr::carve_image(const_cast<char*>(image_buffer), width, height);
    dgr::BinningView bin = dgr::carve_binning(const_cast<char*>(binning_buffer), (size_t)binning_capacity);
    const size_t tiles = (size_t)dgr::tiles_x(width) * dgr::tiles_y(height), N = (size_t)width * height;
    auto copy = [&](const void* src, size_t bytes) -> int {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
        return 0;
    };
    auto geomk = [&](int kind) -> int {
        if (P > 0) hipLaunchKernelGGL(export_geom_kernel, dim3((P + 255) / 256), dim3(256), 0, st, kind, P, g, dst);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    const std::string n(name);
    if (n == "depths") return copy(g.depths, 4 * (size_t)P) ? -1 : P;
    if (n == "radii") return copy(g.radii, 4 * (size_t)P) ? -1 : P;
    if (n == "means2D") return geomk(EX_MEANS2D) ? -1 : 2L * P;
    if (n == "conic_opacity") return geomk(EX_CONIC_OPACITY) ? -1 : 4L * P;
    if (n == "rgb") return geomk(EX_RGB) ? -1 : 3L * P;
    if (n == "clamped") return geomk(EX_CLAMPED) ? -1 : 3L * P;
    if (n == "tiles_touched") return geomk(EX_TILES_TOUCHED) ? -1 : P;
    if (n == "point_list" || n == "contribution_tags" || n == "half_tags") {
        if (num_rendered > 0) {
            const dim3 grid((num_rendered + 255) / 256);
            if (n == "point_list")
                hipLaunchKernelGGL(export_point_list_kernel, grid, dim3(256), 0, st, bin.point_list, (uint32_t*)dst, num_rendered);
            else  // (the tag bytes: in the binning's pair_cov bytes, render_common.h)
                hipLaunchKernelGGL(export_tag_bytes_kernel, grid, dim3(256), 0, st, bin.pair_cov, (uint8_t*)dst, num_rendered, n == "half_tags" ? 1 : 0);
            if (hipGetLastError() != hipSuccess) return -1;
        }
        return num_rendered;
    }
    if (n == "keys") {
        hipLaunchKernelGGL(export_keys_kernel, dim3((unsigned)tiles), dim3(256), 0, st, img, bin, g, (uint64_t*)dst);
        if (hipGetLastError() != hipSuccess) return -1;
        return num_rendered;
    }
    // the light forward's live lists (render_common.h: live_list): per instance slot {Gaussian id, list position << 8 | tag byte}, of
    // which the first live_counts[tile] from the tile's range start on are written; and the per-tile counts
    if (n == "live_list") return copy(bin.pair_keys, 8 * (size_t)num_rendered) ? -1 : 2L * num_rendered;
    if (n == "live_counts") return copy(img.tile_count, 4 * tiles) ? -1 : (long)tiles;
    if (n == "ranges") return copy(img.ranges, 8 * tiles) ? -1 : (long)(2 * tiles);
    if (n == "tile_sched") return copy(img.tile_sched, 16 * tiles) ? -1 : (long)(4 * tiles);
    if (n == "sched_flag") return copy(img.cursor + 3, 4) ? -1 : 1L;  // 1: this frame's blend kernels walk tile_sched, 0: the static band map
    if (n == "n_contrib") return copy(img.n_contrib, 4 * N) ? -1 : (long)N;
    if (n == "n_valid") return copy(img.n_valid, 4 * N) ? -1 : (long)N;
    if (n == "first_contrib") return copy(img.first_contrib, 4 * N) ? -1 : (long)N;  // (full variant: 1-based list position, 0 = none)
    if (n == "final_T") return copy(img.final_T, 4 * N) ? -1 : (long)N;
    dgr::set_last_error("unknown state array: " + n);
    return -1;
}

}  // extern "C"
