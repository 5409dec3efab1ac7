// raycast.hip -- ray-casting the TSDF volume: depth, normals and colour at any pose (include/dgr_hip.h: dgr_tsdf_bricks,
// dgr_tsdf_raycast), gfx950, wave64.  The rule is stated in the header; this file is how it is marched.
//
// raycast: one lane per ray, V views in one launch (blockIdx.z = the view: its pose sits at a wave-uniform address and is read
//   with scalar loads; every other scalar is a kernel argument).  A 256-thread workgroup owns 16 x 16 pixels, a wave an 8 x 8
//   block of them, so that the 64 rays of a wave walk through neighbouring cells and their gathers share cache lines (a row of 64
//   pixels fans out over 64 cells' width at once).  A sample's 8 corners are four 16-byte loads: the x-adjacent (tsdf, weight)
//   pairs are contiguous (8-byte aligned: the hardware takes a dwordx4 at any dword).
//   Every sample is computed from its own index k: z_k = fma(k, step, depth_min), q_k = fma(z_k, dq, q0) in lattice units.  Both
//   are monotone in k on every axis (a rounded fma is monotone in each argument), which is what makes the three short cuts exact
//   instead of merely careful:
//     * the first sample marched, k0, comes from the slab test in float, and is then CHECKED: sample k0 - 1 must lie outside the
//       lattice on the side the ray enters from -- every earlier sample then does too.  A failed check starts at 0.
//     * the march ends at the first sample that lies outside on the side the ray leaves through (every later one does too), at
//       z_k >= depth_max, or at k = 2^24 (where a float stops holding k).
//     * in a dead brick the exit depth gives a candidate for the LAST sample still inside; it is recomputed from its own k and
//       must lie in the same brick on every axis -- then every sample between does -- else the march goes on by one.  The sample
//       it lands on has its own brick tested again.  So no sample of a live brick is ever skipped, whatever the rounding of the
//       exit depth was, and the outputs with and without the map are the same bits.
//   The decisive sample k* found, sample k* - 1 is evaluated from scratch wherever it lies; the hit's depth, normal (six more
//   evaluations) and colour follow from those two alone.
//   Rays of one wave end at different k: the lanes that are done wait, masked, for the wave's last ray (an 8 x 8 block's rays are
//   of similar length; nothing is compacted or refilled).
// bricks: one workgroup per brick of 8 x 8 x 8 cells.  Its 9 x 9 x 9 samples are read once into two bits each in LDS (weight >=
//   min_weight; tsdf <= 0; a sample outside the lattice has neither), a thread then combines the corners of two cells, and the
//   block's OR is the brick's byte.  Comparisons and integer logic only, no atomics.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dgr {
namespace {

constexpr int BRICK = 8, BRICK_SHIFT = 3;  // cells per brick and axis
constexpr int K_CAP = 1 << 24;             // sample indices stay exactly representable in a float

// two x-adjacent samples (tsdf, weight, tsdf, weight): 16 contiguous bytes at an 8-byte boundary, one load
typedef float Pair2Bits __attribute__((ext_vector_type(4), aligned(8)));
struct Pair2 {
    float t0, w0, t1, w1;
};
__device__ __forceinline__ Pair2 load_pair(const float2* __restrict__ p) {
    const Pair2Bits v = *reinterpret_cast<const Pair2Bits*>(p);
    return {v.x, v.y, v.z, v.w};
}

struct Sampled {
    bool valid;
    float F;
};

// the cell of a lattice coordinate: false unless 0 <= floor(q) <= n - 2 on every axis (false on a NaN); the indices are tested
// again as integers, which is what bounds the gathers
__device__ __forceinline__ bool cell_of(const RaycastArgs& a, float qx, float qy, float qz, int& ix, int& iy, int& iz, float& fx,
                                        float& fy, float& fz) {
    const float flx = floorf(qx), fly = floorf(qy), flz = floorf(qz);
    if (!(flx >= 0.0f && flx <= (float)(a.nx - 2) && fly >= 0.0f && fly <= (float)(a.ny - 2) && flz >= 0.0f && flz <= (float)(a.nz - 2)))
        return false;
    ix = (int)flx, iy = (int)fly, iz = (int)flz;
    if (ix < 0 || iy < 0 || iz < 0 || ix > a.nx - 2 || iy > a.ny - 2 || iz > a.nz - 2) return false;
    fx = qx - flx, fy = qy - fly, fz = qz - flz;
    return true;
}

__device__ __forceinline__ float lerp(float f, float a, float b) { return __fmaf_rn(f, b - a, a); }

// the validity-checked trilinear interpolant of the cell (ix, iy, iz), which the caller has bounded
__device__ __forceinline__ Sampled sample_cell(const RaycastArgs& a, int ix, int iy, int iz, float fx, float fy, float fz) {
    const size_t row = (size_t)(unsigned)a.nx, slab = row * (size_t)(unsigned)a.ny;
    const float2* __restrict__ p = a.volume + ((size_t)iz * slab + (size_t)iy * row + (size_t)ix);
    const Pair2 c00 = load_pair(p), c10 = load_pair(p + row), c01 = load_pair(p + slab), c11 = load_pair(p + slab + row);
    const float mw = a.min_weight;
    Sampled s;
    s.valid = (c00.w0 >= mw) & (c00.w1 >= mw) & (c10.w0 >= mw) & (c10.w1 >= mw) & (c01.w0 >= mw) & (c01.w1 >= mw) & (c11.w0 >= mw) & (c11.w1 >= mw);
    const float x00 = lerp(fx, c00.t0, c00.t1), x10 = lerp(fx, c10.t0, c10.t1), x01 = lerp(fx, c01.t0, c01.t1), x11 = lerp(fx, c11.t0, c11.t1);
    s.F = lerp(fz, lerp(fy, x00, x10), lerp(fy, x01, x11));
    return s;
}

__device__ __forceinline__ Sampled sample_at(const RaycastArgs& a, float qx, float qy, float qz) {
    int ix, iy, iz;
    float fx, fy, fz;
    if (!cell_of(a, qx, qy, qz, ix, iy, iz, fx, fy, fz)) return {false, 0.0f};
    return sample_cell(a, ix, iy, iz, fx, fy, fz);
}

struct Ray {
    float q0[3], dq[3];  // lattice coordinates of depth z: fma(z, dq, q0)
    float step, dmin;
    __device__ __forceinline__ float depth(int k) const { return __fmaf_rn((float)k, step, dmin); }
    __device__ __forceinline__ float at(int axis, float z) const { return __fmaf_rn(z, dq[axis], q0[axis]); }
};

// NaN-safe float -> sample index in [lo, K_CAP]
__device__ __forceinline__ int index_of(float v, int lo) { return (int)fminf(fmaxf(v, (float)lo), (float)K_CAP); }

__global__ void __launch_bounds__(256) tsdf_raycast_kernel(RaycastArgs a) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const unsigned v = blockIdx.z;
    if (x >= a.W || y >= a.H) return;
    const float* __restrict__ m = a.view + (size_t)v * 16;  // W2C^T: R[j][i] at [4 i + j], t[j] at [12 + j]
    const float r00 = m[0], r01 = m[4], r02 = m[8], r10 = m[1], r11 = m[5], r12 = m[9], r20 = m[2], r21 = m[6], r22 = m[10];
    const float t0 = m[12], t1 = m[13], t2 = m[14];
    const float dcx = ((float)x - a.cx) / a.fx, dcy = ((float)y - a.cy) / a.fy;
    // p_w = R^T (z d_c - t) = o_w + z dir_w
    const float dirw[3] = {r00 * dcx + r10 * dcy + r20, r01 * dcx + r11 * dcy + r21, r02 * dcx + r12 * dcy + r22};
    const float ow[3] = {-(r00 * t0 + r10 * t1 + r20 * t2), -(r01 * t0 + r11 * t1 + r21 * t2), -(r02 * t0 + r12 * t1 + r22 * t2)};
    const float org[3] = {a.ox, a.oy, a.oz};
    const int n[3] = {a.nx, a.ny, a.nz};
    Ray ray;
    ray.step = a.step, ray.dmin = a.depth_min;
    bool finite = true;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        ray.q0[ax] = (ow[ax] - org[ax]) / a.voxel;
        ray.dq[ax] = dirw[ax] / a.voxel;
        finite = finite && fabsf(ray.q0[ax]) < INFINITY && fabsf(ray.dq[ax]) < INFINITY;  // (false on a NaN)
    }

    int kstar = -1;  // the smallest k whose sample is valid with F <= 0
    float Fstar = 0.0f;
    if (finite) {  // (otherwise every sample's coordinates are NaN or infinite: invalid, a miss)
        // the slab test: where the ray enters the cell range [0, n - 1) of every axis
        float enter = -INFINITY;
        bool never = false;
        float rdq[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            rdq[ax] = 1.0f / ray.dq[ax];
            if (ray.dq[ax] == 0.0f) never = never || !(ray.q0[ax] >= 0.0f && ray.q0[ax] < (float)(n[ax] - 1));
            else enter = fmaxf(enter, ((ray.dq[ax] > 0.0f ? 0.0f : (float)(n[ax] - 1)) - ray.q0[ax]) * rdq[ax]);
        }
        const float rstep = 1.0f / a.step;
        int k = index_of(floorf((enter - a.depth_min) * rstep) - 2.0f, 0);
        if (k > 0) {  // sample k - 1 must lie outside on an entry side
            const float z = ray.depth(k - 1);
            bool before = false;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float q = ray.at(ax, z);
                before = before || (ray.dq[ax] >= 0.0f && q < 0.0f) || (ray.dq[ax] <= 0.0f && floorf(q) > (float)(n[ax] - 2));
            }
            if (!before) k = 0;
        }
        const int bnx = (a.nx - 1 + BRICK - 1) >> BRICK_SHIFT, bny = (a.ny - 1 + BRICK - 1) >> BRICK_SHIFT;
        while (!never && k < K_CAP) {
            const float z = ray.depth(k);
            if (!(z < a.depth_max)) break;
            const float qx = ray.at(0, z), qy = ray.at(1, z), qz = ray.at(2, z);
            int ix, iy, iz;
            float fx, fy, fz;
            if (!cell_of(a, qx, qy, qz, ix, iy, iz, fx, fy, fz)) {
                // outside on a side the ray leaves through: so is every later sample
                const float q[3] = {qx, qy, qz};
                bool behind = false;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax)
                    behind = behind || (ray.dq[ax] >= 0.0f && floorf(q[ax]) > (float)(n[ax] - 2)) || (ray.dq[ax] <= 0.0f && q[ax] < 0.0f);
                if (behind) break;
                ++k;
                continue;
            }
            if (a.bricks) {
                const int bx = ix >> BRICK_SHIFT, by = iy >> BRICK_SHIFT, bz = iz >> BRICK_SHIFT;
                if (a.bricks[((size_t)bz * (unsigned)bny + (unsigned)by) * (unsigned)bnx + (unsigned)bx] == 0) {
                    // a dead brick: the candidate for the last sample inside it, checked from its own index
                    const int b[3] = {bx, by, bz};
                    float leave = INFINITY;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax)
                        if (ray.dq[ax] != 0.0f)
                            leave = fminf(leave, ((float)((b[ax] + (ray.dq[ax] > 0.0f ? 1 : 0)) * BRICK) - ray.q0[ax]) * rdq[ax]);
                    const int kc = index_of(floorf((leave - a.depth_min) * rstep) - 1.0f, 0);
                    int next = k + 1;
                    if (kc > k && kc < K_CAP) {
                        const float zc = ray.depth(kc);
                        bool same = true;
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) {
                            const float fl = floorf(ray.at(ax, zc));
                            same = same && fl >= (float)(b[ax] * BRICK) && fl < (float)((b[ax] + 1) * BRICK);
                        }
                        if (same) next = kc + 1;
                    }
                    k = next;
                    continue;
                }
            }
            const Sampled s = sample_cell(a, ix, iy, iz, fx, fy, fz);
            if (s.valid && s.F <= 0.0f) {
                kstar = k, Fstar = s.F;
                break;
            }
            ++k;
        }
    }

    unsigned flags = 0u;
    float depth = 0.0f;
    float4 vn = make_float4(0.f, 0.f, 0.f, 0.f);
    float col[3] = {0.f, 0.f, 0.f};
    if (kstar >= 0) {
        Sampled prev = {false, 0.0f};
        float zp = 0.0f;
        if (kstar >= 1) {
            zp = ray.depth(kstar - 1);
            prev = sample_at(a, ray.at(0, zp), ray.at(1, zp), ray.at(2, zp));
        }
        if (prev.valid && prev.F > 0.0f) {
            flags = 1u;
            // (not beyond sample k*: the last place of zp + step may differ from that of z_k*)
            depth = fminf(__fmaf_rn(a.step, prev.F / (prev.F - Fstar), zp), ray.depth(kstar));
            const float q[3] = {ray.at(0, depth), ray.at(1, depth), ray.at(2, depth)};
            if (a.vnmap || a.flags) {
                float g[3];
                bool ok = true;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const Sampled hi = sample_at(a, q[0] + (ax == 0 ? 1.0f : 0.0f), q[1] + (ax == 1 ? 1.0f : 0.0f), q[2] + (ax == 2 ? 1.0f : 0.0f));
                    const Sampled lo = sample_at(a, q[0] - (ax == 0 ? 1.0f : 0.0f), q[1] - (ax == 1 ? 1.0f : 0.0f), q[2] - (ax == 2 ? 1.0f : 0.0f));
                    ok = ok && hi.valid && lo.valid;
                    g[ax] = hi.F - lo.F;
                }
                const float len2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
                if (ok && len2 > 0.0f && len2 < INFINITY) {
                    const float len = sqrtf(len2);
                    const float gx = g[0] / len, gy = g[1] / len, gz = g[2] / len;
                    float c0 = r00 * gx + r01 * gy + r02 * gz, c1 = r10 * gx + r11 * gy + r12 * gz, c2 = r20 * gx + r21 * gy + r22 * gz;
                    if (c0 * (dcx * depth) + c1 * (dcy * depth) + c2 * depth > 0.0f) c0 = -c0, c1 = -c1, c2 = -c2;  // facing the camera
                    vn = make_float4(c0, c1, c2, depth);
                } else {
                    flags |= 4u;  // (the same whether the map or only the flags were asked for)
                }
            }
            if (a.color_out) {
                // p*'s cell: between two valid samples' cells on every axis; clamped (a NaN goes to 0) and bounded as integers
                int c[3];
                float f[3];
                bool inside = true;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const float fl = fminf(fmaxf(floorf(q[ax]), 0.0f), (float)(n[ax] - 2));
                    c[ax] = (int)fl;
                    f[ax] = q[ax] - fl;
                    inside = inside && c[ax] >= 0 && c[ax] <= n[ax] - 2;
                }
                if (inside) {
                    const size_t row = (size_t)(unsigned)a.nx, slab = row * (size_t)(unsigned)a.ny;
                    const float4* __restrict__ p = a.color + ((size_t)c[2] * slab + (size_t)c[1] * row + (size_t)c[0]);
                    const float4 c000 = p[0], c100 = p[1], c010 = p[row], c110 = p[row + 1];
                    const float4 c001 = p[slab], c101 = p[slab + 1], c011 = p[slab + row], c111 = p[slab + row + 1];
                    col[0] = lerp(f[2], lerp(f[1], lerp(f[0], c000.x, c100.x), lerp(f[0], c010.x, c110.x)),
                                  lerp(f[1], lerp(f[0], c001.x, c101.x), lerp(f[0], c011.x, c111.x)));
                    col[1] = lerp(f[2], lerp(f[1], lerp(f[0], c000.y, c100.y), lerp(f[0], c010.y, c110.y)),
                                  lerp(f[1], lerp(f[0], c001.y, c101.y), lerp(f[0], c011.y, c111.y)));
                    col[2] = lerp(f[2], lerp(f[1], lerp(f[0], c000.z, c100.z), lerp(f[0], c010.z, c110.z)),
                                  lerp(f[1], lerp(f[0], c001.z, c101.z), lerp(f[0], c011.z, c111.z)));
                }
            }
        } else {
            flags = 2u;
        }
    }
    const size_t pixels = (size_t)(unsigned)a.W * (size_t)(unsigned)a.H;
    const size_t pix = (size_t)(unsigned)y * (unsigned)a.W + (unsigned)x, at = (size_t)v * pixels + pix;
    if (a.depth) a.depth[at] = depth;
    if (a.vnmap) a.vnmap[at] = vn;
    if (a.color_out) {
        float* __restrict__ o = a.color_out + (size_t)v * 3 * pixels + pix;
        o[0] = col[0], o[pixels] = col[1], o[2 * pixels] = col[2];
    }
    if (a.flags) a.flags[at] = (unsigned char)flags;
}

__global__ void __launch_bounds__(256) tsdf_bricks_kernel(BricksArgs a) {
    __shared__ unsigned char bits[9 * 9 * 9];  // bit 0: weight >= min_weight, bit 1: tsdf <= 0
    const int tid = threadIdx.x;
    const unsigned bx = blockIdx.x % a.bnx, byz = blockIdx.x / a.bnx, by = byz % a.bny, bz = byz / a.bny;
    for (int i = tid; i < 729; i += 256) {
        const int lx = i % 9, ly = (i / 9) % 9, lz = i / 81;
        const int sx = (int)(bx * BRICK) + lx, sy = (int)(by * BRICK) + ly, sz = (int)(bz * BRICK) + lz;
        unsigned char b = 0;
        if (sx < a.nx && sy < a.ny && sz < a.nz) {
            const float2 tw = a.volume[((size_t)sz * (unsigned)a.ny + (unsigned)sy) * (unsigned)a.nx + (unsigned)sx];
            b = (unsigned char)((tw.y >= a.min_weight ? 1 : 0) | (tw.x <= 0.0f ? 2 : 0));  // (both false on a NaN)
        }
        bits[i] = b;
    }
    __syncthreads();
    int live = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = tid + 256 * j, cx = c & 7, cy = (c >> 3) & 7, cz = c >> 6;
        unsigned all = 1u, any = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned b = bits[(cz + (k >> 2)) * 81 + (cy + ((k >> 1) & 1)) * 9 + cx + (k & 1)];
            all &= b, any |= b;
        }
        live |= (int)(all & (any >> 1) & 1u);
    }
    live = __syncthreads_or(live);
    if (tid == 0) a.bricks[blockIdx.x] = live ? 1 : 0;
}

}  // namespace

size_t tsdf_brick_count(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    return (size_t)((nx - 1 + BRICK - 1) / BRICK) * (size_t)((ny - 1 + BRICK - 1) / BRICK) * (size_t)((nz - 1 + BRICK - 1) / BRICK);
}

hipError_t launch_tsdf_bricks(const BricksArgs& args, hipStream_t stream) {
    BricksArgs a = args;
    const size_t count = tsdf_brick_count(a.nx, a.ny, a.nz);
    if (count == 0) return hipSuccess;
    a.bnx = (unsigned)((a.nx - 1 + BRICK - 1) / BRICK), a.bny = (unsigned)((a.ny - 1 + BRICK - 1) / BRICK);
    launch(tsdf_bricks_kernel, dim3((unsigned)count), dim3(256), stream, a);
    return hipGetLastError();
}

hipError_t launch_tsdf_raycast(const RaycastArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.W + 15) / 16), (unsigned)((a.H + 15) / 16), (unsigned)a.V);
    launch(tsdf_raycast_kernel, grid, dim3(256), stream, a);
    return hipGetLastError();
}

}  // namespace dgr
