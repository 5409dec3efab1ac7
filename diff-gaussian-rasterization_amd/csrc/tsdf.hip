// tsdf.hip -- TSDF fusion of rendered views and mesh extraction (include/dgr_hip.h: dgr_tsdf_integrate, dgr_mesh_plan,
// dgr_mesh_emit), gfx950, wave64.
//
// The volume is a dense lattice of Nx x Ny x Nz samples, x fastest: `volume` float2 (tsdf, weight) and `color` float4 (r, g, b, 0)
// per sample.  The step is memory-bound, and what it is built around is how often the volume crosses HBM: ONCE per call, whatever
// the number of views.
//
// integrate: one launch.  A 256-thread workgroup owns a brick of 64 x 4 x 1 samples, a wave one row of 64 along x (8-byte and
//   16-byte accesses per lane, consecutive lanes consecutive addresses); ONE thread owns a sample, reads it once, applies the views
//   in index order in registers and writes it at most once -- not at all when no view updated it.  No atomics: the same bits on
//   every run.  Poses and scalars are kernel arguments or loads at wave-uniform addresses (scalar loads).
//   Brick culling: thread t of the workgroup tests view t (+ 256, ...) against the brick's four corners -- behind `near`, or outside
//   one of the image's four side planes, each with a margin for the rounding of the per-sample arithmetic -- and the waves' ballots
//   give the list of views the brick can see.  A brick no view sees leaves before it loads anything; the others walk only their
//   live views (a wave-uniform loop over the set bits).
// mesh: marching tetrahedra on Kuhn's split of a cell into six tetrahedra {0, a, a|b, 7} (corner = bits x 1, y 2, z 4).  The case
//   table is generated at compile time (mesh_table below) from integer geometry: no table is copied from anywhere.
//   count: a thread per cell, a block's triangles into its total.   scan: plan.h's one-workgroup scan; writes count and flags.
//   emit: recompute the cell, rank inside the block, write the triangles that fit.  Order: cell, tetrahedron, triangle.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "kernels.h"
#include "plan.h"

namespace dgr {
namespace {

constexpr int BRICK_X = 64, BRICK_Y = 4;  // a workgroup's samples: a wave per row

// p_c = W2C p_w from the 16 floats of W2C^T (R[j][i] at [4 i + j], t[j] at [12 + j]); the one form both the culling and the
// samples use
struct Pose {
    float r00, r01, r02, r10, r11, r12, r20, r21, r22, t0, t1, t2;
};
__device__ __forceinline__ Pose load_pose(const float* __restrict__ m) {
    return {m[0], m[4], m[8], m[1], m[5], m[9], m[2], m[6], m[10], m[12], m[13], m[14]};
}

// Whether the brick whose lattice corners are (x0 | x1, y0 | y1, z) cannot be updated by the view: every sample fails `z > near`,
// or every sample lands outside the same side of the image.  p_c is linear in p_w, so what holds at the four corners holds between
// them; the margins cover the rounding of the samples' own float arithmetic (a few ulp of the largest term: 1e-5 of the terms'
// absolute sum is twenty times that), and the side planes keep one pixel more.  The side planes need z > 0 of every sample that
// passes the near test, hence near >= 0.  Every comparison is false on a NaN: a NaN pose culls nothing.
__device__ inline bool view_misses_brick(const TsdfIntegrateArgs& a, const Pose& P, float x0, float x1, float y0, float y1, float z) {
    bool behind = true, left = true, right = true, above = true, below = true;
    const float cl = a.cx + 1.5f, cr = a.cx - 0.5f - (float)a.W, ct = a.cy + 1.5f, cb = a.cy - 0.5f - (float)a.H;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float x = c & 1 ? x1 : x0, y = c & 2 ? y1 : y0;
        const float X = P.r00 * x + P.r01 * y + P.r02 * z + P.t0, Y = P.r10 * x + P.r11 * y + P.r12 * z + P.t1;
        const float Z = P.r20 * x + P.r21 * y + P.r22 * z + P.t2;
        const float mx = 1e-5f * (fabsf(P.r00 * x) + fabsf(P.r01 * y) + fabsf(P.r02 * z) + fabsf(P.t0));
        const float my = 1e-5f * (fabsf(P.r10 * x) + fabsf(P.r11 * y) + fabsf(P.r12 * z) + fabsf(P.t1));
        const float mz = 1e-5f * (fabsf(P.r20 * x) + fabsf(P.r21 * y) + fabsf(P.r22 * z) + fabsf(P.t2));
        const float sx = 2.0f * (a.fx * mx + (fabsf(a.cx) + (float)a.W + 2.0f) * mz + 1e-5f * (a.fx * fabsf(X) + (fabsf(a.cx) + (float)a.W + 2.0f) * fabsf(Z)));
        const float sy = 2.0f * (a.fy * my + (fabsf(a.cy) + (float)a.H + 2.0f) * mz + 1e-5f * (a.fy * fabsf(Y) + (fabsf(a.cy) + (float)a.H + 2.0f) * fabsf(Z)));
        behind = behind && (Z + mz <= a.near_z);
        left = left && (a.fx * X + cl * Z < -sx);
        right = right && (a.fx * X + cr * Z > sx);
        above = above && (a.fy * Y + ct * Z < -sy);
        below = below && (a.fy * Y + cb * Z > sy);
    }
    return behind || (a.near_z >= 0.0f && (left || right || above || below));
}

template <bool COLOR>
__global__ void __launch_bounds__(256) tsdf_integrate_kernel(TsdfIntegrateArgs a) {
    __shared__ unsigned long long live[4];  // of a chunk of 256 views: the ones this brick can see
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned bx = blockIdx.x % a.bricks_x, byz = blockIdx.x / a.bricks_x;
    const unsigned by = byz % a.bricks_y, iz = byz / a.bricks_y;
    const int ix = (int)(bx * BRICK_X) + lane, iy = (int)(by * BRICK_Y) + wave;
    const bool mine = ix < a.nx && iy < a.ny;
    const size_t s = ((size_t)iz * (unsigned)a.ny + (unsigned)iy) * (unsigned)a.nx + (unsigned)ix;
    // the brick's corners (those of the lattice where the brick hangs over its edge)
    const float cx0 = a.ox + a.voxel * (float)(bx * BRICK_X), cx1 = a.ox + a.voxel * (float)min((int)(bx * BRICK_X) + BRICK_X - 1, a.nx - 1);
    const float cy0 = a.oy + a.voxel * (float)(by * BRICK_Y), cy1 = a.oy + a.voxel * (float)min((int)(by * BRICK_Y) + BRICK_Y - 1, a.ny - 1);
    const float pz = a.oz + a.voxel * (float)iz;
    const float px = a.ox + a.voxel * (float)ix, py = a.oy + a.voxel * (float)iy;
    const size_t pixels = (size_t)a.W * (size_t)a.H;

    float2 tw = make_float2(0.f, 0.f);
    float4 col = make_float4(0.f, 0.f, 0.f, 0.f);
    bool loaded = false, touched = false;
    for (int v0 = 0; v0 < a.V; v0 += 256) {
        bool sees = false;
        if (v0 + tid < a.V) sees = !view_misses_brick(a, load_pose(a.view + (size_t)(v0 + tid) * 16), cx0, cx1, cy0, cy1, pz);
        const unsigned long long b = __ballot(sees);
        if (v0 > 0) __syncthreads();  // (the previous chunk's masks have been read)
        if (lane == 0) live[wave] = b;
        __syncthreads();
#pragma unroll 1
        for (int w = 0; w < 4; ++w) {
            const unsigned long long lw = live[w];  // (wave-uniform: the loop below is scalar control flow)
            unsigned long long m = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(lw >> 32)) << 32 |
                                   (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)lw);
            if (m != 0ull && !loaded) {  // the first live view: now the sample is worth its load
                loaded = true;
                if (mine) {
                    tw = a.volume[s];
                    if (COLOR) col = a.color[s];
                }
            }
            while (m != 0ull) {
                const int bit = __builtin_ctzll(m);
                m &= m - 1ull;
                const int v = __builtin_amdgcn_readfirstlane(v0 + 64 * w + bit);
                const Pose P = load_pose(a.view + (size_t)v * 16);
                const float z = P.r20 * px + P.r21 * py + P.r22 * pz + P.t2;
                if (!mine || !(z > a.near_z)) continue;
                const float X = P.r00 * px + P.r01 * py + P.r02 * pz + P.t0, Y = P.r10 * px + P.r11 * py + P.r12 * pz + P.t1;
                const float rz = __builtin_amdgcn_rcpf(z);
                const float fu = floorf(a.fx * X * rz + a.cx + 0.5f), fv = floorf(a.fy * Y * rz + a.cy + 0.5f);
                if (!(fu >= 0.0f && fu < (float)a.W && fv >= 0.0f && fv < (float)a.H)) continue;  // (false on a NaN)
                const int qx = (int)fu, qy = (int)fv;
                if ((unsigned)qx >= (unsigned)a.W || (unsigned)qy >= (unsigned)a.H) continue;  // (the gather's own bound, in integers)
                const size_t q = (size_t)v * pixels + (size_t)qy * (unsigned)a.W + (unsigned)qx;
                const float d = a.depth[q];
                if (!(d > a.depth_min && d < a.depth_max)) continue;
                if (a.mask && a.mask[q] <= a.mask_threshold) continue;
                const float sdf = d - z;
                if (sdf < -a.truncation) continue;
                const float t = fminf(1.0f, sdf / a.truncation);
                const float wn = tw.y + a.weight;
                tw.x = (tw.x * tw.y + t * a.weight) / wn;
                if (COLOR) {
                    const float* __restrict__ im = a.image + (size_t)v * 3 * pixels + (size_t)qy * (unsigned)a.W + (unsigned)qx;
                    col.x = (col.x * tw.y + im[0] * a.weight) / wn;
                    col.y = (col.y * tw.y + im[pixels] * a.weight) / wn;
                    col.z = (col.z * tw.y + im[2 * pixels] * a.weight) / wn;
                }
                tw.y = fminf(wn, a.max_weight);
                touched = true;
            }
        }
    }
    if (touched) {
        a.volume[s] = tw;
        if (COLOR) a.color[s] = col;
    }
}

// ---- marching tetrahedra

constexpr int MESH_TETS = 6;
// tetrahedron k = {0, a, a | b, 7} with (a, b) = (1, 2), (1, 4), (2, 1), (2, 4), (4, 1), (4, 2)
__host__ __device__ constexpr int tet_a(int k) { return 1 << (k >> 1); }
__host__ __device__ constexpr int tet_b(int k) { return 1 << ((k & 1) ? ((k >> 1) == 2 ? 1 : 2) : ((k >> 1) == 0 ? 1 : 0)); }

// One triangle = three cell edges, an edge = (A, B) with A < B (corner numbers): 6 bits per edge, 18 per triangle.
struct MeshTable {
    unsigned tri[MESH_TETS][16][2];
};
constexpr int corner_coord(int c, int axis) { return (c >> axis) & 1; }
// 6 x the signed volume of (q - p, r - p, s - p)
constexpr int corner_det(int p, int q, int r, int s) {
    int m[3][3] = {};
    const int o[3] = {q, r, s};
    for (int i = 0; i < 3; ++i)
        for (int ax = 0; ax < 3; ++ax) m[i][ax] = corner_coord(o[i], ax) - corner_coord(p, ax);
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}
constexpr unsigned edge_code(int p, int q) { return p < q ? (unsigned)(p * 8 + q) : (unsigned)(q * 8 + p); }
// The polygon of a case, as a cycle of edges whose normal points away from the inside corners, rotated so that the smallest edge
// code comes first, and fanned from there: (e0, e1, e2) and, for a quadrilateral, (e0, e2, e3).
//   one corner s apart from the other three (p, q, r): the triangle (sp, sq, sr), with det(s; p, q, r) > 0 iff s is the inside one;
//   two inside (p, q), two outside (r, s): the cycle pr, ps, qs, qr (neighbours share a corner), turned so that the normal of
//   (pr, ps, qs) -- with the crossings at the edges' midpoints (s - r) x (q - p) / 4 -- has a positive component along
//   r + s - p - q.  (Integer geometry of the unit cell: the level set of the tetrahedron's linear interpolant is a plane that
//   separates the inside corners from the outside ones wherever the crossings lie, so a case's orientation is that of its midpoints.)
constexpr MeshTable mesh_table() {
    MeshTable T = {};
    for (int k = 0; k < MESH_TETS; ++k) {
        const int c[4] = {0, tet_a(k), tet_a(k) | tet_b(k), 7};
        for (int m = 1; m < 15; ++m) {
            int in[4] = {}, out[4] = {}, n_in = 0, n_out = 0;
            for (int i = 0; i < 4; ++i) {
                if ((m >> i) & 1) in[n_in++] = c[i];
                else out[n_out++] = c[i];
            }
            unsigned e[4] = {};
            int n = 3;
            if (n_in == 2) {
                n = 4;
                const int p = in[0], q = in[1], r = out[0], s = out[1];
                // n = (s - r) x (q - p), w = r + s - p - q: the sign of n . w
                int a3[3] = {}, b3[3] = {}, w3[3] = {};
                for (int ax = 0; ax < 3; ++ax) {
                    a3[ax] = corner_coord(s, ax) - corner_coord(r, ax);
                    b3[ax] = corner_coord(q, ax) - corner_coord(p, ax);
                    w3[ax] = corner_coord(r, ax) + corner_coord(s, ax) - corner_coord(p, ax) - corner_coord(q, ax);
                }
                const int d = w3[0] * (a3[1] * b3[2] - a3[2] * b3[1]) + w3[1] * (a3[2] * b3[0] - a3[0] * b3[2]) +
                              w3[2] * (a3[0] * b3[1] - a3[1] * b3[0]);
                e[0] = edge_code(p, r), e[1] = edge_code(p, s), e[2] = edge_code(q, s), e[3] = edge_code(q, r);
                if (d < 0) { const unsigned t = e[1]; e[1] = e[3]; e[3] = t; }
            } else {
                const bool lone_in = n_in == 1;
                const int s = lone_in ? in[0] : out[0];
                const int* o = lone_in ? out : in;
                e[0] = edge_code(s, o[0]), e[1] = edge_code(s, o[1]), e[2] = edge_code(s, o[2]);
                if ((corner_det(s, o[0], o[1], o[2]) > 0) != lone_in) { const unsigned t = e[1]; e[1] = e[2]; e[2] = t; }
            }
            int first = 0;
            for (int i = 1; i < n; ++i)
                if (e[i] < e[first]) first = i;
            unsigned r4[4] = {};
            for (int i = 0; i < n; ++i) r4[i] = e[(first + i) % n];
            T.tri[k][m][0] = r4[0] | r4[1] << 6 | r4[2] << 12;
            T.tri[k][m][1] = n == 4 ? (r4[0] | r4[2] << 6 | r4[3] << 12) : 0u;
        }
    }
    return T;
}
__constant__ const MeshTable MESH_TABLE = mesh_table();

struct MeshBlock {  // the record of plan.h's scan_block_totals: a block's triangles, after the scan the triangles in front of it
    long long n;
};
__device__ inline MeshBlock totals_zero(const MeshBlock*) { return {0ll}; }
__device__ inline MeshBlock totals_add(MeshBlock a, MeshBlock b) { return {a.n + b.n}; }
__device__ inline MeshBlock totals_sub(MeshBlock a, MeshBlock b) { return {a.n - b.n}; }
__device__ inline MeshBlock totals_shfl_up(MeshBlock v, int d) {
    const unsigned lo = __shfl_up((unsigned)v.n, d), hi = __shfl_up((unsigned)((unsigned long long)v.n >> 32), d);
    return {(long long)((unsigned long long)hi << 32 | lo)};
}

struct MeshCell {
    size_t base;       // the sample of corner 0
    int x, y, z;       // its lattice index
    unsigned inside;   // bit c: corner c has tsdf < 0; 0 for an invalid cell (a cell without a crossing emits nothing either)
    int triangles;
};
// corner c of the cell at sample `base`
__device__ __forceinline__ size_t corner_sample(const MeshArgs& a, size_t base, int c) {
    return base + (c & 1) + (c & 2 ? (size_t)a.nx : 0) + (c & 4 ? (size_t)a.nx * (size_t)a.ny : 0);
}
__device__ inline MeshCell mesh_cell(const MeshArgs& a, size_t cell) {
    MeshCell r;
    const unsigned cxn = (unsigned)a.nx - 1u, cyn = (unsigned)a.ny - 1u;  // (32-bit divisions: the cells are fewer than 2^31)
    const unsigned row = (unsigned)cell / cxn;
    r.x = (int)((unsigned)cell - row * cxn);
    r.z = (int)(row / cyn);
    r.y = (int)(row - (unsigned)r.z * cyn);
    r.base = ((size_t)r.z * (unsigned)a.ny + (unsigned)r.y) * (unsigned)a.nx + (unsigned)r.x;
    bool valid = true;
    unsigned inside = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float2 tw = a.volume[corner_sample(a, r.base, c)];
        valid = valid && tw.y >= a.min_weight;  // (false on a NaN weight)
        inside |= tw.x < 0.0f ? 1u << c : 0u;
    }
    r.inside = valid ? inside : 0u;
    r.triangles = 0;
    if (r.inside != 0u && r.inside != 255u) {
#pragma unroll
        for (int k = 0; k < MESH_TETS; ++k) {
            const int c1 = tet_a(k), c2 = tet_a(k) | tet_b(k);
            const int n = (int)(r.inside & 1u) + (int)((r.inside >> c1) & 1u) + (int)((r.inside >> c2) & 1u) + (int)(r.inside >> 7);
            r.triangles += n == 2 ? 2 : (n == 1 || n == 3) ? 1 : 0;
        }
    }
    return r;
}

__global__ void __launch_bounds__(256) mesh_count_kernel(MeshArgs a, MeshBlock* __restrict__ table) {
    __shared__ uint32_t wsum[4];
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int n = cell < a.cells ? mesh_cell(a, cell).triangles : 0;
    uint32_t total;
    block_exclusive_scan<256>((uint32_t)n, wsum, (int)threadIdx.x, &total);
    if (threadIdx.x == 0) table[blockIdx.x] = {(long long)total};
}

__global__ void __launch_bounds__(256) mesh_scan_kernel(MeshBlock* __restrict__ table, size_t blocks, int max_triangles,
                                                        int* __restrict__ count, int* __restrict__ flags) {
    __shared__ MeshBlock wave_sum[4];
    const MeshBlock all = scan_block_totals(table, blocks, wave_sum);
    if (threadIdx.x == 0) {
        count[0] = (int)(all.n < 0x7fffffffll ? all.n : 0x7fffffffll);
        flags[0] = all.n > (long long)max_triangles ? 1 : 0;
    }
}

// the crossing of edge `code` = (A, B), A < B: t = v_A / (v_A - v_B), p_A + t (p_B - p_A); explicit roundings, so that every cell
// that shares the edge writes the same bits
template <bool COLOR>
__device__ __forceinline__ void mesh_vertex(const MeshArgs& a, const MeshCell& c, unsigned code, float* __restrict__ vout,
                                            float* __restrict__ cout) {
    const int A = (int)(code >> 3) & 7, B = (int)code & 7;
    const size_t sa = corner_sample(a, c.base, A), sb = corner_sample(a, c.base, B);
    const float va = a.volume[sa].x, vb = a.volume[sb].x;
    const float t = __fdiv_rn(va, __fsub_rn(va, vb));
    const float o[3] = {a.ox, a.oy, a.oz};
    const int i0[3] = {c.x, c.y, c.z};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const float pa = __fmaf_rn(a.voxel, (float)(i0[ax] + ((A >> ax) & 1)), o[ax]);
        const float pb = __fmaf_rn(a.voxel, (float)(i0[ax] + ((B >> ax) & 1)), o[ax]);
        vout[ax] = __fmaf_rn(t, __fsub_rn(pb, pa), pa);
    }
    if (COLOR) {
        const float4 ca = a.color[sa], cb = a.color[sb];
        cout[0] = __fmaf_rn(t, __fsub_rn(cb.x, ca.x), ca.x);
        cout[1] = __fmaf_rn(t, __fsub_rn(cb.y, ca.y), ca.y);
        cout[2] = __fmaf_rn(t, __fsub_rn(cb.z, ca.z), ca.z);
    }
}

template <bool COLOR>
__global__ void __launch_bounds__(256) mesh_emit_kernel(MeshArgs a, const MeshBlock* __restrict__ table, int max_triangles,
                                                        float* __restrict__ vertices, float* __restrict__ colors) {
    __shared__ uint32_t wsum[4];
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    MeshCell c;
    c.triangles = 0;
    if (cell < a.cells) c = mesh_cell(a, cell);
    uint32_t total;
    const uint32_t rank = block_exclusive_scan<256>((uint32_t)c.triangles, wsum, (int)threadIdx.x, &total);
    if (c.triangles == 0) return;
    long long tri = table[blockIdx.x].n + (long long)rank;
#pragma unroll 1
    for (int k = 0; k < MESH_TETS; ++k) {
        const int c1 = tet_a(k), c2 = tet_a(k) | tet_b(k);
        const unsigned m = (c.inside & 1u) | ((c.inside >> c1) & 1u) << 1 | ((c.inside >> c2) & 1u) << 2 | (c.inside >> 7) << 3;
        if (m == 0u || m == 15u) continue;
        const int n = __popc(m) == 2 ? 2 : 1;
        for (int j = 0; j < n; ++j, ++tri) {
            if (tri >= (long long)max_triangles) return;  // (ascending: nothing behind it fits either)
            const unsigned packed = MESH_TABLE.tri[k][m][j];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const size_t at = ((size_t)tri * 3 + e) * 3;
                mesh_vertex<COLOR>(a, c, (packed >> (6 * e)) & 63u, vertices + at, COLOR ? colors + at : nullptr);
            }
        }
    }
}

}  // namespace

hipError_t launch_tsdf_integrate(const TsdfIntegrateArgs& args, hipStream_t stream) {
    TsdfIntegrateArgs a = args;
    a.bricks_x = ((unsigned)a.nx + BRICK_X - 1) / BRICK_X;
    a.bricks_y = ((unsigned)a.ny + BRICK_Y - 1) / BRICK_Y;
    const dim3 grid(a.bricks_x * a.bricks_y * (unsigned)a.nz);  // (below 2^31: the samples are)
    if (a.color) launch(tsdf_integrate_kernel<true>, grid, dim3(256), stream, a);
    else launch(tsdf_integrate_kernel<false>, grid, dim3(256), stream, a);
    return hipGetLastError();
}

size_t mesh_cells(int nx, int ny, int nz) { return nx < 2 || ny < 2 || nz < 2 ? 0 : (size_t)(nx - 1) * (size_t)(ny - 1) * (size_t)(nz - 1); }
size_t mesh_scratch_bytes(int nx, int ny, int nz) { return 16 + plan_blocks(mesh_cells(nx, ny, nz)) * sizeof(MeshBlock); }

hipError_t launch_mesh_plan(const MeshArgs& args, int max_triangles, void* scratch, int* count, int* flags, hipStream_t stream) {
    MeshArgs a = args;
    a.cells = mesh_cells(a.nx, a.ny, a.nz);
    const size_t blocks = plan_blocks(a.cells);
    MeshBlock* table = reinterpret_cast<MeshBlock*>(static_cast<char*>(scratch) + 16);
    if (blocks > 0) {
        launch(mesh_count_kernel, dim3((unsigned)blocks), dim3(256), stream, a, table);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    launch(mesh_scan_kernel, dim3(1), dim3(256), stream, table, blocks, max_triangles, count, flags);
    return hipGetLastError();
}

hipError_t launch_mesh_emit(const MeshArgs& args, int max_triangles, const void* scratch, float* vertices, float* colors,
                            hipStream_t stream) {
    MeshArgs a = args;
    a.cells = mesh_cells(a.nx, a.ny, a.nz);
    const size_t blocks = plan_blocks(a.cells);
    if (blocks == 0 || max_triangles <= 0) return hipSuccess;
    const MeshBlock* table = reinterpret_cast<const MeshBlock*>(static_cast<const char*>(scratch) + 16);
    if (colors) launch(mesh_emit_kernel<true>, dim3((unsigned)blocks), dim3(256), stream, a, table, max_triangles, vertices, colors);
    else launch(mesh_emit_kernel<false>, dim3((unsigned)blocks), dim3(256), stream, a, table, max_triangles, vertices, colors);
    return hipGetLastError();
}

}  // namespace dgr
