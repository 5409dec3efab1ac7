// contrib.hip -- per-Gaussian contribution statistics of a rendered view (include/dgr_hip.h: dgr_contribution_stats), gfx950.
//
// A REPLAY of a finished forward's blend, light or full, beside the blend kernels rather than inside them: the forward left the
// tile ranges, the sorted list, the 64-byte records, n_contrib and the contribution tag bytes (render_common.h), and from those
// every (pixel, list position) pair the forward blended can be named again without a termination test:
//     blended  <=>  position <= n_contrib[pixel]  &&  power <= 0  &&  min(0.99, o G) >= ALPHA_MIN
// (the light forward does not blend the entry that ends a pixel, and that entry lies behind n_contrib; the full forward blends
// it, and it IS n_contrib).  alpha comes from pair_p2<AM> / alpha_raw<AM>, the blend kernels' own functions, and the weight
// w = alpha T with T the running product of (1 - alpha) over the pixel's earlier blended pairs, contraction off: the forward's bits.
// Per Gaussian: n_touched = blended pairs (int32), max_weight = largest w (float32), sum_weight = sum of floor(w 2^32) (int64).
//
// Shape (render_light.hip has the family's): one 256-thread workgroup per tile through blend_slot (the frame's schedule applies),
// wave = 8x8 quadrant through tile_pixel, the list staged 256 positions at a time.  The tag bytes are an optimisation only: an
// entry with tag 0 is not loaded, and build_lists hands each wave the entries whose quadrant bits are set (both half bits folded,
// so a forward that walked quadrant lists and one that walked half-wave lists give the same lists here); the per-pair test above
// decides.  Every loop is bounded: batches by min(list length, the tile's largest n_contrib), the pair loop by the wave's list of the batch
// (<= 256) and by the wave's own largest n_contrib.
// Per listed entry a wave reduces in registers (a ballot's popcount, a max of the weights' bits -- w >= 0, so unsigned order is
// float order -- and the Q32 sum as two 16-bit halves, 64 x 65535 < 2^32 each; DPP only) and lane 63 merges the four waves with three LDS
// INTEGER atomics; behind the batch the thread that staged an entry with a nonzero count issues three global integer atomics
// (add, max, 64-bit add): 16 bytes per live (tile, Gaussian) instance, no float atomic anywhere, so the same bits on every run.
// alpha_mode 0, 1 and 2 (alpha_raw<ALPHA_GLIBC> with the workgroup's table) are all supported.
//
// Three launches: contrib_clear_kernel (the per-view arrays and counts), contrib_tiles_kernel, contrib_fold_kernel (counts, and the
// caller's running accumulators -- skipped for a frame whose binning overflowed: its lists are empty, its per-view outputs zero).
#include "render_common.h"

namespace dgr {
namespace {

struct ContribBatch {
    StagedT<DGR_TILE_PIX, unsigned short, 4, true> f;
    uint32_t cnt[DGR_TILE_PIX];            // per staged entry: blended pairs,
    uint32_t mx[DGR_TILE_PIX];             //   the bits of the largest weight,
    unsigned long long sum[DGR_TILE_PIX];  //   the Q32 sum
    int wave_last[4];                      // per quadrant wave: its largest n_contrib
    uint64_t exptab[32];                   // ALPHA_GLIBC: exact_math.h
};

// A wave64 reduction of unsigned values (add or max: 0 is the identity of both) that leaves the result in lane 63.  All DPP, no LDS
// and no scalar code: inside a 16-lane row quad xor 1, quad xor 2, row_half_mirror, row_mirror (every lane of the row then holds
// the row's result), then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3.  Every lane of the wave is active here.
// (ds_bpermute shuffles, 18 per listed entry for the three values, cost the tiles kernel a third of its time: profiles/contrib/)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
template <class OP>
__device__ __forceinline__ uint32_t to_lane63(uint32_t v, OP op) {
    v = op(v, dpp_u32<DPP_QUAD_XOR1, 0xf>(v));
    v = op(v, dpp_u32<DPP_QUAD_XOR2, 0xf>(v));
    v = op(v, dpp_u32<DPP_ROW_HALF_MIRROR, 0xf>(v));
    v = op(v, dpp_u32<DPP_ROW_MIRROR, 0xf>(v));
    v = op(v, dpp_u32<0x142, 0xa>(v));  // row_bcast:15
    v = op(v, dpp_u32<0x143, 0xc>(v));  // row_bcast:31
    return v;
}

template <int AM>
__global__ void __launch_bounds__(256) contrib_tiles_kernel(ContribTilesArgs a) {
    __shared__ ContribBatch sb;
    auto& s = sb.f;
    const int frame_flags = blend_flags(a.sched_flag);
    const uint4 slot = blend_slot(frame_flags, a.sched, a.ranges, a.grid_x * a.grid_y);  // {tile, list start, list end}
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const auto [tx, ty, px, py, inside, pix_id] = tile_pixel((int)slot.x, a.grid_x, a.W, a.H, wave, lane);
    const f2 pxy = {(float)px, (float)py};
    const int total = (int)(slot.z - slot.y);
    const int last = inside ? (int)a.n_contrib[pix_id] : 0;  // 1-based position of the pixel's last blended entry

    int wl = last;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wl = max(wl, __shfl_xor(wl, off, 64));
    if (lane == 0) sb.wave_last[wave] = wl;
    if (tid == 0) write_sentinel(s);
    if (AlphaPath<AM>::TABLE) exp_ref_table_fill(sb.exptab, tid);
    __syncthreads();
    const int wave_last = __builtin_amdgcn_readfirstlane(wl);
    // nothing behind the tile's largest n_contrib was blended (a tile nobody blended, an overflowed frame's empty lists: no batch)
    const int limit = __builtin_amdgcn_readfirstlane(min(total, max(max(sb.wave_last[0], sb.wave_last[1]), max(sb.wave_last[2], sb.wave_last[3]))));
    const uint8_t* const tag8 = half_tags(a.point_list, a.sched_flag) + slot.y;
    const uint32_t* const list = a.point_list + slot.y;

    float T = 1.0f;
    for (int base = 0; base < limit; base += DGR_TILE_PIX) {
        const int cnt = min(DGR_TILE_PIX, limit - base);
        unsigned code = 0;
        uint32_t gid = 0;
        if (tid < cnt) {
            code = fold8((unsigned)tag8[base + tid]);
            if (code != 0u) {  // (untagged entries are not loaded: nobody blended them)
                gid = list[base + tid] & ID_MASK;
                float4 q0, q1, q2;
                gather_record<AM>(a.rec, gid, s.rec[2 * tid], q0, q1, q2);
                s.rec[2 * tid + 1] = make_float4(-AlphaPath<AM>::PSCALE * q1.y, q0.w, __int_as_float(tid), 0.f);
            }
        }
        sb.cnt[tid] = 0u;
        sb.mx[tid] = 0u;
        sb.sum[tid] = 0ull;
        const int n = build_lists(s, code, tid, wave, lane);  // (two barriers: the records and the cleared cells are visible)

        // two entries per iteration, both records in flight before either is used (the list is padded with four sentinel entries,
        // whose record has opacity 0: never blended)
        for (int k = 0; k < n; k += 2) {
            const uint32_t pk = *reinterpret_cast<const uint32_t*>(&s.list[wave][k]);
            const int off2[2] = {__builtin_amdgcn_readfirstlane((int)(pk & 0xffffu)), __builtin_amdgcn_readfirstlane((int)(pk >> 16))};
            if (base + (off2[0] >> 5) >= wave_last) break;  // (list order: every later entry lies behind it too)
            float4 r0[2], r1[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                r0[u] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s.rec) + off2[u]);
                r1[u] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s.rec) + off2[u] + 16);
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int j = off2[u] >> 5;
                f2 dxy;
                const float p2 = pair_p2<AM>(r0[u], r1[u], pxy, dxy);
                const float oG = alpha_raw<AM, true>(r1[u].y, p2, sb.exptab);
                // (as the blend backward words it: "not below", so that a NaN o G stays blended at 0.99 as under the forward's fminf)
                const bool valid = (base + j < last) & (p2 <= 0.0f) & !(oG < ALPHA_MIN);
                const unsigned long long bal = __ballot(valid);
                if (bal != 0ull) {
                    float w = 0.f;
                    if (valid) {
#pragma clang fp contract(off)  // alpha T and T (1 - alpha) round as the forward's do
                        const float alpha = fminf(0.99f, oG);
                        w = alpha * T;
                        T = T * (1.0f - alpha);
                    }
                    // floor(w 2^32): w <= 0.99 and the scale is a power of two, so the product is exact and below 2^32
                    const uint32_t q = (uint32_t)(w * 4294967296.0f);
                    const uint32_t wb = to_lane63(__float_as_uint(w), [](uint32_t x, uint32_t y) { return max(x, y); });
                    const uint32_t lo = to_lane63(q & 0xFFFFu, [](uint32_t x, uint32_t y) { return x + y; });
                    const uint32_t hi = to_lane63(q >> 16, [](uint32_t x, uint32_t y) { return x + y; });
                    if (lane == 63) {
                        atomicAdd(&sb.cnt[j], (uint32_t)__popcll(bal));
                        atomicMax(&sb.mx[j], wb);
                        atomicAdd(&sb.sum[j], ((unsigned long long)hi << 16) + lo);
                    }
                }
            }
        }
        __syncthreads();  // the batch's cells are complete
        if (tid < cnt && sb.cnt[tid] != 0u) {
            atomicAdd(a.n_touched + gid, (int)sb.cnt[tid]);
            atomicMax(a.max_weight_bits + gid, sb.mx[tid]);
            atomicAdd(a.sum_weight + gid, sb.sum[tid]);
        }
        // (no barrier here: a thread clears and restages only its OWN slot and cells, which it has just read; the other waves touch
        //  them again behind build_lists' barriers)
    }
}

__global__ void __launch_bounds__(256) contrib_clear_kernel(long P, int* n_touched, uint32_t* max_weight_bits, unsigned long long* sum_weight,
                                                            int* counts) {
    const long stride = (long)gridDim.x * 256;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < P; g += stride) {
        n_touched[g] = 0;
        max_weight_bits[g] = 0u;
        sum_weight[g] = 0ull;
    }
    if (counts && blockIdx.x == 0 && threadIdx.x < 4) counts[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(256) contrib_fold_kernel(ContribFoldArgs a) {
    __shared__ int red[2][4];
    const bool overflowed = a.sched_flag && (blend_flags(a.sched_flag) & BLEND_FLAG_OVERFLOWED) != 0;
    int touched = 0, observed = 0;
    const long stride = (long)gridDim.x * 256;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < a.P; g += stride) {
        const int n = a.n_touched[g];
        const float m = a.max_weight[g];
        const bool obs = n >= a.min_pixels && m >= a.weight_min;
        touched += n > 0 ? 1 : 0;
        if (overflowed) continue;  // (an overflowed frame saw nothing: it is no view of the map)
        observed += obs ? 1 : 0;
        if (a.touched_total) a.touched_total[g] += (long long)n;
        if (a.max_weight_total) a.max_weight_total[g] = fmaxf(a.max_weight_total[g], m);
        if (a.sum_weight_total) a.sum_weight_total[g] += a.sum_weight[g];
        if (obs && a.views) a.views[g] += 1;
        if (obs && a.last_seen) a.last_seen[g] = a.frame_id;
    }
    if (!a.counts) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        touched += __shfl_xor(touched, off, 64);
        observed += __shfl_xor(observed, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = touched; red[1][threadIdx.x >> 6] = observed; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = red[0][0] + red[0][1] + red[0][2] + red[0][3], o = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        if (t) atomicAdd(a.counts + 0, t);
        if (o) atomicAdd(a.counts + 1, o);
        if (blockIdx.x == 0) a.counts[2] = overflowed ? 1 : 0;  // (counts[3] stays the clear kernel's 0)
    }
}

unsigned per_gaussian_blocks(long P) { return (unsigned)std::min<long>(std::max<long>((P + 255) / 256, 1), 256 * 16); }

}  // namespace

hipError_t launch_contrib_clear(long P, int* n_touched, float* max_weight, long long* sum_weight, int* counts, hipStream_t stream) {
    launch(contrib_clear_kernel, dim3(per_gaussian_blocks(P)), dim3(256), stream, P, n_touched, reinterpret_cast<uint32_t*>(max_weight),
           reinterpret_cast<unsigned long long*>(sum_weight), counts);
    return hipGetLastError();
}
hipError_t launch_contrib_tiles(const ContribTilesArgs& a, int alpha_mode, hipStream_t stream) {
    const int tiles = a.grid_x * a.grid_y;
    if (tiles <= 0) return hipSuccess;
    switch (alpha_mode) {
        case ALPHA_FAST: launch(contrib_tiles_kernel<ALPHA_FAST>, dim3(tiles), dim3(256), stream, a); break;
        case ALPHA_GLIBC: launch(contrib_tiles_kernel<ALPHA_GLIBC>, dim3(tiles), dim3(256), stream, a); break;
        default: launch(contrib_tiles_kernel<ALPHA_REF>, dim3(tiles), dim3(256), stream, a);
    }
    return hipGetLastError();
}
hipError_t launch_contrib_fold(const ContribFoldArgs& a, hipStream_t stream) {
    launch(contrib_fold_kernel, dim3(per_gaussian_blocks(a.P)), dim3(256), stream, a);
    return hipGetLastError();
}
}  // namespace dgr
