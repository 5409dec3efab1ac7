// render_light.hip -- 16x16-tile alpha-blending kernels of the light variant for gfx950.
//
// Replaces renderCUDA forward (L/cuda_rasterizer/forward.cu:261-412) and renderCUDA backward
// (L/cuda_rasterizer/backward.cu:419-699).
//
// Shape of the computation on CDNA4 (wave64, LDS 160 KB/CU, ONE scalar unit per CU):
//  * one 256-thread workgroup per tile, wave w owns the 8x8-pixel quadrant (w&1, w>>1);
//  * the sorted tile list is staged 256 instances at a time into LDS: a 32-byte traversal record
//    {x, y, a2, b2 | c2, opacity, slot, -} plus {r, g, b, depth} and the Gaussian id, one 48-byte gather (one 64-byte line)
//    per thread;
//  * while staging, every thread bounds the region where its Gaussian can reach alpha >= 15/255 (the
//    ellipse q(d) <= 2 ln(255 o / 15), boxed with a safety margin) and tests it against the eight
//    HALVES of the four quadrants (8x4 pixels = lanes 0-31 / 32-63 of the consumer wave).  Wave ballots +
//    mbcnt turn those tests into eight COMPACTED lists of 16-bit record offsets, one per half-wave, in
//    tile-list order (the backward: four lists, one per wave, from the forward's contribution tags, which reach it with the
//    forward's compacted list of the entries it blended -- render_common.h: live_list -- the only entries the backward stages);
//  * each wave walks its two lists side by side, two entries per iteration: one 4-byte LDS read per lane
//    yields two offsets, ds_read_b128 with one address per half-wave fetch the records (the same four
//    LDS cycles as a broadcast), then pure VALU per pixel.  A splat reaches 16 of a quadrant's 64
//    pixels on average and more than half of the pairs stay inside one half, so the halves need 0.73
//    of the steps a quadrant-wide list takes (render_fwd 112 -> 103 us).  The loop has no scalar bit
//    scans and "pixel finished" is a per-lane threshold register rather than a lane mask: the first
//    version of this loop spent ~20 SALU instructions per Gaussian and was bound by the CU's single
//    scalar unit (SQ_INSTS_SALU ~ 0.87 per CU cycle), not by the four SIMDs.
//    A skipped (pixel, Gaussian) pair is one the per-pixel test `power > 0 || alpha < 15/255` would have
//    rejected, so outputs are unchanged; `contributor` (hence n_contrib) is the position in the tile list,
//    which skipping does not alter.
//  * block -> tile through the tile schedule (ImageView::tile_sched, tile_schedule.hip): longest list first, consecutive workgroups
//    going round the XCDs.  (Rounds 1-5 handed every XCD a contiguous band of tiles for L2 reuse between neighbours: no
//    measurable gain, and a factor of two lost on a frame whose Gaussians cluster -- DESIGN.md s4.8.)
//
// alpha: template parameter AM (render_common.h).  ALPHA_REF, the default, evaluates the reference's expression with the
// CPU restatement's bits (exact_math.h: an fp32 polynomial expf; ALPHA_GLIBC: glibc's algorithm in the double pipe): the
// alpha image, n_contrib and the median depth then equal the restatement's bit for bit, which is what the light backward's
// T_final = 1 - alpha needs.  ALPHA_FAST (an option) is
// o * exp2(p2) on a conic pre-scaled by log2(e) -- one v_exp_f32.  Forward and backward of one mode use the identical
// expression, so they agree on every decision.
#include "render_common.h"
#include "block_scan.h"

namespace dgr {
namespace {

// ================================================================================ forward
constexpr int FWD_UNROLL = 2;  // list entries per loop iteration (4 was measured: no faster, more registers)

// HALVES: eight lists, one per half of a quadrant (render_common.h: build_half_lists); the ids stay out of LDS (8 workgroups per CU):
// a thread keeps the id of the instance it staged in a register until it flushes the slot
template <bool HALVES>
struct StagedFwd {
    typedef StagedT<DGR_TILE_PIX, unsigned short, HALVES ? 8 : 4, false> staged_t;
    static constexpr bool HALF_LISTS = HALVES;
    staged_t f;
    float unc[DGR_TILE_PIX];   // per staged instance: sum of (d - gt)^2 alpha T over its median pixels (forward.cu:386)
    uint32_t cnt[DGR_TILE_PIX];
    uint32_t hit[DGR_TILE_PIX];  // byte w of word j != 0 <=> some pixel of quadrant wave w blended staged instance j
    alignas(16) uint32_t live4[4];  // flush_slot: live entries of the flushed batch per staging wave
    uint64_t exptab[32];         // ALPHA_GLIBC: exact_math.h
};

// Per-slot results of the batch staged at position `pos0` of the tile list that starts at `list0`: the median statistics go to the
// Gaussian, the contribution tag into the entry's tag byte (render_common.h), and the entries somebody blended -- tag != 0 -- go,
// compacted in list order, to the tile's live list from `live_base` on (render_common.h: live_list): a ballot and mbcnt per
// wave, the four waves' counts through LDS.  Every thread of the workgroup calls it, once per batch, behind the barrier that ends the
// batch's pair loop; returns the new live_base.
// `gid`: the Gaussian the calling thread staged in its slot -- kept in a register since the staging, so that nothing here waits for
// memory (a re-read of the tile list behind the barrier put its latency at the end of every workgroup).
// Its one barrier also takes the workgroup's vote "every pixel finished" (`my_done` -> `all_done`: L/cuda_rasterizer/forward.cu:329-332),
// so a batch costs no barrier of its own for that.
// Addresses: a workgroup-uniform 64-bit base (scalar arithmetic) and a 32-bit byte offset per lane -- no 64-bit vector adds.
template <class SF>
__device__ __forceinline__ uint32_t flush_slot(SF& sf, const RenderFwdLightArgs& a, uint8_t* tag8, uint2* live, uint32_t list0, uint32_t pos0,
                                               uint32_t live_base, int tid, bool staged, uint32_t gid, bool my_done, bool& all_done) {
    uint32_t t8 = 0u;  // bit 2 w <- upper half of wave w, bit 2 w + 1 <- its lower half
    if (staged) {
        if constexpr (SF::HALF_LISTS) {  // (the half-wave body) lower halves: the bytes of the record's third word
            t8 = tag_byte(sf.hit[tid], __float_as_uint(sf.f.rec[2 * tid + 1].z));
        } else {                         // (the quadrant body) a quadrant's tag stands for both of its halves
            t8 = spread4(pack4(sf.hit[tid])) * 3u;
        }
        *global_at(tag8 + (size_t)(list0 + pos0), (uint32_t)tid) = (uint8_t)t8;  // every staged entry, blended or not: the byte underneath is the binning's
    }
    const unsigned long long bal = __ballot(t8 != 0u);
    if ((tid & 63) == 0) sf.live4[tid >> 6] = (uint32_t)__popcll(bal);
    all_done = __syncthreads_and(my_done);
    const uint4 c = *reinterpret_cast<const uint4*>(sf.live4);
    if (t8 != 0u) {
        const int wave = tid >> 6;
        const uint32_t before = (wave > 0 ? c.x : 0u) + (wave > 1 ? c.y : 0u) + (wave > 2 ? c.z : 0u);
        *global_at(reinterpret_cast<unsigned long long*>(live + (size_t)(list0 + live_base)), (before + (uint32_t)lanes_below(bal)) * 8u) =
            (unsigned long long)gid | ((unsigned long long)(((pos0 + (uint32_t)tid) << 8) | t8) << 32);  // {id, position << 8 | tag}
        if (sf.cnt[tid] != 0u) {                // (a median pixel blended it: it has a tag)
            atomicAdd(&at_byte(a.gau_uncertainty, gid * 4u), sf.unc[tid]);  // (ids stay below 2^28: render_common.h)
            atomicAdd(&at_byte(a.gau_related_pixels, gid * 4u), (int)sf.cnt[tid]);
        }
    }
    return live_base + (uint32_t)__builtin_amdgcn_readfirstlane((int)(c.x + c.y + c.z + c.w));
}

template <int AM, bool HALVES>
__device__ __forceinline__ void render_fwd_light_body(const RenderFwdLightArgs& a, StagedFwd<HALVES>& sf, const uint4 slot, const int frame_flags) {
    typename StagedFwd<HALVES>::staged_t& s = sf.f;
    const int tile = (int)slot.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const auto [tx, ty, px, py, inside, pix_id] = tile_pixel(tile, a.grid_x, a.W, a.H, wave, lane);
    const f2 pxy = {(float)px, (float)py};
    const float tile_x0 = (float)(tx * DGR_BLOCK_X), tile_y0 = (float)(ty * DGR_BLOCK_Y);
    const int my_list = HALVES ? 2 * wave + (lane >> 5) : wave;
    // where this lane marks "blended": byte `wave` of hit[j] -- HALVES: lanes 32-63 in byte `wave` of the record's spare word
    uint8_t* const tag8 = half_tags(a.point_list, a.sched_flag);
    uint2* const live = live_list(a.point_list, a.sched_flag);
    uint32_t live_base = 0;  // live entries of this tile written so far (workgroup-uniform)
    uint32_t my_gid = 0;     // the Gaussian this thread staged in slot tid (flush_slot)
    unsigned char* const mark_base = (HALVES && lane >= 32) ? reinterpret_cast<unsigned char*>(&s.rec[1].z) + wave
                                                             : reinterpret_cast<unsigned char*>(sf.hit) + wave;
    const int mark_stride = (HALVES && lane >= 32) ? 32 : 4;

    const uint2 range = make_uint2(slot.y, slot.z);
    const int total = (int)(range.y - range.x);

    float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f, weight = 0.f, Dd = 0.f, D_median = 0.f;
    uint32_t last_contributor = 0;
    // "done" as a per-lane upper bound on p2: live pixels accept p2 <= 0 (the reference's `power > 0` test),
    // finished pixels compare against -inf and accept nothing
    float ub = inside ? 0.f : -__builtin_inff();
    const float gt_px = inside ? at_byte(a.gt_depth, pix_id * 4u) : 0.f;  // (4 W H <= 2^32: tile_pixel)
    if (tid == 0) write_sentinel(s);
    if (AlphaPath<AM>::TABLE) exp_ref_table_fill(sf.exptab, tid);  // (visible after the first batch's barriers)

    // (every tile has a pixel inside the frame, so no tile is finished before its first batch: the vote "whole tile finished",
    //  L/cuda_rasterizer/forward.cu:329-332, is taken behind each batch -- in flush_slot's barrier -- for the next one)
    int base = 0;
    while (base < total) {
        sf.unc[tid] = 0.f;  // (slot tid: flushed by this thread, below, before it restages it)
        sf.cnt[tid] = 0u;
        sf.hit[tid] = 0u;
        const int cnt = total - base;  // (the batch holds min(256, cnt))
        unsigned code = 0;
        if (tid < cnt) {
            my_gid = *global_at(a.point_list + (size_t)(range.x + (uint32_t)base), (uint32_t)tid * 4u);
            code = stage_one<AM, HALVES>(s, tid, my_gid, a.rec, tile_x0, tile_y0);
        }
        const int n = HALVES ? build_half_lists(s, code, tid, wave, lane) : build_lists(s, code, tid, wave, lane);

        for (int k = 0; k < n; k += FWD_UNROLL) {
            float4 q0[FWD_UNROLL], q1[FWD_UNROLL];
            load2(s, my_list, k, q0, q1);
#pragma unroll
            for (int u = 0; u < FWD_UNROLL; u++) {
                f2 dxy;
                const float p2 = pair_p2<AM>(q0[u], q1[u], pxy, dxy);
                if ((p2 <= ub) & (p2 >= q1[u].w)) {  // cheap log-domain pre-test: the exponential stays off the common path
                  const float alpha = fminf(0.99f, alpha_raw<AM>(q1[u].y, p2, sf.exptab));
                  if (alpha >= ALPHA_MIN) {
#pragma clang fp contract(off)  // T (1 - alpha) and the alpha image's sum round as the reference's do (forward.cu:366-379)
                    const float test_T = T * (1.0f - alpha);
                    if (test_T < 0.0001f) {
                        ub = -__builtin_inff();  // done; this Gaussian is not blended (forward.cu:368-373)
                    } else {
                        const int j = HALVES ? (__float_as_int(q1[u].w) & 0xFF) : __float_as_int(q1[u].z);
                        const float4 cd = s.rgbd[j];
                        mark_base[j * mark_stride] = 1;  // contribution tag
                        const float w = alpha * T;
                        C0 = __builtin_fmaf(cd.x, w, C0); C1 = __builtin_fmaf(cd.y, w, C1); C2 = __builtin_fmaf(cd.z, w, C2);
                        weight = weight + w;
                        Dd = __builtin_fmaf(cd.w, w, Dd);
                        if (T > 0.5f && test_T < 0.5f) {  // forward.cu:381-388
                            D_median = cd.w;
                            const float e = cd.w - gt_px;
                            atomicAdd(&sf.unc[j], e * e * w);
                            atomicAdd(&sf.cnt[j], 1u);
                        }
                        T = test_T;
                        last_contributor = (uint32_t)(base + j + 1);
                    }
                  }
                }
            }
            if (!wave_any(ub >= 0.f)) break;
        }
        __syncthreads();  // the batch's marks and median statistics are complete
        bool all_done;
        live_base = flush_slot(sf, a, tag8, live, range.x, (uint32_t)base, live_base, tid, tid < cnt, my_gid, ub < 0.f, all_done);
        base += DGR_TILE_PIX;
        if (all_done) break;
    }
    // (an empty tile, the empty lists of an overflowed frame, a tile that finished early: what was flushed, 0 if nothing was)
    // (written by the LAST thread: `tid == 0` is the sentinel's test at the top, and the compiler would carry that lane mask through the loops -- in spill lanes)
    if (tid == DGR_TILE_PIX - 1) a.live_counts[tile] = live_base;
    // the tail of a list whose tile finished early was never staged: nobody blended it (render_common.h: the tag bytes' invariant)
    for (int p = base + tid; p < total; p += DGR_TILE_PIX) at_byte(tag8 + (size_t)range.x, (uint32_t)p) = 0;

    // A forward whose binning buffer was too small has rendered EMPTY tile lists (bin_tiles left every range {0, 0}): in lazy mode
    // the host learns of it a call or two later, so the images must not look like a frame -- they are NaN, every value
    // (strict mode retries inside the call and overwrites them).  The flag came with the schedule word (blend_slot): a uniform branch,
    // on the word itself -- one scalar register through the loops, where a bool is a lane mask in two.
    if (frame_flags & BLEND_FLAG_OVERFLOWED) {
        C0 = C1 = C2 = weight = Dd = D_median = __builtin_nanf("");
    }
    if (inside) {
        // The image pointers are needed here and nowhere else: read from the kernel's argument block HERE (late_kernel_args), they
        // occupy no scalar registers through the batch loop -- loaded at the top, as the compiler does with `a`'s own members,
        // sixteen of them were spilled to the lanes of a vector register and read back one by one.
        const auto ka = late_kernel_args<RenderFwdLightArgs>();
        const size_t N = (size_t)((uint32_t)a.W * (uint32_t)a.H);
        // the pixel's byte offset, worked out again from the coordinates the pair loop keeps as floats (exact: below 2^24) rather than
        // carried through the loops in a register of its own -- the kernel has none to spare (opaque, or the compiler carries it)
        float fx = pxy.x, fy = pxy.y;
        asm volatile("" : "+v"(fx), "+v"(fy));
        const uint32_t po = ((uint32_t)fy * (uint32_t)a.W + (uint32_t)fx) * 4u;  // (4 W H <= 2^32: tile_pixel)
        float* const out_color = ka->out_color;
        const float* const bg = ka->bg;
        at_byte(ka->n_contrib, po) = last_contributor;
        at_byte(out_color, po) = C0 + T * bg[0];
        at_byte(out_color + N, po) = C1 + T * bg[1];
        at_byte(out_color + 2 * N, po) = C2 + T * bg[2];
        at_byte(ka->out_alpha, po) = weight;  // forward.cu:407
        at_byte(ka->out_depth, po) = Dd;
        at_byte(ka->out_median, po) = D_median;
        at_byte(ka->out_depth_var, po) = 0.0f;  // forward.cu:317,410
    }
}

// One kernel, both lane mappings: which one a frame takes is the frame's own flag (ImageView::cursor[3] bit 2, written by its binning
// kernel) -- a uniform branch on a word the workgroup reads anyway, so that the choice can be made on the DEVICE for the frame at
// hand (no host policy, nothing to carry from forward to backward: the backward kernels branch on the same word).  The two bodies
// share the workgroup's LDS (a union: 20.0 KB, 8 workgroups per CU) and the register budget of the launch bounds.
template <int AM>
__global__ void __launch_bounds__(256, 8) render_fwd_light_kernel(RenderFwdLightArgs a) {
    __shared__ union { StagedFwd<true> h; StagedFwd<false> q; } sf;
    if (a.rep.host && blockIdx.x == 0 && threadIdx.x == 0) report_status(a.rep, a.status);
    const int frame_flags = blend_flags(a.sched_flag);
    const uint4 slot = blend_slot(frame_flags, a.sched, a.ranges, a.grid_x * a.grid_y);  // {tile, list start, list end}
    if (frame_flags & BLEND_FLAG_QUADRANT_LISTS) render_fwd_light_body<AM, false>(a, sf.q, slot, frame_flags);
    else render_fwd_light_body<AM, true>(a, sf.h, slot, frame_flags);
}

// ================================================================================ backward
// Per-Gaussian gradient sums.  Only ~6 of a wave's 64 pixels are hit by any one Gaussian and LDS float
// atomics retire barely one lane per cycle on gfx950 (measured: 55 % of wave cycles in SQ_WAIT_INST_LDS
// with per-lane ds_add_f32), so the sums are formed in registers: every listed Gaussian is visited
// wave-uniformly (as in the forward), the valid lanes compute their 14 contributions, and ONE butterfly
// (wave_reduce.h, 33 instructions) reduces all 14 across the wave at once, leaving each total in its own
// lane quad.  A single ds_add_f32 with 14 active lanes on 14 distinct banks then merges the four
// quadrant waves in LDS accumulators acc[14][257], which are flushed once per batch with line-coalesced
// global atomics (16 consecutive lanes = one Gaussian's 64-byte accumulator row).  Global float atomics
// drop from 14 per valid (pixel, Gaussian) pair to <= 14 per (tile, Gaussian).
// Tracking mode (map_off) needs only the three sums the pose gradient is built from: a 4-value butterfly.
// (Twelve values since round 3 -- raw moments, the median term as the twelfth -- in accumulator rows 0..10 and 13.)
// Round 8: a Gaussian reaches 16 of a quadrant's 64 pixels on average and more than half of the (quadrant, Gaussian) entries
// live in ONE half of the quadrant.  The forward tags what it blended per half (render_common.h: half_tags); from those tags
// the tracking kernel walks one list per half-wave like the forward, and the mapping kernel pairs neighbouring entries of its
// list that live in different halves into one loop step (build_paired_lists) -- see the HALVES note above the kernel.
constexpr int NACC_LIGHT = 14;

// LIVE entries staged per batch -- the entries the forward blended, read from its compacted live list (render_common.h: live_list;
// until then a batch was 128 list POSITIONS, dead ones included: each cost a tag read, a list read and its share of the batch's
// barriers, accumulator clears and flush).  (256: 5 workgroups per CU, 267 us; 128: 247 us; the deterministic kernel's 64: 8 per CU.)
struct BwdTailLight {
    uint64_t exptab[32];  // ALPHA_GLIBC: exact_math.h
};
template <bool DET, bool HALVES = false, bool ABS = false>  // (render_common.h: BwdBatch; a batch is NB LIVE entries)
using StagedBwd = BwdBatch<StagedLiveT<bwd_batch_entries(DET), HALVES ? 8 : 4>, NACC_LIGHT, DET, ABS, BwdTailLight>;

// 8 waves per SIMD (63 VGPRs, no scratch): measured 258 us at the compiler's own choice of 7, 247 us at 8
//
// DET (dgr_set_option("deterministic_grads", 1)): gradients that are the same bits run after run.  Two sums of the default kernel
// depend on the order in which hardware atomics arrive: the four quadrant waves' totals of a (tile, Gaussian) pair meet in LDS
// float atomics, and the tiles' totals of a Gaussian meet in global float atomics (as in the reference, backward.cu:593-596,
// 666-680).  Here (a) every wave stores its total into its OWN accumulator plane -- a wave visits a list entry once per batch, so
// a plain store suffices -- and the planes are added in wave order; (b) the finished row of a (tile, Gaussian) pair is STORED to
// the pair's own 64-byte row of an instance-major buffer (row = the Gaussian's first instance, det_offsets_kernel, + the tile's
// position in its rectangle; the buffer is zero-filled first: pairs nobody blended stay zero), and det_gather_kernel adds a
// Gaussian's rows -- contiguous -- in ascending order into the accumulator row preprocess_bwd reads.
//
// LEAN: the caller passed no gradient image for the median depth and none for the depth variance (NULL pointers: the loss did
// not use those outputs -- the usual case in CG-SLAM, whose depth_var output is identically zero, forward.cu:317,410).  The
// kernel then drops what only they feed: the variance term of X and of the depth gradient, and the once-per-pixel median test --
// five full-rate and three 4.2-cycle instructions per list entry.  Bit-identical to the full kernel fed all-zero images
// (0 * e^2 adds an exact zero).
//
// HALVES (the tracking backward, map_off): one list per HALF-wave and a loop step that serves the upper half's next entry on
// lanes 0-31 and the lower half's on lanes 32-63, as in the forward.  The lists come from the forward's tags per half
// (render_common.h: half_tags); each half reduces its three sums over its own 32 lanes
// (half_reduce3) and delivers them to its own entry's accumulator column: six lane-atomics per step.  The MAPPING backward
// delivers twelve values per entry and is bound by the LDS array's float atomics in this form.
//
// With DO_MAP, HALVES means PAIRED lists (render_common.h: build_paired_lists): neighbouring entries of a wave's list that live
// in different halves of the quadrant share a loop step (0.87 steps per entry); such a step reduces its twelve sums per half and
// each half delivers to its own entry's column -- every entry is still delivered once.
//
// SILHOUETTE (every form above; not a template axis): the opacity_map A = sum_k alpha_k T_k has dA/dalpha_k = T_final / (1 - alpha_k),
// the shape of the background term.  A caller's dL/dA image (a.dL_dpix_silhouette, nullable) therefore only changes the per-pixel
// constant bg_term, read once before the loop: the pair loop and everything downstream of dL/dalpha stay as they are.
//
// ABS (absgrad, AbsGS's "homodirectional" gradient; mapping only, not DET): each lane also forms its pixel's own dL/dmean2D --
// the formula of the moments -> gradients step below applied to the pixel's q dx, q dy -- and sums the absolute values of its two
// components.  half_reduce3 reduces the pair over each half-wave, and each half adds its totals to its own entry's column of
// accumulator rows 14, 15 (a paired step: two entries; otherwise both halves into one), so the default 12-value network and its
// lane maps stay as they are.  The batch's totals, times W/2 and H/2, go to abs_out [P,3] by global atomics.
template <int AM, bool DO_MAP, bool DO_POSE, bool DET, bool LEAN, bool HALVES, bool ABS = false>
__device__ __forceinline__ void render_bwd_light_body(const RenderBwdLightArgs& a, StagedBwd<DET, HALVES, ABS>& sb, const uint4 slot,
                                                      float* __restrict__ abs_out = nullptr) {
    static_assert(!HALVES || !DET, "half-wave / paired lists: not with the deterministic kernel's planes (LDS)");
    static_assert(!ABS || (DO_MAP && !DET), "absgrad: the mapping backward, not the deterministic kernel");
    constexpr bool PAIRED = HALVES && DO_MAP;
    typedef StagedBwd<DET, HALVES, ABS> SB;
    constexpr int BWD_NB = SB::NB, BWD_LD = SB::LD;
    typename SB::staged_t& s = sb.f;
    const int tile = (int)slot.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const auto [tx, ty, px, py, inside, pix_id] = tile_pixel(tile, a.grid_x, a.W, a.H, wave, lane);
    const uint32_t N = (uint32_t)a.W * (uint32_t)a.H;
    const float pxf = (float)px, pyf = (float)py;
    const f2 pxy = {pxf, pyf};

    // The tile's LIVE entries -- the ones the forward blended for some pixel, compacted in list order (render_common.h: live_list) --
    // are all this kernel walks: none lies past the tile's last contributor, and a tile nobody blended is done here.
    const int total = __builtin_amdgcn_readfirstlane((int)a.live_counts[tile]);
    if (total <= 0) return;
    const uint2* const live = live_list(a.point_list, a.sched_flag) + slot.y;
    const int last_contributor = inside ? (int)a.n_contrib[pix_id] : 0;

    if (tid == 0) write_sentinel_live(s);
    if (AlphaPath<AM>::TABLE) exp_ref_table_fill(sb.t.exptab, tid);  // (visible after the first batch's barriers)

    const float T_final = inside ? (1.0f - a.alphas[pix_id]) : 0.f;
    float T = T_final;
    float dpix0 = 0.f, dpix1 = 0.f, dpix2 = 0.f, dpix_depth = 0.f, dpix_median = 0.f, dpix_var = 0.f, gt_px = 0.f, dpix_sil = 0.f;
    if (inside) {
        // (single-use images, 28 bytes per pixel: nontemporal, so that they do not push the accumulator rows and render records out of
        //  the caches -- preprocess_bwd behind this kernel 45 -> 43.5 us, profiles/r6/ab_nontemporal.txt)
        dpix0 = __builtin_nontemporal_load(a.dL_dpix + pix_id);
        dpix1 = __builtin_nontemporal_load(a.dL_dpix + N + pix_id);
        dpix2 = __builtin_nontemporal_load(a.dL_dpix + 2 * N + pix_id);
        dpix_depth = __builtin_nontemporal_load(a.dL_dpix_depth + pix_id);
        if (a.dL_dpix_silhouette) dpix_sil = __builtin_nontemporal_load(a.dL_dpix_silhouette + pix_id);  // (every form: SILHOUETTE)
        if (!LEAN) {  // (either image may be missing on its own: it then reads as zero)
            if (a.dL_dpix_median) dpix_median = __builtin_nontemporal_load(a.dL_dpix_median + pix_id);
            if (a.dL_dpix_var) dpix_var = __builtin_nontemporal_load(a.dL_dpix_var + pix_id);
            gt_px = __builtin_nontemporal_load(a.gt_depth + pix_id);
        }
    }
    // per-pixel constants of the loop: -T_final (<bg, dL/dpixel> - dL/dsilhouette) (the background and silhouette terms of dL/dalpha
    // are this times 1/(1 - alpha); without a silhouette image the subtracted +0 leaves the bits as they were) and 2 dL/dvar
    const float bg_term = -T_final * ((a.bg[0] * dpix0 + a.bg[1] * dpix1 + a.bg[2] * dpix2) - dpix_sil);
    const float ddelx_dx = 0.5f * a.W, ddely_dy = 0.5f * a.H;
    // The reference keeps five "accumulated behind me" recurrences (3 colours, depth, variance: backward.cu:580-608)
    // only to form dL/dalpha = sum_c (c_j - accum_rec_c) dL/dpixel_c.  They are linear, so one scalar suffices:
    //   X_j = <features_j, dL/dpixel>,   S <- alpha_last X_last + (1 - alpha_last) S,   dL/dalpha = X_j - S.
    float S = 0.f;
    float mid_thr = 0.5f;
    // which accumulator component this lane's quad delivers after the butterfly (-1: none)
    int my_comp;
    if (DO_MAP) {
        // butterfly slots 0..9 = components 0..9; with the pose gradient slot 10 = component 13 (pose depth) and slot 11 =
        // component 10 (median), without it slot 10 = component 10
        const int c = (lane >= 48) ? 12 : wave_reduce12d_comp(lane);  // (rows 2 and 3 hold the same four totals: row 2 delivers)
        my_comp = ((lane & 3) != 0 || c > 11) ? -1 : (c == 10 ? (DO_POSE ? 13 : 10) : c == 11 ? (DO_POSE ? 10 : -1) : c);
    } else if (HALVES) {  // (tracking)
        const int c = half_reduce3_comp(lane);  // {4: gmx, 5: gmy, 13: pose depth} of the lane's half
        my_comp = c == 0 ? 4 : c == 1 ? 5 : c == 2 ? 13 : -1;
    } else {
        const int c = wave_reduce4_comp(lane);  // {4: gmx, 5: gmy, 13: pose depth}
        my_comp = ((lane & 15) == 0 && c < 3) ? (c == 0 ? 4 : c == 1 ? 5 : 13) : -1;
    }
    const int my_list = HALVES ? 2 * wave + (lane >> 5) : wave;

    // this lane's accumulator row (column = slot); DET: in its wave's own plane
    float* const my_acc = sb.acc + (DET ? wave * SB::PLANE : 0) + (my_comp >= 0 ? my_comp : 0) * BWD_LD;

    // back-to-front: batches cover the live entries [lo, hi) with hi walking down from `total`
    // (batches of equal size: 150 live entries go as 75 + 75, not 128 + 22 -- a full batch of LIVE entries leaves about twice the
    //  entries per quadrant list that 128 positions did, and the pairing pass takes lists of up to 64: profiles/live_lists/notes.md)
    // (only where lists are paired; any size with nbatch * per >= total serves: the quotient through the float reciprocal, rounded up)
    int per = BWD_NB;
    if (PAIRED && total > BWD_NB) {
        const int nbatch = (total + BWD_NB - 1) / BWD_NB;
        per = min(BWD_NB, (int)((float)total * __builtin_amdgcn_rcpf((float)nbatch)) + 1);
    }
    for (int hi = total; hi > 0; hi -= per) {
        const int lo = max(0, hi - per);
        const int cnt = hi - lo;
        __syncthreads();  // previous batch fully flushed / consumed
        unsigned code = 0;
        if (tid < cnt) code = stage_live<AM, !HALVES>(s, tid, live[lo + tid], a.rec);
        if (!DET) clear_acc(sb, tid);
        unsigned long long split[2] = {0ull, 0ull};  // PAIRED: the steps that serve two entries
        const int n = PAIRED   ? build_paired_lists(s, code, tid, wave, lane, split)
                      : HALVES ? build_half_lists(s, code, tid, wave, lane)
                               : build_lists(s, code, tid, wave, lane);

        // (the list is padded with sentinels to a multiple of 4, so a multiple of 2 is always readable)
        // PAIRED: one step per iteration -- the second step's records in flight cost eight registers that this kernel does not have
        // (its lists' base is a per-lane value, the half-wave sums cross a branch); the other waves of the SIMD cover the LDS latency
        constexpr int U = PAIRED ? 1 : 2;
        for (int k = ((n + U - 1) / U) * U - U; k >= 0; k -= U) {
            float4 q0[2], q1[2];
            unsigned off[2];
            if (U == 2) {
                const uint2 pk = *reinterpret_cast<const uint2*>(&s.list[my_list][k]);
                off[0] = pk.x;
                off[1] = pk.y;
            } else {
                off[0] = off[1] = s.list[my_list][k];
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                q0[u] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s.rec) + off[u]);
                q1[u] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s.rec) + off[u] + 16);
            }
#pragma unroll
            for (int u = U - 1; u >= 0; u--) {
                f2 dxy;
                const float p2 = pair_p2<AM>(q0[u], q1[u], pxy, dxy);
                const float dx = dxy.x, dy = dxy.y;
                const int j4 = __float_as_int(q1[u].z);  // 4 * slot
                // every listed entry was blended by some pixel of this wave (contribution tags): no wave-level tests
                const float oG = alpha_raw<AM, true>(q1[u].y, p2, sb.t.exptab);  // o G: alpha before the 0.99 clamp, and dalpha/dG * G
                // (the reference tests min(0.99, o G) >= 15/255; 0.99 is above the threshold, so o G itself decides)
                // (written as "not below", so that a NaN o G -- a poisoned opacity -- stays a valid pair with alpha 0.99 as under
                //  the reference's min(0.99f, NaN))
                // (the entry's own position in the tile list against the pixel's last contributor)
                const bool valid = (__float_as_int(q1[u].w) < last_contributor) & (p2 <= 0.0f) & !(oG < ALPHA_MIN);
                // No branch: a lane the Gaussian does not reach runs the same instructions with alpha = 0 and o G = 0, which
                // leave its state untouched -- 1/(1 - 0) is exactly 1, so T, and S = 0 X + 1 S, keep their bits -- and
                // make every one of its contributions 0.  (The list's sentinel entries have opacity 0 and an all-zero
                // rgbd entry.)  Valid lanes execute the operations of the reference's order unchanged.  One select (on o G;
                // the clamp of 0 is 0): a select and a compare issue at 4.2 cycles each, a multiply at 2.4.
                const float oGm = valid ? oG : 0.f;
                const float alpha = fminf(0.99f, oGm);
                const float4 cd = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s.rec) + off[u] + 32);  // {r, g, b, depth} behind the record
                const float om = 1.f - alpha;
                float inv;
                T = t_div<AM>(T, om, inv);  // backward.cu:570
                const float w = alpha * T;  // dchannel_dcolor = dpixel_depth_ddepth
                const float e = cd.w - gt_px;
                const float X = LEAN ? cd.x * dpix0 + cd.y * dpix1 + cd.z * dpix2 + cd.w * dpix_depth
                                     : cd.x * dpix0 + cd.y * dpix1 + cd.z * dpix2 + cd.w * dpix_depth + (e * e) * dpix_var;
                const float dL_dalpha = (X - S) * T + bg_term * inv;
                S = alpha * X + om * S;  // what the NEXT valid pair (towards the front) subtracts: same operations, same order
                const float qq = oGm * dL_dalpha;  // o G dL/dalpha  (dL_dG * G)
                // Per-lane contributions are the raw moments of qq over the pixel offsets; the factors that depend on the
                // Gaussian only (conic, 1/opacity, the ndc scale) are applied once per (tile, Gaussian) in finish_rows().
                const float qdx = qq * dx, qdy = qq * dy;
                const float wd = w * dpix_depth;
                float tot;
                if (DO_MAP) {
                    // backward.cu:654-664, once per pixel -- at its first valid pair from the back with T > 0.5: the
                    // median-depth term of dL/dmean3D is (v_k - v_{k+1} mul3) * dL/dmedian with factors that depend on
                    // the Gaussian alone, so only the pixel sum of dL/dmedian is formed here, as one more value of the
                    // butterfly (its twelfth slot is free); preprocess_bwd applies the factors.  `mid_thr` turns to +inf
                    // once the pixel has fired.
                    float gmed = 0.f;
                    if (!LEAN) {
                        const bool fire = valid & (T > mid_thr);
                        gmed = fire ? dpix_median : 0.f;
                        mid_thr = fire ? __builtin_inff() : mid_thr;
                    }
                    float g[12];
                    g[0] = w * dpix0;
                    g[1] = w * dpix1;
                    g[2] = w * dpix2;
                    g[3] = LEAN ? wd : wd + 2.f * ((dpix_var * w) * e);  // (2 dL/dvar: the factor is exact wherever it stands)
                    g[4] = qdx;        // sum q dx
                    g[5] = qdy;        // sum q dy
                    g[6] = qdx * dx;   // sum q dx^2
                    g[7] = qdx * dy;   // sum q dx dy
                    g[8] = qdy * dy;   // sum q dy^2
                    g[9] = qq;         // sum q
                    g[10] = DO_POSE ? wd : gmed;   // -> accumulator component 13 / 10
                    g[11] = DO_POSE ? gmed : 0.f;  // -> accumulator component 10
                    if (ABS) abs_pair_terms<AM, NACC_LIGHT, BWD_LD>(sb.acc, q0[u], q1[u], qdx, qdy, j4, lane);
                    if (PAIRED) {
                        float u0, u1;
                        wave_reduce12d_head(g, u0, u1);
                        const int st = k + u;  // (wave-uniform: scalar code)
                        if ((split[st >> 6] >> (st & 63)) & 1ull) {
                            // a pair: each half's own totals to its own entry's column (j4 is uniform in each half)
                            // (the rows are worked out here, one step in nine, rather than kept in registers through the loop)
                            const float r0 = quad_sum(u0), r1 = quad_sum(u1);
                            auto comp_of = [](int slot) { return slot < 10 ? slot : slot == 10 ? (DO_POSE ? 13 : 10) : (DO_POSE ? 10 : -1); };
                            const int s1 = wave_reduce12d_half_slot1(lane);
                            const int c0 = (lane & 3) == 0 ? comp_of(wave_reduce12d_half_slot0(lane)) : -1;
                            const int c1 = ((lane & 3) == 0 && s1 >= 0) ? comp_of(s1) : -1;
                            deliver_pair<BWD_LD>(sb.acc, j4, c0, c1, r0, r1);
                            continue;
                        }
                        tot = wave_reduce12d_tail(u0, u1);
                    } else {
                        tot = wave_reduce12d(g);
                    }
                } else if (HALVES) {
                    tot = half_reduce3(qdx, qdy, wd);
                } else {
                    float g4[4] = {qdx, qdy, wd, 0.f};
                    tot = wave_reduce4(g4);
                }
                // j4 is wave-uniform here (every lane read the same record; HALVES: uniform in each half-wave)
                if (my_comp >= 0) {
                    float* const cell = reinterpret_cast<float*>(reinterpret_cast<char*>(my_acc) + j4);
                    if (DET) *cell = tot; else atomicAdd(cell, tot);
                }
            }
        }

        __syncthreads();
        if (DET && tid < BWD_NB) {
            // the four planes in wave order into plane 0, and the pair's row in the instance-major buffer
            uint32_t row = ~0u;
            if (code != 0u) {
                // (the components this instance's lanes deliver: my_comp above)
                det_fold_planes<NACC_LIGHT, SB::PLANE, BWD_LD>(sb.acc, code, tid, [](int k) {
                    return DO_MAP ? (k <= 9 || k == 10 || (DO_POSE && k == 13)) : (k == 4 || k == 5 || k == 13);
                });
                row = det_row_of(a.det_rect, a.det_goff, s.id[tid], tx, ty);
            }
            sb.inst[tid] = row;
        }
        if (DET) __syncthreads();
        // moments -> gradients, one thread per staged Gaussian (backward.cu:627-631, 669-678):
        //   dL/dmean2D = -(a Sx + b Sy) W/2, -(c Sy + b Sx) H/2;  dL/dconic = -Sxx/2, -Sxy/2, -Syy/2;  dL/dopacity = S0/o
        if (code != 0u) {
            const float4 r0 = s.rec[3 * tid], r1 = s.rec[3 * tid + 1];
            mean2d_from_moments(unscaled_conic<AM>(r0, r1), sb.acc[4 * BWD_LD + tid], sb.acc[5 * BWD_LD + tid], ddelx_dx, ddely_dy);
            if (ABS) abs_flush<NACC_LIGHT, BWD_LD>(sb.acc, s.id, tid, ddelx_dx, ddely_dy, abs_out);
            if (DO_MAP) {
                sb.acc[6 * BWD_LD + tid] *= -0.5f;
                sb.acc[7 * BWD_LD + tid] *= -0.5f;
                sb.acc[8 * BWD_LD + tid] *= -0.5f;
                sb.acc[9 * BWD_LD + tid] *= __builtin_amdgcn_rcpf(r1.y);
            }
        }
        __syncthreads();
        if (DET) {
            det_store_rows<NACC_LIGHT, BWD_LD>(sb.acc, sb.inst, cnt, a.det_rows, a.det_R, tid);
        } else {
            flush_acc<NACC_LIGHT, BWD_LD>(sb.acc, s.id, cnt, a.acc, tid);
        }
    }
}

// absgrad (ABS above): the mapping instances only, lane lists by the frame's flag as in the default kernel (quadrant lists for the
// glibc form, which is refused: api.hip).  Two more LDS rows (1 KB) and the pair reduction's registers: the lean instances stay at
// 8 waves per SIMD; the others would spill at 64 VGPRs and run at 7.
template <int AM, bool DO_POSE, bool LEAN, bool BY_FRAME>
__global__ void __launch_bounds__(256, LEAN ? 8 : 7) render_bwd_light_abs_kernel(RenderBwdLightArgs a, float* abs_out) {
    __shared__ union { StagedBwd<false, BY_FRAME, true> h; StagedBwd<false, false, true> q; } sb;
    bool quadrant_lists = true;
    const uint4 slot = blend_slot(a.sched, a.ranges, a.sched_flag, a.grid_x * a.grid_y, nullptr, BY_FRAME ? &quadrant_lists : nullptr);
    if (BY_FRAME && !quadrant_lists) render_bwd_light_body<AM, true, DO_POSE, false, LEAN, BY_FRAME, true>(a, sb.h, slot, abs_out);
    else render_bwd_light_body<AM, true, DO_POSE, false, LEAN, false, true>(a, sb.q, slot, abs_out);
}

// BY_FRAME: half-wave / paired lists or quadrant lists by the frame's flag (render_fwd_light_kernel above: the forward that wrote the
// tags took the same branch -- a quadrant-list forward sets both halves' bits of a quadrant, which a half-wave backward could walk
// correctly but to no gain).  Without it: quadrant lists, for which the tag bytes of either forward are folded to four bits -- the
// deterministic kernels (LDS for the planes) and the glibc form (an A/B mode that spills a register with eight lists).
template <int AM, bool DO_MAP, bool DO_POSE, bool DET = false, bool LEAN = false, bool BY_FRAME = false>
__global__ void __launch_bounds__(256, 8) render_bwd_light_kernel(RenderBwdLightArgs a) {
    static_assert(!BY_FRAME || !DET, "the deterministic kernel walks quadrant lists");
    __shared__ union { StagedBwd<DET, BY_FRAME> h; StagedBwd<DET, false> q; } sb;
    bool quadrant_lists = true;
    const uint4 slot = blend_slot(a.sched, a.ranges, a.sched_flag, a.grid_x * a.grid_y, nullptr, BY_FRAME ? &quadrant_lists : nullptr);
    if (BY_FRAME && !quadrant_lists) render_bwd_light_body<AM, DO_MAP, DO_POSE, DET, LEAN, BY_FRAME>(a, sb.h, slot);
    else render_bwd_light_body<AM, DO_MAP, DO_POSE, DET, LEAN, false>(a, sb.q, slot);
}

// ---- deterministic gradients: the kernels around the DET blend backward
// n = tiles of a Gaussian's rectangle; goff = exclusive prefix of n over the Gaussians (the reference's point_offsets,
// L/cuda_rasterizer/rasterizer_impl.cu:283, which the segment binning never needs): per-block sums, then per-block bases.
__device__ __forceinline__ uint32_t rect_tiles(ushort4 r) { return (r.z > r.x && r.w > r.y) ? (uint32_t)(r.z - r.x) * (uint32_t)(r.w - r.y) : 0u; }
__global__ void __launch_bounds__(256) det_block_sums_kernel(int P, const ushort4* __restrict__ rect, uint32_t* __restrict__ blk) {
    __shared__ uint32_t red[4];
    const int g = blockIdx.x * 256 + threadIdx.x;
    uint32_t v = g < P ? rect_tiles(rect[g]) : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void __launch_bounds__(256) det_offsets_kernel(int P, const ushort4* __restrict__ rect, const uint32_t* __restrict__ blk,
                                                          uint32_t* __restrict__ goff) {
    __shared__ uint32_t red[4], wsum[4];
    uint32_t before = 0;  // instances of the blocks in front of this one (integer sums: any order)
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) before += blk[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = before;
    const int g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t n = g < P ? rect_tiles(rect[g]) : 0u;
    const uint32_t incl = wave_inclusive_scan(n, (int)(threadIdx.x & 63));
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t base = red[0] + red[1] + red[2] + red[3];
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) base += wsum[w];
    if (g < P) goff[g] = base + incl - n;
}
// a Gaussian's rows, contiguous from goff, added in ascending order: 16 lanes per Gaussian, a lane per component
__global__ void __launch_bounds__(256) det_gather_kernel(int P, const ushort4* __restrict__ rect, const uint32_t* __restrict__ goff,
                                                         const float* __restrict__ rows, uint32_t R, float* __restrict__ acc) {
    const int g = blockIdx.x * 16 + (threadIdx.x >> 4), comp = threadIdx.x & 15;
    if (g >= P) return;
    uint32_t n = rect_tiles(rect[g]);
    if (n == 0u) return;
    const uint32_t first = goff[g];
    // R (the caller's: a lazy forward's capacity, or a wrong value) smaller than the rectangles' total: this Gaussian's rows were
    // not all written -- a truncated sum would be a plausible gradient, so the row is NaN instead (and every gradient of the
    // Gaussian with it: preprocess_bwd reads the row)
    if (first >= R || n > R - first) {
        acc[(size_t)g * DGR_ACC_STRIDE + comp] = __builtin_nanf("");
        return;
    }
    const float* r = rows + (size_t)first * DGR_ACC_STRIDE + comp;
    float v = 0.f;
    for (uint32_t i = 0; i < n; i++) v += r[(size_t)i * DGR_ACC_STRIDE];
    acc[(size_t)g * DGR_ACC_STRIDE + comp] = v;
}

// (map_off, track_off) -> the <DO_MAP, DO_POSE> instance: mapping + pose, mapping only, tracking (both off: the callers return first).
// f(DO_MAP, DO_POSE) takes the two as std::integral_constant types.
template <class F>
void with_map_pose(const RenderBwdLightArgs& a, F&& f) {
    if (!a.map_off && !a.track_off) f(std::true_type(), std::true_type());
    else if (!a.map_off) f(std::true_type(), std::false_type());
    else f(std::false_type(), std::true_type());
}
template <int AM, bool DET, bool LEAN, bool BY_FRAME>
void launch_bwd_light_instance(const RenderBwdLightArgs& a, int tiles, hipStream_t stream) {
    with_map_pose(a, [&](auto do_map, auto do_pose) {
        launch_blend((render_bwd_light_kernel<AM, decltype(do_map)::value, decltype(do_pose)::value, DET, LEAN, BY_FRAME>), dim3(tiles), dim3(256), stream, a);
    });
}
// (absgrad: the mapping instances only, so DO_MAP is ignored.  The caller returns under map_off; with_map_pose's third branch, which
//  would be tracking, therefore never runs, and what it instantiates -- DO_POSE = true -- is the first branch's instance: no new kernel)
template <int AM, bool LEAN>
void launch_bwd_light_abs_instance(const RenderBwdLightArgs& a, float* abs_out, int tiles, hipStream_t stream) {
    with_map_pose(a, [&](auto, auto do_pose) {
        launch_blend((render_bwd_light_abs_kernel<AM, decltype(do_pose)::value, LEAN, true>), dim3(tiles), dim3(256), stream, a, abs_out);
    });
}

template <int AM>
void launch_bwd_light_mode(const RenderBwdLightArgs& a, int tiles, hipStream_t stream) {
    // (the lane lists -- half-wave / paired or per quadrant -- are the frame's own choice: render_bwd_light_kernel)
    constexpr bool BF = AM != ALPHA_GLIBC;  // (the glibc form, an A/B mode, spills a register with the eight lists: quadrant lists)
    if (AM == ALPHA_REF && a.det_rows) launch_bwd_light_instance<ALPHA_REF, true, false, false>(a, tiles, stream);
    else if (AM == ALPHA_REF && !a.dL_dpix_median && !a.dL_dpix_var) launch_bwd_light_instance<ALPHA_REF, false, true, true>(a, tiles, stream);
    else launch_bwd_light_instance<AM, false, false, BF>(a, tiles, stream);
}
}  // namespace

hipError_t launch_render_fwd_light(const RenderFwdLightArgs& a, int alpha_mode, hipStream_t stream) {
    const int tiles = a.grid_x * a.grid_y;
    if (tiles <= 0) return hipSuccess;
    switch (alpha_mode) {
        case ALPHA_FAST: launch_blend(render_fwd_light_kernel<ALPHA_FAST>, dim3(tiles), dim3(256), stream, a); break;
        case ALPHA_GLIBC: launch_blend(render_fwd_light_kernel<ALPHA_GLIBC>, dim3(tiles), dim3(256), stream, a); break;
        default: launch_blend(render_fwd_light_kernel<ALPHA_REF>, dim3(tiles), dim3(256), stream, a);
    }
    return hipGetLastError();
}
hipError_t launch_render_bwd_light(const RenderBwdLightArgs& a, int alpha_mode, hipStream_t stream) {
    const int tiles = a.grid_x * a.grid_y;
    if (tiles <= 0 || (a.track_off && a.map_off)) return hipSuccess;
    switch (alpha_mode) {
        case ALPHA_FAST: launch_bwd_light_mode<ALPHA_FAST>(a, tiles, stream); break;
        case ALPHA_GLIBC: launch_bwd_light_mode<ALPHA_GLIBC>(a, tiles, stream); break;
        default: launch_bwd_light_mode<ALPHA_REF>(a, tiles, stream);
    }
    return hipGetLastError();
}
hipError_t launch_render_bwd_light_abs(const RenderBwdLightArgs& a, float* dL_dmean2D_abs, int alpha_mode, hipStream_t stream) {
    const int tiles = a.grid_x * a.grid_y;
    if (tiles <= 0 || a.map_off) return hipSuccess;
    const bool lean = !a.dL_dpix_median && !a.dL_dpix_var;
    // (the instances of launch_bwd_light_mode's non-deterministic mapping branches)
    if (alpha_mode == ALPHA_FAST) launch_bwd_light_abs_instance<ALPHA_FAST, false>(a, dL_dmean2D_abs, tiles, stream);
    else if (alpha_mode == ALPHA_REF && lean) launch_bwd_light_abs_instance<ALPHA_REF, true>(a, dL_dmean2D_abs, tiles, stream);
    else if (alpha_mode == ALPHA_REF) launch_bwd_light_abs_instance<ALPHA_REF, false>(a, dL_dmean2D_abs, tiles, stream);
    else return hipErrorInvalidValue;  // (alpha_mode 2: refused by the entry points)
    return hipGetLastError();
}
namespace {
__global__ void __launch_bounds__(256) zero_floats_kernel(float* dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = 0.f;
}
}  // namespace
hipError_t launch_zero_floats(float* dst, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 256 * 16);
    launch(zero_floats_kernel, dim3(blocks), dim3(256), stream, dst, n);
    return hipGetLastError();
}
hipError_t launch_det_offsets(int P, const ushort4* rect, uint32_t* blk, uint32_t* goff, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    const int nb = (P + 255) / 256;
    launch(det_block_sums_kernel, dim3(nb), dim3(256), stream, P, rect, blk);
    launch(det_offsets_kernel, dim3(nb), dim3(256), stream, P, rect, (const uint32_t*)blk, goff);
    return hipGetLastError();
}
hipError_t launch_det_gather(int P, const ushort4* rect, const uint32_t* goff, const float* rows, uint32_t R, float* acc, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    launch(det_gather_kernel, dim3((P + 15) / 16), dim3(256), stream, P, rect, goff, rows, R, acc);
    return hipGetLastError();
}
}  // namespace dgr
