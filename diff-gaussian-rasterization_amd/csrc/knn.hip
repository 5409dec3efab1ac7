// knn.hip -- exact k-nearest-neighbour search (include/dgr_hip.h: dgr_knn_build, dgr_knn_search), gfx950, wave64.  The rule (the
// distance, the order of the candidates, what is admitted) is stated in the header; this file is how the answer is found fast.
//
// build: the bounding box of the valid points (integer atomics on order-mapped float bits), a 30-bit Morton key per point on
//   that box (invalid points: 0xFFFFFFFF), a stable LSD radix sort of (key, index) -- four passes of 8 bits, each a histogram
//   launch, plan.h's one-workgroup scan of the [digit][block] table and a ranking launch whose ranks come from ballots -- then
//   the sorted float4 (x, y, z, bits of index) records and, per leaf of 256 consecutive records, its exact fp32 box, its first
//   key and its count.  n_valid stays on the device; leaves past it are empty and are never visited.
// search: one lane per query, one single-wave workgroup per 64 queries that are consecutive in Morton order (self mode: the
//   sorted records themselves; cross mode: the queries keyed on the index's box, sorted by the same sort).  The wave visits its
//   own leaf first, then sweeps the blocks of 64 leaves outwards from its own: lane = leaf tests 64 boxes against the wave's
//   query box and its largest bound, the ballot is walked, each set leaf is tested again with every lane's own bound and visited
//   only if some lane still needs it.  A visit stages 64 records in LDS and every lane reads them as broadcasts; a lane inserts
//   into K sorted registers (K = 1, 3, 4, 8, 16: k rounded up, fully unrolled, no scratch).
// Why the index cannot change a bit: a box's bound is the SAME rounded formula evaluated at the box's nearest point (per-axis gap
//   max(0, lo - q, q - hi) by one rounded subtraction), rounding is monotone, so the bound never exceeds the fp32 d2 of a point
//   inside; a leaf is skipped only on bound > limit, and the candidates are totally ordered by (d2, index), so the k smallest
//   are the same set in whatever order the leaves are visited.
// Every operation of the distance is rounded once: the file is compiled with contraction off.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "plan.h"

#pragma clang fp contract(off)

namespace dgr {
namespace {

constexpr int LEAF = 256;                           // records per leaf
constexpr int SORT_ROUNDS = 16;                     // keys per lane and pass
constexpr int SORT_WAVE_KEYS = 64 * SORT_ROUNDS;    // a wave's consecutive keys
constexpr int SORT_BLOCK_KEYS = 4 * SORT_WAVE_KEYS;  // a workgroup's
constexpr unsigned KEY_INVALID = 0xFFFFFFFFu;
constexpr int KNN_MAX = 1 << 24;
constexpr int NO_INDEX = 0x7fffffff;  // an empty slot's index: every real candidate orders before it

struct KnnHeader {  // 64 bytes at the start of the index
    unsigned lo[3], hi[3];  // the box of the valid points as order-mapped bits
    int n_valid;
    int pad[9];
};
struct KnnIndexView {
    KnnHeader* head;
    float4* recs;     // [P] sorted (x, y, z, bits of index)
    float4* leaf_lo;  // [B] (min, bits of the first key)
    float4* leaf_hi;  // [B] (max, bits of the count)
};
inline size_t leaves_of(size_t P) { return (P + LEAF - 1) / LEAF; }
inline KnnIndexView index_view(void* index, size_t P) {
    char* p = static_cast<char*>(index);
    KnnIndexView v;
    v.head = reinterpret_cast<KnnHeader*>(p);
    v.recs = reinterpret_cast<float4*>(p + 64);
    v.leaf_lo = v.recs + P;
    v.leaf_hi = v.leaf_lo + leaves_of(P);
    return v;
}
inline size_t sort_blocks(size_t n) { return (n + SORT_BLOCK_KEYS - 1) / SORT_BLOCK_KEYS; }
inline size_t words16(size_t n) { return (n * 4 + 15) & ~(size_t)15; }  // bytes of n words, a 16-byte multiple
inline size_t sort_bytes(size_t n) { return 4 * words16(n) + sort_blocks(n) * 256 * 4; }

// the block totals' record for plan.h's scan
struct SortCount {
    int n;
};
__device__ inline SortCount totals_zero(const SortCount*) { return {0}; }
__device__ inline SortCount totals_add(SortCount a, SortCount b) { return {a.n + b.n}; }
__device__ inline SortCount totals_sub(SortCount a, SortCount b) { return {a.n - b.n}; }
__device__ inline SortCount totals_shfl_up(SortCount v, int d) { return {__shfl_up(v.n, d)}; }

struct SortBuffers {
    unsigned *keys[2], *vals[2];
    SortCount* table;
};
inline SortBuffers sort_view(void* scratch, size_t n) {
    char* p = static_cast<char*>(scratch);
    SortBuffers s;
    s.keys[0] = reinterpret_cast<unsigned*>(p);
    s.keys[1] = reinterpret_cast<unsigned*>(p + words16(n));
    s.vals[0] = reinterpret_cast<unsigned*>(p + 2 * words16(n));
    s.vals[1] = reinterpret_cast<unsigned*>(p + 3 * words16(n));
    s.table = reinterpret_cast<SortCount*>(p + 4 * words16(n));
    return s;
}

__device__ __forceinline__ bool finite_bits(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return finite_bits(x) && finite_bits(y) && finite_bits(z); }
// floats as unsigned integers of the same order
__device__ __forceinline__ unsigned order_bits(float f) {
    const unsigned u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float order_float(unsigned u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// ---- the key
__device__ __forceinline__ unsigned quantise(float p, float lo, float hi) {  // 10 bits; an axis of zero or non-finite extent: 0
    const float e = hi - lo;
    if (!(e > 0.0f) || !finite_bits(e)) return 0u;
    const float t = (p - lo) / e * 1024.0f;
    return t >= 1023.0f ? 1023u : (t > 0.0f ? (unsigned)t : 0u);
}
__device__ __forceinline__ unsigned spread3(unsigned x) {
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x30000ffu;
    x = (x | (x << 8)) & 0x300f00fu;
    x = (x | (x << 4)) & 0x30c30c3u;
    x = (x | (x << 2)) & 0x9249249u;
    return x;
}
__device__ __forceinline__ unsigned morton_key(const KnnHeader* h, float x, float y, float z) {
    if (!finite3(x, y, z)) return KEY_INVALID;
    const unsigned qx = quantise(x, order_float(h->lo[0]), order_float(h->hi[0]));
    const unsigned qy = quantise(y, order_float(h->lo[1]), order_float(h->hi[1]));
    const unsigned qz = quantise(z, order_float(h->lo[2]), order_float(h->hi[2]));
    return spread3(qx) | (spread3(qy) << 1) | (spread3(qz) << 2);
}

__global__ void knn_init_kernel(KnnHeader* h) {
    const int t = threadIdx.x;
    if (t < 3) h->lo[t] = 0xFF800000u;  // +inf
    else if (t < 6) h->hi[t - 3] = 0x007FFFFFu;  // -inf
    else if (t < 16) reinterpret_cast<int*>(h)[t] = 0;
}

__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, d));
    return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, d));
    return v;
}

// the box and the number of the valid points: 1024 points per workgroup, six integer atomics and one add per wave
__global__ __launch_bounds__(256) void knn_bbox_kernel(int P, const float* __restrict__ pts, KnnHeader* h) {
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    int n = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t i = (size_t)blockIdx.x * 1024 + r * 256 + threadIdx.x;
        if (i < (size_t)P) {
            const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
            if (finite3(x, y, z)) {
                const unsigned b[3] = {order_bits(x), order_bits(y), order_bits(z)};
#pragma unroll
                for (int a = 0; a < 3; ++a) lo[a] = min(lo[a], b[a]), hi[a] = max(hi[a], b[a]);
                ++n;
            }
        }
    }
    const unsigned long long any = __ballot(n > 0);
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = wave_min(lo[a]), hi[a] = wave_max(hi[a]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
    if ((threadIdx.x & 63) == 0 && any) {
#pragma unroll
        for (int a = 0; a < 3; ++a) atomicMin(&h->lo[a], lo[a]), atomicMax(&h->hi[a], hi[a]);
        atomicAdd(&h->n_valid, n);
    }
}

__global__ __launch_bounds__(256) void knn_keys_kernel(int n, const float* __restrict__ pts, const KnnHeader* __restrict__ h,
                                                        unsigned* __restrict__ keys, unsigned* __restrict__ vals) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    keys[i] = morton_key(h, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    vals[i] = (unsigned)i;
}

// ---- the sort: one pass of 8 bits
// the lanes of the wave that hold the same digit (and are valid), by eight ballots
__device__ __forceinline__ unsigned long long digit_peers(unsigned digit, bool valid) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const bool b = (digit >> bit) & 1u;
        const unsigned long long m = __ballot(b);
        peers &= b ? m : ~m;
    }
    return peers;
}
__device__ __forceinline__ size_t sort_item(int round) {
    return (size_t)blockIdx.x * SORT_BLOCK_KEYS + (size_t)(threadIdx.x >> 6) * SORT_WAVE_KEYS + (size_t)round * 64 + (threadIdx.x & 63);
}

// table[digit * blocks + block] = how many of the block's keys hold the digit
__global__ __launch_bounds__(256) void knn_sort_count_kernel(int n, const unsigned* __restrict__ keys, int shift, SortCount* __restrict__ table) {
    __shared__ int hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const size_t i = sort_item(r);
        const bool valid = i < (size_t)n;
        const unsigned digit = valid ? (keys[i] >> shift) & 255u : 0u;
        const unsigned long long peers = digit_peers(digit, valid);
        if (valid && lane == __ffsll((long long)peers) - 1) atomicAdd(&hist[digit], __popcll(peers));
    }
    __syncthreads();
    table[(size_t)threadIdx.x * gridDim.x + blockIdx.x].n = hist[threadIdx.x];
}

__global__ __launch_bounds__(256) void knn_sort_scan_kernel(SortCount* table, size_t entries) {
    __shared__ SortCount wave_sum[4];
    scan_block_totals(table, entries, wave_sum);
}

// stable: a key's place is the table's offset of (digit, block), plus the keys of that digit in the block's earlier waves, plus
// those earlier in its own wave -- each wave owns SORT_WAVE_KEYS consecutive keys and walks them in order
__global__ __launch_bounds__(256) void knn_sort_rank_kernel(int n, const unsigned* __restrict__ keys_in, const unsigned* __restrict__ vals_in,
                                                             int shift, const SortCount* __restrict__ table, unsigned* __restrict__ keys_out,
                                                             unsigned* __restrict__ vals_out) {
    __shared__ int base[4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int w = 0; w < 4; ++w) base[w][threadIdx.x] = 0;
    __syncthreads();
    // `mine` is this wave's row, touched by no other wave between the barriers.  Its lanes hand the running offsets to each other
    // from round to round through it: a round's leader lanes write, any lane may read the entry in the next round.  That is in
    // order because the loops are wave-uniform and a wave's LDS operations complete in issue order; the volatile accesses keep
    // the compiler from caching an entry in a register, and the wave barrier after each write from moving accesses across it.
    volatile int* mine = base[wave];
    for (int r = 0; r < SORT_ROUNDS; ++r) {  // the wave's counts, in its own row
        const size_t i = sort_item(r);
        const bool valid = i < (size_t)n;
        const unsigned digit = valid ? (keys_in[i] >> shift) & 255u : 0u;
        const unsigned long long peers = digit_peers(digit, valid);
        if (valid && lane == __ffsll((long long)peers) - 1) mine[digit] = mine[digit] + __popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {  // counts -> where each wave's first key of the digit goes
        int at = table[(size_t)threadIdx.x * gridDim.x + blockIdx.x].n;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = base[w][threadIdx.x];
            base[w][threadIdx.x] = at;
            at += c;
        }
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const size_t i = sort_item(r);
        const bool valid = i < (size_t)n;
        const unsigned key = valid ? keys_in[i] : 0u;
        const unsigned digit = (key >> shift) & 255u;
        const unsigned long long peers = digit_peers(digit, valid);
        if (valid) {
            const int first = mine[digit];
            const int at = first + __popcll(peers & below);  // (a permutation of 0 .. n - 1: the counts above are of these keys)
            keys_out[at] = key;
            vals_out[at] = vals_in[i];
            if (lane == __ffsll((long long)peers) - 1) mine[digit] = first + __popcll(peers);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- sorted records and leaves
__device__ __forceinline__ float wave_fmin(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ float wave_fmax(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

// one workgroup per 256 sorted places: recs[j] = (point vals[j], bits of vals[j]); LEAVES: the leaf's box, first key and count
template <bool LEAVES>
__global__ __launch_bounds__(256) void knn_records_kernel(int n, const float* __restrict__ pts, const unsigned* __restrict__ keys,
                                                           const unsigned* __restrict__ vals, const KnnHeader* __restrict__ h,
                                                           float4* __restrict__ recs, float4* __restrict__ leaf_lo, float4* __restrict__ leaf_hi) {
    __shared__ float box[4][6];
    const size_t j = (size_t)blockIdx.x * LEAF + threadIdx.x;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (j < (size_t)n) {
        const size_t i = vals[j];
        x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        recs[j] = make_float4(x, y, z, __int_as_float((int)i));
    }
    if (!LEAVES) return;
    const int n_valid = h->n_valid;
    const bool valid = j < (size_t)n_valid;
    const float inf = __int_as_float(0x7f800000);
    const float lo[3] = {wave_fmin(valid ? x : inf), wave_fmin(valid ? y : inf), wave_fmin(valid ? z : inf)};
    const float hi[3] = {wave_fmax(valid ? x : -inf), wave_fmax(valid ? y : -inf), wave_fmax(valid ? z : -inf)};
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) box[wave][a] = lo[a], box[wave][3 + a] = hi[a];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float l[3], u[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            l[a] = fminf(fminf(box[0][a], box[1][a]), fminf(box[2][a], box[3][a]));
            u[a] = fmaxf(fmaxf(box[0][3 + a], box[1][3 + a]), fmaxf(box[2][3 + a], box[3][3 + a]));
        }
        const long long first = (long long)blockIdx.x * LEAF;
        const int count = first >= n_valid ? 0 : (n_valid - first > LEAF ? LEAF : (int)(n_valid - first));
        leaf_lo[blockIdx.x] = make_float4(l[0], l[1], l[2], __uint_as_float(count > 0 ? keys[first] : KEY_INVALID));
        leaf_hi[blockIdx.x] = make_float4(u[0], u[1], u[2], __int_as_float(count));
    }
}

// ---- the search
struct KnnSearchArgs {
    const KnnHeader* head;
    const float4 *recs, *leaf_lo, *leaf_hi;
    const float4* qrecs;  // the queries in Morton order, (x, y, z, bits of the row they answer)
    int Q, k, exclude_self, self;
    float max_d2;
    float* dist2;
    int* idx;
    int* count;
    float* mean;
};

// the rule's distance: every operation rounded once (contraction is off in this file)
__device__ __forceinline__ float dist2_rn(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}
// the same formula at the nearest point of the box [lo, hi] to q, or of the box to the box [qlo, qhi]: never above the distance
// of any point inside (rounding is monotone)
__device__ __forceinline__ float gap_rn(float lo, float hi, float qlo, float qhi) { return fmaxf(0.0f, fmaxf(lo - qhi, qlo - hi)); }
__device__ __forceinline__ float box_bound(const float4& lo, const float4& hi, float qlx, float qly, float qlz, float qhx, float qhy, float qhz) {
    const float gx = gap_rn(lo.x, hi.x, qlx, qhx), gy = gap_rn(lo.y, hi.y, qly, qhy), gz = gap_rn(lo.z, hi.z, qlz, qhz);
    return (gx * gx + gy * gy) + gz * gz;
}

template <int K>
struct Best {
    float d[K];
    int i[K];
    float kd;  // slot k - 1: what a candidate has to beat
    int ki;
};
template <int K>
__device__ __forceinline__ void best_kth(Best<K>& b, int k) {
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j == k - 1) b.kd = b.d[j], b.ki = b.i[j];
}
template <int K>
__device__ __forceinline__ void best_insert(Best<K>& b, float cd, int ci) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool lt = cd < b.d[j] || (cd == b.d[j] && ci < b.i[j]);
        const float td = b.d[j];
        const int ti = b.i[j];
        b.d[j] = lt ? cd : td, b.i[j] = lt ? ci : ti;
        cd = lt ? td : cd, ci = lt ? ti : ci;
    }
}

// one record against every lane's query
template <int K>
__device__ __forceinline__ void consider(const KnnSearchArgs& a, const float4 p, bool valid, float qx, float qy, float qz, int excl,
                                         Best<K>& best) {
    const float d2 = dist2_rn(p.x, p.y, p.z, qx, qy, qz);
    const int pi = __float_as_int(p.w);
    const bool take = valid && d2 <= a.max_d2 && pi != excl && (d2 < best.kd || (d2 == best.kd && pi < best.ki));
    if (__any(take)) {
        if (take) {
            best_insert(best, d2, pi);
            best_kth(best, a.k);
        }
    }
}

// the wave reads leaf `leaf` (count records) through LDS, 64 records at a time, every lane against its own query.  (Measured
// against reading each record as a wave-uniform load straight from memory: equal at 100 k points, the LDS stage 12 - 17 % faster
// at 500 k, profiles/knn/ab_uniform_loads.txt.)
template <int K>
__device__ __forceinline__ void visit_leaf(const KnnSearchArgs& a, int leaf, int count, float4* stage, bool valid, float qx, float qy,
                                           float qz, int excl, Best<K>& best) {
    const int lane = threadIdx.x;
    for (int c = 0; c < count; c += 64) {
        const int m = count - c < 64 ? count - c : 64;
        __syncthreads();  // (one wave: orders the LDS accesses)
        if (lane < m) stage[lane] = a.recs[(size_t)leaf * LEAF + c + lane];
        __syncthreads();
        for (int r = 0; r < m; ++r) consider<K>(a, stage[r], valid, qx, qy, qz, excl, best);
    }
}

template <int K>
__global__ __launch_bounds__(64) void knn_search_kernel(KnnSearchArgs a) {
    __shared__ float4 stage[64];
    const int lane = threadIdx.x;
    const size_t qpos = (size_t)blockIdx.x * 64 + lane;
    const int n_valid = a.head->n_valid;
    const int nleaves = (n_valid + LEAF - 1) / LEAF;
    const float inf = __int_as_float(0x7f800000);
    const bool inside = qpos < (size_t)a.Q;
    const float4 q = inside ? a.qrecs[qpos] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int row = __float_as_int(q.w);
    const bool valid = inside && finite3(q.x, q.y, q.z);
    const int excl = a.exclude_self ? row : -1;
    Best<K> best;
#pragma unroll
    for (int j = 0; j < K; ++j) best.d[j] = inf, best.i[j] = NO_INDEX;
    best.kd = inf, best.ki = NO_INDEX;

    const unsigned long long live = __ballot(valid);
    if (live != 0ull && nleaves > 0) {
        // the leaf the sweep starts from: the wave's first valid query's own
        int own;
        if (a.self) {
            own = (int)(((size_t)blockIdx.x * 64) / LEAF);
        } else {
            const unsigned key = morton_key(a.head, q.x, q.y, q.z);
            int l = 0, r = nleaves;  // the last leaf whose first key is not above the query's (or leaf 0)
            for (int it = 0; it < 32 && r - l > 1; ++it) {
                const int mid = (l + r) >> 1;
                if (__float_as_uint(a.leaf_lo[mid].w) <= key) l = mid;
                else r = mid;
            }
            own = __shfl(l, __ffsll((long long)live) - 1);
        }
        own = __builtin_amdgcn_readfirstlane(own);
        own = own < 0 ? 0 : (own >= nleaves ? nleaves - 1 : own);
        visit_leaf<K>(a, own, __float_as_int(a.leaf_hi[own].w), stage, valid, q.x, q.y, q.z, excl, best);

        // the wave's query box
        const float wlx = wave_fmin(valid ? q.x : inf), wly = wave_fmin(valid ? q.y : inf), wlz = wave_fmin(valid ? q.z : inf);
        const float whx = wave_fmax(valid ? q.x : -inf), why = wave_fmax(valid ? q.y : -inf), whz = wave_fmax(valid ? q.z : -inf);
        const int blocks = (nleaves + 63) >> 6, own_block = own >> 6;
        for (int step = 0; step <= 2 * blocks; ++step) {  // own_block, -1, +1, -2, +2, ...
            const int off = (step + 1) >> 1;
            const int blk = (step & 1) ? own_block - off : own_block + off;
            if (blk < 0 || blk >= blocks) continue;
            // what a leaf may not exceed for some lane of the wave
            const float wave_limit = wave_fmax(valid ? fminf(best.kd, a.max_d2) : -1.0f);
            const int mine = blk * 64 + lane;
            bool open = false;
            if (mine < nleaves && mine != own) {
                const float4 lo = a.leaf_lo[mine], hi = a.leaf_hi[mine];
                open = __float_as_int(hi.w) > 0 && box_bound(lo, hi, wlx, wly, wlz, whx, why, whz) <= wave_limit;
            }
            unsigned long long todo = __ballot(open);
            while (todo) {
                const int leaf = blk * 64 + (__ffsll((long long)todo) - 1);
                todo &= todo - 1ull;
                const float4 lo = a.leaf_lo[leaf], hi = a.leaf_hi[leaf];
                const float bound = box_bound(lo, hi, q.x, q.y, q.z, q.x, q.y, q.z);
                if (!__any(valid && bound <= fminf(best.kd, a.max_d2))) continue;
                visit_leaf<K>(a, leaf, __float_as_int(hi.w), stage, valid, q.x, q.y, q.z, excl, best);
            }
        }
    }

    if (!inside) return;
    const int k = a.k;
    int found = 0;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k && best.i[j] != NO_INDEX) ++found;
    if (a.dist2 || a.idx) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j < k) {
                const bool has = best.i[j] != NO_INDEX;
                if (a.dist2) a.dist2[(size_t)row * k + j] = has ? best.d[j] : inf;
                if (a.idx) a.idx[(size_t)row * k + j] = has ? best.i[j] : -1;
            }
        }
    }
    if (a.count) a.count[row] = found;
    if (a.mean) {
        float s = best.d[0];  // (an empty slot holds +inf)
#pragma unroll
        for (int j = 1; j < K; ++j)
            if (j < k) s = s + best.d[j];
        a.mean[row] = s / (float)k;
    }
}

// (key, index) pairs of s.keys[0], s.vals[0] sorted by key, stable; the result is back in buffers 0
void launch_sort(const SortBuffers& s, int n, hipStream_t stream) {
    const unsigned blocks = (unsigned)sort_blocks((size_t)n);
    for (int pass = 0; pass < 4; ++pass) {
        const int in = pass & 1, out = in ^ 1;
        launch(knn_sort_count_kernel, dim3(blocks), dim3(256), stream, n, (const unsigned*)s.keys[in], 8 * pass, s.table);
        launch(knn_sort_scan_kernel, dim3(1), dim3(256), stream, s.table, (size_t)blocks * 256);
        launch(knn_sort_rank_kernel, dim3(blocks), dim3(256), stream, n, (const unsigned*)s.keys[in], (const unsigned*)s.vals[in], 8 * pass,
               (const SortCount*)s.table, s.keys[out], s.vals[out]);
    }
}

}  // namespace

size_t knn_index_bytes(int n_points) {
    if (n_points < 1 || n_points > KNN_MAX) return 0;
    return 64 + 16 * (size_t)n_points + 32 * leaves_of((size_t)n_points);
}
size_t knn_scratch_bytes(int n_points, int n_queries) {
    if (n_points < 1 || n_points > KNN_MAX || n_queries < 1 || n_queries > KNN_MAX) return 0;
    const size_t build = sort_bytes((size_t)n_points), search = sort_bytes((size_t)n_queries) + 16 * (size_t)n_queries;
    return build > search ? build : search;
}

hipError_t launch_knn_build(int P, const float* points, void* index, void* scratch, hipStream_t stream) {
    const KnnIndexView v = index_view(index, (size_t)P);
    const SortBuffers s = sort_view(scratch, (size_t)P);
    launch(knn_init_kernel, dim3(1), dim3(64), stream, v.head);
    launch(knn_bbox_kernel, dim3((unsigned)((P + 1023) / 1024)), dim3(256), stream, P, points, v.head);
    launch(knn_keys_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), stream, P, points, (const KnnHeader*)v.head, s.keys[0], s.vals[0]);
    launch_sort(s, P, stream);
    launch(knn_records_kernel<true>, dim3((unsigned)leaves_of((size_t)P)), dim3(256), stream, P, points, (const unsigned*)s.keys[0],
           (const unsigned*)s.vals[0], (const KnnHeader*)v.head, v.recs, v.leaf_lo, v.leaf_hi);
    return hipGetLastError();
}

hipError_t launch_knn_search(const KnnSearchCall& c, hipStream_t stream) {
    const KnnIndexView v = index_view(const_cast<void*>(c.index), (size_t)c.n_points);
    KnnSearchArgs a{};
    a.head = v.head, a.recs = v.recs, a.leaf_lo = v.leaf_lo, a.leaf_hi = v.leaf_hi;
    a.Q = c.n_queries, a.k = c.k, a.exclude_self = c.exclude_self, a.self = c.queries ? 0 : 1, a.max_d2 = c.max_dist2;
    a.dist2 = c.dist2, a.idx = c.idx, a.count = c.count, a.mean = c.mean_dist2;
    if (c.queries) {
        const int Q = c.n_queries;
        const SortBuffers s = sort_view(c.scratch, (size_t)Q);
        float4* qrecs = reinterpret_cast<float4*>(static_cast<char*>(c.scratch) + sort_bytes((size_t)Q));
        launch(knn_keys_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), stream, Q, c.queries, (const KnnHeader*)v.head, s.keys[0], s.vals[0]);
        launch_sort(s, Q, stream);
        launch(knn_records_kernel<false>, dim3((unsigned)leaves_of((size_t)Q)), dim3(256), stream, Q, c.queries, (const unsigned*)s.keys[0],
               (const unsigned*)s.vals[0], (const KnnHeader*)v.head, qrecs, (float4*)nullptr, (float4*)nullptr);
        a.qrecs = qrecs;
    } else {
        a.qrecs = v.recs;
    }
    const dim3 grid((unsigned)((c.n_queries + 63) / 64));
    const int k = c.k;
    if (k == 1) launch(knn_search_kernel<1>, grid, dim3(64), stream, a);
    else if (k <= 3) launch(knn_search_kernel<3>, grid, dim3(64), stream, a);
    else if (k == 4) launch(knn_search_kernel<4>, grid, dim3(64), stream, a);
    else if (k <= 8) launch(knn_search_kernel<8>, grid, dim3(64), stream, a);
    else launch(knn_search_kernel<16>, grid, dim3(64), stream, a);
    return hipGetLastError();
}

}  // namespace dgr
