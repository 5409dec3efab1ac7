// philox.h -- the counter-based generator of the map-upkeep steps (densify-and-prune's children in optim.hip, relocation's draws
// and the position noise in relocate.hip): Philox4x32-10 (Salmon et al., SC'11) keyed by the caller's seed.  A value is a pure
// function of (seed, counter): it does not depend on the grid, on the launch order or on which other rows draw.
#pragma once
#include <hip/hip_runtime.h>

namespace dgr {

// the four words of counter (row, sample, stream) under key `seed`
__device__ inline uint4 philox_words(unsigned long long seed, unsigned long long row, unsigned sample, unsigned stream) {
    unsigned c0 = (unsigned)row, c1 = (unsigned)(row >> 32), c2 = sample, c3 = stream;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// Box-Muller turns the four words of counter (row, sample, 0) into four standard normals; `component` 0 .. 3 picks one.
__device__ inline float philox_normal(unsigned long long seed, unsigned long long row, unsigned sample, int component) {
    const uint4 w = philox_words(seed, row, sample, 0u);
    const unsigned a = component < 2 ? w.x : w.z, b = component < 2 ? w.y : w.w;
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;  // (0, 1]
    const float u2 = (float)(b >> 8) * 0x1p-24f;         // [0, 1)
    const float radius = sqrtf(-2.0f * logf(u1)), angle = 6.283185307179586f * u2;
    return radius * ((component & 1) ? sinf(angle) : cosf(angle));
}

}  // namespace dgr
