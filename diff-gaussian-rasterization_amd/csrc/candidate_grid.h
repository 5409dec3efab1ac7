// candidate_grid.h -- the candidate pixels of a frame, as map expansion (seed.hip) and the keyframe overlap scores
// (keyframe_overlap.hip) number them: every stride-th pixel of every stride-th row, row-major.
#pragma once
#include <hip/hip_runtime.h>

namespace dgr {

struct CandidateGrid {  // the candidates: pixel (cx * stride, cy * stride), cx < wc, cy < hc, numbered cy * wc + cx
    int W, H, stride, wc, hc;
    __host__ __device__ size_t candidates() const { return (size_t)wc * (size_t)hc; }
};
__host__ __device__ inline CandidateGrid candidate_grid(int W, int H, int stride) {
    return CandidateGrid{W, H, stride, (int)(((long long)W + stride - 1) / stride), (int)(((long long)H + stride - 1) / stride)};
}

// candidate c -> its grid cell (cx, cy), and its pixel (x, y) = (cx * stride, cy * stride)
__device__ inline void candidate_cell(size_t c, int wc, unsigned& cx, unsigned& cy) {
    cy = (unsigned)(c / (unsigned)wc);
    cx = (unsigned)(c - (size_t)cy * (unsigned)wc);
}
__device__ inline void candidate_pixel(size_t c, int wc, int stride, unsigned& x, unsigned& y) {
    candidate_cell(c, wc, x, y);
    x *= (unsigned)stride, y *= (unsigned)stride;
}

}  // namespace dgr
