// C entry points around the reference rasterizer as oracle/build_ref.py compiles it for gfx950 (one library per variant:
// -DDGR_REF_FULL selects the full one).  TEST INFRASTRUCTURE ONLY.  Our own text: it includes the reference's rasterizer.h /
// rasterizer_impl.h from the copied sources under oracle/_ref/ and calls Rasterizer::forward / backward with the reference's
// arguments in the reference's order.
//
// Every pointer argument is a HOST pointer (NULL where the reference's Python layer passes an empty tensor); the wrapper
// uploads the inputs, zero-fills the outputs as rasterize_points.cu does, and copies the results back.  The three
// std::function<char*(size_t)> callbacks are served from device buffers that the state object owns and grows.  The reference
// works on the null stream with blocking copies: hipDeviceSynchronize() on entry and on exit; the return value is the HIP
// error code (0 = success), or a negative number for a call that the wrapper refuses:
//   -1  prefiltered = true (in_frustum would print and trap)      -2  P <= 0 (forward reads point_offsets[P - 1])
//   -3  the reference threw                                        -4  backward without a forward, or of a frame with R = 0
// NaN inputs are the caller's to avoid.  The full variant's backward is NOT exposed (ComputePG returns ahead of block-wide
// barriers).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "rasterizer_impl.h"

using namespace CudaRasterizer;

namespace {

struct DevBuf {
    char* p = nullptr;
    size_t cap = 0, size = 0;
    char* grow(size_t n) {
        if (n > cap) {
            if (p) (void)hipFree(p);
            p = nullptr;
            cap = 0;
            if (hipMalloc(reinterpret_cast<void**>(&p), n) != hipSuccess) throw std::runtime_error("hipMalloc");
            cap = n;
        }
        size = n;
        return p;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

struct State {
    DevBuf geom, binning, img, radii;
    int P = 0, W = 0, H = 0, R = -1;
};

// device copies / zero-filled device arrays that live for one call
struct Call {
    std::vector<void*> owned;
    hipError_t err = hipSuccess;
    void note(hipError_t e) {
        if (err == hipSuccess) err = e;
    }
    template <typename T>
    T* zeros(size_t n) {
        void* d = nullptr;
        note(hipMalloc(&d, (n ? n : 1) * sizeof(T)));
        if (!d) throw std::runtime_error("hipMalloc");
        owned.push_back(d);
        note(hipMemset(d, 0, (n ? n : 1) * sizeof(T)));
        return static_cast<T*>(d);
    }
    template <typename T>
    T* up(const T* h, size_t n) {
        if (!h || !n) return nullptr;
        T* d = zeros<T>(n);
        note(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    template <typename T>
    void down(T* h, const T* d, size_t n) {
        if (h && n) note(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
    }
    ~Call() {
        for (void* d : owned) (void)hipFree(d);
    }
};

long copy_out(void* dst, long cap_bytes, const void* src, size_t n, size_t elem) {
    if (static_cast<size_t>(cap_bytes) < n * elem) return -2;
    if (n && hipMemcpy(dst, src, n * elem, hipMemcpyDeviceToHost) != hipSuccess) return -3;
    return static_cast<long>(n);
}

}  // namespace

extern "C" {

const char* dgr_ref_variant() {
#ifdef DGR_REF_FULL
    return "full";
#else
    return "light";
#endif
}

void* dgr_ref_state_new() { return new State(); }

void dgr_ref_state_free(void* h) {
    (void)hipDeviceSynchronize();
    delete static_cast<State*>(h);
}

int dgr_ref_state_num_rendered(void* h) { return static_cast<State*>(h)->R; }

// One field of GeometryState / BinningState / ImageState, located by the reference's own fromChunk, copied to `dst` (host,
// `cap_bytes` large).  Returns the element count, -1 for an unknown name, -2 if dst is too small, -3 on a HIP error.
long dgr_ref_state_get(void* h, const char* name, void* dst, long cap_bytes) {
    State& st = *static_cast<State*>(h);
    if (st.R < 0 || hipDeviceSynchronize() != hipSuccess) return -3;
    const size_t P = st.P, N = static_cast<size_t>(st.W) * st.H, R = st.R;
    const size_t tiles = static_cast<size_t>((st.W + 15) / 16) * ((st.H + 15) / 16);
    const std::string n(name);
    if (n == "radii") return copy_out(dst, cap_bytes, st.radii.p, P, 4);
    char* c = st.geom.p;
    GeometryState g = GeometryState::fromChunk(c, P);
    if (n == "depths") return copy_out(dst, cap_bytes, g.depths, P, 4);
    if (n == "means2D") return copy_out(dst, cap_bytes, g.means2D, 2 * P, 4);
    if (n == "conic_opacity") return copy_out(dst, cap_bytes, g.conic_opacity, 4 * P, 4);
    if (n == "rgb") return copy_out(dst, cap_bytes, g.rgb, 3 * P, 4);
    if (n == "clamped") return copy_out(dst, cap_bytes, g.clamped, 3 * P, 1);
    if (n == "cov3D") return copy_out(dst, cap_bytes, g.cov3D, 6 * P, 4);
    if (n == "tiles_touched") return copy_out(dst, cap_bytes, g.tiles_touched, P, 4);
    if (n == "point_offsets") return copy_out(dst, cap_bytes, g.point_offsets, P, 4);
    c = st.img.p;
    ImageState im = ImageState::fromChunk(c, N);
    if (n == "ranges") return copy_out(dst, cap_bytes, im.ranges, 2 * tiles, 4);
    if (n == "n_contrib") return copy_out(dst, cap_bytes, im.n_contrib, N, 4);
#ifdef DGR_REF_FULL
    if (n == "accum_alpha") return copy_out(dst, cap_bytes, im.accum_alpha, N, 4);
    if (n == "n_valid_contrib") return copy_out(dst, cap_bytes, im.n_valid_contrib, N, 4);
#endif
    if (n == "point_list" || n == "keys" || n == "point_list_keys") {
        if (R == 0) return 0;
        c = st.binning.p;
        BinningState b = BinningState::fromChunk(c, R);
        if (n == "point_list") return copy_out(dst, cap_bytes, b.point_list, R, 4);
        return copy_out(dst, cap_bytes, b.point_list_keys, R, 8);
    }
    return -1;
}

#ifndef DGR_REF_FULL
int dgr_ref_forward(void* h, int P, int D, int M, const float* bg, int W, int H, const float* means,
                    const float* shs, const float* colors, const float* opac, const float* scales,
                    float mod, const float* rots, const float* cov, const float* view,
                    const float* proj, const float* cam, float tanx, float tany, int prefiltered,
                    float* o_color, float* o_depth, float* o_median, float* o_alpha, const float* gt,
                    float* o_var, float* o_gau_unc, int* o_gau_pix, int* radii, int* n_rendered) {
    State& st = *static_cast<State*>(h);
    st.R = -1;
    if (prefiltered) return -1;
    if (P <= 0 || W <= 0 || H <= 0) return -2;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    const size_t N = static_cast<size_t>(W) * H, p = P;
    try {
        Call c;
        st.P = P, st.W = W, st.H = H;
        int* d_radii = reinterpret_cast<int*>(st.radii.grow(p * sizeof(int)));
        c.note(hipMemset(d_radii, 0, p * sizeof(int)));
        float *d_color = c.zeros<float>(3 * N), *d_depth = c.zeros<float>(N), *d_median = c.zeros<float>(N);
        float *d_alpha = c.zeros<float>(N), *d_var = c.zeros<float>(N), *d_unc = c.zeros<float>(p);
        int* d_rel = c.zeros<int>(p);
        const float *d_bg = c.up(bg, 3), *d_means = c.up(means, 3 * p), *d_shs = c.up(shs, 3 * p * M);
        const float *d_cp = c.up(colors, 3 * p), *d_op = c.up(opac, p), *d_sc = c.up(scales, 3 * p);
        const float *d_rot = c.up(rots, 4 * p), *d_cov = c.up(cov, 6 * p), *d_view = c.up(view, 16);
        const float *d_proj = c.up(proj, 16), *d_cam = c.up(cam, 3), *d_gt = c.up(gt, N);
        if (c.err != hipSuccess) return c.err;
        const int R = Rasterizer::forward([&](size_t n) { return st.geom.grow(n); }, [&](size_t n) { return st.binning.grow(n); },
                                          [&](size_t n) { return st.img.grow(n); }, P, D, M, d_bg, W, H, d_means, d_shs,
                                          d_cp, d_op, d_sc, mod, d_rot, d_cov, d_view, d_proj, d_cam, tanx, tany,
                                          false, d_color, d_depth, d_median, d_alpha, d_gt, d_var, d_unc, d_rel, d_radii, false);
        c.note(hipDeviceSynchronize());
        c.note(hipGetLastError());
        if (c.err != hipSuccess) return c.err;
        c.down(o_color, d_color, 3 * N), c.down(o_depth, d_depth, N), c.down(o_median, d_median, N);
        c.down(o_alpha, d_alpha, N), c.down(o_var, d_var, N), c.down(o_gau_unc, d_unc, p);
        c.down(o_gau_pix, d_rel, p), c.down(radii, d_radii, p);
        if (c.err != hipSuccess) return c.err;
        st.R = R;
        *n_rendered = R;
    } catch (const std::exception&) {
        return -3;
    }
    return hipDeviceSynchronize();
}

// dgndcs_dviewmatrix [P,12,2], dg_camd_dviewmatrix [P,4] and o_view [H W,16] are allocated here, zeroed, as rasterize_points.cu
// does; `o_view` (host) receives the PER-PIXEL [H W,16] array: its sum over the pixels is the caller's, as in the reference's
// __init__.py.  `radii`: the forward's, host.
int dgr_ref_backward(void* h, int P, int D, int M, int R, const float* bg, int W, int H, const float* means,
                     const float* shs, const float* colors, const float* alpha_img, const float* scales,
                     float mod, const float* rots, const float* cov, const float* view,
                     const float* proj, const float* cam, float tanx, float tany, const int* radii,
                     const float* in_gc, const float* in_gd, const float* in_gm,
                     const float* in_gv, float* o_m2, float* o_con, float* o_op, float* o_col,
                     float* o_dep, float* o_m3, float* o_cov, float* o_sh, float* o_sc, float* o_rot,
                     const float* persp, float* o_view, const float* gt, int track_off, int map_off) {
    State& st = *static_cast<State*>(h);
    if (st.R <= 0 || R != st.R || P != st.P || W != st.W || H != st.H || !radii) return -4;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    const size_t N = static_cast<size_t>(W) * H, p = P;
    try {
        Call c;
        float *g_m2 = c.zeros<float>(3 * p), *g_con = c.zeros<float>(4 * p), *g_op = c.zeros<float>(p), *g_col = c.zeros<float>(3 * p);
        float *g_dep = c.zeros<float>(p), *g_m3 = c.zeros<float>(3 * p), *g_cov = c.zeros<float>(6 * p);
        float *g_sh = c.zeros<float>(3 * p * M), *g_sc = c.zeros<float>(3 * p), *g_rot = c.zeros<float>(4 * p);
        float *d_dgndcs = c.zeros<float>(24 * p), *d_dgcamd = c.zeros<float>(4 * p), *g_view = c.zeros<float>(16 * N);
        const float *d_bg = c.up(bg, 3), *d_means = c.up(means, 3 * p), *d_shs = c.up(shs, 3 * p * M);
        const float *d_cp = c.up(colors, 3 * p), *d_al = c.up(alpha_img, N), *d_sc = c.up(scales, 3 * p);
        const float *d_rot = c.up(rots, 4 * p), *d_cov = c.up(cov, 6 * p), *d_view = c.up(view, 16);
        const float *d_proj = c.up(proj, 16), *d_cam = c.up(cam, 3), *d_gt = c.up(gt, N);
        const float *d_gc = c.up(in_gc, 3 * N), *d_gd = c.up(in_gd, N), *d_gm = c.up(in_gm, N);
        const float *d_gv = c.up(in_gv, N), *d_persp = c.up(persp, 16);
        const int* d_radii = c.up(radii, p);
        if (c.err != hipSuccess) return c.err;
        if (!d_al || !d_gt || !d_gc || !d_gd || !d_gm || !d_gv || !d_persp) return -4;
        Rasterizer::backward(P, D, M, R, d_bg, W, H, d_means, d_shs, d_cp, d_al, d_sc, mod, d_rot, d_cov, d_view,
                             d_proj, d_cam, tanx, tany, d_radii, st.geom.p, st.binning.p, st.img.p, d_gc, d_gd, d_gm, d_gv,
                             g_m2, g_con, g_op, g_col, g_dep, g_m3, g_cov, g_sh, g_sc, g_rot, false, d_dgndcs, d_persp, g_view,
                             d_dgcamd, d_gt, track_off != 0, map_off != 0);
        c.note(hipDeviceSynchronize());
        c.note(hipGetLastError());
        if (c.err != hipSuccess) return c.err;
        c.down(o_m2, g_m2, 3 * p), c.down(o_con, g_con, 4 * p), c.down(o_op, g_op, p);
        c.down(o_col, g_col, 3 * p), c.down(o_dep, g_dep, p), c.down(o_m3, g_m3, 3 * p);
        c.down(o_cov, g_cov, 6 * p), c.down(o_sh, g_sh, 3 * p * M), c.down(o_sc, g_sc, 3 * p);
        c.down(o_rot, g_rot, 4 * p), c.down(o_view, g_view, 16 * N);
        if (c.err != hipSuccess) return c.err;
    } catch (const std::exception&) {
        return -3;
    }
    return hipDeviceSynchronize();
}

#else  // ------------------------------------------------------------------------------------------ full: forward only

int dgr_ref_forward(void* h, int P, int D, int M, const float* bg, int W, int H, const float* means,
                    const float* shs, const float* colors, const float* opac, const float* scales,
                    float mod, const float* rots, const float* cov, const float* view,
                    const float* proj, const float* cam, float tanx, float tany, int prefiltered,
                    float* o_color, float* o_depth, const float* gt, float* o_unc, int* radii,
                    int* n_rendered, int* n_related) {
    State& st = *static_cast<State*>(h);
    st.R = -1;
    if (prefiltered) return -1;
    if (P <= 0 || W <= 0 || H <= 0) return -2;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    const size_t N = static_cast<size_t>(W) * H, p = P;
    try {
        Call c;
        st.P = P, st.W = W, st.H = H;
        int* d_radii = reinterpret_cast<int*>(st.radii.grow(p * sizeof(int)));
        c.note(hipMemset(d_radii, 0, p * sizeof(int)));
        float *d_color = c.zeros<float>(3 * N), *d_depth = c.zeros<float>(N), *d_unc = c.zeros<float>(N);
        const float *d_bg = c.up(bg, 3), *d_means = c.up(means, 3 * p), *d_shs = c.up(shs, 3 * p * M);
        const float *d_cp = c.up(colors, 3 * p), *d_op = c.up(opac, p), *d_sc = c.up(scales, 3 * p);
        const float *d_rot = c.up(rots, 4 * p), *d_cov = c.up(cov, 6 * p), *d_view = c.up(view, 16);
        const float *d_proj = c.up(proj, 16), *d_cam = c.up(cam, 3), *d_gt = c.up(gt, N);
        if (c.err != hipSuccess) return c.err;
        int R = 0, NG = 0;
        std::tie(R, NG) = Rasterizer::forward([&](size_t n) { return st.geom.grow(n); }, [&](size_t n) { return st.binning.grow(n); },
                                              [&](size_t n) { return st.img.grow(n); }, P, D, M, d_bg, W, H, d_means,
                                              d_shs, d_cp, d_op, d_sc, mod, d_rot, d_cov, d_view, d_proj, d_cam,
                                              tanx, tany, false, d_color, d_depth, d_gt, d_unc, d_radii);
        c.note(hipDeviceSynchronize());
        c.note(hipGetLastError());
        if (c.err != hipSuccess) return c.err;
        c.down(o_color, d_color, 3 * N), c.down(o_depth, d_depth, N), c.down(o_unc, d_unc, N);
        c.down(radii, d_radii, p);
        if (c.err != hipSuccess) return c.err;
        st.R = R;
        *n_rendered = R;
        *n_related = NG;
    } catch (const std::exception&) {
        return -3;
    }
    return hipDeviceSynchronize();
}
#endif

}  // extern "C"
