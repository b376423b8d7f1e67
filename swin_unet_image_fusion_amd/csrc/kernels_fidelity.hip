// VIF (with its two per-source parts) and Nabf / Labf of fused images against their infrared and visible sources: the five values of
// swf_fusion_fidelity (include/swinfuse.h has the definitions).  They are restated from the published definitions and the common
// open evaluators (vifp_mscale; Kumar's objective fusion performance scheme); no MATLAB, VIFB or sewar copy is available to this
// build, so PARITY WITH ANY OF THEM IS UNPINNED.  tests/fidelity_restatement.py is the same text in numpy fp64 and is
// what these kernels are checked against.
//
// Every value is a function of 8-bit levels (levels.h, the quantiser of kernels_metrics.hip).  Everything after the quantiser is
// fp64: the variances are differences of sums of products up to 65 025, and fp32 leaves 1e-8 to 3e-6 of error in VIF where any fp64
// order leaves 3e-13.  Every sum has a fixed order (unrolled taps, LDS trees, per-tile partials); no atomics of any kind; every
// workspace element that is read has been written by the same call, so nothing needs zeroing.
//
// Kernels, all on one stream (A, B, F = levels of ir, vis, fusion):
//   gauss_moments_kernel<N, QUANT, VifRule> (metric_frag.h)  one per pyramid scale, N = 17, 9, 5, 3 taps; scale 1 reads the fp32 images
//                          and quantises while loading, later scales read the fp64 planes of the workspace.  Both pairs (A, F) and
//                          (B, F) are evaluated per output pixel from the shared moments and the tile's four sums num_A, den_A, num_B,
//                          den_B are written.
//   vif_down_kernel<N>     N = 9, 5, 3: the input of scale s from the input of scale s - 1, "valid" filtering with scale s's window
//                          at even rows and columns only, 16x16 outputs per workgroup.  A kernel of its own because its window is the
//                          NEXT scale's: it shares the loaded tile with the moment kernel of scale s - 1 but not one product, and
//                          fusing the two would put a 2x wider tile behind the 16x32 one.
//   nabf_kernel            32x32 tiles with a replicated 1-pixel halo of the three level images in LDS: Sobel, Q_AF, Q_BF and the
//                          weights per pixel in fp64; three sums per tile (artifacts, loss, weights).
//   fidelity_finish_kernel one workgroup per image adds the per-tile sums in a fixed order and writes the row.
// The window weights are computed on the host in fp64 and passed by value.
#include "kernels_fidelity.h"
#include "metric_frag.h"

#include <algorithm>
#include <cmath>

namespace swf {
namespace {

constexpr int kScales = 4;
constexpr int kTD = 16;                // tile of the decimating kernels (outputs): one per thread
constexpr double kHalfPi = 1.57079632679489661923;
constexpr double kTwoOverPi = 0.63661977236758134308;
static_assert(kTD * kTD == kThreads && kTD == 16, "the thread -> pixel map of the decimating kernels");

// ------------------------------------------------------------------------------------------------------------------------------
// VIF: evaluation of one scale's moments
// ------------------------------------------------------------------------------------------------------------------------------
// gauss_moments_kernel's rule for one output pixel of vifp(R, D): the five rules of the header in their order, adding to the
// numerator and the denominator.  No contraction: the variances are the differences the restatement forms, product rounded first.
struct VifRule {
    static __device__ __forceinline__ void pixel(double muR, double muD, double RR, double DD, double RD, double sigma_nsq, double eps,
                                                 double& num, double& den) {
#pragma clang fp contract(off)
        double s1 = RR - muR * muR, s2 = DD - muD * muD;
        const double s12 = RD - muR * muD;
        s1 = s1 < 0.0 ? 0.0 : s1;
        s2 = s2 < 0.0 ? 0.0 : s2;
        double gg = s12 / (s1 + eps);
        double sv = s2 - gg * s12;
        if (s1 < eps) { gg = 0.0; sv = s2; s1 = 0.0; }
        if (s2 < eps) { gg = 0.0; sv = 0.0; }
        if (gg < 0.0) { sv = s2; gg = 0.0; }
        if (sv <= eps) sv = eps;
        num += log10(1.0 + gg * gg * s1 / (sv + sigma_nsq));
        den += log10(1.0 + s1 / sigma_nsq);
    }
};

// dst[B][dst_stride]: planes A, B, F of dh x dw, dh = ceil((h - N + 1) / 2), dw likewise: output (y, x) is the "valid" response at
// (2 y, 2 x), whose taps reach row 2 y + N - 1 <= h - 1.
template <int N, bool QUANT>
__global__ __launch_bounds__(kThreads) void vif_down_kernel(Source src, int h, int w, double* __restrict__ dst, int64_t dst_stride,
                                                            int dh, int dw, int tiles_x, Window<N> win) {
    constexpr int PD = 2 * (kTD - 1) + N;
    __shared__ double in[3][PD * PD];
    __shared__ double tmp[3][PD * kTD];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kTD, tx0 = (blockIdx.x % tiles_x) * kTD;
    const int64_t img = (int64_t)b * src.stride;
    for (int i = tid; i < PD * PD; i += kThreads) {
        const int y = 2 * ty0 + i / PD, x = 2 * tx0 + i % PD;
        const bool ok = y < h && x < w;
        const int64_t o = img + (int64_t)y * w + x;
#pragma unroll
        for (int k = 0; k < 3; ++k) in[k][i] = ok ? load_px<QUANT>(src.p[k], o) : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < 3 * PD * kTD; i += kThreads) {       // rows, at even columns
        const int p = i / (PD * kTD), rem = i - p * (PD * kTD);
        const int r = rem >> 4, c = rem & 15;
        const double* row = &in[p][r * PD + 2 * c];
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) acc += win.g[k] * row[k];
        tmp[p][rem] = acc;
    }
    __syncthreads();
    const int lx = tid & 15, ly = tid >> 4;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y < dh && x < dw) {
        double* out = dst + (int64_t)b * dst_stride + (int64_t)y * dw + x;
#pragma unroll
        for (int p = 0; p < 3; ++p) {                          // columns, at even rows
            const double* col = &tmp[p][2 * ly * kTD + lx];
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) acc += win.g[k] * col[k * kTD];
            out[(int64_t)p * dh * dw] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Nabf / Labf
// ------------------------------------------------------------------------------------------------------------------------------
struct Edge {
    int n;         // gv^2 + gh^2 of the unnormalised Sobel sums = 64 g^2: what every comparison is made on
    double g, a;
};

// p = top-left of the 3x3 patch.  gv with [-1 0 1; -2 0 2; -1 0 1] / 8 = sx / 8, gh with [-1 -2 -1; 0 0 0; 1 2 1] / 8 = -sy / 8.
__device__ __forceinline__ Edge edge_at(const int* p) {
    int gv, sy;
    sobel3x3(p, kLP, gv, sy);
    const int gh = -sy;
    Edge r;
    r.n = gv * gv + gh * gh;
    r.g = sqrt((double)r.n) / 8.0;
    r.a = gh == 0 ? (gv > 0 ? kHalfPi : (gv < 0 ? -kHalfPi : 0.0)) : atan((double)gv / (double)gh);
    return r;
}

__device__ __forceinline__ double q_xf(const swf_fidelity_desc& d, const Edge& X, const Edge& F) {
    const double G = (X.n == 0 || F.n == 0) ? 0.0 : (X.n > F.n ? F.g / X.g : X.g / F.g);
    const double A = fabs(fabs(X.a - F.a) - kHalfPi) * kTwoOverPi;
    const double Qg = d.Nrg / (1.0 + exp(-d.kg * (G - d.sg)));
    const double Qa = d.Nra / (1.0 + exp(-d.ka * (A - d.sa)));
    return sqrt(Qg * Qa);
}

// part: [B][part_stride] doubles, the Sobel tiles from part_off on, three per tile: sum na loss, sum (1 - na) loss, sum (w_A + w_B)
__global__ __launch_bounds__(kThreads) void nabf_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                        const float* __restrict__ vis, double* __restrict__ part, int64_t part_stride,
                                                        int64_t part_off, int H, int W, int tiles_x, swf_fidelity_desc d) {
    __shared__ int sL[3][kLP * kLP];
    __shared__ double red[3][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kLT, tx0 = (blockIdx.x % tiles_x) * kLT;
    load_level_tile<true>(sL, fusion, ir, vis, (int64_t)b * H * W, ty0, tx0, H, W);   // replicated border
    const double td2 = 64.0 * d.Td * d.Td;
    double art = 0.0, loss_sum = 0.0, wsum = 0.0;
    walk_level_tile(ty0, tx0, H, W, [&](int o, int, int) {
        const Edge F = edge_at(&sL[0][o]), A = edge_at(&sL[1][o]), Bv = edge_at(&sL[2][o]);
        const double wA = (double)A.n >= td2 ? A.g * sqrt(A.g) : d.wt_min;
        const double wB = (double)Bv.n >= td2 ? Bv.g * sqrt(Bv.g) : d.wt_min;
        const double loss = (1.0 - q_xf(d, A, F)) * wA + (1.0 - q_xf(d, Bv, F)) * wB;
        if (F.n > A.n && F.n > Bv.n)
            art += loss;
        else
            loss_sum += loss;
        wsum += wA + wB;
    });
    red[0][tid] = art;
    red[1][tid] = loss_sum;
    red[2][tid] = wsum;
    SWF_TILE_TREE(3, red);
    if (tid < 3) part[(int64_t)b * part_stride + part_off + (int64_t)blockIdx.x * 3 + tid] = red[tid][0];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Finish: one workgroup per image
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fidelity_finish_kernel(const double* __restrict__ part, int64_t part_stride, int64_t vif_tiles,
                                                                   int64_t nabf_tiles, double* __restrict__ out) {
    __shared__ double red[4][kThreads];
    const double* pv = part + (int64_t)blockIdx.x * part_stride;   // [vif_tiles][4], the scales one after the other
    double v[4], n[3];   // num_A, den_A, num_B, den_B; artifacts, loss, weights
    tile_sums<4>(pv, vif_tiles, red, v);
    tile_sums<3>(pv + vif_tiles * 4, nabf_tiles, red, n);   // [nabf_tiles][3]
    if (threadIdx.x == 0) {
        const double vA = v[1] == 0.0 ? 0.0 : v[0] / v[1], vB = v[3] == 0.0 ? 0.0 : v[2] / v[3];
        double* o = out + (int64_t)blockIdx.x * SWF_FIDELITY_COUNT;
        o[SWF_FIDELITY_VIF] = vA + vB;
        o[SWF_FIDELITY_VIF_IR] = vA;
        o[SWF_FIDELITY_VIF_VIS] = vB;
        o[SWF_FIDELITY_NABF] = n[0] / n[2];    // the weights sum to >= 2 wt_min per pixel
        o[SWF_FIDELITY_LABF] = n[1] / n[2];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int kTaps[kScales] = {17, 9, 5, 3};

struct FidelityPlan {
    int nscales;            // scales that contribute: a scale whose input is smaller than its window ends the pyramid
    Scale s[kScales];
    int64_t vif_tiles, planes_per_image;
    int nabf_tiles_x, nabf_tiles;
    int64_t part_stride;    // doubles of partial sums per image
    double* part;
    double* planes;
};

FidelityPlan carve_fidelity(Carver& ws, int B, int H, int W) {
    FidelityPlan f{};
    int h = H, w = W;
    for (int i = 0; i < kScales; ++i) {
        const int n = kTaps[i];
        if (h < n || w < n) break;
        Scale& s = f.s[i];
        if (i > 0) {
            h = (h - n + 2) / 2;   // ceil((h - n + 1) / 2)
            w = (w - n + 2) / 2;
            if (h < n || w < n) break;
            s.plane_off = f.planes_per_image;
            f.planes_per_image += (int64_t)3 * h * w;
        }
        s.size(h, w, n);
        s.part_off = f.vif_tiles * 4;
        f.vif_tiles += s.ntiles;
        f.nscales = i + 1;
    }
    f.nabf_tiles_x = cdiv(W, kLT);
    f.nabf_tiles = f.nabf_tiles_x * cdiv(H, kLT);
    f.part_stride = f.vif_tiles * 4 + (int64_t)f.nabf_tiles * 3;
    f.part = reinterpret_cast<double*>(ws.floats((int64_t)B * f.part_stride * 2));
    f.planes = reinterpret_cast<double*>(ws.floats((int64_t)B * f.planes_per_image * 2));
    return f;
}

// The window of N taps: sigma = N / 5.
template <int N>
Window<N> vif_window() {
    return make_window<N>(N / 5.0);
}

template <int N, bool QUANT>
int launch_moments(const FidelityPlan& f, int i, const Source& src, const swf_fidelity_desc& d, int B, hipStream_t stream) {
    const Scale& s = f.s[i];
    gauss_moments_kernel<N, QUANT, VifRule><<<dim3(s.ntiles, B), kThreads, 0, stream>>>(
        src, s.h, s.w, s.oh, s.ow, s.tiles_x, f.part, f.part_stride, s.part_off, vif_window<N>(), d.sigma_nsq, d.eps);
    return check_launch("gauss_moments_kernel");
}

// Scale i's planes from scale i - 1's input.
template <int N, bool QUANT>
int launch_down(const FidelityPlan& f, int i, const Source& src, int B, hipStream_t stream) {
    const Scale &from = f.s[i - 1], &to = f.s[i];
    const int tiles_x = cdiv(to.w, kTD);
    vif_down_kernel<N, QUANT><<<dim3(tiles_x * cdiv(to.h, kTD), B), kThreads, 0, stream>>>(src, from.h, from.w, f.planes + to.plane_off,
                                                                                         f.planes_per_image, to.h, to.w, tiles_x,
                                                                                         vif_window<N>());
    return check_launch("vif_down_kernel");
}

}  // namespace

size_t fusion_fidelity_workspace_bytes(int B, int H, int W) {
    Carver ws = Carver::measure();
    carve_fidelity(ws, B, H, W);
    return ws.bytes();
}

int fusion_fidelity(const swf_fidelity_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H, int W,
                    void* workspace, size_t workspace_bytes, hipStream_t stream) {
    Carver ws(workspace, workspace_bytes);
    const FidelityPlan f = carve_fidelity(ws, B, H, W);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "fusion_fidelity: workspace of %zu bytes, %zu needed", workspace_bytes, ws.bytes());
    const int stages = stage_mask("SWF_FIDELITY_STAGES");   // 1 VIF moments, 2 VIF decimation, 4 Nabf, 8 finish
    const Source images{{ir, vis, fusion}, (int64_t)H * W};
    if (f.nscales > 0 && (stages & 1)) SWF_TRY((launch_moments<17, true>(f, 0, images, d, B, stream)));
    if (f.nscales > 1) {
        if (stages & 2) SWF_TRY((launch_down<9, true>(f, 1, images, B, stream)));
        if (stages & 1) SWF_TRY((launch_moments<9, false>(f, 1, plane_source(f, 1), d, B, stream)));
    }
    if (f.nscales > 2) {
        if (stages & 2) SWF_TRY((launch_down<5, false>(f, 2, plane_source(f, 1), B, stream)));
        if (stages & 1) SWF_TRY((launch_moments<5, false>(f, 2, plane_source(f, 2), d, B, stream)));
    }
    if (f.nscales > 3) {
        if (stages & 2) SWF_TRY((launch_down<3, false>(f, 3, plane_source(f, 2), B, stream)));
        if (stages & 1) SWF_TRY((launch_moments<3, false>(f, 3, plane_source(f, 3), d, B, stream)));
    }
    if (stages & 4) {
        nabf_kernel<<<dim3(f.nabf_tiles, B), kThreads, 0, stream>>>(fusion, ir, vis, f.part, f.part_stride, f.vif_tiles * 4, H, W,
                                                                    f.nabf_tiles_x, d);
        SWF_TRY(check_launch("nabf_kernel"));
    }
    if (stages & 8) {
        fidelity_finish_kernel<<<B, kThreads, 0, stream>>>(f.part, f.part_stride, f.vif_tiles, f.nabf_tiles, out);
        SWF_TRY(check_launch("fidelity_finish_kernel"));
    }
    return SWF_OK;
}

}  // namespace swf
