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
//   vif_moments_kernel<N>  one per pyramid scale, N = 17, 9, 5, 3 taps.  A workgroup owns a 16x32 tile of the "valid" output: the tile
//                          plus its N - 1 halo of A, B, F goes to LDS as fp64 (scale 1 reads the fp32 images and quantises while
//                          loading, later scales read the fp64 planes of the workspace), then the eight planes A, B, F, AA, BB, FF,
//                          AF, BF are filtered one after the other, rows first (products formed on the fly), columns second into
//                          registers; both pairs (A, F) and (B, F) are evaluated per output pixel from the shared moments and the
//                          tile's four sums num_A, den_A, num_B, den_B are written.
//   vif_down_kernel<N>     N = 9, 5, 3: the input of scale s from the input of scale s - 1, "valid" filtering with scale s's window
//                          at even rows and columns only, 16x16 outputs per workgroup.  A kernel of its own because its window is the
//                          NEXT scale's: it shares the loaded tile with the moment kernel of scale s - 1 but not one product, and
//                          fusing the two would put a 2x wider tile behind the 16x32 one.
//   nabf_kernel            32x32 tiles with a replicated 1-pixel halo of the three level images in LDS: Sobel, Q_AF, Q_BF and the
//                          weights per pixel in fp64; three sums per tile (artifacts, loss, weights).
//   fidelity_finish_kernel one workgroup per image adds the per-tile sums in a fixed order and writes the row.
// The window weights are computed on the host in fp64 and passed by value.
#include "kernels_fidelity.h"
#include "levels.h"

#include <algorithm>
#include <cmath>

namespace swf {
namespace {

constexpr int kMaxPixels = 1 << 30;    // as the other metrics: int pixel indices with room for the tile strides
constexpr int kMaxBatch = 65535;       // grid.y
constexpr int kScales = 4;
constexpr int kThreads = 256;
constexpr int kTX = 32, kTY = 16;      // tile of the moment kernels (outputs): two output pixels per thread
constexpr int kTD = 16;                // tile of the decimating kernels (outputs): one per thread
constexpr int kST = 32, kSP = kST + 2; // Sobel tile and its padded pitch
constexpr double kHalfPi = 1.57079632679489661923;
constexpr double kTwoOverPi = 0.63661977236758134308;
static_assert(kTX * kTY == 2 * kThreads && kTD * kTD == kThreads && kTX == 32 && kTD == 16, "the thread -> pixel maps below");

template <int N>
struct Window {
    double g[N];
};

// g[i] = exp(-(i - c)^2 / (2 (N/5)^2)), c = (N - 1) / 2, normalised to sum 1: the 1-D factor of the separable window.
template <int N>
Window<N> make_window() {
    Window<N> w;
    const double sd = N / 5.0, c = (N - 1) / 2;
    double sum = 0.0;
    for (int i = 0; i < N; ++i) {
        w.g[i] = std::exp(-((i - c) * (i - c)) / (2.0 * sd * sd));
        sum += w.g[i];
    }
    for (int i = 0; i < N; ++i) w.g[i] /= sum;
    return w;
}

// The three input planes of a scale, in the order A, B, F: image 0's planes and the distance between images, in elements.
struct Source {
    const void* p[3];
    int64_t stride;
};

// QUANT: an fp32 image, quantised here; else an fp64 plane of the workspace.
template <bool QUANT>
__device__ __forceinline__ double load_px(const void* p, int64_t o) {
    if (QUANT) return (double)level(static_cast<const float*>(p)[o]);
    return static_cast<const double*>(p)[o];
}

// Sum over the workgroup's kThreads values in a fixed order (tree over LDS); the result is red[0] after the call.
__device__ __forceinline__ void tree_sum(double* red) {
    const int tid = threadIdx.x;
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// VIF: moments and evaluation of one scale
// ------------------------------------------------------------------------------------------------------------------------------
// One output pixel of vifp(R, D): the five rules of the header in their order.  No contraction: the variances are the differences the
// restatement forms, product rounded first.
__device__ __forceinline__ void vif_pixel(double muR, double muD, double RR, double DD, double RD, double sigma_nsq, double eps,
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

// h, w: the scale's input; oh = h - N + 1, ow = w - N + 1 >= 1: its "valid" output.  part: [B][part_stride] doubles, this scale's tiles
// from part_off on, four per tile.
template <int N, bool QUANT>
__global__ __launch_bounds__(kThreads) void vif_moments_kernel(Source src, int h, int w, int oh, int ow, int tiles_x,
                                                               double* __restrict__ part, int64_t part_stride, int64_t part_off,
                                                               Window<N> win, double sigma_nsq, double eps) {
    constexpr int PW = kTX + N - 1, PH = kTY + N - 1;
    __shared__ double in[3][PH * PW];
    __shared__ double tmp[PH * kTX];
    __shared__ double red[4][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kTY, tx0 = (blockIdx.x % tiles_x) * kTX;
    const int64_t img = (int64_t)b * src.stride;
    for (int i = tid; i < PH * PW; i += kThreads) {
        const int y = ty0 + i / PW, x = tx0 + i % PW;
        const bool ok = y < h && x < w;
        const int64_t o = img + (int64_t)y * w + x;
#pragma unroll
        for (int k = 0; k < 3; ++k) in[k][i] = ok ? load_px<QUANT>(src.p[k], o) : 0.0;
    }
    __syncthreads();
    const int lx = tid & 31, ly0 = tid >> 5;
    double m[8][2];   // A, B, F, AA, BB, FF, AF, BF at output pixels (ly0, lx) and (ly0 + 8, lx)
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int pa = p < 3 ? p : (p < 6 ? p - 3 : p - 6);   // first factor
        const int pb = p < 6 ? p - 3 : 2;                     // second factor of a product plane
        for (int i = tid; i < PH * kTX; i += kThreads) {      // rows
            const int r = i >> 5, c = i & 31;
            const double* ra = &in[pa][r * PW + c];
            const double* rb = &in[p < 3 ? 0 : pb][r * PW + c];
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) acc += win.g[k] * (p < 3 ? ra[k] : ra[k] * rb[k]);
            tmp[i] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {                          // columns
            const double* col = &tmp[(ly0 + 8 * j) * kTX + lx];
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) acc += win.g[k] * col[k * kTX];
            m[p][j] = acc;
        }
        __syncthreads();
    }
    double numA = 0.0, denA = 0.0, numB = 0.0, denB = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (ty0 + ly0 + 8 * j < oh && tx0 + lx < ow) {
            vif_pixel(m[0][j], m[2][j], m[3][j], m[5][j], m[6][j], sigma_nsq, eps, numA, denA);
            vif_pixel(m[1][j], m[2][j], m[4][j], m[5][j], m[7][j], sigma_nsq, eps, numB, denB);
        }
    }
    red[0][tid] = numA;
    red[1][tid] = denA;
    red[2][tid] = numB;
    red[3][tid] = denB;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + s];
        }
        __syncthreads();
    }
    if (tid < 4) part[(int64_t)b * part_stride + part_off + (int64_t)blockIdx.x * 4 + tid] = red[tid][0];
}

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

// p = top-left of the 3x3 patch.  gv with [-1 0 1; -2 0 2; -1 0 1] / 8, gh with [-1 -2 -1; 0 0 0; 1 2 1] / 8.
__device__ __forceinline__ Edge edge_at(const int* p) {
    const int a = p[0], b = p[1], c = p[2], d = p[kSP], e = p[kSP + 2], f = p[2 * kSP], g = p[2 * kSP + 1], h = p[2 * kSP + 2];
    const int gv = (c - a) + 2 * (e - d) + (h - f);
    const int gh = (f + 2 * g + h) - (a + 2 * b + c);
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
    __shared__ int sL[3][kSP * kSP];
    __shared__ double red[3][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kST, tx0 = (blockIdx.x % tiles_x) * kST;
    const int64_t img = (int64_t)b * H * W;
    for (int i = tid; i < kSP * kSP; i += kThreads) {
        const int hh = min(max(ty0 + i / kSP - 1, 0), H - 1), w = min(max(tx0 + i % kSP - 1, 0), W - 1);   // replicated border
        const int64_t o = img + (int64_t)hh * W + w;
        sL[0][i] = level(fusion[o]);
        sL[1][i] = level(ir[o]);
        sL[2][i] = level(vis[o]);
    }
    __syncthreads();
    const double td2 = 64.0 * d.Td * d.Td;
    double art = 0.0, loss_sum = 0.0, wsum = 0.0;
    const int lx = tid & 31;
#pragma unroll 1
    for (int k = 0; k < kST / 8; ++k) {
        const int ly = (tid >> 5) + 8 * k;
        if (ty0 + ly < H && tx0 + lx < W) {
            const int o = ly * kSP + lx;   // top-left of the patch centred on (ly + 1, lx + 1)
            const Edge F = edge_at(&sL[0][o]), A = edge_at(&sL[1][o]), Bv = edge_at(&sL[2][o]);
            const double wA = (double)A.n >= td2 ? A.g * sqrt(A.g) : d.wt_min;
            const double wB = (double)Bv.n >= td2 ? Bv.g * sqrt(Bv.g) : d.wt_min;
            const double loss = (1.0 - q_xf(d, A, F)) * wA + (1.0 - q_xf(d, Bv, F)) * wB;
            if (F.n > A.n && F.n > Bv.n)
                art += loss;
            else
                loss_sum += loss;
            wsum += wA + wB;
        }
    }
    red[0][tid] = art;
    red[1][tid] = loss_sum;
    red[2][tid] = wsum;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + s];
        }
        __syncthreads();
    }
    if (tid < 3) part[(int64_t)b * part_stride + part_off + (int64_t)blockIdx.x * 3 + tid] = red[tid][0];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Finish: one workgroup per image
// ------------------------------------------------------------------------------------------------------------------------------
// Sum of p[t * step] over t < n in a fixed order (per-thread strided sequences, then the tree), returned to every thread.
__device__ __forceinline__ double strided_sum(const double* p, int64_t n, int step, double* red) {
    double v = 0.0;
    for (int64_t t = threadIdx.x; t < n; t += kThreads) v += p[t * step];
    red[threadIdx.x] = v;
    __syncthreads();
    tree_sum(red);
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kThreads) void fidelity_finish_kernel(const double* __restrict__ part, int64_t part_stride, int64_t vif_tiles,
                                                                   int64_t nabf_tiles, double* __restrict__ out) {
    __shared__ double red[kThreads];
    const double* pv = part + (int64_t)blockIdx.x * part_stride;   // [vif_tiles][4], the scales one after the other
    const double* pn = pv + vif_tiles * 4;                         // [nabf_tiles][3]
    const double numA = strided_sum(pv, vif_tiles, 4, red), denA = strided_sum(pv + 1, vif_tiles, 4, red);
    const double numB = strided_sum(pv + 2, vif_tiles, 4, red), denB = strided_sum(pv + 3, vif_tiles, 4, red);
    const double art = strided_sum(pn, nabf_tiles, 3, red), loss = strided_sum(pn + 1, nabf_tiles, 3, red);
    const double wsum = strided_sum(pn + 2, nabf_tiles, 3, red);
    if (threadIdx.x == 0) {
        const double vA = denA == 0.0 ? 0.0 : numA / denA, vB = denB == 0.0 ? 0.0 : numB / denB;
        double* o = out + (int64_t)blockIdx.x * SWF_FIDELITY_COUNT;
        o[SWF_FIDELITY_VIF] = vA + vB;
        o[SWF_FIDELITY_VIF_IR] = vA;
        o[SWF_FIDELITY_VIF_VIS] = vB;
        o[SWF_FIDELITY_NABF] = art / wsum;    // wsum >= 2 wt_min per pixel
        o[SWF_FIDELITY_LABF] = loss / wsum;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int kTaps[kScales] = {17, 9, 5, 3};

struct Scale {
    int h, w;               // input of the scale
    int oh, ow;             // "valid" output of its moments
    int tiles_x, ntiles;    // moment tiles
    int64_t plane_off;      // scales 2-4: offset of the scale's three planes within an image's planes, in doubles
    int64_t part_off;       // offset of the scale's partial sums within an image's, in doubles
};

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
        s.h = h;
        s.w = w;
        s.oh = h - n + 1;
        s.ow = w - n + 1;
        s.tiles_x = cdiv(s.ow, kTX);
        s.ntiles = s.tiles_x * cdiv(s.oh, kTY);
        s.part_off = f.vif_tiles * 4;
        f.vif_tiles += s.ntiles;
        f.nscales = i + 1;
    }
    f.nabf_tiles_x = cdiv(W, kST);
    f.nabf_tiles = f.nabf_tiles_x * cdiv(H, kST);
    f.part_stride = f.vif_tiles * 4 + (int64_t)f.nabf_tiles * 3;
    f.part = reinterpret_cast<double*>(ws.floats((int64_t)B * f.part_stride * 2));
    f.planes = reinterpret_cast<double*>(ws.floats((int64_t)B * f.planes_per_image * 2));
    return f;
}

// The three planes of scale i (>= 1) in the workspace.
Source plane_source(const FidelityPlan& f, int i) {
    const Scale& s = f.s[i];
    const double* base = f.planes + s.plane_off;
    const int64_t n = (int64_t)s.h * s.w;
    return Source{{base, base + n, base + 2 * n}, f.planes_per_image};
}

template <int N, bool QUANT>
int launch_moments(const FidelityPlan& f, int i, const Source& src, const swf_fidelity_desc& d, int B, hipStream_t stream) {
    const Scale& s = f.s[i];
    vif_moments_kernel<N, QUANT><<<dim3(s.ntiles, B), kThreads, 0, stream>>>(src, s.h, s.w, s.oh, s.ow, s.tiles_x, f.part, f.part_stride,
                                                                             s.part_off, make_window<N>(), d.sigma_nsq, d.eps);
    return check_launch("vif_moments_kernel");
}

// Scale i's planes from scale i - 1's input.
template <int N, bool QUANT>
int launch_down(const FidelityPlan& f, int i, const Source& src, int B, hipStream_t stream) {
    const Scale &from = f.s[i - 1], &to = f.s[i];
    const int tiles_x = cdiv(to.w, kTD);
    vif_down_kernel<N, QUANT><<<dim3(tiles_x * cdiv(to.h, kTD), B), kThreads, 0, stream>>>(src, from.h, from.w, f.planes + to.plane_off,
                                                                                         f.planes_per_image, to.h, to.w, tiles_x,
                                                                                         make_window<N>());
    return check_launch("vif_down_kernel");
}

// Tools only (SWF_DEBUG_SWITCHES=1), read at every call so that tools/fidelity_bench.py can time the parts in one process:
// SWF_FIDELITY_STAGES = bit mask of what to enqueue (1 VIF moments, 2 VIF decimation, 4 Nabf, 8 finish).
int stage_mask() {
    const char* e = debug_env("SWF_FIDELITY_STAGES");
    return e ? atoi(e) : 15;
}

}  // namespace

bool fusion_fidelity_shape_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && B <= kMaxBatch && (int64_t)H * W <= kMaxPixels;
}

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
    const int stages = stage_mask();
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
