// What the evaluation kernels (kernels_metrics.hip, kernels_fidelity.hip, kernels_structure.hip) share, defined here and nowhere
// else: the shape limits, the Gaussian window and the one separable moment kernel, the 3x3 Sobel, the 34-pitch tile of level
// images, the K-wide reduction tree with its per-image finishing sum, and the host-side scale and stage helpers.  Every sum keeps a
// fixed order, so a value is bit-identical from call to call and the three families cannot drift apart.
#pragma once
#include "levels.h"
#include "swf_common.h"

#include <cmath>

namespace swf {

constexpr int kMaxPixels = 1 << 30;    // int pixel indices with room for the loop and tile strides; u32 counters hold 2^32 - 1
constexpr int kMaxBatch = 65535;       // grid.z / grid.y

// What the kernels' counters and grids hold: H * W <= 2^30 pixels per image, B <= 65535 images per call.
inline bool metric_shape_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && B <= kMaxBatch && (int64_t)H * W <= kMaxPixels; }

namespace {

constexpr int kThreads = 256;
constexpr int kTX = 32, kTY = 16;      // tile of the moment kernels (outputs): two outputs per thread
constexpr int kLT = 32, kLP = kLT + 2; // tile of the Sobel kernels and its padded pitch
static_assert(kTX * kTY == 2 * kThreads && kTX == 32 && kLT == 32, "the thread -> output maps below");

// ------------------------------------------------------------------------------------------------------------------------------
// Window, source and pixel load
// ------------------------------------------------------------------------------------------------------------------------------
template <int N>
struct Window {
    double g[N];
};

// g[i] = exp(-(i - c)^2 / (2 sd^2)), c = (N - 1) / 2, normalised to sum 1: the 1-D factor of the separable window.
template <int N>
inline Window<N> make_window(double sd) {
    Window<N> w;
    double sum = 0.0;
    for (int i = 0; i < N; ++i) {
        const double d = i - (N - 1) / 2;
        w.g[i] = std::exp(-(d * d) / (2.0 * sd * sd));
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

// ------------------------------------------------------------------------------------------------------------------------------
// Reduction trees
// ------------------------------------------------------------------------------------------------------------------------------
// SWF_TILE_TREE(K, red): sums of the workgroup's arrays red[0..K-1][kThreads] of doubles, each in a fixed order (one tree over LDS for
// all of them); the results are red[k][0] afterwards.  SWF_TILE_TREE_INT(K, red, WITH_INT, ired): the same, and if WITH_INT the
// integers of ired[kThreads] ride along.  A macro, and no function: a __shared__ array reaches a function as a generic pointer, and
// the compiler then emits other code for the steps than it does with the loop written in the kernel (seen in the ISA of every kernel
// that has this tree).
#define SWF_TILE_TREE_INT(K, red, WITH_INT, ired)                                                        \
    do {                                                                                                 \
        const int t_ = threadIdx.x;                                                                      \
        __syncthreads();                                                                                 \
        for (int s_ = kThreads / 2; s_ > 0; s_ >>= 1) {                                                  \
            if (t_ < s_) {                                                                               \
                _Pragma("unroll") for (int k_ = 0; k_ < (K); ++k_) (red)[k_][t_] += (red)[k_][t_ + s_]; \
                if (WITH_INT) (ired)[t_] += (ired)[t_ + s_];                                             \
            }                                                                                            \
            __syncthreads();                                                                             \
        }                                                                                                \
    } while (0)
#define SWF_TILE_TREE(K, red) SWF_TILE_TREE_INT(K, red, false, static_cast<unsigned long long*>(nullptr))

// r[k] <- the sum of p[t * K + k] over t < n, k < K, in a fixed order (per-thread strided sequences, then one tree for the K),
// returned to every thread.  WITH_INT: *isum <- the sum of the int64 values kept in the bits of slot 2, exact, so its order is immaterial.
template <int K, bool WITH_INT = false>
__device__ __forceinline__ void tile_sums(const double* p, int64_t n, double (*red)[kThreads], double r[K],
                                          unsigned long long* ired = nullptr, long long* isum = nullptr) {
    const int tid = threadIdx.x;
    double v[K] = {};
    unsigned long long iv = 0;
    for (int64_t t = tid; t < n; t += kThreads) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (!(WITH_INT && k == 2)) v[k] += p[t * K + k];   // slot 2 of a box tile is no double: r[2] stays 0
        if (WITH_INT) iv += (unsigned long long)__double_as_longlong(p[t * K + 2]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][tid] = v[k];
    if (WITH_INT) ired[tid] = iv;
    SWF_TILE_TREE_INT(K, red, WITH_INT, ired);
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = red[k][0];
    if (WITH_INT) *isum = (long long)ired[0];
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------------------------
// Gaussian moments and evaluation of one scale
// ------------------------------------------------------------------------------------------------------------------------------
// A workgroup owns a 16x32 tile of the "valid" output: the tile plus its N - 1 halo of A, B, F goes to LDS as fp64, then the eight
// planes A, B, F, AA, BB, FF, AF, BF are filtered one after the other, rows first (products formed on the fly), columns second into
// registers; RULE::pixel(muX, muF, XX, FF, XF, c0, c1, s0, s1) evaluates both pairs (A, F) and (B, F) per output pixel from the shared
// moments and adds to its two sums.  h, w: the scale's input; oh = h - N + 1, ow = w - N + 1 >= 1: its output.  part: [B][part_stride]
// doubles, this scale's tiles from part_off on, four per tile: s0 and s1 of (A, F), then of (B, F).
template <int N, bool QUANT, class RULE>
__global__ __launch_bounds__(kThreads) void gauss_moments_kernel(Source src, int h, int w, int oh, int ow, int tiles_x,
                                                                 double* __restrict__ part, int64_t part_stride, int64_t part_off,
                                                                 Window<N> win, double c0, double c1) {
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
    double s0A = 0.0, s1A = 0.0, s0B = 0.0, s1B = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (ty0 + ly0 + 8 * j < oh && tx0 + lx < ow) {
            RULE::pixel(m[0][j], m[2][j], m[3][j], m[5][j], m[6][j], c0, c1, s0A, s1A);
            RULE::pixel(m[1][j], m[2][j], m[4][j], m[5][j], m[7][j], c0, c1, s0B, s1B);
        }
    }
    red[0][tid] = s0A;
    red[1][tid] = s1A;
    red[2][tid] = s0B;
    red[3][tid] = s1B;
    SWF_TILE_TREE(4, red);
    if (tid < 4) part[(int64_t)b * part_stride + part_off + (int64_t)blockIdx.x * 4 + tid] = red[tid][0];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Sobel 3x3 and the tile of level images under it
// ------------------------------------------------------------------------------------------------------------------------------
// p = top-left of the 3x3 patch, pitch in elements.  sx = [-1 0 1; -2 0 2; -1 0 1], sy = [1 2 1; 0 0 0; -1 -2 -1] applied as written;
// conv2's flip negates both, which changes neither their magnitude nor sy / sx.
template <typename T>
__device__ __forceinline__ void sobel3x3(const T* p, int pitch, int& sx, int& sy) {
    const int a = p[0], b = p[1], c = p[2], d = p[pitch], e = p[pitch + 2], f = p[2 * pitch], g = p[2 * pitch + 1], h = p[2 * pitch + 2];
    sx = (c - a) + 2 * (e - d) + (h - f);
    sy = (a + 2 * b + c) - (f + 2 * g + h);
}

// sL[0..2] <- the levels of fusion, ir, vis under the 32x32 tile at (ty0, tx0) of image offset img, with a 1-pixel halo: zero outside
// the image, or (REPLICATE) the nearest pixel of the image.  Ends with the barrier that makes the tile readable.
template <bool REPLICATE>
__device__ __forceinline__ void load_level_tile(int (*sL)[kLP * kLP], const float* __restrict__ fusion, const float* __restrict__ ir,
                                                const float* __restrict__ vis, int64_t img, int ty0, int tx0, int H, int W) {
    for (int i = threadIdx.x; i < kLP * kLP; i += kThreads) {
        int hh = ty0 + i / kLP - 1, w = tx0 + i % kLP - 1;
        const bool in = REPLICATE || (hh >= 0 && hh < H && w >= 0 && w < W);
        if (REPLICATE) {
            hh = min(max(hh, 0), H - 1);
            w = min(max(w, 0), W - 1);
        }
        const int64_t o = img + (int64_t)hh * W + w;
        sL[0][i] = in ? level(fusion[o]) : 0;
        sL[1][i] = in ? level(ir[o]) : 0;
        sL[2][i] = in ? level(vis[o]) : 0;
    }
    __syncthreads();
}

// The pixel walk of a level tile: thread tid visits (ly, lx) = ((tid >> 5) + 8 k, tid & 31), k = 0..3, and calls
// body(o, hh, w) for those inside the image; o = top-left of the 3x3 patch centred on the pixel, (hh, w) = its place in the image.
template <class BODY>
__device__ __forceinline__ void walk_level_tile(int ty0, int tx0, int H, int W, BODY body) {
    const int lx = threadIdx.x & 31;
#pragma unroll 1
    for (int k = 0; k < kLT / 8; ++k) {
        const int ly = (threadIdx.x >> 5) + 8 * k;
        const int hh = ty0 + ly, w = tx0 + lx;
        if (hh < H && w < W) body(ly * kLP + lx, hh, w);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------------------------------------------
struct Scale {
    int h, w;               // input of the scale
    int oh, ow;             // "valid" output of its moments
    int tiles_x, ntiles;    // moment tiles
    int64_t plane_off;      // scales 2 on: offset of the scale's three planes within an image's planes, in doubles
    int64_t part_off;       // offset of the scale's partial sums within an image's, in doubles

    void size(int h_, int w_, int taps) {
        h = h_;
        w = w_;
        oh = h - taps + 1;
        ow = w - taps + 1;
        tiles_x = cdiv(ow, kTX);
        ntiles = tiles_x * cdiv(oh, kTY);
    }
};

// The three planes of scale i (>= 1) in the workspace; PLAN has planes, planes_per_image and the scales s[].
template <class PLAN>
inline Source plane_source(const PLAN& f, int i) {
    const Scale& s = f.s[i];
    const double* base = f.planes + s.plane_off;
    const int64_t n = (int64_t)s.h * s.w;
    return Source{{base, base + n, base + 2 * n}, f.planes_per_image};
}

// Tools only (SWF_DEBUG_SWITCHES=1), read at every call so that a family's tools/*_bench.py can time the parts in one process:
// the bit mask of what to enqueue, every stage by default.
inline int stage_mask(const char* env) {
    const char* e = debug_env(env);
    return e ? atoi(e) : 15;
}

}  // namespace
}  // namespace swf
