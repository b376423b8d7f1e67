// FMI_pixel, FMI_dct, FMI_w and FMI_edge of fused images against their infrared and visible sources: the four values of
// swf_fusion_feature (include/swinfuse.h has the definitions).  They are restated from memory of Haghighat & Razian's feature mutual
// information and of the common open evaluators; no paper and no evaluator is available to this build, so PARITY WITH ANY OF THEM IS
// UNPINNED.  tests/feature_restatement.py is the same text in numpy and is what these kernels are checked against.
//
// Every value is a function of 8-bit levels (levels.h), fp64 after the quantiser.  Every floating-point sum has a fixed order (a
// thread's own sequences, LDS trees, per-tile partials); no atomics.  Every workspace element that is read has been written by the
// same call.
//
// Kernels, all on one stream (A, B, F = levels of ir, vis, fusion; three planes per image):
//   fmi_tables_kernel      D_H and the transpose of D_W, the dense orthonormal DCT-II matrices; shared by the whole batch
//   fmi_levels_kernel      the three level planes as doubles, the operand of the first product
//   fmi_haar_kernel        the three Haar mosaics [LL LH; HL HH], one thread per 2 x 2 block
//   dft_gemm_kernel        X D_W^T, then D_H (X D_W^T), over the 3 B planes (dft_frag.h; plain load, plain store)
//   fmi_window_kernel      <window, source>: a workgroup owns 16 x 16 windows, one per thread; the tile plus its window - 1 halo of
//                          F, A, B goes to LDS as fp64 (pixel and edge from the 34-pitch level tile of metric_frag.h, the Haar and
//                          DCT planes from the workspace, the DCT coefficients snapped as they are loaded); one sum per tile
//   fmi_finish_kernel      one workgroup per image adds the per-tile sums of each feature in a fixed order; writes the four means.
//
// A thread keeps the cdf Q of F's window (window^2 doubles) in registers and nothing else of that size: p, q and P are formed again
// from the LDS tile where they are needed (the same expression, so the same bits), and the joint cdf is walked row by row from P_i,
// P_(i-1) and Q, two evaluations per cell, once for rho and once for the joint entropy.
#include "kernels_feature.h"
#include "metric_frag.h"
#include "dft_frag.h"

#include <algorithm>

namespace swf {
namespace {

constexpr int kImgPlanes = 3;          // A, B, F
constexpr int kWT = 16;                // a tile is kWT x kWT windows
static_assert(kWT * kWT == kThreads, "one thread per window");
constexpr int kMaxAxisFmi = 16384;     // H^2 <= 2^28 elements in a DCT matrix
constexpr int kMaxImagesFmi = 65535 / kImgPlanes;
enum { kSrcPixel, kSrcEdge, kSrcPlane, kSrcPlaneSnap };

// ------------------------------------------------------------------------------------------------------------------------------
// Planes
// ------------------------------------------------------------------------------------------------------------------------------
// D_n[k][i] = s_k sqrt(2 / n) cos(pi ((2 i + 1) k mod 4 n) / (2 n)), the argument reduced in integers before cospi.
__device__ __forceinline__ double dct_entry(int k, int i, int n) {
    const int64_t m = ((int64_t)(2 * i + 1) * k) % ((int64_t)4 * n);
    const double s = k == 0 ? 1.0 / sqrt(2.0) : 1.0;
    return s * sqrt(2.0 / (double)n) * cospi((double)m / (double)(2 * n));
}

// dh[H][H] <- D_H (row k, column i); dwt[W][W] <- D_W transposed (row i, column k).
__global__ __launch_bounds__(kThreads) void fmi_tables_kernel(double* __restrict__ dh, double* __restrict__ dwt, int H, int W) {
    int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nH = (int64_t)H * H, nW = (int64_t)W * W;
    if (i < nH) {
        dh[i] = dct_entry((int)(i / H), (int)(i % H), H);
        return;
    }
    i -= nH;
    if (i < nW) dwt[i] = dct_entry((int)(i % W), (int)(i / W), W);
}

// X[B][3][n] <- the levels of ir, vis, fusion.  grid (ceil(n / 256), B).
__global__ __launch_bounds__(kThreads) void fmi_levels_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                              const float* __restrict__ vis, int64_t n, double* __restrict__ X) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int b = blockIdx.y;
    const int64_t o = (int64_t)b * n + i;
    double* x = X + (int64_t)b * kImgPlanes * n + i;
    x[0] = (double)level(ir[o]);
    x[n] = (double)level(vis[o]);
    x[2 * n] = (double)level(fusion[o]);
}

// V[B][3][2 hh][2 wh] <- the mosaic [LL LH; HL HH] of ir, vis, fusion; hh = H / 2, wh = W / 2 (an odd trailing row or column is
// dropped).  All values are multiples of 1/2: exact.  grid (ceil(hh wh / 256), B).
__global__ __launch_bounds__(kThreads) void fmi_haar_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                            const float* __restrict__ vis, int H, int W, int hh, int wh,
                                                            double* __restrict__ V) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)hh * wh) return;
    const int b = blockIdx.y, r = (int)(i / wh), c = (int)(i % wh);
    const int64_t o = (int64_t)b * H * W + (int64_t)(2 * r) * W + 2 * c, nv = (int64_t)4 * hh * wh;
    const int pitch = 2 * wh;
#pragma unroll
    for (int k = 0; k < kImgPlanes; ++k) {
        const float* src = k == 0 ? ir : (k == 1 ? vis : fusion);
        const double p = (double)level(src[o]), q = (double)level(src[o + 1]), s = (double)level(src[o + W]), t = (double)level(src[o + W + 1]);
        double* v = V + ((int64_t)b * kImgPlanes + k) * nv;
        v[(int64_t)r * pitch + c] = (p + q + s + t) / 2.0;
        v[(int64_t)r * pitch + wh + c] = (p + q - s - t) / 2.0;
        v[(int64_t)(hh + r) * pitch + c] = (p - q + s - t) / 2.0;
        v[(int64_t)(hh + r) * pitch + wh + c] = (p - q - s + t) / 2.0;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Windows
// ------------------------------------------------------------------------------------------------------------------------------
// A window sample scaled to [0, 1] by the window's range; 1 in a flat window.
__device__ __forceinline__ double fmi_unit(double v, double mn, double rng, bool flat) { return flat ? 1.0 : (v - mn) / rng; }

// The Frechet bound of the joint cdf: the upper one for c >= 0, the lower one for c < 0.
__device__ __forceinline__ double fmi_bound(double P, double Q, bool upper) { return upper ? fmin(P, Q) : fmax(P + Q - 1.0, 0.0); }

// SWF_FMI_WALK(k, off): for k = 0 .. L - 1 in MATLAB's (:) order, off = the sample's offset in a tile of pitch PT (k = column * WIN + row).
#define SWF_FMI_WALK(k, off) for (int k = 0, off = 0, r_ = 0; k < L; ++k, off += (++r_ == WIN ? (r_ = 0, 1 - (WIN - 1) * PT) : PT))

// part[b * part_stride + part_off + tile] <- the sum over the tile's windows of (I(A, F) + I(B, F)) / 2.  h, w: the plane.  SRC pixel and
// edge read the images (H = h, W = w), the others planes[B][3][h w] in the order A, B, F.  grid (tiles, B).
template <int WIN, int SRC>
__global__ __launch_bounds__(kThreads) void fmi_window_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                              const float* __restrict__ vis, const double* __restrict__ planes, int h, int w,
                                                              int tiles_x, double step, double* __restrict__ part, int64_t part_stride,
                                                              int64_t part_off) {
    constexpr int PT = kWT + WIN - 1, L = WIN * WIN;
    static_assert(PT + 2 <= kLP, "the plane tile and the halo of its Sobel patches lie inside the level tile");
    __shared__ double sT[3][PT * PT];       // F, A, B
    __shared__ double red[1][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kWT, tx0 = (blockIdx.x % tiles_x) * kWT;
    if constexpr (SRC == kSrcPixel || SRC == kSrcEdge) {
        __shared__ int sL[3][kLP * kLP];    // F, A, B with a 1-pixel replicated halo: level (y, x) of the tile at [(y + 1) kLP + x + 1]
        load_level_tile<true>(sL, fusion, ir, vis, (int64_t)b * h * w, ty0, tx0, h, w);
        for (int i = tid; i < PT * PT; i += kThreads) {
            const int y = i / PT, x = i % PT;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (SRC == kSrcPixel) {
                    sT[k][i] = (double)sL[k][(y + 1) * kLP + x + 1];
                } else {
                    int sx, sy;
                    sobel3x3(&sL[k][y * kLP + x], kLP, sx, sy);
                    sT[k][i] = (double)(abs(sx) + abs(sy));
                }
            }
        }
    } else {
        const int64_t n = (int64_t)h * w;
        const double* img = planes + (int64_t)b * kImgPlanes * n;
        for (int i = tid; i < PT * PT; i += kThreads) {
            const int y = ty0 + i / PT, x = tx0 + i % PT;
            const bool ok = y < h && x < w;
            const int64_t o = (int64_t)y * w + x;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double v = ok ? img[(int64_t)((k + 2) % 3) * n + o] : 0.0;
                if (SRC == kSrcPlaneSnap) v = rint(v / step) * step;
                sT[k][i] = v;
            }
        }
    }
    __syncthreads();

    const int lx = tid & (kWT - 1), ly = tid / kWT;
    double value = 0.0;
    if (ty0 + ly < h - WIN + 1 && tx0 + lx < w - WIN + 1) {
        constexpr double inv = 1.0 / (double)L;
        const double* f = &sT[0][ly * PT + lx];
        double fmn = f[0], fmx = f[0];
        SWF_FMI_WALK(k, off) {
            fmn = fmin(fmn, f[off]);
            fmx = fmax(fmx, f[off]);
        }
        const bool fflat = fmx == fmn;
        const double frng = fmx - fmn;
        double Sf = 0.0;
        SWF_FMI_WALK(k, off) Sf += fmi_unit(f[off], fmn, frng, fflat);
        double Q[L], Hq = 0.0, muq = 0.0, m2q = 0.0, sqq = 0.0;
        {
            double run = 0.0;
#pragma unroll
            for (int k = 0; k < L; ++k) {       // unrolled: Q stays in registers
                const double q = fmi_unit(f[(k % WIN) * PT + k / WIN], fmn, frng, fflat) / Sf;
                run += q;
                Q[k] = run;
                if (q > 0.0) Hq -= q * log2(q);
                muq += (double)(k + 1) * q;
                m2q += (double)((k + 1) * (k + 1)) * q;
                sqq += (q - inv) * (q - inv);
            }
        }
        const double sgq = sqrt(fmax(m2q - muq * muq, 0.0));
#pragma unroll 1
        for (int s = 1; s <= 2; ++s) {
            const double* x = &sT[s][ly * PT + lx];
            double mn = x[0], mx = x[0];
            bool same = true;
            SWF_FMI_WALK(k, off) {
                mn = fmin(mn, x[off]);
                mx = fmax(mx, x[off]);
                same = same && x[off] == f[off];
            }
            if (same) {
                value += 1.0;
                continue;
            }
            const bool flat = mx == mn;
            const double rng = mx - mn;
            double S = 0.0;
            SWF_FMI_WALK(k, off) S += fmi_unit(x[off], mn, rng, flat);
            double Hp = 0.0, mup = 0.0, m2p = 0.0, spp = 0.0, spq = 0.0;
#pragma unroll 1
            SWF_FMI_WALK(k, off) {
                const double p = fmi_unit(x[off], mn, rng, flat) / S, q = fmi_unit(f[off], fmn, frng, fflat) / Sf;
                if (p > 0.0) Hp -= p * log2(p);
                mup += (double)(k + 1) * p;
                m2p += (double)((k + 1) * (k + 1)) * p;
                spp += (p - inv) * (p - inv);
                spq += (p - inv) * (q - inv);
            }
            const double den = sqrt(spp * sqq), c = den == 0.0 ? 0.0 : spq / den;
            const double ss = sqrt(fmax(m2p - mup * mup, 0.0)) * sgq;
            const bool upper = c >= 0.0;
            double excess = 0.0, P = 0.0;       // sum of G - P Q over the cells
#pragma unroll 1
            SWF_FMI_WALK(i, off) {
                P += fmi_unit(x[off], mn, rng, flat) / S;
#pragma unroll
                for (int j = 0; j < L; ++j) excess += fmi_bound(P, Q[j], upper) - P * Q[j];
            }
            const double rho = ss == 0.0 ? 0.0 : excess / ss;
            const double phi = rho == 0.0 ? 0.0 : fmin(fmax(c / rho, 0.0), 1.0), cophi = 1.0 - phi;
            double Hj = 0.0;
            P = 0.0;
#pragma unroll 1
            SWF_FMI_WALK(i, off) {
                const double Pm = P;
                P += fmi_unit(x[off], mn, rng, flat) / S;
                double left = 0.0, upleft = 0.0;   // J(i, j - 1) and J(i - 1, j - 1)
#pragma unroll
                for (int j = 0; j < L; ++j) {
                    const double here = phi * fmi_bound(P, Q[j], upper) + cophi * (P * Q[j]);
                    const double up = i == 0 ? 0.0 : phi * fmi_bound(Pm, Q[j], upper) + cophi * (Pm * Q[j]);
                    const double t = (here - up) - (left - upleft);
                    if (t > 0.0) Hj -= t * log2(t);
                    left = here;
                    upleft = up;
                }
            }
            const double Hs = Hp + Hq;
            value += Hs == 0.0 ? 0.0 : 2.0 * (Hs - Hj) / Hs;
        }
        value /= 2.0;
    }
    red[0][tid] = value;
    SWF_TILE_TREE(1, red);
    if (tid == 0) part[(int64_t)b * part_stride + part_off + blockIdx.x] = red[0][0];
}

struct FmiFinish {
    int64_t off[SWF_FEATURE_COUNT];     // a feature's tiles within an image's partial sums
    int tiles[SWF_FEATURE_COUNT];
    double windows[SWF_FEATURE_COUNT];  // 0: no window, the value is 0
};

// One workgroup per image: each feature's per-tile sums in a fixed order, over its window count.
__global__ __launch_bounds__(kThreads) void fmi_finish_kernel(const double* __restrict__ part, int64_t part_stride, FmiFinish fin,
                                                              double* __restrict__ out) {
    __shared__ double red[1][kThreads];
    const int b = blockIdx.x;
#pragma unroll 1
    for (int k = 0; k < SWF_FEATURE_COUNT; ++k) {
        double s[1];
        tile_sums<1>(part + (int64_t)b * part_stride + fin.off[k], fin.tiles[k], red, s);
        if (threadIdx.x == 0) out[(int64_t)b * SWF_FEATURE_COUNT + k] = fin.windows[k] > 0.0 ? s[0] / fin.windows[k] : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------------------------------------------
// Tiles of kWT x kWT windows of an h x w plane.
struct WindowGrid {
    int tiles_x, tiles;
    double windows;
};
WindowGrid window_grid(int h, int w, int win) {
    const int oh = std::max(h - win + 1, 0), ow = std::max(w - win + 1, 0);
    return WindowGrid{cdiv(ow, kWT), cdiv(ow, kWT) * cdiv(oh, kWT), (double)oh * (double)ow};
}

struct FeaturePlan {
    int hh, wh;                    // Haar blocks per axis; the mosaic is 2 hh x 2 wh
    int64_t n, nv;                 // doubles per image plane and per mosaic
    int64_t part_stride;           // partial sums per image: 3 t0 + tw at window 3, the most tiles any window has
    double *dh, *dwt, *X, *Y, *V, *part;
};

FeaturePlan carve_feature(Carver& ws, int B, int H, int W) {
    FeaturePlan f{};
    f.hh = H / 2;
    f.wh = W / 2;
    f.n = (int64_t)H * W;
    f.nv = (int64_t)4 * f.hh * f.wh;
    f.part_stride = (int64_t)3 * window_grid(H, W, 3).tiles + window_grid(2 * f.hh, 2 * f.wh, 3).tiles;
    f.dh = carve_doubles(ws, (int64_t)H * H);
    f.dwt = carve_doubles(ws, (int64_t)W * W);
    f.X = carve_doubles(ws, (int64_t)B * kImgPlanes * f.n);
    f.Y = carve_doubles(ws, (int64_t)B * kImgPlanes * f.n);
    f.V = carve_doubles(ws, (int64_t)B * kImgPlanes * f.nv);
    f.part = carve_doubles(ws, (int64_t)B * f.part_stride);
    return f;
}

template <int WIN>
int launch_windows(const FeaturePlan& f, const swf_feature_desc& d, const float* fusion, const float* ir, const float* vis, int B, int H,
                   int W, FmiFinish& fin, hipStream_t stream) {
    const WindowGrid g0 = window_grid(H, W, WIN), gw = window_grid(2 * f.hh, 2 * f.wh, WIN);
    const int order[SWF_FEATURE_COUNT] = {SWF_FEATURE_FMI_PIXEL, SWF_FEATURE_FMI_DCT, SWF_FEATURE_FMI_W, SWF_FEATURE_FMI_EDGE};
    int64_t off = 0;
    for (int k : order) {
        const WindowGrid& g = k == SWF_FEATURE_FMI_W ? gw : g0;
        fin.off[k] = off;
        fin.tiles[k] = g.tiles;
        fin.windows[k] = g.windows;
        off += g.tiles;
    }
    // Tools only (SWF_DEBUG_SWITCHES=1), as the stage mask is: the features whose window kernel is enqueued, bit k = feature k.
    const char* e = debug_env("SWF_FEATURE_WINDOWS");
    const int which = e ? atoi(e) : 15;
    const dim3 grid(g0.tiles, B);
    if (g0.tiles > 0 && (which & (1 << SWF_FEATURE_FMI_PIXEL))) {
        fmi_window_kernel<WIN, kSrcPixel><<<grid, kThreads, 0, stream>>>(fusion, ir, vis, nullptr, H, W, g0.tiles_x, 0.0, f.part, f.part_stride,
                                                                          fin.off[SWF_FEATURE_FMI_PIXEL]);
        SWF_TRY(check_launch("fmi_window_kernel (pixel)"));
    }
    if (g0.tiles > 0 && (which & (1 << SWF_FEATURE_FMI_DCT))) {
        fmi_window_kernel<WIN, kSrcPlaneSnap><<<grid, kThreads, 0, stream>>>(nullptr, nullptr, nullptr, f.X, H, W, g0.tiles_x, d.dct_step, f.part,
                                                                              f.part_stride, fin.off[SWF_FEATURE_FMI_DCT]);
        SWF_TRY(check_launch("fmi_window_kernel (dct)"));
    }
    if (g0.tiles > 0 && (which & (1 << SWF_FEATURE_FMI_EDGE))) {
        fmi_window_kernel<WIN, kSrcEdge><<<grid, kThreads, 0, stream>>>(fusion, ir, vis, nullptr, H, W, g0.tiles_x, 0.0, f.part, f.part_stride,
                                                                         fin.off[SWF_FEATURE_FMI_EDGE]);
        SWF_TRY(check_launch("fmi_window_kernel (edge)"));
    }
    if (gw.tiles > 0 && (which & (1 << SWF_FEATURE_FMI_W))) {
        fmi_window_kernel<WIN, kSrcPlane><<<dim3(gw.tiles, B), kThreads, 0, stream>>>(nullptr, nullptr, nullptr, f.V, 2 * f.hh, 2 * f.wh,
                                                                                       gw.tiles_x, 0.0, f.part, f.part_stride,
                                                                                       fin.off[SWF_FEATURE_FMI_W]);
        SWF_TRY(check_launch("fmi_window_kernel (w)"));
    }
    return SWF_OK;
}

}  // namespace

bool feature_shape_ok(int B, int H, int W) {
    return metric_shape_ok(B, H, W) && H <= kMaxAxisFmi && W <= kMaxAxisFmi && B <= kMaxImagesFmi;
}

size_t fusion_feature_workspace_bytes(int B, int H, int W) {
    Carver ws = Carver::measure();
    carve_feature(ws, B, H, W);
    return ws.bytes();
}

int fusion_feature(const swf_feature_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H, int W,
                   void* workspace, size_t workspace_bytes, hipStream_t stream) {
    Carver ws(workspace, workspace_bytes);
    const FeaturePlan f = carve_feature(ws, B, H, W);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "fusion_feature: workspace of %zu bytes, %zu needed", workspace_bytes, ws.bytes());
    // 1 tables, levels, Haar mosaics; 2 the two products of the DCT; 4 the window kernels; 8 finish
    const int stages = stage_mask("SWF_FEATURE_STAGES");
    const int planes = B * kImgPlanes, win = (int)d.window;
    if (stages & 1) {
        fmi_tables_kernel<<<(unsigned)cdiv64((int64_t)H * H + (int64_t)W * W, kThreads), kThreads, 0, stream>>>(f.dh, f.dwt, H, W);
        SWF_TRY(check_launch("fmi_tables_kernel"));
        fmi_levels_kernel<<<dim3((unsigned)cdiv64(f.n, kThreads), B), kThreads, 0, stream>>>(fusion, ir, vis, f.n, f.X);
        SWF_TRY(check_launch("fmi_levels_kernel"));
        if (f.nv > 0) {
            fmi_haar_kernel<<<dim3((unsigned)cdiv64(f.nv / 4, kThreads), B), kThreads, 0, stream>>>(fusion, ir, vis, H, W, f.hh, f.wh, f.V);
            SWF_TRY(check_launch("fmi_haar_kernel"));
        }
    }
    if (stages & 2) {   // Y = X D_W^T, then X <- D_H Y: the levels are no longer needed, the coefficients take their place
        Gemm g{};
        g = Gemm{f.X, f.dwt, f.Y, f.n, 0, f.n, W, W, H, W, W, 0, nullptr, 1, 1, 1};
        SWF_TRY(launch_gemm<kStorePlain>(g, planes, stream));
        g = Gemm{f.dh, f.Y, f.X, 0, f.n, f.n, H, W, H, W, H, 0, nullptr, 1, 1, 1};
        SWF_TRY(launch_gemm<kStorePlain>(g, planes, stream));
    }
    FmiFinish fin{};
    if (stages & 4) {
        if (win == 3)
            SWF_TRY(launch_windows<3>(f, d, fusion, ir, vis, B, H, W, fin, stream));
        else
            SWF_TRY(launch_windows<5>(f, d, fusion, ir, vis, B, H, W, fin, stream));
    }
    if (stages & 8) {
        fmi_finish_kernel<<<B, kThreads, 0, stream>>>(f.part, f.part_stride, fin, out);
        SWF_TRY(check_launch("fmi_finish_kernel"));
    }
    return SWF_OK;
}

}  // namespace swf
