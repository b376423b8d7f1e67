// Chen & Blum's Q_CB, Chen & Varshney's Q_CV, CE, EI and RMSE of fused images against their infrared and visible sources: the five
// values of swf_fusion_perception (include/swinfuse.h has the definitions).  They are restated from the published definitions and the
// open MATLAB evaluators; none is available to this build, so PARITY WITH ANY OF THEM IS UNPINNED.
// tests/perception_restatement.py is the same text in numpy and is what these kernels are checked against.
//
// Every value is a function of 8-bit levels (levels.h), fp64 after the quantiser.  Every sum has a fixed order (unrolled taps, LDS
// trees, per-tile partials); no atomics of any kind, the histograms included; every workspace element that is read has been written
// by the same call, so nothing needs zeroing.
//
// spec(X, G) = Re(IDFT2(DFT2(X) o G)) for a real image X and a real, even filter G runs as four real fp64 GEMMs on the matrix cores
// (v_mfma_f64_16x16x4_f64) over the half spectrum v = 0 .. Wh - 1, Wh = floor(W / 2) + 1, with C, S = cos, sin(2 pi ((j k) mod n) / n):
//   1  [Tr | Ti] = X [C_W | -S_W]                    H x W   by W x 2Wh     stored as [Tr; Ti]
//   2  [Zr; Zi]  = [C_H S_H; -S_H C_H] [Tr; Ti]      2H x 2H by 2H x Wh     times G'(u, v) = G(u, v) c_v / (H W) in the epilogue,
//                                                                            c_v = 1 for v = 0 and the Nyquist column, else 2
//   3  [Ur; Ui]  = [C_H -S_H; S_H C_H] [Zr; Zi]      2H x 2H by 2H x Wh     stored as [Ur | Ui]
//   4  Y         = [Ur | Ui] [C_W; -S_W]             H x 2Wh by 2Wh x W
// The other half of the spectrum is the conjugate of this one (X real, G even), which is what c_v stands for.
// The twiddle matrices, the GEMM kernel and its launch are dft_frag.h's, shared with kernels_comparative.hip.
//
// Kernels, all on one stream (A, B, F = levels of ir, vis, fusion; five planes per image: stretch(A), stretch(B), stretch(F) for Q_CB,
// stretch(A) - stretch(F) and stretch(B) - stretch(F) for Q_CV):
//   tables_kernel          the four twiddle matrices and the two filter tables G' (Q_CB's difference of Gaussians, Q_CV's
//                          Mannos-Sakrison), arguments reduced in integers before sincospi; shared by the whole batch
//   minmax_kernel          one workgroup per image and source: min and max level
//   stretch_kernel         the five planes
//   dft_gemm_kernel<STORE, NF>  64 x 16 NF tile (NF = 3 or 4, whichever pads N less), K step 16, a wave per 16 rows; launched four
//                          times over all 5 B planes
//   qcb_kernel             a workgroup owns a 16x32 tile: per plane the tile plus its 15-pixel halo of X' goes to LDS, both 31-tap
//                          filters run rows into LDS and columns into registers from that one tile, C' stays in registers; then the
//                          pointwise Q map and one tree: one sum per tile
//   qcv_kernel             one workgroup per 16x16 block: zero-border Sobel of stretch(A), stretch(B), G^alpha, squared filtered error;
//                          two sums per block (lambda_A D_A + lambda_B D_B, lambda_A + lambda_B)
//   levels_kernel          32x32 level tiles: the three 256-bin histograms of the tile (thread k scans for level k), F's Sobel
//                          magnitude under a replicated border, the squared differences
//   perception_finish_kernel  one workgroup per image adds the per-tile sums in a fixed order and writes the row.
#include "kernels_perception.h"
#include "metric_frag.h"
#include "dft_frag.h"

#include <cmath>

namespace swf {
namespace {

constexpr int kPlanes = 5;             // per image: sA, sB, sF, sA - sF, sB - sF
constexpr int kCbPlanes = 3;           // the first three take Q_CB's filter, the other two Q_CV's
constexpr int kTaps = 31, kHalo = 15;  // Q_CB's Gaussian kernels, x = -15 .. 15
constexpr int kBlock = 16;             // Q_CV's blocks
constexpr int kMaxAxis = 16384;        // 4 H^2 <= 2^30 elements in a twiddle matrix
constexpr int kMaxImages = 65535 / kPlanes;

// ------------------------------------------------------------------------------------------------------------------------------
// Tables
// ------------------------------------------------------------------------------------------------------------------------------
struct Tables {
    Twiddles w;         // the four twiddle matrices (dft_frag.h)
    double* g;          // [2][H][Wh]: G' of Q_CB, then of Q_CV
};

__global__ __launch_bounds__(kThreads) void tables_kernel(Tables t, int H, int W, int Wh, double f0, double f1, double a) {
    const int64_t nG = (int64_t)H * Wh;
    int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (fill_twiddle(t.w, i, H, W, Wh)) return;
    i -= twiddle_count(H, W, Wh);
    if (i < nG) {
        const int u = (int)(i / Wh), v = (int)(i % Wh);
        const int64_t su = u < (H + 1) / 2 ? u : u - H;   // s(v, W)^2 = v^2 for every v <= W / 2
        const double rho = sqrt((double)(su * su + (int64_t)v * v));
        const double scale = ((v == 0 || 2 * v == W) ? 1.0 : 2.0) / ((double)H * (double)W);
        const double rb = rho / 15.0, rv = rho / 4.0;
        const double e0 = rb / f0, e1 = rb / f1;
        t.g[i] = (exp(-(e0 * e0)) - a * exp(-(e1 * e1))) * scale;
        t.g[nG + i] = 2.6 * (0.0192 + 0.144 * rv) * exp(-pow(0.144 * rv, 1.1)) * scale;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Min / max and the five planes
// ------------------------------------------------------------------------------------------------------------------------------
// mm[B][3][2]: min and max level of A, B, F.  grid (3, B).
__global__ __launch_bounds__(kThreads) void minmax_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                          const float* __restrict__ vis, int64_t n, int* __restrict__ mm) {
    __shared__ int lo[kThreads], hi[kThreads];
    const int tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const float* src = (s == 0 ? ir : (s == 1 ? vis : fusion)) + (int64_t)b * n;
    int l = 255, h = 0;
    for (int64_t i = tid; i < n; i += kThreads) {
        const int v = level(src[i]);
        l = min(l, v);
        h = max(h, v);
    }
    lo[tid] = l;
    hi[tid] = h;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) {
        if (tid < st) {
            lo[tid] = min(lo[tid], lo[tid + st]);
            hi[tid] = max(hi[tid], hi[tid + st]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        mm[(b * 3 + s) * 2] = lo[0];
        mm[(b * 3 + s) * 2 + 1] = hi[0];
    }
}

__device__ __forceinline__ double stretch(int v, int lo, int hi) {
    return hi == lo ? 0.0 : rint((255.0 * (double)(v - lo)) / (double)(hi - lo));
}

// X[B][5][n] <- the planes.  grid (ceil(n / 256), B).
__global__ __launch_bounds__(kThreads) void stretch_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                           const float* __restrict__ vis, int64_t n, const int* __restrict__ mm,
                                                           double* __restrict__ X) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int b = blockIdx.y;
    const int* m = mm + b * 6;
    const int64_t o = (int64_t)b * n + i;
    const double sa = stretch(level(ir[o]), m[0], m[1]), sb = stretch(level(vis[o]), m[2], m[3]), sf = stretch(level(fusion[o]), m[4], m[5]);
    double* x = X + (int64_t)b * kPlanes * n + i;
    x[0] = sa;
    x[n] = sb;
    x[2 * n] = sf;
    x[3 * n] = sa - sf;
    x[4 * n] = sb - sf;
}

// ------------------------------------------------------------------------------------------------------------------------------
// The DFT products
// ------------------------------------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------------------------------------
// Q_CB: local contrast of the three filtered planes and the pointwise quality map
// ------------------------------------------------------------------------------------------------------------------------------
// Y: [B][5][plane_stride], planes 0..2 = X' of A, B, F as [H][W].  part[B][ntiles]: the tile's sum of lambda_A Q_AF + (1 - lambda_A) Q_BF.
__global__ __launch_bounds__(kThreads) void qcb_kernel(const double* __restrict__ Y, int64_t plane_stride, int H, int W, int tiles_x,
                                                       Window<kHalo + 1> g1, Window<kHalo + 1> g2, double p, double q, double Z,
                                                       double* __restrict__ part, int ntiles) {
    constexpr int PW = kTX + kTaps - 1, PH = kTY + kTaps - 1;
    __shared__ double in[PH * PW];
    __shared__ double tmp1[PH * kTX], tmp2[PH * kTX];
    __shared__ double red[1][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kTY, tx0 = (blockIdx.x % tiles_x) * kTX;
    const int lx = tid & 31, ly0 = tid >> 5;
    double cp[kCbPlanes][2];   // C' of A, B, F at output pixels (ly0, lx) and (ly0 + 8, lx)
#pragma unroll
    for (int k = 0; k < kCbPlanes; ++k) {                      // unrolled: cp stays in registers
        const double* src = Y + ((int64_t)b * kPlanes + k) * plane_stride;
        for (int i = tid; i < PH * PW; i += kThreads) {
            const int y = ty0 - kHalo + i / PW, x = tx0 - kHalo + i % PW;
            in[i] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(int64_t)y * W + x] : 0.0;   // zero padding
        }
        __syncthreads();
        for (int i = tid; i < PH * kTX; i += kThreads) {      // rows
            const double* r = &in[(i >> 5) * PW + (i & 31)];
            double a1 = g1.g[kHalo] * r[kHalo], a2 = g2.g[kHalo] * r[kHalo];
#pragma unroll
            for (int t = 0; t < kHalo; ++t) {                  // the kernels are even: taps t and 30 - t share a weight
                const double pair = r[t] + r[kTaps - 1 - t];
                a1 += g1.g[t] * pair;
                a2 += g2.g[t] * pair;
            }
            tmp1[i] = a1;
            tmp2[i] = a2;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {                          // columns
            const int o = (ly0 + 8 * j) * kTX + lx;
            double b1 = g1.g[kHalo] * tmp1[o + kHalo * kTX], b2 = g2.g[kHalo] * tmp2[o + kHalo * kTX];
#pragma unroll
            for (int t = 0; t < kHalo; ++t) {
                b1 += g1.g[t] * (tmp1[o + t * kTX] + tmp1[o + (kTaps - 1 - t) * kTX]);
                b2 += g2.g[t] * (tmp2[o + t * kTX] + tmp2[o + (kTaps - 1 - t) * kTX]);
            }
            const double c = b2 == 0.0 ? 0.0 : fabs(b1 / b2 - 1.0);
            cp[k][j] = pow(c, p) / (pow(c, q) + Z);
        }
        __syncthreads();
    }
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (ty0 + ly0 + 8 * j < H && tx0 + lx < W) {
            const double ca = cp[0][j], cb = cp[1][j], cf = cp[2][j];
            const double qa = (ca == 0.0 && cf == 0.0) ? 1.0 : fmin(ca, cf) / fmax(ca, cf);
            const double qb = (cb == 0.0 && cf == 0.0) ? 1.0 : fmin(cb, cf) / fmax(cb, cf);
            const double den = ca * ca + cb * cb;
            const double lam = den == 0.0 ? 0.5 : (ca * ca) / den;
            sum += lam * qa + (1.0 - lam) * qb;
        }
    }
    red[0][tid] = sum;
    SWF_TILE_TREE(1, red);
    if (tid == 0) part[(int64_t)b * ntiles + blockIdx.x] = red[0][0];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Q_CV: edge saliency and filtered error per 16x16 block
// ------------------------------------------------------------------------------------------------------------------------------
// X: [B][5][n]: planes 0, 1 = stretch(A), stretch(B).  Y: [B][5][plane_stride]: planes 3, 4 = spec(sA - sF), spec(sB - sF) as [H][W].
// part[B][nblocks][2]: lambda_A D_A + lambda_B D_B and lambda_A + lambda_B of the block.
__global__ __launch_bounds__(kThreads) void qcv_kernel(const double* __restrict__ X, const double* __restrict__ Y, int64_t plane_stride,
                                                       int H, int W, int blocks_x, double alpha, double* __restrict__ part, int nblocks) {
    __shared__ double red[4][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int y = (blockIdx.x / blocks_x) * kBlock + (tid >> 4), x = (blockIdx.x % blocks_x) * kBlock + (tid & 15);
    const int64_t n = (int64_t)H * W;
    double v[4] = {0.0, 0.0, 0.0, 0.0};   // G_A^alpha, G_B^alpha, Y_A^2, Y_B^2
    if (y < H && x < W) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double* s = X + ((int64_t)b * kPlanes + k) * n;
            auto px = [&](int yy, int xx) { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? (int)s[(int64_t)yy * W + xx] : 0; };
            const int a = px(y - 1, x - 1), bb = px(y - 1, x), c = px(y - 1, x + 1), d = px(y, x - 1), e = px(y, x + 1);
            const int f = px(y + 1, x - 1), gg = px(y + 1, x), h = px(y + 1, x + 1);
            const int sx = (c - a) + 2 * (e - d) + (h - f), sy = (a + 2 * bb + c) - (f + 2 * gg + h);
            v[k] = pow(sqrt((double)(sx * sx + sy * sy)), alpha);
            const double e2 = Y[((int64_t)b * kPlanes + kCbPlanes + k) * plane_stride + (int64_t)y * W + x];
            v[2 + k] = e2 * e2;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][tid] = v[k];
    SWF_TILE_TREE(4, red);
    if (tid == 0) {
        const double la = red[0][0], lb = red[1][0], da = red[2][0] / (double)(kBlock * kBlock), db = red[3][0] / (double)(kBlock * kBlock);
        double* o = part + ((int64_t)b * nblocks + blockIdx.x) * 2;
        o[0] = la * da + lb * db;
        o[1] = la + lb;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// CE, EI, RMSE: one pass over the levels
// ------------------------------------------------------------------------------------------------------------------------------
// hist[B][ntiles][3][256]: the tile's counts of F, A, B.  part[B][ntiles][4]: sum of F's Sobel magnitude (replicated border),
// sum (A - F)^2, sum (B - F)^2 (integers under 2^27, exact as doubles), 0.
__global__ __launch_bounds__(kThreads) void levels_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                          const float* __restrict__ vis, int H, int W, int tiles_x,
                                                          unsigned* __restrict__ hist, double* __restrict__ part, int ntiles) {
    __shared__ int sL[3][kLP * kLP];
    __shared__ double red[3][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kLT, tx0 = (blockIdx.x % tiles_x) * kLT;
    load_level_tile<true>(sL, fusion, ir, vis, (int64_t)b * H * W, ty0, tx0, H, W);
    const int ny = min(kLT, H - ty0), nx = min(kLT, W - tx0);
    unsigned cnt[3] = {0, 0, 0};           // thread k counts level k: every lane reads the same word, a broadcast
    for (int ly = 0; ly < ny; ++ly)
        for (int lx = 0; lx < nx; ++lx) {
            const int o = (ly + 1) * kLP + lx + 1;
#pragma unroll
            for (int k = 0; k < 3; ++k) cnt[k] += sL[k][o] == tid;
        }
    unsigned* h = hist + ((int64_t)b * ntiles + blockIdx.x) * 768;
#pragma unroll
    for (int k = 0; k < 3; ++k) h[k * 256 + tid] = cnt[k];
    double sg = 0.0, da = 0.0, db = 0.0;
    walk_level_tile(ty0, tx0, H, W, [&](int o, int, int) {
        int sx, sy;
        sobel3x3(&sL[0][o], kLP, sx, sy);
        sg += sqrt((double)(sx * sx + sy * sy));
        const int c = o + kLP + 1, ea = sL[1][c] - sL[0][c], eb = sL[2][c] - sL[0][c];
        da += (double)(ea * ea);
        db += (double)(eb * eb);
    });
    red[0][tid] = sg;
    red[1][tid] = da;
    red[2][tid] = db;
    SWF_TILE_TREE(3, red);
    if (tid < 4) part[((int64_t)b * ntiles + blockIdx.x) * 4 + tid] = tid < 3 ? red[tid][0] : 0.0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Finish: one workgroup per image
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void perception_finish_kernel(const double* __restrict__ qcb_part, int cb_tiles,
                                                                     const double* __restrict__ qcv_part, int cv_blocks,
                                                                     const double* __restrict__ lev_part, const unsigned* __restrict__ hist,
                                                                     int lev_tiles, double count, double* __restrict__ out) {
    __shared__ double red[4][kThreads];
    const int tid = threadIdx.x, b = blockIdx.x;
    double cb[1], cv[2], lv[4];
    tile_sums<1>(qcb_part + (int64_t)b * cb_tiles, cb_tiles, red, cb);
    tile_sums<2>(qcv_part + (int64_t)b * cv_blocks * 2, cv_blocks, red, cv);
    tile_sums<4>(lev_part + (int64_t)b * lev_tiles * 4, lev_tiles, red, lv);
    unsigned n[3] = {0, 0, 0};             // level tid in F, A, B
    const unsigned* h = hist + (int64_t)b * lev_tiles * 768;
    for (int t = 0; t < lev_tiles; ++t)
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] += h[(int64_t)t * 768 + k * 256 + tid];
    const double pf = (double)n[0] / count;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double px = (double)n[1 + k] / count;
        red[k][tid] = (n[0] > 0 && n[1 + k] > 0) ? px * log2(px / pf) : 0.0;
    }
    SWF_TILE_TREE(2, red);
    if (tid == 0) {
        double* o = out + (int64_t)b * SWF_PERCEPTION_COUNT;
        o[SWF_PERCEPTION_QCB] = cb[0] / count;
        o[SWF_PERCEPTION_QCV] = cv[1] == 0.0 ? 0.0 : cv[0] / cv[1];
        o[SWF_PERCEPTION_CE] = (red[0][0] + red[1][0]) / 2.0;
        o[SWF_PERCEPTION_EI] = lv[0] / count;
        o[SWF_PERCEPTION_RMSE] = (sqrt(lv[1] / count) / 255.0 + sqrt(lv[2] / count) / 255.0) / 2.0;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------------------------------------------
struct PerceptionPlan {
    int Wh;
    int cb_tiles_x, cb_tiles;      // Q_CB's 16x32 tiles
    int cv_blocks_x, cv_blocks;    // Q_CV's 16x16 blocks
    int lev_tiles_x, lev_tiles;    // the 32x32 level tiles
    int64_t n, plane;              // doubles per image plane: H W, and 2 H Wh (>= H W) of the transform buffers
    Tables t;
    int* mm;
    double *X, *T, *Z;
    double *qcb_part, *qcv_part, *lev_part;
    unsigned* hist;
};

PerceptionPlan carve_perception(Carver& ws, int B, int H, int W) {
    PerceptionPlan f{};
    f.Wh = W / 2 + 1;
    f.cb_tiles_x = cdiv(W, kTX);
    f.cb_tiles = f.cb_tiles_x * cdiv(H, kTY);
    f.cv_blocks_x = cdiv(W, kBlock);
    f.cv_blocks = f.cv_blocks_x * cdiv(H, kBlock);
    f.lev_tiles_x = cdiv(W, kLT);
    f.lev_tiles = f.lev_tiles_x * cdiv(H, kLT);
    f.n = (int64_t)H * W;
    f.plane = (int64_t)2 * H * f.Wh;
    f.t.w.a2 = carve_doubles(ws, (int64_t)4 * H * H);
    f.t.w.a3 = carve_doubles(ws, (int64_t)4 * H * H);
    f.t.w.bw1 = carve_doubles(ws, (int64_t)2 * W * f.Wh);
    f.t.w.bw4 = carve_doubles(ws, (int64_t)2 * W * f.Wh);
    f.t.g = carve_doubles(ws, (int64_t)2 * H * f.Wh);
    f.mm = reinterpret_cast<int*>(ws.floats((int64_t)B * 6));
    f.X = carve_doubles(ws, (int64_t)B * kPlanes * f.n);
    f.T = carve_doubles(ws, (int64_t)B * kPlanes * f.plane);
    f.Z = carve_doubles(ws, (int64_t)B * kPlanes * f.plane);
    f.qcb_part = carve_doubles(ws, (int64_t)B * f.cb_tiles);
    f.qcv_part = carve_doubles(ws, (int64_t)B * f.cv_blocks * 2);
    f.lev_part = carve_doubles(ws, (int64_t)B * f.lev_tiles * 4);
    f.hist = reinterpret_cast<unsigned*>(ws.floats((int64_t)B * f.lev_tiles * 768));
    return f;
}

// The 1-D factor of exp(-(x^2 + y^2) / (2 sd^2)) / (2 pi sd^2) over x = -15 .. 0 (even in x; not normalised to sum 1).
Window<kHalo + 1> gauss_factor(double sd) {
    Window<kHalo + 1> w;
    for (int i = 0; i <= kHalo; ++i) {
        const double x = i - kHalo;
        w.g[i] = std::exp(-(x * x) / (2.0 * sd * sd)) / std::sqrt(2.0 * M_PI * sd * sd);
    }
    return w;
}

}  // namespace

bool perception_shape_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && H <= kMaxAxis && W <= kMaxAxis && B <= kMaxImages; }

size_t fusion_perception_workspace_bytes(int B, int H, int W) {
    Carver ws = Carver::measure();
    carve_perception(ws, B, H, W);
    return ws.bytes();
}

int fusion_perception(const swf_perception_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H,
                      int W, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    Carver ws(workspace, workspace_bytes);
    const PerceptionPlan f = carve_perception(ws, B, H, W);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "fusion_perception: workspace of %zu bytes, %zu needed", workspace_bytes, ws.bytes());
    const int stages = stage_mask("SWF_PERCEPTION_STAGES");   // 1 tables, min / max, planes; 2 the four products; 4 maps and levels; 8 finish
    const int Wh = f.Wh, planes = B * kPlanes;
    if (stages & 1) {
        const int64_t total = (int64_t)4 * H * H + (int64_t)W * Wh + (int64_t)H * Wh;
        tables_kernel<<<(unsigned)cdiv64(total, kThreads), kThreads, 0, stream>>>(f.t, H, W, Wh, d.f0, d.f1, d.a);
        SWF_TRY(check_launch("tables_kernel"));
        minmax_kernel<<<dim3(3, B), kThreads, 0, stream>>>(fusion, ir, vis, f.n, f.mm);
        SWF_TRY(check_launch("minmax_kernel"));
        stretch_kernel<<<dim3((unsigned)cdiv64(f.n, kThreads), B), kThreads, 0, stream>>>(fusion, ir, vis, f.n, f.mm, f.X);
        SWF_TRY(check_launch("stretch_kernel"));
    }
    if (stages & 2) {
        Gemm g{};
        g = Gemm{f.X, f.t.w.bw1, f.T, f.n, 0, f.plane, W, 2 * Wh, H, 2 * Wh, W, Wh, nullptr};
        SWF_TRY(launch_gemm<kStoreFoldCols>(g, planes, stream));
        g = Gemm{f.t.w.a2, f.T, f.Z, 0, f.plane, f.plane, 2 * H, Wh, 2 * H, Wh, 2 * H, H, f.t.g, kPlanes, kCbPlanes};
        SWF_TRY(launch_gemm<kStoreScale>(g, planes, stream));
        g = Gemm{f.t.w.a3, f.Z, f.T, 0, f.plane, f.plane, 2 * H, Wh, 2 * H, Wh, 2 * H, H, nullptr};
        SWF_TRY(launch_gemm<kStoreFoldRows>(g, planes, stream));
        g = Gemm{f.T, f.t.w.bw4, f.Z, f.plane, 0, f.plane, 2 * Wh, W, H, W, 2 * Wh, 0, nullptr};
        SWF_TRY(launch_gemm<kStorePlain>(g, planes, stream));
    }
    if (stages & 4) {
        qcb_kernel<<<dim3(f.cb_tiles, B), kThreads, 0, stream>>>(f.Z, f.plane, H, W, f.cb_tiles_x, gauss_factor(2.0), gauss_factor(4.0), d.p,
                                                                 d.q, d.Z, f.qcb_part, f.cb_tiles);
        SWF_TRY(check_launch("qcb_kernel"));
        qcv_kernel<<<dim3(f.cv_blocks, B), kThreads, 0, stream>>>(f.X, f.Z, f.plane, H, W, f.cv_blocks_x, d.alpha, f.qcv_part, f.cv_blocks);
        SWF_TRY(check_launch("qcv_kernel"));
        levels_kernel<<<dim3(f.lev_tiles, B), kThreads, 0, stream>>>(fusion, ir, vis, H, W, f.lev_tiles_x, f.hist, f.lev_part, f.lev_tiles);
        SWF_TRY(check_launch("levels_kernel"));
    }
    if (stages & 8) {
        perception_finish_kernel<<<B, kThreads, 0, stream>>>(f.qcb_part, f.cb_tiles, f.qcv_part, f.cv_blocks, f.lev_part, f.hist,
                                                             f.lev_tiles, (double)f.n, out);
        SWF_TRY(check_launch("perception_finish_kernel"));
    }
    return SWF_OK;
}

}  // namespace swf
