// SSIM (with its two per-source parts), MS-SSIM, Piella's Q_S / Q_W / Q_E, Cvejic's Q_C and Yang's Q_Y of fused images against their
// infrared and visible sources: the nine values of swf_fusion_structure (include/swinfuse.h has the definitions).  They are restated
// from the published definitions; no MATLAB or toolbox copy is available to this build, so PARITY WITH ANY OF THEM IS UNPINNED
// (DESIGN.md 6c).  tests/structure_restatement.py is the same text in numpy and is what these kernels are checked against.
//
// Every value is a function of 8-bit levels (levels.h).  The Gaussian group is fp64 after the quantiser, as kernels_fidelity.hip is
// and for its reason.  The box group keeps its window sums as integers: int32 sums of levels and of products, int64 for
// V = n S_XX - S_X^2 and C = n S_XY - S_X S_Y, every zero test on those integers, then one fp64 expression per window.  Every sum has
// a fixed order (unrolled taps, LDS trees, per-tile partials); no atomics of any kind; every workspace element that is read has been
// written by the same call, so nothing needs zeroing.
//
// Kernels, all on one stream (A, B, F = levels of ir, vis, fusion):
//   box_moments_kernel<WN, EDGE>  WN = 8 (Piella, Cvejic) or 7 (Yang).  A workgroup owns a 16x32 tile of the window positions: the tile
//                          plus its WN - 1 halo of A, B, F goes to LDS as 16-bit integers (EDGE: the levels with one more pixel of
//                          zero border first, then the Sobel-L1 edge image |sx| + |sy| <= 2040 formed from them in the tile), the nine
//                          moments A, B, F, AA, BB, FF, AF, BF, AB are summed along rows into LDS and down columns into registers,
//                          two windows per thread; four sums per tile: t, m t, m (an integer) and Q_C's (WN = 8) or Q_Y's (WN = 7)
//                          term.  Launched three times: <8, levels>, <8, edges>, <7, levels>.
//   gauss_moments_kernel<11, QUANT, SsimRule> (metric_frag.h)  one per scale, both pairs sharing F; four sums per tile: l cs and cs
//                          of (A, F) and of (B, F).
//   mean2x2_kernel<QUANT>  the three planes of scale j + 1 from those of scale j (QUANT: from the fp32 images, quantised here).
//   structure_finish_kernel  one workgroup per image adds the per-tile sums in a fixed order and writes the row.
// The window weights are computed on the host in fp64 and passed by value.
#include "kernels_structure.h"
#include "metric_frag.h"

#include <algorithm>
#include <cmath>

namespace swf {
namespace {

constexpr int kScales = 5;
constexpr int kTaps = 11;              // the Gaussian window: g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1
constexpr double kSigma = 1.5;
constexpr int kMinMs = kTaps << (kScales - 1);   // 176: the smallest axis whose scale-5 plane still holds one window
constexpr int kBoxLaunches = 3;        // <8, levels>, <8, edges>, <7, levels>

// ------------------------------------------------------------------------------------------------------------------------------
// Box group
// ------------------------------------------------------------------------------------------------------------------------------
// s(X, Y) of the header from the integer sums of one window.  No contraction: the restatement rounds every product.
__device__ __forceinline__ double s_index(int SX, int SY, int64_t VX, int64_t VY, int64_t CXY, double n, double C1, double C2) {
#pragma clang fp contract(off)
    const double n2 = n * n;
    const double mx = (double)SX / n, my = (double)SY / n;
    const double vx = (double)VX / n2, vy = (double)VY / n2, cxy = (double)CXY / n2;
    return ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2));
}

// The Sobel-L1 edge strength |sx| + |sy| of the 3x3 patch of levels whose top-left is p, pitch in elements.
__device__ __forceinline__ int sobel_l1(const unsigned short* p, int pitch) {
    int sx, sy;
    sobel3x3(p, pitch, sx, sy);
    return abs(sx) + abs(sy);
}

// oh = H - WN + 1, ow = W - WN + 1 >= 1: the window positions.  part: [B][part_stride] doubles, this launch's tiles from part_off on,
// four per tile: sum t, sum m t, sum m (an int64 in the slot's bits), sum of the Q_C term (WN = 8) or of the Q_Y term (WN = 7).
template <int WN, bool EDGE>
__global__ __launch_bounds__(kThreads) void box_moments_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                               const float* __restrict__ vis, int H, int W, int oh, int ow, int tiles_x,
                                                               double* __restrict__ part, int64_t part_stride, int64_t part_off,
                                                               double C1, double C2, double Ty) {
    constexpr int PW = kTX + WN - 1, PH = kTY + WN - 1;
    constexpr int RW = PW + 2, RH = PH + 2;            // EDGE: the levels under the tile with the Sobel masks' pixel around them
    __shared__ unsigned short raw[EDGE ? 3 * RH * RW : 1];
    __shared__ unsigned short in[3][PH * PW];
    __shared__ int tmp[9][PH * kTX];
    __shared__ double red[3][kThreads];
    __shared__ unsigned long long redm[kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kTY, tx0 = (blockIdx.x % tiles_x) * kTX;
    const int64_t img = (int64_t)b * H * W;
    const float* src[3] = {ir, vis, fusion};
    if (EDGE) {
        for (int i = tid; i < RH * RW; i += kThreads) {
            const int y = ty0 + i / RW - 1, x = tx0 + i % RW - 1;
            const bool ok = y >= 0 && x >= 0 && y < H && x < W;   // zero border
            const int64_t o = img + (int64_t)y * W + x;
#pragma unroll
            for (int k = 0; k < 3; ++k) raw[k * RH * RW + i] = ok ? (unsigned short)level(src[k][o]) : (unsigned short)0;
        }
        __syncthreads();
        for (int i = tid; i < PH * PW; i += kThreads) {
            const int r = i / PW, c = i % PW;
            const bool ok = ty0 + r < H && tx0 + c < W;
#pragma unroll
            for (int k = 0; k < 3; ++k) in[k][i] = ok ? (unsigned short)sobel_l1(&raw[k * RH * RW + r * RW + c], RW) : (unsigned short)0;
        }
    } else {
        for (int i = tid; i < PH * PW; i += kThreads) {
            const int y = ty0 + i / PW, x = tx0 + i % PW;
            const bool ok = y < H && x < W;
            const int64_t o = img + (int64_t)y * W + x;
#pragma unroll
            for (int k = 0; k < 3; ++k) in[k][i] = ok ? (unsigned short)level(src[k][o]) : (unsigned short)0;
        }
    }
    __syncthreads();
    for (int i = tid; i < PH * kTX; i += kThreads) {       // rows: at most 8 * 2040^2 < 2^31
        const int r = i >> 5, c = i & 31;
        const unsigned short *pa = &in[0][r * PW + c], *pb = &in[1][r * PW + c], *pf = &in[2][r * PW + c];
        int s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < WN; ++k) {
            const int a = pa[k], bb = pb[k], f = pf[k];
            s[0] += a;
            s[1] += bb;
            s[2] += f;
            s[3] += a * a;
            s[4] += bb * bb;
            s[5] += f * f;
            s[6] += a * f;
            s[7] += bb * f;
            s[8] += a * bb;
        }
#pragma unroll
        for (int m = 0; m < 9; ++m) tmp[m][i] = s[m];
    }
    __syncthreads();
    const int lx = tid & 31, ly0 = tid >> 5;
    constexpr int64_t n = WN * WN;
    double st = 0.0, smt = 0.0, sx = 0.0;
    long long sm = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ly = ly0 + 8 * j;
        if (ty0 + ly < oh && tx0 + lx < ow) {
            int s[9];                                      // columns: at most 64 * 2040^2 < 2^31
#pragma unroll
            for (int m = 0; m < 9; ++m) {
                int acc = 0;
#pragma unroll
                for (int k = 0; k < WN; ++k) acc += tmp[m][(ly + k) * kTX + lx];
                s[m] = acc;
            }
            const int64_t SA = s[0], SB = s[1], SF = s[2];
            const int64_t VA = n * s[3] - SA * SA, VB = n * s[4] - SB * SB, VF = n * s[5] - SF * SF;
            const int64_t CAF = n * s[6] - SA * SF, CBF = n * s[7] - SB * SF, CAB = n * s[8] - SA * SB;
            const double sAF = s_index(s[0], s[2], VA, VF, CAF, (double)n, C1, C2);
            const double sBF = s_index(s[1], s[2], VB, VF, CBF, (double)n, C1, C2);
            const double lam = VA + VB == 0 ? 0.5 : (double)VA / (double)(VA + VB);
            const double t = lam * sAF + (1.0 - lam) * sBF;
            const int64_t mi = VA > VB ? VA : VB;
            st += t;
            smt += (double)mi * t;
            sm += mi;
            if (WN == 8) {
                double sim = CAF + CBF == 0 ? 0.5 : (double)CAF / (double)(CAF + CBF);
                sim = sim < 0.0 ? 0.0 : (sim > 1.0 ? 1.0 : sim);
                sx += sim * sAF + (1.0 - sim) * sBF;
            } else {
                const double sAB = s_index(s[0], s[1], VA, VB, CAB, (double)n, C1, C2);
                sx += sAB >= Ty ? t : (sAF > sBF ? sAF : sBF);
            }
        }
    }
    red[0][tid] = st;
    red[1][tid] = smt;
    red[2][tid] = sx;
    redm[tid] = (unsigned long long)sm;
    SWF_TILE_TREE_INT(3, red, true, redm);
    if (tid == 0) {
        double* p = part + (int64_t)b * part_stride + part_off + (int64_t)blockIdx.x * 4;
        p[0] = red[0][0];
        p[1] = red[1][0];
        p[2] = __longlong_as_double((long long)redm[0]);
        p[3] = red[2][0];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Gaussian group: evaluation of one scale's moments
// ------------------------------------------------------------------------------------------------------------------------------
// gauss_moments_kernel's rule for one output pixel of ssim(X, Y), adding to sum l cs and sum cs: biased moments, not clamped.  No
// contraction: the variances are the differences the restatement forms, product rounded first.
struct SsimRule {
    static __device__ __forceinline__ void pixel(double muX, double muY, double XX, double YY, double XY, double C1, double C2, double& lcs,
                                                 double& cs) {
#pragma clang fp contract(off)
        const double vx = XX - muX * muX, vy = YY - muY * muY, cxy = XY - muX * muY;
        const double l = (2.0 * muX * muY + C1) / (muX * muX + muY * muY + C1);
        const double c = (2.0 * cxy + C2) / (vx + vy + C2);
        lcs += l * c;
        cs += c;
    }
};

// dst[B][dst_stride]: planes A, B, F of dh x dw, dh = floor(h / 2), dw = floor(w / 2): output (y, x) is the mean of the 2x2 block at
// (2 y, 2 x), whose last row 2 y + 1 <= h - 1.  Exact: the planes hold multiples of 4^-j below 256.
template <bool QUANT>
__global__ __launch_bounds__(kThreads) void mean2x2_kernel(Source src, int w, double* __restrict__ dst, int64_t dst_stride, int dh, int dw) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x, n = (int64_t)dh * dw;
    if (i >= n) return;
    const int y = (int)(i / dw), x = (int)(i % dw);
    const int64_t o = (int64_t)blockIdx.y * src.stride + (int64_t)(2 * y) * w + 2 * x;
    double* out = dst + (int64_t)blockIdx.y * dst_stride + i;
#pragma unroll
    for (int p = 0; p < 3; ++p)
        out[(int64_t)p * n] = 0.25 * ((load_px<QUANT>(src.p[p], o) + load_px<QUANT>(src.p[p], o + 1)) +
                                      (load_px<QUANT>(src.p[p], o + w) + load_px<QUANT>(src.p[p], o + w + 1)));
}

// ------------------------------------------------------------------------------------------------------------------------------
// Finish: one workgroup per image
// ------------------------------------------------------------------------------------------------------------------------------
struct FinishArgs {
    int nscales;                       // 0, 1 or kScales
    int64_t g_tiles[kScales];          // Gaussian tiles per scale; their partials lie one scale after the other from 0 on
    double g_count[kScales];           // output pixels per scale
    int64_t box_tiles[kBoxLaunches];   // 0: the image is smaller than the window
    int64_t box_off[kBoxLaunches];
    double box_count[kBoxLaunches];    // window positions
    double alpha;
};

__global__ __launch_bounds__(kThreads) void structure_finish_kernel(const double* __restrict__ part, int64_t part_stride, FinishArgs a,
                                                                    double* __restrict__ out) {
    __shared__ double red[4][kThreads];
    __shared__ unsigned long long ired[kThreads];
    const double* p = part + (int64_t)blockIdx.x * part_stride;
    const double wgt[kScales] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    double ssim[2] = {0.0, 0.0}, ms[2] = {1.0, 1.0};
    const double* pg = p;
    for (int s = 0; s < a.nscales; ++s) {
        double r[4];   // sum l cs and sum cs of (A, F), then of (B, F)
        tile_sums<4>(pg, a.g_tiles[s], red, r);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double lcs = r[2 * k] / a.g_count[s], cs = r[2 * k + 1] / a.g_count[s];
            if (s == 0) ssim[k] = lcs;
            const double v = s == kScales - 1 ? lcs : cs;
            ms[k] *= pow(v < 0.0 ? 0.0 : v, wgt[s]);
        }
        pg += a.g_tiles[s] * 4;
    }
    if (a.nscales < kScales) ms[0] = ms[1] = 0.0;
    double q[kBoxLaunches][3] = {};   // Q_S, Q_W and the mean of the fourth sum, per launch
    for (int i = 0; i < kBoxLaunches; ++i) {
        if (a.box_tiles[i] == 0) continue;
        double r[4];   // sum t, sum m t, (slot 2: see sm), sum of the launch's own term
        long long sm;  // sum m
        tile_sums<4, true>(p + a.box_off[i], a.box_tiles[i], red, r, ired, &sm);
        q[i][0] = r[0] / a.box_count[i];
        q[i][1] = sm == 0 ? q[i][0] : r[1] / (double)sm;
        q[i][2] = r[3] / a.box_count[i];
    }
    if (threadIdx.x == 0) {
        double* o = out + (int64_t)blockIdx.x * SWF_STRUCTURE_COUNT;
        o[SWF_STRUCTURE_SSIM] = ssim[0] + ssim[1];
        o[SWF_STRUCTURE_SSIM_IR] = ssim[0];
        o[SWF_STRUCTURE_SSIM_VIS] = ssim[1];
        o[SWF_STRUCTURE_MS_SSIM] = ms[0] + ms[1];
        o[SWF_STRUCTURE_QS] = q[0][0];
        o[SWF_STRUCTURE_QW] = q[0][1];
        o[SWF_STRUCTURE_QE] = a.box_tiles[0] == 0 ? 0.0 : q[0][1] * pow(q[1][1] < 0.0 ? 0.0 : q[1][1], a.alpha);
        o[SWF_STRUCTURE_QC] = q[0][2];
        o[SWF_STRUCTURE_QY] = q[2][2];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------------------------------------------
struct Box {
    int oh, ow;             // window positions
    int tiles_x, ntiles;    // 0 tiles: the image is smaller than the window
    int64_t part_off;
};

struct StructurePlan {
    int nscales;            // 0 under 11 pixels in an axis, kScales from 176 on, else 1
    Scale s[kScales];
    Box box[kBoxLaunches];
    int64_t part_stride, planes_per_image;   // doubles per image
    double* part;
    double* planes;
};

constexpr int kBoxWindow[kBoxLaunches] = {8, 8, 7};

StructurePlan carve_structure(Carver& ws, int B, int H, int W) {
    StructurePlan f{};
    const int small = std::min(H, W);
    f.nscales = small < kTaps ? 0 : (small < kMinMs ? 1 : kScales);
    int h = H, w = W;
    for (int i = 0; i < f.nscales; ++i) {
        Scale& s = f.s[i];
        if (i > 0) {
            h /= 2;
            w /= 2;
            s.plane_off = f.planes_per_image;
            f.planes_per_image += (int64_t)3 * h * w;
        }
        s.size(h, w, kTaps);
        s.part_off = f.part_stride;
        f.part_stride += (int64_t)s.ntiles * 4;
    }
    for (int i = 0; i < kBoxLaunches; ++i) {
        Box& x = f.box[i];
        x.part_off = f.part_stride;
        if (small < kBoxWindow[i]) continue;
        x.oh = H - kBoxWindow[i] + 1;
        x.ow = W - kBoxWindow[i] + 1;
        x.tiles_x = cdiv(x.ow, kTX);
        x.ntiles = x.tiles_x * cdiv(x.oh, kTY);
        f.part_stride += (int64_t)x.ntiles * 4;
    }
    f.part = reinterpret_cast<double*>(ws.floats((int64_t)B * f.part_stride * 2));
    f.planes = reinterpret_cast<double*>(ws.floats((int64_t)B * f.planes_per_image * 2));
    return f;
}

template <int WN, bool EDGE>
int launch_box(const StructurePlan& f, int i, const swf_structure_desc& d, double C1, double C2, const float* fusion, const float* ir,
               const float* vis, int B, int H, int W, hipStream_t stream) {
    const Box& x = f.box[i];
    if (x.ntiles == 0) return SWF_OK;
    box_moments_kernel<WN, EDGE><<<dim3(x.ntiles, B), kThreads, 0, stream>>>(fusion, ir, vis, H, W, x.oh, x.ow, x.tiles_x, f.part,
                                                                            f.part_stride, x.part_off, C1, C2, d.Ty);
    return check_launch("box_moments_kernel");
}

}  // namespace

size_t fusion_structure_workspace_bytes(int B, int H, int W) {
    Carver ws = Carver::measure();
    carve_structure(ws, B, H, W);
    return ws.bytes();
}

int fusion_structure(const swf_structure_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H, int W,
                     void* workspace, size_t workspace_bytes, hipStream_t stream) {
    Carver ws(workspace, workspace_bytes);
    const StructurePlan f = carve_structure(ws, B, H, W);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "fusion_structure: workspace of %zu bytes, %zu needed", workspace_bytes, ws.bytes());
    const int stages = stage_mask("SWF_STRUCTURE_STAGES");   // 1 Gaussian moments, 2 2x2 means, 4 box moments, 8 finish
    const double c1 = 255.0 * d.K1, c2 = 255.0 * d.K2;
    const double C1 = c1 * c1, C2 = c2 * c2;
    const Window<kTaps> win = make_window<kTaps>(kSigma);
    const Source images{{ir, vis, fusion}, (int64_t)H * W};
    for (int i = 0; i < f.nscales; ++i) {
        const Scale& s = f.s[i];
        if (i > 0 && (stages & 2)) {
            const dim3 grid((unsigned)cdiv64((int64_t)s.h * s.w, kThreads), B);
            if (i == 1)
                mean2x2_kernel<true><<<grid, kThreads, 0, stream>>>(images, f.s[0].w, f.planes + s.plane_off, f.planes_per_image, s.h, s.w);
            else
                mean2x2_kernel<false><<<grid, kThreads, 0, stream>>>(plane_source(f, i - 1), f.s[i - 1].w, f.planes + s.plane_off,
                                                                     f.planes_per_image, s.h, s.w);
            SWF_TRY(check_launch("mean2x2_kernel"));
        }
        if (stages & 1) {
            const dim3 grid(s.ntiles, B);
            if (i == 0)
                gauss_moments_kernel<kTaps, true, SsimRule><<<grid, kThreads, 0, stream>>>(images, s.h, s.w, s.oh, s.ow, s.tiles_x, f.part,
                                                                                           f.part_stride, s.part_off, win, C1, C2);
            else
                gauss_moments_kernel<kTaps, false, SsimRule><<<grid, kThreads, 0, stream>>>(plane_source(f, i), s.h, s.w, s.oh, s.ow, s.tiles_x,
                                                                                            f.part, f.part_stride, s.part_off, win, C1, C2);
            SWF_TRY(check_launch("gauss_moments_kernel"));
        }
    }
    if (stages & 4) {
        SWF_TRY((launch_box<8, false>(f, 0, d, C1, C2, fusion, ir, vis, B, H, W, stream)));
        SWF_TRY((launch_box<8, true>(f, 1, d, C1, C2, fusion, ir, vis, B, H, W, stream)));
        SWF_TRY((launch_box<7, false>(f, 2, d, C1, C2, fusion, ir, vis, B, H, W, stream)));
    }
    if (stages & 8) {
        FinishArgs a{};
        a.nscales = f.nscales;
        for (int i = 0; i < f.nscales; ++i) {
            a.g_tiles[i] = f.s[i].ntiles;
            a.g_count[i] = (double)((int64_t)f.s[i].oh * f.s[i].ow);
        }
        for (int i = 0; i < kBoxLaunches; ++i) {
            a.box_tiles[i] = f.box[i].ntiles;
            a.box_off[i] = f.box[i].part_off;
            a.box_count[i] = (double)((int64_t)f.box[i].oh * f.box[i].ow);
        }
        a.alpha = d.alpha;
        structure_finish_kernel<<<B, kThreads, 0, stream>>>(f.part, f.part_stride, a, out);
        SWF_TRY(check_launch("structure_finish_kernel"));
    }
    return SWF_OK;
}

}  // namespace swf
