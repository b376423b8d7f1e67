// Fusion-quality metrics of fused images against their infrared and visible sources: EN, MI, SD, SF, AG, CC, SCD, MSE, PSNR, Qabf
// (include/swinfuse.h has the definitions).  They are restated from the published definitions and the common open evaluators; no
// MATLAB or VIFB toolkit is available to this build, so PARITY WITH ANY OF THEM IS UNPINNED.
// tests/metrics_restatement.py is the same text in numpy fp64 and is what these kernels are checked against.
//
// Every metric is a function of 8-bit levels: level(x) = (int) min(max(fadd(fmul(x, 255), 0.5), 0), 255) in fp32 with two roundings
// (torchvision save_image's quantiser; NaN -> 0).  Counts and sums of integer products are exact integers (u32 counters, u64 sums,
// integer atomics); the per-pixel arithmetic of AG and Qabf is fp64; every floating-point sum has a fixed order (per-thread
// sequences, LDS trees, per-tile partials), so the ten values are bit-identical from call to call.
//
// Kernels, all on one stream:
//   metrics_zero_kernel    zeroes the histograms and sums the next kernel accumulates into.
//   metrics_hist_kernel    grid (tiles of 8192 pixels, 2 sources, B).  The 256x256 joint histogram of (fusion, source) of the tile is
//                          built in LDS as packed 16-bit counters (128 KB; a tile has fewer than 65536 pixels, so no counter wraps),
//                          and the non-zero words are added to the image's u32 histogram with vector integer atomics.  The source-0
//                          workgroups also sum ir * vis, the source-1 workgroups the squared row and column differences of fusion
//                          (u32 per wave, u64 atomics).  <false>: the same with every pixel's atomic sent straight to global memory.
//   metrics_grad_kernel    32x32 tiles with a 1-pixel halo of the three level images in LDS: zero-border Sobel, the Qabf numerator
//                          and denominator and the AG sum in fp64; one partial triple per tile.
//   metrics_finish_kernel  one workgroup per image: marginals from the joint counts, then EN, MI, the moments (centred sums over
//                          bins and cells), CC, SCD, MSE, PSNR; adds the tile partials in a fixed order; writes the ten doubles.
//
// gfx950 cross-compile (hipcc -O3): no scratch in any kernel; VGPRs hist<true> / hist<false> / grad / finish as reported in DESIGN.md 6c.
#include "kernels_metrics.h"
#include "metric_frag.h"

#include <algorithm>
#include <cmath>

namespace swf {
namespace {

constexpr int kCells = 256 * 256;
constexpr int kHistTile = 8192;        // pixels per workgroup of the histogram pass
constexpr int kHistThreads = 1024;
constexpr int kHistLdsBytes = kCells * 2;
static_assert(kHistTile <= 65535, "a packed 16-bit counter must hold a whole tile");
static_assert((int64_t)(kHistTile / kHistThreads) * 255 * 255 * 64 < (int64_t(1) << 32), "a wave's u32 partial sum must not wrap");
constexpr int kSumsPerImage = 4;       // sum ir*vis, sum row diff^2, sum col diff^2, (pad)
constexpr int kFinThreads = 1024;
constexpr double kHalfPi = 1.57079632679489661923;

typedef unsigned long long u64;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Zeroes the histograms and sums.  A kernel of the library's own, not a memset: with a hipMemsetAsync node in its place the call
// captured into a hipGraph and replayed gave other histogram values than the eager call on this ROCm version (cause not established).
__global__ __launch_bounds__(256) void metrics_zero_kernel(uint4* __restrict__ p, int64_t n16) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Joint histograms, sum ir*vis, SF sums
// ------------------------------------------------------------------------------------------------------------------------------
template <bool PRIVATE>
__global__ __launch_bounds__(kHistThreads) void metrics_hist_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                                    const float* __restrict__ vis, uint32_t* __restrict__ hist,
                                                                    u64* __restrict__ sums, int H, int W) {
    extern __shared__ uint32_t cells[];   // PRIVATE: kCells / 2 words, cell c in half (c & 1) of word c >> 1
    const int tid = threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    const int n = H * W;
    const int64_t img = (int64_t)b * n;
    const float* f = fusion + img;
    const float* x = (s == 0 ? ir : vis) + img;
    uint32_t* h = hist + ((int64_t)b * 2 + s) * kCells;
    if (PRIVATE) {
        for (int i = tid; i < kCells / 2; i += kHistThreads) cells[i] = 0;
        __syncthreads();
    }
    const int begin = blockIdx.x * kHistTile, end = min(n, begin + kHistTile);
    uint32_t acc0 = 0, acc1 = 0;
    for (int p = begin + tid; p < end; p += kHistThreads) {
        const int lf = level(f[p]), lx = level(x[p]);
        const int c = lf * 256 + lx;
        if (PRIVATE)
            atomicAdd(&cells[c >> 1], 1u << ((c & 1) * 16));
        else
            atomicAdd(&h[c], 1u);
        if (s == 0) {
            acc0 += (uint32_t)(lx * level(vis[img + p]));
        } else {
            const int hh = p / W, w = p - hh * W;
            if (w > 0) {
                const int d = lf - level(f[p - 1]);
                acc0 += (uint32_t)(d * d);
            }
            if (hh > 0) {
                const int d = lf - level(f[p - W]);
                acc1 += (uint32_t)(d * d);
            }
        }
    }
    acc0 = wave_sum(acc0);
    acc1 = wave_sum(acc1);
    if ((tid & 63) == 0) {
        if (acc0) atomicAdd(&sums[(int64_t)b * kSumsPerImage + (s == 0 ? 0 : 1)], (u64)acc0);
        if (acc1) atomicAdd(&sums[(int64_t)b * kSumsPerImage + 2], (u64)acc1);
    }
    if (PRIVATE) {
        __syncthreads();
        for (int i = tid; i < kCells / 2; i += kHistThreads) {
            const uint32_t v = cells[i];
            if (v & 0xffffu) atomicAdd(&h[2 * i], v & 0xffffu);
            if (v >> 16) atomicAdd(&h[2 * i + 1], v >> 16);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Sobel (zero border), Qabf numerator / denominator, AG
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double edge_angle(int sx, int sy) { return sx == 0 ? kHalfPi : atan((double)sy / (double)sx); }

// Q_X g_X of one source at one pixel; n = sx^2 + sy^2 as integers, g = sqrt(n), a = edge_angle
__device__ __forceinline__ double qabf_term(const swf_metrics_desc& d, int nF, double gF, double aF, int nX, double gX, double aX) {
    const double G = nX > nF ? gF / gX : (nX == nF ? gF : gX / gF);
    const double A = 1.0 - fabs(aX - aF) / kHalfPi;
    const double Qg = d.Tg / (1.0 + exp(d.kg * (G - d.Dg)));
    const double Qa = d.Ta / (1.0 + exp(d.ka * (A - d.Da)));
    return Qg * Qa * gX;
}

__global__ __launch_bounds__(kThreads) void metrics_grad_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                                const float* __restrict__ vis, double* __restrict__ part,
                                                                int H, int W, int tiles_x, swf_metrics_desc d) {
    __shared__ int sL[3][kLP * kLP];
    __shared__ double red[3][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kLT, tx0 = (blockIdx.x % tiles_x) * kLT;
    load_level_tile<false>(sL, fusion, ir, vis, (int64_t)b * H * W, ty0, tx0, H, W);   // zero border
    double num = 0.0, den = 0.0, ag = 0.0;
    walk_level_tile(ty0, tx0, H, W, [&](int o, int hh, int w) {
        int sx, sy;
        sobel3x3(&sL[0][o], kLP, sx, sy);
        const int nF = sx * sx + sy * sy;
        const double gF = sqrt((double)nF), aF = edge_angle(sx, sy);
        sobel3x3(&sL[1][o], kLP, sx, sy);
        const int nA = sx * sx + sy * sy;
        const double gA = sqrt((double)nA), aA = edge_angle(sx, sy);
        sobel3x3(&sL[2][o], kLP, sx, sy);
        const int nB = sx * sx + sy * sy;
        const double gB = sqrt((double)nB), aB = edge_angle(sx, sy);
        num += qabf_term(d, nF, gF, aF, nA, gA, aA) + qabf_term(d, nF, gF, aF, nB, gB, aB);
        den += gA + gB;
        if (hh < H - 1 && w < W - 1) {
            const int c = sL[0][o + kLP + 1], gx = sL[0][o + kLP + 2] - c, gy = sL[0][o + 2 * kLP + 1] - c;
            ag += sqrt((double)(gx * gx + gy * gy) / 2.0);
        }
    });
    red[0][tid] = num;
    red[1][tid] = den;
    red[2][tid] = ag;
    SWF_TILE_TREE(3, red);
    if (tid < 3) part[((int64_t)b * gridDim.x + blockIdx.x) * 3 + tid] = red[tid][0];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Finish: one workgroup per image
// ------------------------------------------------------------------------------------------------------------------------------
// Sum of v over the workgroup in a fixed order (tree over LDS), returned to every thread.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kFinThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

// Pearson's coefficient from a covariance and two variances; 0 when either variance is 0.
__device__ __forceinline__ double pearson(double cov, double va, double vb) { return (va == 0.0 || vb == 0.0) ? 0.0 : cov / sqrt(va * vb); }

__global__ __launch_bounds__(kFinThreads) void metrics_finish_kernel(const uint32_t* __restrict__ hist, const u64* __restrict__ sums,
                                                                     const double* __restrict__ part, double* __restrict__ out,
                                                                     int H, int W, int ntiles) {
    __shared__ uint32_t hF[256], hA[256], hB[256];
    __shared__ double redd[kFinThreads];
    __shared__ u64 redu[kFinThreads];
    const int tid = threadIdx.x, b = blockIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t* JA = hist + (int64_t)b * 2 * kCells;
    const uint32_t* JB = JA + kCells;
    const double N = (double)H * (double)W;
    if (tid < 256) hA[tid] = hB[tid] = 0;
    __syncthreads();
    // marginals: rows of either joint histogram give fusion's counts, columns the source's
    uint32_t colA[4] = {0, 0, 0, 0}, colB[4] = {0, 0, 0, 0};
    for (int f = wave; f < 256; f += kFinThreads / 64) {
        uint32_t row = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t ca = JA[f * 256 + lane + 64 * j], cb = JB[f * 256 + lane + 64 * j];
            colA[j] += ca;
            colB[j] += cb;
            row += ca;
        }
        row = wave_sum(row);
        if (lane == 0) hF[f] = row;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        atomicAdd(&hA[lane + 64 * j], colA[j]);
        atomicAdd(&hB[lane + 64 * j], colB[j]);
    }
    __syncthreads();
    const bool bin = tid < 256;
    const double k = (double)tid;
    const uint32_t cF = bin ? hF[tid] : 0, cA = bin ? hA[tid] : 0, cB = bin ? hB[tid] : 0;
    const u64 SF = block_sum<u64>((u64)tid * cF, redu), SA = block_sum<u64>((u64)tid * cA, redu), SB = block_sum<u64>((u64)tid * cB, redu);
    const double mF = (double)SF / N, mA = (double)SA / N, mB = (double)SB / N;
    const double pF = (double)cF / N;
    const double en = 0.0 - block_sum<double>(cF ? pF * log2(pF) : 0.0, redd);
    const double varF = block_sum<double>((double)cF * (k - mF) * (k - mF), redd) / N;
    const double varA = block_sum<double>((double)cA * (k - mA) * (k - mA), redd) / N;
    const double varB = block_sum<double>((double)cB * (k - mB) * (k - mB), redd) / N;
    // cells of the two joint histograms: MI, cov(F, X), sum (F - X)^2, var(F - X)
    const double mDA = (double)((long long)SF - (long long)SA) / N, mDB = (double)((long long)SF - (long long)SB) / N;
    double miA = 0.0, miB = 0.0, cvA = 0.0, cvB = 0.0, vdA = 0.0, vdB = 0.0;
    u64 seA = 0, seB = 0;
    for (int i = tid; i < kCells; i += kFinThreads) {
        const int f = i >> 8, x = i & 255, dd = f - x;
        const double pf = (double)hF[f] / N, df = (double)f - mF;
        const uint32_t ca = JA[i], cb = JB[i];
        if (ca) {
            const double c = (double)ca, p = c / N;
            miA += p * log2(p / (pf * ((double)hA[x] / N)));
            cvA += c * df * ((double)x - mA);
            vdA += c * ((double)dd - mDA) * ((double)dd - mDA);
            seA += (u64)ca * (u64)(dd * dd);
        }
        if (cb) {
            const double c = (double)cb, p = c / N;
            miB += p * log2(p / (pf * ((double)hB[x] / N)));
            cvB += c * df * ((double)x - mB);
            vdB += c * ((double)dd - mDB) * ((double)dd - mDB);
            seB += (u64)cb * (u64)(dd * dd);
        }
    }
    miA = block_sum<double>(miA, redd);
    miB = block_sum<double>(miB, redd);
    const double covFA = block_sum<double>(cvA, redd) / N, covFB = block_sum<double>(cvB, redd) / N;
    const double varDA = block_sum<double>(vdA, redd) / N, varDB = block_sum<double>(vdB, redd) / N;   // var(F - A), var(F - B)
    seA = block_sum<u64>(seA, redu);
    seB = block_sum<u64>(seB, redu);
    // tile partials of the gradient pass
    double num = 0.0, den = 0.0, ag = 0.0;
    const double* pp = part + (int64_t)b * ntiles * 3;
    for (int t = tid; t < ntiles; t += kFinThreads) {
        num += pp[(int64_t)t * 3];
        den += pp[(int64_t)t * 3 + 1];
        ag += pp[(int64_t)t * 3 + 2];
    }
    num = block_sum<double>(num, redd);
    den = block_sum<double>(den, redd);
    ag = block_sum<double>(ag, redd);
    if (tid == 0) {
        const u64* sm = sums + (int64_t)b * kSumsPerImage;
        const double covAB = (double)sm[0] / N - mA * mB;
        const double rf2 = W > 1 ? (double)sm[1] / ((double)H * (double)(W - 1)) : 0.0;
        const double cf2 = H > 1 ? (double)sm[2] / ((double)(H - 1) * (double)W) : 0.0;
        const double mse = ((double)seA / N + (double)seB / N) / 2.0;
        double* o = out + (int64_t)b * SWF_METRIC_COUNT;
        o[SWF_METRIC_EN] = en;
        o[SWF_METRIC_MI] = miA + miB;
        o[SWF_METRIC_SD] = sqrt(varF);
        o[SWF_METRIC_SF] = sqrt(rf2 + cf2);
        o[SWF_METRIC_AG] = (H > 1 && W > 1) ? ag / ((double)(H - 1) * (double)(W - 1)) : 0.0;
        o[SWF_METRIC_CC] = (pearson(covFA, varA, varF) + pearson(covFB, varB, varF)) / 2.0;
        o[SWF_METRIC_SCD] = pearson(covFA - covAB, varDB, varA) + pearson(covFB - covAB, varDA, varB);
        o[SWF_METRIC_MSE] = mse;
        o[SWF_METRIC_PSNR] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(255.0 * 255.0 / mse);
        o[SWF_METRIC_QABF] = den == 0.0 ? 0.0 : num / den;
    }
}

struct MetricsBufs {
    uint32_t* hist;   // [B][2][kCells], followed by
    u64* sums;        // [B][kSumsPerImage]: zeroed together
    size_t zero_bytes;
    double* part;     // [B][tiles][3]
    int tiles_x, ntiles;
};
MetricsBufs carve_metrics(Carver& ws, int B, int H, int W) {
    MetricsBufs m{};
    m.tiles_x = cdiv(W, kLT);
    m.ntiles = m.tiles_x * cdiv(H, kLT);
    const int64_t words = (int64_t)B * (2 * kCells + kSumsPerImage * 2);
    float* z = ws.floats(words);
    m.hist = reinterpret_cast<uint32_t*>(z);
    m.sums = z ? reinterpret_cast<u64*>(z + (int64_t)B * 2 * kCells) : nullptr;
    m.zero_bytes = (size_t)words * sizeof(float);
    m.part = reinterpret_cast<double*>(ws.floats((int64_t)B * m.ntiles * 3 * 2));
    return m;
}

// Tools only (SWF_DEBUG_SWITCHES=1), read at every call so that tools/metrics_bench.py can time both in one process:
// SWF_METRICS_HIST=global sends the histogram atomics straight to global memory.
bool hist_private() {
    const char* e = debug_env("SWF_METRICS_HIST");
    return !(e && e[0] == 'g');
}

}  // namespace

size_t fusion_metrics_workspace_bytes(int B, int H, int W) {
    Carver ws = Carver::measure();
    carve_metrics(ws, B, H, W);
    return ws.bytes();
}

int fusion_metrics(const swf_metrics_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H, int W,
                   void* workspace, size_t workspace_bytes, hipStream_t stream) {
    Carver ws(workspace, workspace_bytes);
    const MetricsBufs m = carve_metrics(ws, B, H, W);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "fusion_metrics: workspace of %zu bytes, %zu needed", workspace_bytes, ws.bytes());
    const int stages = stage_mask("SWF_METRICS_STAGES");   // 1 zeroing, 2 histograms, 4 gradients, 8 finish
    if (stages & 1) {
        const int64_t n16 = (int64_t)(m.zero_bytes / 16);   // B * (2 * kCells + 8) words: a multiple of 16 bytes
        metrics_zero_kernel<<<(unsigned)std::min<int64_t>(cdiv64(n16, 256), 2048), 256, 0, stream>>>(reinterpret_cast<uint4*>(m.hist), n16);
        SWF_TRY(check_launch("metrics_zero_kernel"));
    }
    if (stages & 2) {
        const dim3 grid((unsigned)cdiv64((int64_t)H * W, kHistTile), 2, B);
        if (hist_private()) {
            SWF_TRY((raise_lds_limit<metrics_hist_kernel<true>>(kHistLdsBytes, "metrics_hist_kernel")));
            metrics_hist_kernel<true><<<grid, kHistThreads, kHistLdsBytes, stream>>>(fusion, ir, vis, m.hist, m.sums, H, W);
        } else {
            metrics_hist_kernel<false><<<grid, kHistThreads, 0, stream>>>(fusion, ir, vis, m.hist, m.sums, H, W);
        }
        SWF_TRY(check_launch("metrics_hist_kernel"));
    }
    if (stages & 4) {
        metrics_grad_kernel<<<dim3(m.ntiles, B), kThreads, 0, stream>>>(fusion, ir, vis, m.part, H, W, m.tiles_x, d);
        SWF_TRY(check_launch("metrics_grad_kernel"));
    }
    if (stages & 8) {
        metrics_finish_kernel<<<B, kFinThreads, 0, stream>>>(m.hist, m.sums, m.part, out, H, W, m.ntiles);
        SWF_TRY(check_launch("metrics_finish_kernel"));
    }
    return SWF_OK;
}

}  // namespace swf
