// Q_MI, Q_TE, Q_NCIE, Q_M, Q_SF and Q_P of fused images against their infrared and visible sources: the six values of
// swf_fusion_comparative (include/swinfuse.h has the definitions), the half of Liu et al.'s twelve that the other calls lack.  They are
// restated from memory of the published definitions; no paper and no evaluator is available to this build, so PARITY WITH ANY OF THEM
// IS UNPINNED.  tests/comparative_restatement.py is the same text in numpy and is what these kernels are checked against.
//
// Every value is a function of 8-bit levels (levels.h), fp64 after the quantiser.  Counts are integers (u32, integer atomics: exact, so
// their order is immaterial); every floating-point sum has a fixed order (LDS trees, per-tile partials); no floating-point atomics.
// The histograms are zeroed by a kernel of this call; every other workspace element that is read has been written by the same call.
//
// Q_P's EO_so = IDFT2(DFT2(X) G_s spread_o) is complex because spread_o is one-sided.  With K = G_s spread_o, K_e and K_o its even and
// odd parts under (u, v) -> (-u, -v) on the index grid, DFT2(X) K_e is Hermitian and inverts to the real E, DFT2(X) K_o is
// anti-Hermitian and inverts to i O, so O is the real inverse of -i DFT2(X) K_o: two real inverse transforms over the half spectrum
// (steps 3 and 4 of dft_frag.h) per filter, the filter (with c_v / (H W) folded in) applied as step 3 loads the spectrum.
//
// Kernels, all on one stream (A, B, F = levels of ir, vis, fusion; three planes per image):
//   cmp_tables_kernel      the four twiddle matrices and the 24 x 2 filter tables; shared by the whole batch
//   cmp_levels_kernel      the three level planes as doubles
//   cmp_zero_kernel, cmp_hist_kernel   the joint histograms of (A, F), (F, B), (B, A) (rows, columns): packed 16-bit counters in LDS
//                          per tile of 8192 pixels, non-zero words added to the image's u32 cells, as kernels_metrics.hip does
//   cmp_cells_kernel       32 workgroups per image: marginals as column sums, then the MI, Tsallis and joint-entropy sums over 2048 cells
//                          of each pair; nine sums per workgroup
//   cmp_info_kernel        one workgroup per image: the marginal entropies, those sums added in a fixed order, the 3 x 3 Jacobi
//                          sweeps; writes Q_MI, Q_TE, Q_NCIE
//   cmp_sfm_kernel         32x32 level tiles with a 1-pixel halo: the eight difference sums of Q_SF and both Haar scales of Q_M (a tile
//                          holds whole 4x4 blocks); twelve sums per tile
//   dft_gemm_kernel        steps 1 and 2 once over the 3 B planes, then per orientation steps 3 (filtered load) and 4 over 3 B x 8
//                          planes: E and O of the four scales
//   cmp_median_kernel      one workgroup per image plane: radix select (8 bits a pass, both middle ranks at once) of An at s = 1
//   cmp_pc_kernel          per pixel: PC_o from the eight planes, added to the four accumulator planes (p, sum (PC cos)^2,
//                          sum (PC sin)^2, sum PC^2 cos sin); the first orientation stores
//   cmp_moment1_kernel     p, M, m of A, B, F and the three pointwise maxima: twelve sums per 1024 pixels
//   cmp_moment2_kernel     the 21 centred second moments against those means
//   cmp_finish_kernel      one workgroup per image adds the per-tile sums in a fixed order; writes Q_M, Q_SF, Q_P.
#include "kernels_comparative.h"
#include "kernels_perception.h"
#include "metric_frag.h"
#include "dft_frag.h"

#include <algorithm>
#include <cmath>

namespace swf {
namespace {

constexpr int kImgPlanes = 3;          // A, B, F
constexpr int kScales = 4, kOrients = 6;
constexpr int kFilt = 2 * kScales;     // planes per image plane and orientation: (E, O) of every scale
constexpr int kMaxImagesCmp = 65535 / (kImgPlanes * kFilt);
constexpr int kCells = 256 * 256;
constexpr int kHistTile = 8192, kHistThreads = 1024, kHistLdsBytes = kCells * 2;
static_assert(kHistTile <= 65535, "a packed 16-bit counter must hold a whole tile");
constexpr int kInfoChunks = 32, kInfo = 9;  // workgroups per image over the cells of the joint histograms, and their sums
static_assert(kCells % (kInfoChunks * 256) == 0, "whole strides per chunk");
constexpr int kSelThreads = 1024;
constexpr int kMomPix = 4 * kThreads;  // pixels per workgroup of the moment passes
constexpr int kSfm = 12, kM1 = 12, kM2 = 21;
constexpr double kPi = 3.14159265358979323846;

// ------------------------------------------------------------------------------------------------------------------------------
// Tables
// ------------------------------------------------------------------------------------------------------------------------------
struct PcConsts {
    double fs[kScales];     // centre frequencies 1 / (min_wavelength mult^s)
    double lsig2;           // 2 ln(sigma_onf)^2
};

// G_s spread_o at bin (u, v) of the full index grid, unscaled.
__device__ __forceinline__ double pc_filter(int u, int v, int H, int W, double fs, double lsig2, double ca, double sa) {
    if (u == 0 && v == 0) return 0.0;
    const int su = u < (H + 1) / 2 ? u : u - H, sv = v < (W + 1) / 2 ? v : v - W;
    const double fx = (double)sv / (double)W, fy = (double)su / (double)H;
    const double rho = sqrt(fx * fx + fy * fy), theta = atan2(-fy, fx);
    const double lp = 1.0 / (1.0 + pow(rho / 0.45, 30.0));
    const double l = log(rho / fs);
    const double G = exp(-(l * l) / lsig2) * lp;
    const double st = sin(theta), ct = cos(theta);
    const double ds = st * ca - ct * sa, dc = ct * ca + st * sa;
    const double dth = fmin(fabs(atan2(ds, dc)) * 3.0, kPi);
    return G * ((cos(dth) + 1.0) / 2.0);
}

// gtab[o][s][2][H][Wh]: the even and the odd part of G_s spread_o, times c_v / (H W).
__global__ __launch_bounds__(kThreads) void cmp_tables_kernel(Twiddles t, double* __restrict__ gtab, int H, int W, int Wh, PcConsts pc) {
    const int64_t nG = (int64_t)H * Wh;
    int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (fill_twiddle(t, i, H, W, Wh)) return;
    i -= twiddle_count(H, W, Wh);
    if (i >= nG * kOrients * kScales) return;
    const int os = (int)(i / nG), o = os / kScales, s = os % kScales;
    const int64_t e = i % nG;
    const int u = (int)(e / Wh), v = (int)(e % Wh);
    double sa, ca;
    sincospi((double)o / 6.0, &sa, &ca);
    const double k = pc_filter(u, v, H, W, pc.fs[s], pc.lsig2, ca, sa);
    const double kn = pc_filter((H - u) % H, (W - v) % W, H, W, pc.fs[s], pc.lsig2, ca, sa);
    const double scale = ((v == 0 || 2 * v == W) ? 1.0 : 2.0) / ((double)H * (double)W);
    double* g = gtab + (int64_t)os * 2 * nG;
    g[e] = ((k + kn) / 2.0) * scale;
    g[nG + e] = ((k - kn) / 2.0) * scale;
}

// X[B][3][n] <- the levels of ir, vis, fusion.  grid (ceil(n / 256), B).
__global__ __launch_bounds__(kThreads) void cmp_levels_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
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

// ------------------------------------------------------------------------------------------------------------------------------
// Joint histograms and the information measures
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cmp_zero_kernel(uint4* __restrict__ p, int64_t n16) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// hist[B][3][kCells]: pair 0 cell (A, F), pair 1 (F, B), pair 2 (B, A), row * 256 + column.  grid (tiles of 8192 pixels, 3, B).
__global__ __launch_bounds__(kHistThreads) void cmp_hist_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                                const float* __restrict__ vis, uint32_t* __restrict__ hist, int n) {
    extern __shared__ uint32_t cells[];   // kCells / 2 words, cell c in half (c & 1) of word c >> 1
    const int tid = threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    const int64_t img = (int64_t)b * n;
    const float* row = (s == 0 ? ir : (s == 1 ? fusion : vis)) + img;
    const float* col = (s == 0 ? fusion : (s == 1 ? vis : ir)) + img;
    uint32_t* h = hist + ((int64_t)b * 3 + s) * kCells;
    for (int i = tid; i < kCells / 2; i += kHistThreads) cells[i] = 0;
    __syncthreads();
    const int begin = blockIdx.x * kHistTile, end = min(n, begin + kHistTile);
    for (int p = begin + tid; p < end; p += kHistThreads) {
        const int c = level(row[p]) * 256 + level(col[p]);
        atomicAdd(&cells[c >> 1], 1u << ((c & 1) * 16));
    }
    __syncthreads();
    for (int i = tid; i < kCells / 2; i += kHistThreads) {
        const uint32_t v = cells[i];
        if (v & 0xffffu) atomicAdd(&h[2 * i], v & 0xffffu);
        if (v >> 16) atomicAdd(&h[2 * i + 1], v >> 16);
    }
}

// Eigenvalues of the symmetric 3 x 3 matrix with unit diagonal and off-diagonals r01, r02, r12, by cyclic Jacobi sweeps.
__device__ void jacobi3(double r01, double r02, double r12, double lam[3]) {
    double a[3][3] = {{1.0, r01, r02}, {r01, 1.0, r12}, {r02, r12, 1.0}};
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        if (off <= 1e-60) break;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            const int r = 3 - p - q;
            const double app = a[p][p], aqq = a[q][q], arp = a[r][p], arq = a[r][q];
            a[p][p] = app - t * apq;
            a[q][q] = aqq + t * apq;
            a[p][q] = a[q][p] = 0.0;
            a[r][p] = a[p][r] = c * arp - s * arq;
            a[r][q] = a[q][r] = s * arp + c * arq;
        }
    }
    lam[0] = a[0][0];
    lam[1] = a[1][1];
    lam[2] = a[2][2];
}

// The marginals of image b as column sums of its three joint histograms: pm[0..2][tid] <- p_A, p_B, p_F of level tid; the counts returned.
__device__ __forceinline__ void cmp_marginals(const uint32_t* __restrict__ J, double N, double (*pm)[256], uint32_t c[3]) {
    const int tid = threadIdx.x;
    uint32_t cF = 0, cB = 0, cA = 0;       // column sums: F of (A, F), B of (F, B), A of (B, A)
    for (int r = 0; r < 256; ++r) {
        cF += J[r * 256 + tid];
        cB += J[kCells + r * 256 + tid];
        cA += J[2 * kCells + r * 256 + tid];
    }
    c[0] = cA;
    c[1] = cB;
    c[2] = cF;
#pragma unroll
    for (int k = 0; k < 3; ++k) pm[k][tid] = (double)c[k] / N;
    __syncthreads();
}

// part[B][kInfoChunks][9]: per pair (A, F), (F, B), (B, A) the chunk's sums of p log2(p / (p_r p_c)), p^q / (p_r p_c)^(q - 1) and
// -p log2 p over its 2048 cells.  grid (kInfoChunks, B): the pow and log2 of up to 3 x 65536 cells are too much for one workgroup.
__global__ __launch_bounds__(kThreads) void cmp_cells_kernel(const uint32_t* __restrict__ hist, double N, double q, double* __restrict__ part) {
    __shared__ double pm[3][256];          // p_A, p_B, p_F
    __shared__ double red[kInfo][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const uint32_t* J = hist + (int64_t)b * 3 * kCells;
    uint32_t cnt[3];
    cmp_marginals(J, N, pm, cnt);
    constexpr int per = kCells / kInfoChunks;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double* pr = pm[k == 0 ? 0 : (k == 1 ? 2 : 1)];
        const double* pc = pm[k == 0 ? 2 : (k == 1 ? 1 : 0)];
        double mi = 0.0, ts = 0.0, hj = 0.0;
        for (int i = blockIdx.x * per + tid; i < (blockIdx.x + 1) * per; i += kThreads) {
            const uint32_t c = J[k * kCells + i];
            if (!c) continue;
            const double p = (double)c / N, pp = pr[i >> 8] * pc[i & 255];
            mi += p * log2(p / pp);
            ts += pow(p, q) / pow(pp, q - 1.0);
            hj -= p * log2(p);
        }
        red[k][tid] = mi;
        red[3 + k][tid] = ts;
        red[6 + k][tid] = hj;
    }
    SWF_TILE_TREE(kInfo, red);
    if (tid < kInfo) part[((int64_t)b * kInfoChunks + blockIdx.x) * kInfo + tid] = red[tid][0];
}

// One workgroup per image: the marginal entropies, the chunks' sums in a fixed order, the three values.
__global__ __launch_bounds__(kThreads) void cmp_info_kernel(const uint32_t* __restrict__ hist, const double* __restrict__ part, double N,
                                                            double q, double* __restrict__ out) {
    __shared__ double pm[3][256];
    __shared__ double red[kInfo][kThreads];
    const int tid = threadIdx.x, b = blockIdx.x;
    uint32_t cnt[3];
    cmp_marginals(hist + (int64_t)b * 3 * kCells, N, pm, cnt);
    const double pA = pm[0][tid], pB = pm[1][tid], pF = pm[2][tid];
    double cs[kInfo];                      // MI, Tsallis sum, joint entropy of (A, F), (F, B), (B, A)
    tile_sums<kInfo>(part + (int64_t)b * kInfoChunks * kInfo, kInfoChunks, red, cs);
    red[0][tid] = cnt[0] ? -(pA * log2(pA)) : 0.0;
    red[1][tid] = cnt[1] ? -(pB * log2(pB)) : 0.0;
    red[2][tid] = cnt[2] ? -(pF * log2(pF)) : 0.0;
    red[3][tid] = cnt[0] ? pow(pA, q) : 0.0;
    red[4][tid] = cnt[1] ? pow(pB, q) : 0.0;
    SWF_TILE_TREE(5, red);
    if (tid == 0) {
        const double HA = red[0][0], HB = red[1][0], HF = red[2][0];
        const double qmi = 2.0 * ((HA + HF == 0.0 ? 0.0 : cs[0] / (HA + HF)) + (HB + HF == 0.0 ? 0.0 : cs[1] / (HB + HF)));
        const double iAF = (1.0 - cs[3]) / (1.0 - q), iBF = (1.0 - cs[4]) / (1.0 - q), iAB = (1.0 - cs[5]) / (1.0 - q);
        const double hqA = (1.0 - red[3][0]) / (q - 1.0), hqB = (1.0 - red[4][0]) / (q - 1.0);
        const double dte = hqA + hqB - iAB;
        const double nAF = HA / 8.0 + HF / 8.0 - cs[6] / 8.0, nBF = HF / 8.0 + HB / 8.0 - cs[7] / 8.0;
        const double nAB = HB / 8.0 + HA / 8.0 - cs[8] / 8.0;
        double lam[3];
        jacobi3(nAB, nAF, nBF, lam);
        double ncie = 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double l = lam[k] / 3.0;
            if (lam[k] > 0.0) ncie += l * (log2(l) / 8.0);
        }
        double* o = out + (int64_t)b * SWF_COMPARATIVE_COUNT;
        o[SWF_COMPARATIVE_QMI] = qmi;
        o[SWF_COMPARATIVE_QTE] = dte == 0.0 ? 0.0 : (iAF + iBF) / dte;
        o[SWF_COMPARATIVE_QNCIE] = ncie;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Q_SF and Q_M: one pass over level tiles
// ------------------------------------------------------------------------------------------------------------------------------
struct Haar {
    double ll, lh, hl, hh;
};
__device__ __forceinline__ Haar haar(double a, double b, double c, double d) {
    return Haar{(a + b + c + d) / 2.0, (a + b - c - d) / 2.0, (a - b + c - d) / 2.0, (a - b - c + d) / 2.0};
}
// EP_A w_A + EP_B w_B and w_A + w_B of one coefficient position.
__device__ __forceinline__ void qm_term(const Haar& f, const Haar& a, const Haar& b, double& num, double& den) {
    const double epa = (exp(-fabs(a.lh - f.lh)) + exp(-fabs(a.hl - f.hl)) + exp(-fabs(a.hh - f.hh))) / 3.0;
    const double epb = (exp(-fabs(b.lh - f.lh)) + exp(-fabs(b.hl - f.hl)) + exp(-fabs(b.hh - f.hh))) / 3.0;
    const double wa = a.lh * a.lh + a.hl * a.hl + a.hh * a.hh, wb = b.lh * b.lh + b.hl * b.hl + b.hh * b.hh;
    num += epa * wa + epb * wb;
    den += wa + wb;
}

// part[B][ntiles][12]: sums of D_h^2, D_v^2, D_md^2, D_sd^2 of F, then of the per-pixel maxima over A, B (integers under 2^28, exact
// as doubles), then numerator and denominator of Q_M's scale 1 and of its scale 2.
__global__ __launch_bounds__(kThreads) void cmp_sfm_kernel(const float* __restrict__ fusion, const float* __restrict__ ir,
                                                           const float* __restrict__ vis, int H, int W, int tiles_x,
                                                           double* __restrict__ part, int ntiles) {
    __shared__ int sL[3][kLP * kLP];        // F, A, B
    __shared__ double sLL[3][kThreads];     // scale-1 approximations of the tile's 16 x 16 blocks
    __shared__ double red[kSfm][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kLT, tx0 = (blockIdx.x % tiles_x) * kLT;
    load_level_tile<false>(sL, fusion, ir, vis, (int64_t)b * H * W, ty0, tx0, H, W);
    int sf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    walk_level_tile(ty0, tx0, H, W, [&](int o, int hh, int w) {
        const int c = o + kLP + 1;
        const int nb[4] = {o + kLP, o + 1, o, o + 2};   // (i, j-1), (i-1, j), (i-1, j-1), (i-1, j+1)
        const bool ok[4] = {w > 0, hh > 0, hh > 0 && w > 0, hh > 0 && w < W - 1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!ok[k]) continue;
            const int df = sL[0][c] - sL[0][nb[k]], da = abs(sL[1][c] - sL[1][nb[k]]), db = abs(sL[2][c] - sL[2][nb[k]]);
            const int dr = max(da, db);
            sf[k] += df * df;
            sf[4 + k] += dr * dr;
        }
    });
#pragma unroll
    for (int k = 0; k < 8; ++k) red[k][tid] = (double)sf[k];
    // scale 1: thread t owns the 2 x 2 block (t >> 4, t & 15) of the tile
    double n1 = 0.0, d1 = 0.0, n2 = 0.0, d2 = 0.0;
    {
        const int br = tid >> 4, bc = tid & 15;
        const bool in = ty0 + 2 * br + 1 < H && tx0 + 2 * bc + 1 < W;
        const int c = (2 * br + 1) * kLP + 2 * bc + 1;
        Haar h[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            h[k] = haar((double)sL[k][c] / 255.0, (double)sL[k][c + 1] / 255.0, (double)sL[k][c + kLP] / 255.0,
                        (double)sL[k][c + kLP + 1] / 255.0);
            sLL[k][tid] = h[k].ll;
        }
        if (in) qm_term(h[0], h[1], h[2], n1, d1);
    }
    __syncthreads();
    if (tid < 64) {                          // scale 2: thread t owns the 4 x 4 pixel block (t >> 3, t & 7) of the tile
        const int br = tid >> 3, bc = tid & 7;
        const bool in = ty0 / 2 + 2 * br + 1 < H / 2 && tx0 / 2 + 2 * bc + 1 < W / 2;
        const int c = (2 * br) * 16 + 2 * bc;
        if (in) {
            Haar h[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) h[k] = haar(sLL[k][c], sLL[k][c + 1], sLL[k][c + 16], sLL[k][c + 17]);
            qm_term(h[0], h[1], h[2], n2, d2);
        }
    }
    red[8][tid] = n1;
    red[9][tid] = d1;
    red[10][tid] = n2;
    red[11][tid] = d2;
    SWF_TILE_TREE(kSfm, red);
    if (tid < kSfm) part[((int64_t)b * ntiles + blockIdx.x) * kSfm + tid] = red[tid][0];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Q_P: median, phase congruency of one orientation, moments
// ------------------------------------------------------------------------------------------------------------------------------
// Y: [3 B][8][n], planes 0 and 1 of an image plane = E and O at s = 1.  med[3 B] <- the median of sqrt(E^2 + O^2) over the n pixels:
// radix select from the top byte down over the bit patterns (non-negative doubles order as their patterns do), both middle ranks in
// the same passes; the counts are integers, so their order is immaterial.  The select runs on E^2 + O^2 and the root is taken of the
// two values it finds: the root is monotonic and correctly rounded, so those are the middle values of the roots.  grid 3 B.
__global__ __launch_bounds__(kSelThreads) void cmp_median_kernel(const double* __restrict__ Y, int64_t n, double* __restrict__ med) {
    __shared__ uint32_t hist[2][256];
    __shared__ unsigned long long prefix[2], rank[2];
    const int tid = threadIdx.x;
    const double* e = Y + (int64_t)blockIdx.x * kFilt * n;
    const double* o = e + n;
    if (tid < 2) {
        prefix[tid] = 0;
        rank[tid] = tid == 0 ? (unsigned long long)((n - 1) / 2) : (unsigned long long)(n / 2);
    }
    unsigned long long mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) hist[0][tid] = hist[1][tid] = 0;
        __syncthreads();
        const unsigned long long p0 = prefix[0], p1 = prefix[1];
        const bool shared = p0 == p1;        // both ranks still in one bucket: one histogram serves both
        int last[2] = {0, 0};                // a run of equal digits is one atomic: the top bytes are the same for most of the plane
        uint32_t run[2] = {0, 0};
        for (int64_t i = tid; i < n; i += kSelThreads) {
            const double ev = e[i], ov = o[i];
            const unsigned long long bits = (unsigned long long)__double_as_longlong(ev * ev + ov * ov);
            const int d = (int)((bits >> shift) & 255);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if ((bits & mask) != (k == 0 ? p0 : p1) || (k == 1 && shared)) continue;
                if (run[k] && d != last[k]) {
                    atomicAdd(&hist[k][last[k]], run[k]);
                    run[k] = 0;
                }
                last[k] = d;
                ++run[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (run[k]) atomicAdd(&hist[k][last[k]], run[k]);
        __syncthreads();
        if (tid < 2) {
            const uint32_t* hh = hist[shared ? 0 : tid];
            unsigned long long k = rank[tid], cum = 0;
            int d = 0;
            for (; d < 255; ++d) {
                if (cum + hh[d] > k) break;
                cum += hh[d];
            }
            rank[tid] = k - cum;
            prefix[tid] |= (unsigned long long)d << shift;
        }
        mask |= 0xffull << shift;
        __syncthreads();
    }
    if (tid == 0)
        med[blockIdx.x] = (sqrt(__longlong_as_double((long long)prefix[0])) + sqrt(__longlong_as_double((long long)prefix[1]))) / 2.0;
}

struct PcParams {
    double ca, sa;          // cos, sin of the orientation's angle
    double noise;           // T / tau: (1 - (1 / mult)^4) / (1 - 1 / mult) (sqrt(pi / 2) + k sqrt((4 - pi) / 2)) / sqrt(ln 4)
    double eps, cutoff, g;
    int first;              // the first orientation stores, the others add
};

// acc[3 B][4][n] (+)= PC_o, (PC_o cos a)^2, (PC_o sin a)^2, PC_o^2 cos a sin a.  grid (ceil(n / 256), 3 B).
__global__ __launch_bounds__(kThreads) void cmp_pc_kernel(const double* __restrict__ Y, const double* __restrict__ med, int64_t n,
                                                          PcParams P, double* __restrict__ acc) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int ip = blockIdx.y;
    const double* y = Y + (int64_t)ip * kFilt * n + i;
    double E[kScales], O[kScales], sumE = 0.0, sumO = 0.0, sumAn = 0.0, maxAn = 0.0;
#pragma unroll
    for (int s = 0; s < kScales; ++s) {
        E[s] = y[(int64_t)(2 * s) * n];
        O[s] = y[(int64_t)(2 * s + 1) * n];
        const double an = sqrt(E[s] * E[s] + O[s] * O[s]);
        sumE += E[s];
        sumO += O[s];
        sumAn += an;
        maxAn = s == 0 ? an : fmax(maxAn, an);
    }
    const double XE = sqrt(sumE * sumE + sumO * sumO) + P.eps, mE = sumE / XE, mO = sumO / XE;
    double energy = 0.0;
#pragma unroll
    for (int s = 0; s < kScales; ++s) energy += E[s] * mE + O[s] * mO - fabs(E[s] * mO - O[s] * mE);
    energy = fmax(energy - med[ip] * P.noise, 0.0);
    const double width = (sumAn / (maxAn + P.eps) - 1.0) / 3.0;
    const double weight = 1.0 / (1.0 + exp((P.cutoff - width) * P.g));
    const double pc = weight * energy / (sumAn + P.eps);
    const double v[4] = {pc, (pc * P.ca) * (pc * P.ca), (pc * P.sa) * (pc * P.sa), pc * pc * P.ca * P.sa};
    double* a = acc + (int64_t)ip * 4 * n + i;
#pragma unroll
    for (int k = 0; k < 4; ++k) a[(int64_t)k * n] = P.first ? v[k] : a[(int64_t)k * n] + v[k];
}

// p, M, m at pixel i of image plane a (= acc + ip 4 n).
__device__ __forceinline__ void pc_maps(const double* a, int64_t n, int64_t i, double eps, double m[3]) {
    const double cx2 = a[n + i] / 3.0, cy2 = a[2 * n + i] / 3.0, cxy = a[3 * n + i] / 3.0;
    const double den = sqrt(cxy * cxy + (cx2 - cy2) * (cx2 - cy2)) + eps;
    m[0] = a[i];
    m[1] = (cy2 + cx2 + den) / 2.0;
    m[2] = (cy2 + cx2 - den) / 2.0;
}

// The twelve maps of a pixel: per kind k of p, M, m: v[4 k ..] = X_A, X_B, X_F, max(X_A, X_B).
__device__ __forceinline__ void pc_twelve(const double* acc_img, int64_t n, int64_t i, double eps, double v[kM1]) {
    double a[3], b[3], f[3];
    pc_maps(acc_img, n, i, eps, a);
    pc_maps(acc_img + 4 * n, n, i, eps, b);
    pc_maps(acc_img + 8 * n, n, i, eps, f);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[4 * k] = a[k];
        v[4 * k + 1] = b[k];
        v[4 * k + 2] = f[k];
        v[4 * k + 3] = fmax(a[k], b[k]);
    }
}

// part1[B][tiles][12]: the sums of the twelve maps over the tile's 1024 pixels.  grid (tiles, B).
__global__ __launch_bounds__(kThreads) void cmp_moment1_kernel(const double* __restrict__ acc, int64_t n, double eps,
                                                               double* __restrict__ part1, int tiles) {
    __shared__ double red[kM1][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const double* a = acc + (int64_t)b * kImgPlanes * 4 * n;
    double s[kM1] = {};
    for (int j = 0; j < kMomPix / kThreads; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kMomPix + j * kThreads + tid;
        if (i >= n) break;
        double v[kM1];
        pc_twelve(a, n, i, eps, v);
#pragma unroll
        for (int k = 0; k < kM1; ++k) s[k] += v[k];
    }
#pragma unroll
    for (int k = 0; k < kM1; ++k) red[k][tid] = s[k];
    SWF_TILE_TREE(kM1, red);
    if (tid < kM1) part1[((int64_t)b * tiles + blockIdx.x) * kM1 + tid] = red[tid][0];
}

// part2[B][tiles][21]: per kind the centred sums dA^2, dB^2, dF^2, dS^2, dA dF, dB dF, dS dF; every workgroup adds part1 in the same
// fixed order for the means.  grid (tiles, B).
__global__ __launch_bounds__(kThreads) void cmp_moment2_kernel(const double* __restrict__ acc, int64_t n, double eps,
                                                               const double* __restrict__ part1, double* __restrict__ part2, int tiles) {
    __shared__ double red[kM2][kThreads];
    const int tid = threadIdx.x, b = blockIdx.y;
    const double* a = acc + (int64_t)b * kImgPlanes * 4 * n;
    double mean[kM1];
    tile_sums<kM1>(part1 + (int64_t)b * tiles * kM1, tiles, red, mean);
#pragma unroll
    for (int k = 0; k < kM1; ++k) mean[k] /= (double)n;
    double s[kM2] = {};
    for (int j = 0; j < kMomPix / kThreads; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kMomPix + j * kThreads + tid;
        if (i >= n) break;
        double v[kM1];
        pc_twelve(a, n, i, eps, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double da = v[4 * k] - mean[4 * k], db = v[4 * k + 1] - mean[4 * k + 1], df = v[4 * k + 2] - mean[4 * k + 2],
                         ds = v[4 * k + 3] - mean[4 * k + 3];
            s[7 * k] += da * da;
            s[7 * k + 1] += db * db;
            s[7 * k + 2] += df * df;
            s[7 * k + 3] += ds * ds;
            s[7 * k + 4] += da * df;
            s[7 * k + 5] += db * df;
            s[7 * k + 6] += ds * df;
        }
    }
#pragma unroll
    for (int k = 0; k < kM2; ++k) red[k][tid] = s[k];
    SWF_TILE_TREE(kM2, red);
    if (tid < kM2) part2[((int64_t)b * tiles + blockIdx.x) * kM2 + tid] = red[tid][0];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Finish: one workgroup per image
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cmp_finish_kernel(const double* __restrict__ sfm_part, int sfm_tiles,
                                                              const double* __restrict__ part2, int mom_tiles, int H, int W,
                                                              swf_comparative_desc d, double* __restrict__ out) {
    __shared__ double red[kM2][kThreads];
    const int b = blockIdx.x;
    double sf[kSfm], mo[kM2];
    tile_sums<kSfm>(sfm_part + (int64_t)b * sfm_tiles * kSfm, sfm_tiles, red, sf);
    tile_sums<kM2>(part2 + (int64_t)b * mom_tiles * kM2, mom_tiles, red, mo);
    if (threadIdx.x == 0) {
        const double N = (double)H * (double)W, wd = 1.0 / sqrt(2.0);
        const double sff = sqrt((sf[0] + sf[1] + wd * sf[2] + wd * sf[3]) / N), sfr = sqrt((sf[4] + sf[5] + wd * sf[6] + wd * sf[7]) / N);
        const double q1 = (H < 2 || W < 2) ? 1.0 : (sf[9] == 0.0 ? 0.0 : sf[8] / sf[9]);
        const double q2 = (H < 4 || W < 4) ? 1.0 : (sf[11] == 0.0 ? 0.0 : sf[10] / sf[11]);
        const double ex[3] = {d.ep, d.eM, d.em};
        double qp = 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double* s = mo + 7 * k;
            const double sa = sqrt(s[0] / N), sb = sqrt(s[1] / N), sF = sqrt(s[2] / N), ss = sqrt(s[3] / N);
            const double ca = (s[4] / N + d.C) / (sa * sF + d.C), cb = (s[5] / N + d.C) / (sb * sF + d.C), cs = (s[6] / N + d.C) / (ss * sF + d.C);
            qp *= pow(fmax(fmax(fmax(ca, cb), cs), 0.0), ex[k]);
        }
        double* o = out + (int64_t)b * SWF_COMPARATIVE_COUNT;
        o[SWF_COMPARATIVE_QM] = pow(q1, d.alpha1) * pow(q2, d.alpha2);
        o[SWF_COMPARATIVE_QSF] = sfr == 0.0 ? 0.0 : (sff - sfr) / sfr;
        o[SWF_COMPARATIVE_QP] = qp;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------------------------------------------
struct ComparativePlan {
    int Wh;
    int sfm_tiles_x, sfm_tiles;    // the 32x32 level tiles
    int mom_tiles;                 // the 1024-pixel runs of the moment passes
    int64_t n, plane;              // doubles per image plane: H W, and 2 H Wh (>= H W) of the transform buffers
    Twiddles t;
    double* gtab;                  // [6][4][2][H][Wh]
    double *X, *Z, *T, *Y, *acc, *med;
    double *info_part, *sfm_part, *part1, *part2;
    uint32_t* hist;
    size_t hist_bytes;
};

ComparativePlan carve_comparative(Carver& ws, int B, int H, int W) {
    ComparativePlan f{};
    f.Wh = W / 2 + 1;
    f.sfm_tiles_x = cdiv(W, kLT);
    f.sfm_tiles = f.sfm_tiles_x * cdiv(H, kLT);
    f.n = (int64_t)H * W;
    f.mom_tiles = (int)cdiv64(f.n, kMomPix);
    f.plane = (int64_t)2 * H * f.Wh;
    f.t.a2 = carve_doubles(ws, (int64_t)4 * H * H);
    f.t.a3 = carve_doubles(ws, (int64_t)4 * H * H);
    f.t.bw1 = carve_doubles(ws, (int64_t)2 * W * f.Wh);
    f.t.bw4 = carve_doubles(ws, (int64_t)2 * W * f.Wh);
    f.gtab = carve_doubles(ws, (int64_t)kOrients * kFilt * H * f.Wh);
    f.X = carve_doubles(ws, (int64_t)B * kImgPlanes * f.n);
    f.Z = carve_doubles(ws, (int64_t)B * kImgPlanes * f.plane);
    f.T = carve_doubles(ws, (int64_t)B * kImgPlanes * kFilt * f.plane);
    f.Y = carve_doubles(ws, (int64_t)B * kImgPlanes * kFilt * f.n);
    f.acc = carve_doubles(ws, (int64_t)B * kImgPlanes * 4 * f.n);
    f.med = carve_doubles(ws, (int64_t)B * kImgPlanes);
    f.info_part = carve_doubles(ws, (int64_t)B * kInfoChunks * kInfo);
    f.sfm_part = carve_doubles(ws, (int64_t)B * f.sfm_tiles * kSfm);
    f.part1 = carve_doubles(ws, (int64_t)B * f.mom_tiles * kM1);
    f.part2 = carve_doubles(ws, (int64_t)B * f.mom_tiles * kM2);
    f.hist = reinterpret_cast<uint32_t*>(ws.floats((int64_t)B * 3 * kCells));
    f.hist_bytes = (size_t)B * 3 * kCells * sizeof(uint32_t);
    return f;
}

}  // namespace

bool comparative_shape_ok(int B, int H, int W) { return perception_shape_ok(B, H, W) && B <= kMaxImagesCmp; }

size_t fusion_comparative_workspace_bytes(int B, int H, int W) {
    Carver ws = Carver::measure();
    carve_comparative(ws, B, H, W);
    return ws.bytes();
}

int fusion_comparative(const swf_comparative_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H,
                       int W, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    Carver ws(workspace, workspace_bytes);
    const ComparativePlan f = carve_comparative(ws, B, H, W);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "fusion_comparative: workspace of %zu bytes, %zu needed", workspace_bytes, ws.bytes());
    // 1 tables, levels, histograms and their measures, the Q_SF / Q_M pass; 2 the transforms; 4 medians and phase congruency; 8 moments, finish
    const int stages = stage_mask("SWF_COMPARATIVE_STAGES");
    const int Wh = f.Wh, planes = B * kImgPlanes;
    if (stages & 1) {
        PcConsts pc{};
        for (int s = 0; s < kScales; ++s) pc.fs[s] = 1.0 / (d.min_wavelength * std::pow(d.mult, (double)s));
        pc.lsig2 = 2.0 * std::log(d.sigma_onf) * std::log(d.sigma_onf);
        const int64_t total = twiddle_count(H, W, Wh) + (int64_t)kOrients * kScales * H * Wh;
        cmp_tables_kernel<<<(unsigned)cdiv64(total, kThreads), kThreads, 0, stream>>>(f.t, f.gtab, H, W, Wh, pc);
        SWF_TRY(check_launch("cmp_tables_kernel"));
        cmp_levels_kernel<<<dim3((unsigned)cdiv64(f.n, kThreads), B), kThreads, 0, stream>>>(fusion, ir, vis, f.n, f.X);
        SWF_TRY(check_launch("cmp_levels_kernel"));
        const int64_t n16 = (int64_t)(f.hist_bytes / 16);
        cmp_zero_kernel<<<(unsigned)std::min<int64_t>(cdiv64(n16, 256), 2048), 256, 0, stream>>>(reinterpret_cast<uint4*>(f.hist), n16);
        SWF_TRY(check_launch("cmp_zero_kernel"));
        SWF_TRY((raise_lds_limit<cmp_hist_kernel>(kHistLdsBytes, "cmp_hist_kernel")));
        cmp_hist_kernel<<<dim3((unsigned)cdiv64(f.n, kHistTile), 3, B), kHistThreads, kHistLdsBytes, stream>>>(fusion, ir, vis, f.hist, (int)f.n);
        SWF_TRY(check_launch("cmp_hist_kernel"));
        cmp_cells_kernel<<<dim3(kInfoChunks, B), kThreads, 0, stream>>>(f.hist, (double)f.n, d.q, f.info_part);
        SWF_TRY(check_launch("cmp_cells_kernel"));
        cmp_info_kernel<<<B, kThreads, 0, stream>>>(f.hist, f.info_part, (double)f.n, d.q, out);
        SWF_TRY(check_launch("cmp_info_kernel"));
        cmp_sfm_kernel<<<dim3(f.sfm_tiles, B), kThreads, 0, stream>>>(fusion, ir, vis, H, W, f.sfm_tiles_x, f.sfm_part, f.sfm_tiles);
        SWF_TRY(check_launch("cmp_sfm_kernel"));
    }
    if (stages & 2) {
        Gemm g{};
        g = Gemm{f.X, f.t.bw1, f.T, f.n, 0, f.plane, W, 2 * Wh, H, 2 * Wh, W, Wh, nullptr, 1, 1, 1};
        SWF_TRY(launch_gemm<kStoreFoldCols>(g, planes, stream));
        g = Gemm{f.t.a2, f.T, f.Z, 0, f.plane, f.plane, 2 * H, Wh, 2 * H, Wh, 2 * H, H, nullptr, 1, 1, 1};
        SWF_TRY(launch_gemm<kStorePlain>(g, planes, stream));
    }
    const double im = 1.0 / d.mult;
    const double noise = (1.0 - im * im * im * im) / (1.0 - im) * (std::sqrt(M_PI / 2.0) + d.k * std::sqrt((4.0 - M_PI) / 2.0)) /
                         std::sqrt(std::log(4.0));
    for (int o = 0; o < kOrients; ++o) {
        if (stages & 2) {
            Gemm g{};
            g = Gemm{f.t.a3, f.Z, f.T, 0, f.plane, f.plane, 2 * H, Wh, 2 * H, Wh, 2 * H, H, f.gtab + (int64_t)o * kFilt * H * Wh, 1, 1, kFilt};
            SWF_TRY((launch_gemm<kStoreFoldRows, kLoadFilter>(g, planes * kFilt, stream)));
            g = Gemm{f.T, f.t.bw4, f.Y, f.plane, 0, f.n, 2 * Wh, W, H, W, 2 * Wh, 0, nullptr, 1, 1, 1};
            SWF_TRY(launch_gemm<kStorePlain>(g, planes * kFilt, stream));
        }
        if (stages & 4) {
            cmp_median_kernel<<<planes, kSelThreads, 0, stream>>>(f.Y, f.n, f.med);
            SWF_TRY(check_launch("cmp_median_kernel"));
            const PcParams P{std::cos(o * M_PI / 6.0), std::sin(o * M_PI / 6.0), noise, d.eps, d.cutoff, d.g, o == 0};
            cmp_pc_kernel<<<dim3((unsigned)cdiv64(f.n, kThreads), planes), kThreads, 0, stream>>>(f.Y, f.med, f.n, P, f.acc);
            SWF_TRY(check_launch("cmp_pc_kernel"));
        }
    }
    if (stages & 8) {
        cmp_moment1_kernel<<<dim3(f.mom_tiles, B), kThreads, 0, stream>>>(f.acc, f.n, d.eps, f.part1, f.mom_tiles);
        SWF_TRY(check_launch("cmp_moment1_kernel"));
        cmp_moment2_kernel<<<dim3(f.mom_tiles, B), kThreads, 0, stream>>>(f.acc, f.n, d.eps, f.part1, f.part2, f.mom_tiles);
        SWF_TRY(check_launch("cmp_moment2_kernel"));
        cmp_finish_kernel<<<B, kThreads, 0, stream>>>(f.sfm_part, f.sfm_tiles, f.part2, f.mom_tiles, H, W, d, out);
        SWF_TRY(check_launch("cmp_finish_kernel"));
    }
    return SWF_OK;
}

}  // namespace swf
