// The dense fp64 DFT on the matrix cores that the evaluation kernels with whole-image transforms share (kernels_perception.hip,
// kernels_comparative.hip), defined here and nowhere else: the twiddle matrices, the one GEMM kernel with its stores and its filtered
// operand load, and its launch.  Include after metric_frag.h (kThreads).
//
// For a real image X the half spectrum v = 0 .. Wh - 1, Wh = floor(W / 2) + 1, is enough; with C, S = cos, sin(2 pi ((j k) mod n) / n):
//   1  [Tr | Ti] = X [C_W | -S_W]                    H x W   by W x 2Wh     stored as [Tr; Ti]
//   2  [Zr; Zi]  = [C_H S_H; -S_H C_H] [Tr; Ti]      2H x 2H by 2H x Wh     DFT2(X) on the half spectrum
//   3  [Ur; Ui]  = [C_H -S_H; S_H C_H] [Zr; Zi]      2H x 2H by 2H x Wh     stored as [Ur | Ui]
//   4  Y         = [Ur | Ui] [C_W; -S_W]             H x 2Wh by 2Wh x W     Re of the sum over the half spectrum
// Y = Re(IDFT2(Z)) when Z has been scaled by c_v / (H W), c_v = 1 for v = 0 and the Nyquist column, else 2: the other half of the
// spectrum is the conjugate of this one.
#pragma once
#include "swf_common.h"

namespace swf {
namespace {

struct Twiddles {
    double *a2, *a3;    // [2H][2H]: [C S; -S C] and [C -S; S C]
    double *bw1;        // [W][2Wh]: [C | -S]
    double *bw4;        // [2Wh][W]: [C; -S]
};

__host__ __device__ inline int64_t twiddle_count(int H, int W, int Wh) { return (int64_t)4 * H * H + (int64_t)W * Wh; }

// Element i < twiddle_count of the tables, arguments reduced in integers before sincospi.  Returns false for i beyond them.
__device__ __forceinline__ bool fill_twiddle(const Twiddles& t, int64_t i, int H, int W, int Wh) {
    const int64_t nH = (int64_t)4 * H * H, nW = (int64_t)W * Wh;
    if (i < nH) {
        const int r = (int)(i / (2 * H)), c = (int)(i % (2 * H));
        const int64_t m = ((int64_t)(r % H) * (c % H)) % H;
        double sn, cs;
        sincospi(2.0 * (double)m / (double)H, &sn, &cs);
        const bool lower = r >= H, right = c >= H;
        const double v2 = lower == right ? cs : (right ? sn : -sn);
        t.a2[i] = v2;
        t.a3[i] = lower == right ? cs : -v2;
        return true;
    }
    i -= nH;
    if (i < nW) {
        const int k = (int)(i / Wh), v = (int)(i % Wh);
        const int64_t m = ((int64_t)k * v) % W;
        double sn, cs;
        sincospi(2.0 * (double)m / (double)W, &sn, &cs);
        t.bw1[(int64_t)k * 2 * Wh + v] = cs;
        t.bw1[(int64_t)k * 2 * Wh + Wh + v] = -sn;
        t.bw4[(int64_t)v * W + k] = cs;
        t.bw4[(int64_t)(Wh + v) * W + k] = -sn;
        return true;
    }
    return false;
}

constexpr int kBM = 64, kBK = 16;      // a tile of C is 64 rows by 48 or 64 columns (NF = 3 or 4 MFMA tiles of 16)
constexpr int kLdsPitch = kBM + 16;    // 160 dwords = 32 mod 64 banks: the k rows a half-wave reads fall on disjoint banks

typedef double v4d __attribute__((ext_vector_type(4)));

enum { kStorePlain, kStoreFoldCols, kStoreScale, kStoreFoldRows };
enum { kLoadPlain, kLoadFilter };

struct Gemm {
    const double* A;    // [M][K], pitch lda; a_batch elements between planes (0: shared)
    const double* B;    // [K][N], pitch ldb
    double* C;
    int64_t a_batch, b_batch, c_batch;
    int lda, ldb, M, N, K;
    int half;           // FoldCols: N / 2; Scale, FoldRows and LoadFilter: M / 2 = K / 2
    const double* g;    // Scale: [2][half][N], the second table for planes p with p mod g_period >= g_first.  LoadFilter: [nf][half][N]
    int g_period, g_first;
    int nf;             // LoadFilter: grid.z = planes of B times nf, filter f = z mod nf on plane z / nf of B; odd f takes the odd part
};

// C = A B in fp64 on the matrix cores.  A workgroup owns a 64 x 16 NF tile of C, wave w its rows 16 w .. 16 w + 15 as NF MFMA tiles
// side by side; operands go through LDS k-major, 16 of K at a time, the next step's global loads in flight under this step's MFMAs.
// NF = 3 or 4, whichever pads N less: the half spectrum of a power-of-two width is 2^k + 1 columns, which 64-wide tiles would
// compute half as many again of.
// v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; result register r is
// C[row (l >> 4) + 4 r][col l & 15] (not the row map of the other MFMAs).
// Stores: Plain C[m][n]; FoldCols [Cl | Cr] -> [Cl; Cr]; Scale C[m][n] g[..][m mod half][n]; FoldRows [Ct; Cb] -> [Ct | Cb].
// LoadFilter: B = [Zr; Zi] is a spectrum and the operand is the spectrum times a real filter table G[half][N], formed as it is loaded:
// an even f reads [Zr G; Zi G] (G the even part of a filter: the product's inverse transform is real), an odd f reads [Zi G; -Zr G],
// which is -i Z G (G the odd part: the inverse transform of Z G is imaginary, and steps 3 and 4 then give that imaginary part).
template <int STORE, int NF, int LOAD = kLoadPlain>
__global__ __launch_bounds__(kThreads) void dft_gemm_kernel(Gemm g) {
    constexpr int BN = 16 * NF;
    __shared__ double sA[kBK * kLdsPitch], sB[kBK * kLdsPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * kBM, n0 = blockIdx.x * BN;
    const int64_t plane = blockIdx.z;
    const int64_t bplane = LOAD == kLoadFilter ? plane / g.nf : plane;
    const int filt = LOAD == kLoadFilter ? (int)(plane % g.nf) : 0;
    const double* __restrict__ A = g.A + plane * g.a_batch;
    const double* __restrict__ B = g.B + bplane * g.b_batch;
    const double* __restrict__ F = LOAD == kLoadFilter ? g.g + (int64_t)filt * g.half * g.N : nullptr;
    double* __restrict__ C = g.C + plane * g.c_batch;
    const int am = tid >> 2, ak = (tid & 3) * 4;   // A: row m0 + am, k = ak .. ak + 3
    const bool a_in = m0 + am < g.M;
    const double* pa = A + (int64_t)(m0 + am) * g.lda + ak;
    double ra[4], rb[NF];                          // B: element tid + 256 i of the 16 x BN tile, row-major
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = (a_in && k0 + ak + i < g.K) ? pa[k0 + i] : 0.0;
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int e = tid + kThreads * i, k = k0 + e / BN, n = n0 + e % BN;
            if (LOAD == kLoadPlain) {
                rb[i] = (k < g.K && n < g.N) ? B[(int64_t)k * g.ldb + n] : 0.0;
            } else {
                double v = 0.0;
                if (k < g.K && n < g.N) {
                    const int u = k % g.half;
                    const bool lower = k >= g.half;
                    const double w = F[(int64_t)u * g.N + n];
                    if (filt & 1)
                        v = lower ? -(B[(int64_t)u * g.ldb + n] * w) : B[(int64_t)(u + g.half) * g.ldb + n] * w;
                    else
                        v = B[(int64_t)k * g.ldb + n] * w;
                }
                rb[i] = v;
            }
        }
    };
    v4d acc[NF] = {};
    fetch(0);
    const int fr = lane & 15, fk = lane >> 4;
    for (int k0 = 0; k0 < g.K; k0 += kBK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) sA[(ak + i) * kLdsPitch + am] = ra[i];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int e = tid + kThreads * i;
            sB[(e / BN) * kLdsPitch + e % BN] = rb[i];
        }
        __syncthreads();
        if (k0 + kBK < g.K) fetch(k0 + kBK);
#pragma unroll
        for (int kk = 0; kk < kBK; kk += 4) {
            const double a = sA[(kk + fk) * kLdsPitch + wave * 16 + fr];
            const double* qb = &sB[(kk + fk) * kLdsPitch + fr];
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, qb[16 * j], acc[j], 0, 0, 0);
        }
    }
    const double* gt = STORE == kStoreScale ? g.g + ((int)(plane % g.g_period) >= g.g_first ? (int64_t)g.half * g.N : 0) : nullptr;
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wave * 16 + fk + 4 * r, n = n0 + j * 16 + fr;
            if (m >= g.M || n >= g.N) continue;
            const double v = acc[j][r];
            if (STORE == kStorePlain) C[(int64_t)m * g.N + n] = v;
            if (STORE == kStoreFoldCols) C[((int64_t)m + (int64_t)(n / g.half) * g.M) * g.half + n % g.half] = v;
            if (STORE == kStoreScale) C[(int64_t)m * g.N + n] = v * gt[(int64_t)(m % g.half) * g.N + n];
            if (STORE == kStoreFoldRows) C[(int64_t)(m % g.half) * 2 * g.N + (int64_t)(m / g.half) * g.N + n] = v;
        }
}

template <int STORE, int LOAD = kLoadPlain>
int launch_gemm(const Gemm& g, int planes, hipStream_t stream) {
    const dim3 grid48(cdiv(g.N, 48), cdiv(g.M, kBM), planes), grid64(cdiv(g.N, 64), cdiv(g.M, kBM), planes);
    if (grid48.x * 48 < grid64.x * 64)   // the narrower tile pads N less
        dft_gemm_kernel<STORE, 3, LOAD><<<grid48, kThreads, 0, stream>>>(g);
    else
        dft_gemm_kernel<STORE, 4, LOAD><<<grid64, kThreads, 0, stream>>>(g);
    return check_launch("dft_gemm_kernel");
}

inline double* carve_doubles(Carver& ws, int64_t n) { return reinterpret_cast<double*>(ws.floats(2 * n)); }

}  // namespace
}  // namespace swf
