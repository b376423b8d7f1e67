// Gradient GEMMs of the exact-fp32 backward on the matrix cores (gfx950: v_mfma_f32_16x16x4_f32).
//
//   bwd_dx_mfma_kernel   out[M][K] (+)= dY[M][N] . W[N][K]          (the NN product; the forward's gemm_f32_kernel is the NT one)
//   bwd_dw_mfma_kernel   partial[chunk][N][K + 1] = dY^T . X over the chunk's 256 tokens (the TN product) + the column sums of dY
//
// The f32-input MFMA is a k-ordered fmaf chain with one rounding per product, so these kernels are required to return THE SAME BITS
// as bwd_dx_kernel / bwd_dw_kernel of kernels_bwd.hip: one accumulator per output element, started at zero, the reduction index taken in
// ascending order (16 per staging step, 4 per instruction), zeros beyond the edge (fmaf(0, 0, acc) == acc).  The weight-gradient
// kernel keeps the scratch layout of the scalar kernel, so the fixed reduce_rows tree behind it is shared.
//
// Both kernels: a 64 x 64 output tile per 256-thread workgroup as 4 x 4 MFMA tiles of 16 x 16.  Wave (wr, wc) owns the tiles
// (wr + 2 i, wc + 2 j), i, j in {0, 1} — interleaved, so that a narrow matrix (24 or 4 live columns) still spreads over the four
// SIMDs — and skips a tile that lies wholly outside the matrix (wave-uniform).  Operands go to LDS 16 reduction indices at a time with
// 16-byte loads where base and row stride allow, scalar loads otherwise; the next step's loads are issued before the current MFMAs.
#include "kernels_bwdgemm.h"

#include "win_frag.h"

namespace swf {

using namespace wf;

namespace {

constexpr int RK = 16;            // reduction indices per staging step
constexpr int ALD = RK + 4;       // [row][reduction] image: 80-B rows, the b32 fragment reads of 16 rows x 4 indices hit 64 banks once
constexpr int RLD = 64 + 16;      // [reduction][column] image: 320-B rows, 4 indices x 16 columns likewise

// four floats at (row, col .. col + 3) of a row-major matrix with `rows` x `cols` entries, zeros outside
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int64_t row, int col, int64_t rows, int cols, int vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row >= rows || col >= cols) return v;
    const float* q = p + row * cols + col;
    if (vec && col + 4 <= cols) return *reinterpret_cast<const float4*>(q);
    v.x = q[0];
    if (col + 1 < cols) v.y = q[1];
    if (col + 2 < cols) v.z = q[2];
    if (col + 3 < cols) v.w = q[3];
    return v;
}

__global__ __launch_bounds__(256) void bwd_dx_mfma_kernel(const float* __restrict__ dY, const float* __restrict__ W, float* __restrict__ out,
                                                           int M, int N, int K, int accumulate, int vecA, int vecB) {
    __shared__ __attribute__((aligned(16))) float As[64 * ALD];   // dY tile [m][n]
    __shared__ __attribute__((aligned(16))) float Bs[RK * RLD];   // W tile  [n][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, fq = lane >> 4;
    const int m0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    const int ar = tid >> 2, ac = (tid & 3) * 4;     // staging: dY row, first of 4 reduction indices
    const int br = tid >> 4, bc = (tid & 15) * 4;    //          W row (reduction index), first of 4 columns
    bool live[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) live[i][j] = m0 + (wr + 2 * i) * 16 < M && k0 + (wc + 2 * j) * 16 < K;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    float4 va = load4(dY, m0 + ar, ac, M, N, vecA), vb = load4(W, br, k0 + bc, N, K, vecB);
    for (int n0 = 0; n0 < N; n0 += RK) {
        __syncthreads();   // the previous step's fragment reads are done
        *reinterpret_cast<float4*>(&As[ar * ALD + ac]) = va;
        *reinterpret_cast<float4*>(&Bs[br * RLD + bc]) = vb;
        __syncthreads();
        if (n0 + RK < N) {
            va = load4(dY, m0 + ar, n0 + RK + ac, M, N, vecA);
            vb = load4(W, n0 + RK + br, k0 + bc, N, K, vecB);
        }
#pragma unroll
        for (int kk = 0; kk < RK / 4; ++kk) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[((wr + 2 * i) * 16 + fr) * ALD + kk * 4 + fq];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[(kk * 4 + fq) * RLD + (wc + 2 * j) * 16 + fr];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (live[i][j]) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    // C/D map of the 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + (wc + 2 * j) * 16 + fr;
            if (k >= K) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wr + 2 * i) * 16 + fq * 4 + r;
                if (m >= M) continue;
                float* o = out + (int64_t)m * K + k;
                *o = accumulate ? *o + acc[i][j][r] : acc[i][j][r];
            }
        }
}

__global__ __launch_bounds__(256) void bwd_dw_mfma_kernel(const float* __restrict__ dY, const float* __restrict__ X, float* __restrict__ partial,
                                                           int M, int N, int K, int vecA, int vecB) {
    __shared__ __attribute__((aligned(16))) float As[RK * RLD];   // dY tile [m][n]
    __shared__ __attribute__((aligned(16))) float Bs[RK * RLD];   // X tile  [m][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, fq = lane >> 4;
    const int n0 = blockIdx.y * 64, k0 = blockIdx.x * 64, chunk = blockIdx.z;
    const int mlo = chunk * kBwdChunk, mhi = min(M, mlo + kBwdChunk);
    const int sr = tid >> 4, sc = (tid & 15) * 4;   // staging: token row, first of 4 columns
    bool live[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) live[i][j] = n0 + (wr + 2 * i) * 16 < N && k0 + (wc + 2 * j) * 16 < K;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;   // threads 0..63 of the k-tile-0 workgroups: column n0 + tid of dY, tokens in ascending order

    float4 va = load4(dY, mlo + sr, n0 + sc, mhi, N, vecA), vb = load4(X, mlo + sr, k0 + sc, mhi, K, vecB);
    for (int m0 = mlo; m0 < mhi; m0 += RK) {
        __syncthreads();   // the previous step's fragment reads are done
        *reinterpret_cast<float4*>(&As[sr * RLD + sc]) = va;
        *reinterpret_cast<float4*>(&Bs[sr * RLD + sc]) = vb;
        __syncthreads();
        if (m0 + RK < mhi) {
            va = load4(dY, m0 + RK + sr, n0 + sc, mhi, N, vecA);
            vb = load4(X, m0 + RK + sr, k0 + sc, mhi, K, vecB);
        }
        if (blockIdx.x == 0 && tid < 64) {
#pragma unroll
            for (int m = 0; m < RK; ++m) bsum += As[m * RLD + tid];
        }
#pragma unroll
        for (int kk = 0; kk < RK / 4; ++kk) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[(kk * 4 + fq) * RLD + (wr + 2 * i) * 16 + fr];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[(kk * 4 + fq) * RLD + (wc + 2 * j) * 16 + fr];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (live[i][j]) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    float* p = partial + (int64_t)chunk * N * (K + 1);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + (wc + 2 * j) * 16 + fr;
            if (k >= K) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + (wr + 2 * i) * 16 + fq * 4 + r;
                if (n < N) p[(int64_t)n * K + k] = acc[i][j][r];
            }
        }
    if (blockIdx.x == 0 && tid < 64 && n0 + tid < N) p[(int64_t)N * K + n0 + tid] = bsum;
}

// 16-byte loads need a 16-byte base and rows that are a multiple of four floats (torch hands out 4-byte-aligned views)
int vec_ok(const float* p, int ld) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 4 == 0; }

}  // namespace

int launch_bwd_dx_mfma(const float* dY, const float* W, float* out, int64_t M, int N, int K, int accumulate, hipStream_t stream) {
    dim3 grid((unsigned)cdiv64(M, 64), cdiv(K, 64));
    hipLaunchKernelGGL(bwd_dx_mfma_kernel, grid, dim3(256), 0, stream, dY, W, out, (int)M, N, K, accumulate, vec_ok(dY, N), vec_ok(W, K));
    return check_launch("bwd_dx_mfma");
}

int launch_bwd_dw_mfma(const float* dY, const float* X, float* partial, int64_t M, int N, int K, hipStream_t stream) {
    dim3 grid(cdiv(K, 64), cdiv(N, 64), (unsigned)cdiv64(M, kBwdChunk));
    hipLaunchKernelGGL(bwd_dw_mfma_kernel, grid, dim3(256), 0, stream, dY, X, partial, (int)M, N, K, vec_ok(dY, N), vec_ok(X, K));
    return check_launch("bwd_dw_mfma");
}

}  // namespace swf
