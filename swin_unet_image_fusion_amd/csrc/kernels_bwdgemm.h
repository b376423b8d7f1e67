// Gradient GEMMs of the exact-fp32 backward on the f32-input MFMA (kernels_bwdgemm.hip): the second family behind dx() / dw() of
// kernels_bwd.hip, bit-equal to the scalar-FMA family (same chains: one accumulator per output element from zero, reduction index
// ascending), selected per call through swf_bwd_options.gemm.
#pragma once
#include "swf_common.h"

namespace swf {

constexpr int kBwdChunk = 256;   // tokens per partial sum of the weight-gradient kernels of both families

// out[M][K] (+)= dY[M][N] . W[N][K]
int launch_bwd_dx_mfma(const float* dY, const float* W, float* out, int64_t M, int N, int K, int accumulate, hipStream_t stream);
// partial[chunk] = { [N][K]: sum over the chunk's tokens of dY[m][n] X[m][k];  [N]: column sums of dY }, chunk = kBwdChunk tokens
int launch_bwd_dw_mfma(const float* dY, const float* X, float* partial, int64_t M, int N, int K, hipStream_t stream);

}  // namespace swf
