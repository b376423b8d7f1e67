// The human-perception group of fusion metrics in one call (kernels_perception.hip): Chen & Blum's Q_CB and Chen & Varshney's Q_CV,
// whose contrast-sensitivity filtering runs as dense fp64 DFT products on the matrix cores against twiddle matrices the call builds,
// with CE, EI and RMSE from one pass over the levels; per-tile fp64 partial sums, one finishing workgroup per image.
#pragma once
#include "swf_common.h"

namespace swf {

// What the kernels' int indices and grids hold: H, W <= 16384 (the 2H x 2H twiddle matrix has 4 H^2 <= 2^30 elements) and
// B <= 13107 (five transform planes per image in grid.z).
bool perception_shape_ok(int B, int H, int W);

// Bytes of workspace swf_fusion_perception needs: the twiddle matrices and the two filter tables (shared by the batch), per image five
// planes of three transform buffers, and the per-tile partial sums and histograms.
size_t fusion_perception_workspace_bytes(int B, int H, int W);

// out[B][SWF_PERCEPTION_COUNT] <- the five values of every image.  Arguments are already validated (swf_api.hip).
int fusion_perception(const swf_perception_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H,
                      int W, void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
