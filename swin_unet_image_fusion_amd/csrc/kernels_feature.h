// Feature mutual information of fused images against their sources in one call (kernels_feature.hip): FMI on the level plane, on
// the snapped orthonormal DCT (dense fp64 products on the matrix cores, dft_frag.h), on one level of the Haar transform and on the
// Sobel edge plane; one thread per window, per-tile fp64 partial sums, one finishing workgroup per image.
#pragma once
#include "swf_common.h"

namespace swf {

// What the kernels' int indices and grids hold: metric_shape_ok, H, W <= 16384 (the DCT matrices are dense) and B <= 21845 (three
// transform planes per image in grid.z).
bool feature_shape_ok(int B, int H, int W);

// Bytes of workspace swf_fusion_feature needs (include/swinfuse.h states the formula).
size_t fusion_feature_workspace_bytes(int B, int H, int W);

// out[B][SWF_FEATURE_COUNT] <- the four values of every image.  Arguments are already validated (swf_api.hip).
int fusion_feature(const swf_feature_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H, int W,
                   void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
