// The structural-similarity group of fusion metrics in one call (kernels_structure.hip): Wang's SSIM and MS-SSIM of the fused image
// against each source (11-tap Gaussian, fp64), Piella's Q_S / Q_W / Q_E, Cvejic's Q_C (8x8 boxes) and Yang's Q_Y (7x7 boxes) on exact
// integer window sums; per-tile fp64 partial sums, one finishing workgroup per image.
#pragma once
#include "swf_common.h"

namespace swf {

// Bytes of workspace swf_fusion_structure needs: per image the per-tile partial sums (four per Gaussian tile and scale, four per box
// tile and launch) and, for images of 176 pixels or more in both axes, the fp64 planes of pyramid scales 2-5 (three per scale).
size_t fusion_structure_workspace_bytes(int B, int H, int W);

// out[B][SWF_STRUCTURE_COUNT] <- the nine values of every image.  Arguments are already validated (swf_api.hip).
int fusion_structure(const swf_structure_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H, int W,
                     void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
