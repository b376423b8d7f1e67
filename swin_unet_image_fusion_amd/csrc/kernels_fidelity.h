// VIF (multi-scale pixel-domain visual information fidelity, per source and summed) and Nabf / Labf (Kumar's fusion artifacts and
// fusion loss) of a batch of fused images against their two sources in one call (kernels_fidelity.hip): per pyramid scale a
// separable fp64 moment filter, between scales a filter-and-decimate pass, one Sobel pass, one finishing workgroup per image.
#pragma once
#include "swf_common.h"

namespace swf {

// Bytes of workspace swf_fusion_fidelity needs: per image the fp64 planes of pyramid scales 2-4 (three per scale) and the per-tile
// fp64 partial sums (four per VIF tile, three per Sobel tile).
size_t fusion_fidelity_workspace_bytes(int B, int H, int W);

// out[B][SWF_FIDELITY_COUNT] <- the five values of every image.  Arguments are already validated (swf_api.hip).
int fusion_fidelity(const swf_fidelity_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H, int W,
                    void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
