// The comparative-study group of fusion metrics in one call (kernels_comparative.hip): Q_MI, Q_TE and Q_NCIE from three joint
// histograms, Q_SF and Q_M from one pass over level tiles, and Zhao's Q_P, whose phase congruency runs as dense fp64 DFT products on
// the matrix cores (dft_frag.h); per-tile fp64 partial sums, finishing workgroups per image.
#pragma once
#include "swf_common.h"

namespace swf {

// What the kernels' int indices and grids hold: the perception group's limits on H and W (<= 16384) and B <= 2730 (24 transform planes
// per image in grid.z).
bool comparative_shape_ok(int B, int H, int W);

// Bytes of workspace swf_fusion_comparative needs (include/swinfuse.h states the formula).
size_t fusion_comparative_workspace_bytes(int B, int H, int W);

// out[B][SWF_COMPARATIVE_COUNT] <- the six values of every image.  Arguments are already validated (swf_api.hip).
int fusion_comparative(const swf_comparative_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H,
                       int W, void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
