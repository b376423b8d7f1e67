// Fusion-quality metrics (EN, MI, SD, SF, AG, CC, SCD, MSE, PSNR, Qabf) of a batch of fused images against their two sources in one
// call (kernels_metrics.hip): a joint-histogram pass, a Sobel / gradient pass and one finishing workgroup per image.
#pragma once
#include "swf_common.h"

namespace swf {

// Bytes of workspace swf_fusion_metrics needs: per image two 256x256 u32 joint histograms and three u64 sums (zeroed by the call),
// and three fp64 partial sums per 32x32 tile.
size_t fusion_metrics_workspace_bytes(int B, int H, int W);

// out[B][SWF_METRIC_COUNT] <- the ten values of every image.  Arguments are already validated (swf_api.hip).
int fusion_metrics(const swf_metrics_desc& d, const float* fusion, const float* ir, const float* vis, double* out, int B, int H, int W,
                   void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
