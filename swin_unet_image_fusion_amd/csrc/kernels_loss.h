// The reference's fusion loss (a008 MyLoss) as fused forward / backward kernels (kernels_loss.hip): separable Gaussian moments on an
// LDS-resident tile, Sobel / intensity / PSNR terms in a second small pass, fixed-order reductions.
#pragma once
#include "swf_common.h"

namespace swf {

// Floats of workspace swf_fusion_loss needs: per-tile partial sums, two mean squared errors, and (with a gradient of the SSIM term)
// the 4 adjoint maps of every Gaussian scale.
size_t fusion_loss_workspace_bytes(const swf_loss_desc& d, int B, int H, int W, bool with_grad);

// terms[5] <- S, T, I, P, total; grad (may be NULL) <- d total / d fusion.  Arguments are already validated (swf_api.hip).
int fusion_loss(const swf_loss_desc& d, const float* fusion, const float* ir, const float* vis, float* terms, float* grad,
                int B, int H, int W, void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
