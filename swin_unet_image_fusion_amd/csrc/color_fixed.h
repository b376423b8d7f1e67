// OpenCV's published 8-bit fixed-point BGR -> YCrCb forward transform (yuv_shift 14, CV_DESCALE rounding, saturate), shared by the
// colour kernels (kernels_color.hip) and the dataset kernel (kernels_data.hip).  Parity is pinned by formula only: cv2 itself is not
// available to this build.
#pragma once
#include "swf_common.h"

namespace swf {

constexpr int kB2Y = 1868, kG2Y = 9617, kR2Y = 4899;   // sum = 1 << 14
constexpr int kYCrI = 11682, kYCbI = 9241;

__device__ __forceinline__ int descale14(int x) { return (x + (1 << 13)) >> 14; }
__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// uint8 luma of one BGR pixel (before saturation; the coefficients sum to 1 << 14, so it is already in [0, 255])
__device__ __forceinline__ int bgr_to_y8(int b, int g, int r) { return descale14(b * kB2Y + g * kG2Y + r * kR2Y); }

}  // namespace swf
