// The 8-bit level of a unit-range fp32 pixel, shared by every kernel file that evaluates images on levels (kernels_metrics.hip,
// kernels_fidelity.hip, kernels_structure.hip): torchvision save_image's quantiser, (int) min(max(x * 255 + 0.5, 0), 255) in fp32 with two roundings.
#pragma once
#include <hip/hip_runtime.h>

namespace swf {

// Two roundings.  hipcc contracts __fadd_rn(__fmul_rn(x, 255.f), 0.5f) into one v_fma_f32 (the intrinsics are a plain * and + inside
// its headers, compiled with contraction on), which moves a level about 7 times per million pixels; plain operators under the pragma
// are what keeps the pair apart (checked in the ISA: no v_fma_f32 / v_fmac_f32 / v_mad_f32 in the metric kernels).
__device__ __forceinline__ int level(float x) {
#pragma clang fp contract(off)
    const float m = x * 255.f;
    const float v = m + 0.5f;
    return (int)fminf(fmaxf(v, 0.f), 255.f);   // fmaxf(NaN, 0) = 0
}

}  // namespace swf
