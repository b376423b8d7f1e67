// The pointwise activation of the MLPs, the patch layers and the head (swf_activation): what every epilogue of the generic family
// applies, and its derivative from the pre-activation u for the backward.  As torch.nn defines them; no fast-math substitutes.
#pragma once
#include <cmath>

#include "swf_common.h"

namespace swf {

// What a launcher's `act` argument carries: nothing (on == 0), or the activation `fn`.  An int converts as it always did: 0 none,
// 1 the default ELU(alpha = 1), so a caller without a descriptor reads as before.
struct Act {
    int on;
    swf_activation fn;
    Act(int on_ = 0) : on(on_ != 0), fn{SWF_ACT_ELU1, 0.f} {}
    Act(const swf_activation& f) : on(1), fn(f) {}
};

inline bool act_is_default(const swf_activation& a) { return a.kind == SWF_ACT_ELU1; }
inline swf_activation act_or_default(const swf_activation* a) { return a ? *a : swf_activation{SWF_ACT_ELU1, 0.f}; }
// SWF_OK, or SWF_ERR_UNSUPPORTED for an unknown kind or a non-finite parameter of a kind that reads it
inline int check_activation(const swf_activation& a, const char* what) {
    if (a.kind < SWF_ACT_ELU1 || a.kind > SWF_ACT_SILU) return fail(SWF_ERR_UNSUPPORTED, "%s: unknown activation kind %d", what, a.kind);
    if ((a.kind == SWF_ACT_ELU || a.kind == SWF_ACT_LEAKY_RELU) && !std::isfinite(a.param))
        return fail(SWF_ERR_UNSUPPORTED, "%s: activation parameter %g is not finite", what, (double)a.param);
    return SWF_OK;
}

constexpr float kSqrtHalf = 0.70710678118654752440f;      // 1 / sqrt(2)
constexpr float kSqrt2OverPi = 0.79788456080286535588f;   // sqrt(2 / pi)
constexpr float kInvSqrt2Pi = 0.39894228040143267794f;    // 1 / sqrt(2 pi)
constexpr float kGeluCubic = 0.044715f;

// act(v).  The default kind keeps the arithmetic it always had.
__device__ __forceinline__ float act_apply(float v, int kind, float p) {
    switch (kind) {
        case SWF_ACT_ELU1: return v > 0.f ? v : expm1f(v);
        case SWF_ACT_ELU: return v > 0.f ? v : p * expm1f(v);
        case SWF_ACT_RELU: return v > 0.f ? v : 0.f;
        case SWF_ACT_LEAKY_RELU: return v > 0.f ? v : v * p;
        case SWF_ACT_GELU: return 0.5f * v * (1.0f + erff(v * kSqrtHalf));
        case SWF_ACT_GELU_TANH: return 0.5f * v * (1.0f + tanhf(kSqrt2OverPi * (v + kGeluCubic * v * v * v)));
        default: return v / (1.0f + expf(-v));   // SWF_ACT_SILU
    }
}
__device__ __forceinline__ float act_apply(float v, const Act& a) { return act_apply(v, a.fn.kind, a.fn.param); }

// act'(u) from the pre-activation.  At the kinks as torch: ReLU'(0) = 0, LeakyReLU'(0) = slope, ELU'(u <= 0) = alpha exp(u).
__device__ __forceinline__ float act_grad(float u, int kind, float p) {
    switch (kind) {
        case SWF_ACT_ELU1: return u > 0.f ? 1.0f : expf(u);
        case SWF_ACT_ELU: return u > 0.f ? 1.0f : p * expf(u);
        case SWF_ACT_RELU: return u > 0.f ? 1.0f : 0.f;
        case SWF_ACT_LEAKY_RELU: return u > 0.f ? 1.0f : p;
        case SWF_ACT_GELU: return 0.5f * (1.0f + erff(u * kSqrtHalf)) + u * kInvSqrt2Pi * expf(-0.5f * u * u);
        case SWF_ACT_GELU_TANH: {
            const float t = tanhf(kSqrt2OverPi * (u + kGeluCubic * u * u * u));
            return 0.5f * (1.0f + t) + 0.5f * u * (1.0f - t * t) * kSqrt2OverPi * (1.0f + 3.0f * kGeluCubic * u * u);
        }
        default: {   // SWF_ACT_SILU
            const float s = 1.0f / (1.0f + expf(-u));
            return s * (1.0f + u * (1.0f - s));
        }
    }
}

}  // namespace swf
