// Dropout of the training side (the reference's attention_drop_layer, linear_drop_layer and dropout_{x,y}_{1,2}: a001:351-354,
// a001:412-414, a003:25-31) as counter-based masks: nothing is stored between the forward and the backward, every kernel that applies
// a mask regenerates it from (seed, stream, site, element index).  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as
// 1, 2, 3", SC'11): one call gives four 32-bit words, so one thread serves four consecutive elements.
//
//   dropout_kernel<MODE>   MASK     out = factor
//                          MUL      out = a * factor                       (sites 0 and 2 in the forward, every mask in the backward)
//                          ADD      out = res + a * factor                 (sites 1 and 3: the dropped branch onto its residual)
//                          ELU_BWD  out = a * factor * ELU'(u) from h = b  (the hidden gradient through site 2 and the activation)
#include "kernels_dropout.h"

namespace swf {
namespace {

enum { kMask = 0, kMul = 1, kAdd = 2, kEluBwd = 3 };

struct Philox4 { uint32_t w[4]; };

// Philox4x32 with 10 rounds (Random123's philox4x32_R(10, ctr, key)): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key bumps
// 0x9E3779B9 / 0xBB67AE85 between rounds.
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// keep iff (r >> 8) * 2^-24 >= p (the 24-bit value is exact in fp32); a kept element is scaled by 1 / (1 - p)
__device__ __forceinline__ float keep_factor(uint32_t r, float p, float scale) {
    return (float)(r >> 8) * 5.9604644775390625e-8f >= p ? scale : 0.0f;
}

template <int MODE>
__device__ __forceinline__ float apply(float f, float a, float b) {
    if (MODE == kMask) return f;
    if (MODE == kMul) return __fmul_rn(a, f);
    if (MODE == kAdd) return __fadd_rn(b, __fmul_rn(a, f));
    return __fmul_rn(__fmul_rn(a, f), b > 0.f ? 1.0f : b + 1.0f);   // kEluBwd: ELU'(u) = 1 (u > 0) or exp(u) = h + 1
}

// thread g: elements 4g .. 4g + 3 (counter word 0/1 = g, 2 = site, 3 = stream; key = seed).  VEC: n % 4 == 0 and every pointer
// 16-byte aligned, so the four elements move as one float4.
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(const float* a, const float* b, float* out, int64_t n,
                                                      uint64_t seed, uint32_t stream, uint32_t site, float p, float scale) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i0 = 4 * g;
    if (i0 >= n) return;
    const Philox4 r = philox4x32_10((uint32_t)g, (uint32_t)((uint64_t)g >> 32), site, stream, (uint32_t)seed, (uint32_t)(seed >> 32));
    if (VEC) {
        float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MODE != kMask) av = *reinterpret_cast<const float4*>(a + i0);
        if (MODE == kAdd || MODE == kEluBwd) bv = *reinterpret_cast<const float4*>(b + i0);
        float4 o;
        o.x = apply<MODE>(keep_factor(r.w[0], p, scale), av.x, bv.x);
        o.y = apply<MODE>(keep_factor(r.w[1], p, scale), av.y, bv.y);
        o.z = apply<MODE>(keep_factor(r.w[2], p, scale), av.z, bv.z);
        o.w = apply<MODE>(keep_factor(r.w[3], p, scale), av.w, bv.w);
        *reinterpret_cast<float4*>(out + i0) = o;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = i0 + j;
            if (i < n) {
                const float av = MODE != kMask ? a[i] : 0.f;
                const float bv = (MODE == kAdd || MODE == kEluBwd) ? b[i] : 0.f;
                out[i] = apply<MODE>(keep_factor(r.w[j], p, scale), av, bv);
            }
        }
    }
}

bool aligned16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int MODE>
int launch(const float* a, const float* b, float* out, int64_t n, const DropSite& s, hipStream_t st, const char* what) {
    if (n <= 0) return SWF_OK;
    const int64_t threads = cdiv64(n, 4);
    if (cdiv64(threads, 256) > INT32_MAX) return fail(SWF_ERR_UNSUPPORTED, "%s: %lld elements", what, (long long)n);
    const dim3 grid((unsigned)cdiv64(threads, 256));
    if (n % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(out))
        hipLaunchKernelGGL((dropout_kernel<MODE, true>), grid, dim3(256), 0, st, a, b, out, n, s.seed, s.stream, s.site, s.p, s.scale);
    else
        hipLaunchKernelGGL((dropout_kernel<MODE, false>), grid, dim3(256), 0, st, a, b, out, n, s.seed, s.stream, s.site, s.p, s.scale);
    return check_launch(what);
}

}  // namespace

int launch_dropout_mask(float* out, int64_t n, const DropSite& s, hipStream_t st) {
    return launch<kMask>(nullptr, nullptr, out, n, s, st, "dropout_mask");
}
int launch_dropout_mul(const float* a, float* out, int64_t n, const DropSite& s, hipStream_t st) {
    return launch<kMul>(a, nullptr, out, n, s, st, "dropout_mul");
}
int launch_dropout_add(const float* a, const float* res, float* out, int64_t n, const DropSite& s, hipStream_t st) {
    return launch<kAdd>(a, res, out, n, s, st, "dropout_add");
}
int launch_dropout_elu_bwd(float* dh, const float* h, int64_t n, const DropSite& s, hipStream_t st) {
    return launch<kEluBwd>(dh, h, dh, n, s, st, "dropout_elu_bwd");
}

}  // namespace swf
