// Dropout of the training side (kernels_dropout.hip): counter-based masks (Philox4x32-10) regenerated wherever they are applied.
#pragma once
#include "swf_common.h"

namespace swf {

// One dropout site of one stream.  Element i of a [tokens][width] tensor (token = image-order row, i = token * width + channel) keeps
// its value, scaled by `scale`, iff ((r >> 8) * 2^-24) >= p, where r is word i % 4 of Philox4x32-10 with key (seed lo, seed hi) and
// counter (i / 4 lo, i / 4 hi, site, stream); a dropped element becomes 0 (include/swinfuse.h, swf_dropout_mask).
struct DropSite {
    uint64_t seed;
    uint32_t stream, site;
    float p, scale;   // scale = 1 / (1 - p) in fp32
};
inline DropSite drop_site(uint64_t seed, int stream, int site, float p) {
    return DropSite{seed, (uint32_t)stream, (uint32_t)site, p, 1.0f / (1.0f - p)};
}
enum { kDropAttn = 0, kDropProj = 1, kDropHidden = 2, kDropMlpOut = 3 };   // the four sites of a BasicBlock stream

// out[i] = factor(i)
int launch_dropout_mask(float* out, int64_t n, const DropSite& s, hipStream_t stream);
// out[i] = a[i] * factor(i)  (out may be a)
int launch_dropout_mul(const float* a, float* out, int64_t n, const DropSite& s, hipStream_t stream);
// out[i] = res[i] + a[i] * factor(i)  (out may be a or res)
int launch_dropout_add(const float* a, const float* res, float* out, int64_t n, const DropSite& s, hipStream_t stream);
// dh[i] = dh[i] * factor(i) * ELU'(u[i]), ELU'(u) taken from the UNDROPPED activation h = ELU(u) as elu_bwd_kernel does
int launch_dropout_elu_bwd(float* dh, const float* h, int64_t n, const DropSite& s, hipStream_t stream);

}  // namespace swf
