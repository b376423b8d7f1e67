// The attention core of the exact-fp32 backward: the problem description the kernel families share, and the "phased" family
// (kernels_bwdattn.hip, SWF_BWD_ATTN_PHASED), which never holds more than two operand tiles of a (window, head) in LDS.
#pragma once
#include "swf_common.h"

namespace swf {

// One workgroup = one (window, head) of one stream; grid (B * nwy * nwx, heads, streams).
struct AttnBwdProb {
    const float* Q; const float* K; const float* V; const float* dO;   // [tokens][heads*d], row stride ld
    float* dQ; float* dK; float* dV;
    const float* bias_table;
    float* dtable_partial;   // [windows * heads][table entries]
};
struct AttnBwdBatch { AttnBwdProb p[2]; };

constexpr size_t kAttnBwdLdsMax = 160 * 1024;   // the LDS of a CU: no form of the attention backward may ask for more

// padded channels per row of the phased kernel (0: head_dim > 64) and its dynamic LDS in bytes for a wh x ww window at that width:
// two operand tiles, the bias table, three statistics per query, one private table-gradient partial per wave
int attn_bwd_phased_width(int d);
size_t attn_bwd_lds_phased(int wh, int ww, int dp);
// what launch_attn_bwd_phased would refuse, asked before the first launch of an entry
int check_attn_bwd_phased_shape(const char* what, int wh, int ww, int d);
int launch_attn_bwd_phased(const AttnBwdBatch& batch, int nprob, int ld, int B, int H, int W, int wh, int ww, int heads, int d, int shift,
                           swf_bwd_route* route, hipStream_t stream);

}  // namespace swf
