// What the register-resident block kernels of levels 0 / 1 / 2 (kernels_win24.hip, kernels_win48.hip, kernels_win96.hip) share
// with their callers: the kernel argument structs, the launch modes, and the table of host entries through which the dispatcher
// of kernels_window.hip reaches a level.  The entries themselves are written once, in win_host.h.
#pragma once
#include "swf_common.h"

namespace swf {

struct WinArgs {
    const float* in[2];
    float* out[2];       // half-block modes: a NULL out[s] drops that stream's stores (its waves only feed K / V to the other stream)
    const char* packed[2];
    const char* warm[2];
    int B, H, W, shift, cross, warm_bytes;
    int ntok[2];         // MLP half (WIN_MLP): token count of each stream's flat token list
};

// What one launch computes (template parameter MODE of window24 / 48 / 96_kernel, `mode` of launch_window_half):
//   WIN_BLOCK  the whole BasicBlock (a005:127-145)
//   WIN_ATTN   x + proj(attention(LN1 ...)) — AddAndLayerNormWithOtherModule around AutoPathWinAtt (a004:29-38, a002:58-82); with
//              RAW: proj(attention(q, k, v)) on un-normalised inputs and no residual — WindowAttention.forward (a001:448-474),
//              stream 0 = the query tensor and the output, stream 1 = the key / value tensor (its waves stop after K / V)
//   WIN_MLP    x + fc2(ELU(fc1(LN2 x))) — AddAndLayerNormWithOtherModule around AutoPathMLP (a004:29-38, a003:46-50); with RAW:
//              fc2(ELU(fc1 x)) — AutoPathMLP.forward.  Tokens are a flat list (no windows): 64 per workgroup step and stream
constexpr int WIN_BLOCK = 0, WIN_ATTN = 1, WIN_MLP = 2;

struct WinPackArgs {
    swf_block_stream_params p[2];
    char* dst[2];
    int ws;   // window side (7, 8 or 16)
};

// Host entries of one level (win_host.h: win_level<L>()).  Same contracts as the window_block / window_half family of
// kernels_window.h, which picks the level by channel count and calls through this table.
struct WinLevel {
    bool (*supported)(const swf_block_desc& d);
    size_t (*packed_bytes)(const swf_block_desc& d);   // ONE stream (fragment-major split-bf16 images, fp32 vectors, bias matrix); 0 = not covered
    size_t (*half_packed_bytes)(int hidden);           // ONE stream of a half-block launch (the attention half uses the wide layout); 0 = not covered
    // packs whatever weights the stream parameters hold (a missing half packs as zeros, a missing norm as identity)
    int (*pack)(const swf_block_desc& d, const swf_block_stream_params& px, const swf_block_stream_params& py, void* packed_x,
                void* packed_y, hipStream_t stream);
    // Half-block launches (8x8 / 7x7 windows).  mode WIN_ATTN: x_out = x + proj(attention(LN1 ...)) for both streams (raw = 0), or
    // out = proj(attention(q, kv, kv)) with q = x_in, kv = y_in, y_out = NULL (raw = 1; packed_y = packed_x).  mode WIN_MLP: tokens
    // as flat lists of ntok_x / ntok_y rows (H, W ignored).  A NULL output drops that stream's stores.
    int (*launch_half)(const swf_block_desc& d, int mode, int raw, const void* packed_x, const void* packed_y, const float* x_in,
                       const float* y_in, float* x_out, float* y_out, int B, int H, int W, int ntok_x, int ntok_y, hipStream_t stream);
    int (*launch)(const swf_block_desc& d, const void* packed_x, const void* packed_y, const float* x_in, const float* y_in,
                  float* x_out, float* y_out, int B, int H, int W, hipStream_t stream, const void* next_packed_x,
                  const void* next_packed_y, size_t next_bytes, int* route);   // route: see launch_window_block
};

const WinLevel& win24_level();   // C = 24 (kernels_win24.hip)
const WinLevel& win48_level();   // C = 48
const WinLevel& win96_level();   // C = 96

}  // namespace swf
