// The host entries of a register-resident level (win_level.h: WinLevel) and the parts of its pack kernel that do not depend on
// the level's channel layout, written once.  Included by kernels_win24.hip / kernels_win48.hip / kernels_win96.hip only: a
// kernel template must be instantiated in the file that launches it, so each of them describes itself by a traits type L
//
//   static constexpr int C, D;                    channels, head dimension (8 heads)
//   static constexpr int HID_WIDE, HID_NARROW;    the two hidden widths (encoder / decoder)
//   static constexpr int PACK_GRID, WAVES;        grid.x of the pack kernel; resident workgroups per CU of the 8x8 / 7x7 kernel
//   static constexpr const char *name, *pack_name;   "win24", "pack_win24": prefixes of the error texts
//   template <int HID> using G = ...;             the level's geometry (p_total, p_total16, ...)
//   template <int HID> static void pack(dim3 grid, const WinPackArgs&, hipStream_t);   launches the pack kernel
//   template <int HID, int WS, int MODE, bool RAW>
//   static int launch(const swf_block_desc&, const WinArgs&, int grid, hipStream_t, int* route);   8x8 / 7x7: which kernel, LDS; launch + check
//                                                 (route: trace_block, where the level has more than one kernel for a block)
//   template <int HID> static int launch16(const WinArgs&, int nwin, hipStream_t);     16x16: the level's own grid; launch + check
//
// and defines winNN_level() to return win_level<L>().
#pragma once
#include "win_frag.h"
#include "win_level.h"

#include <algorithm>

namespace swf {
namespace {

// ---------------------------------------------------------------------------------------------------------------
// pack kernels
// ---------------------------------------------------------------------------------------------------------------
// k index (input channel / virtual channel / hidden unit offset) of element e of k-step s in lane half hf, for an operand
// produced as accumulator tiles: step s covers registers 8(s&1).. of tile s>>1
__host__ __device__ constexpr int kslot(int s, int hf, int e) { return 32 * (s >> 1) + wf::rho(8 * (s & 1) + e, hf); }

// (the half-block entries pack only the half they run: a missing layer packs as zeros)
__device__ __forceinline__ float pack_wgt(const swf_linear& l, int i) { return l.weight ? l.weight[i] : 0.f; }
__device__ __forceinline__ float pack_bia(const swf_linear& l, int n) { return (l.weight && l.bias) ? l.bias[n] : 0.f; }

// Relative-position bias section of a packed image (a001:113-144), exp2 units: the S^T accumulator registers (key = row
// rho(reg, lane half), query = lane & 31) of every (query tile, key tile) pair, as 1024-float tiles in the order the level's
// kernel loads them: LANE_MAJOR (level 0) [lane][key tile][reg], else (levels 1, 2) [key tile][reg / 4][lane][reg % 4].
//   8x8 / 7x7: [query block 2] x [key tile 2]; the padding tokens of a 7x7 window carry -inf as keys (probability 0).
//   16x16    : one tile per distance d = kt - qb + 7 between key tile and query tile (a tile = two window rows of 16 tokens,
//              so the relative positions of a tile pair depend on that distance only); |dy| <= 2 * 7 + 1 stays inside the table.
template <bool LANE_MAJOR>
__device__ __forceinline__ void pack_rel_bias(float* bm, const float* table, int ws, int gtid, int gsz) {
    const int ktb = ws == 16 ? 0 : 1;   // log2(key tiles per outer index)
    for (int i = gtid; i < (ws == 16 ? 15 : 4) * 1024; i += gsz) {
        const int outer = i >> (10 + ktb);   // query block, or distance
        const int reg = LANE_MAJOR ? i & 15 : 4 * ((i >> 8) & 3) + (i & 3);
        const int kt = ((LANE_MAJOR ? i >> 4 : i >> 10)) & ((1 << ktb) - 1);
        const int lane = (LANE_MAJOR ? i >> (4 + ktb) : i >> 2) & 63;
        const int key = 32 * kt + wf::rho(reg, lane >> 5), q = lane & 31;
        if (ws == 16) {
            const int dy = 2 * (outer - 7) + (key >> 4) - (q >> 4), dx = (key & 15) - (q & 15);
            bm[i] = table[(dy + 15) * 31 + (dx + 15)] * wf::kLog2e;
        } else {
            const int ky = key >> 3, kx = key & 7, qy = 4 * outer + (q >> 3), qx = q & 7, tw = 2 * ws - 1;
            float v = 0.f;
            if (ky >= ws || kx >= ws) v = -INFINITY;   // padding token of a 7x7 window as key: probability 0
            else if (qy < ws && qx < ws) v = table[(ky - qy + ws - 1) * tw + (kx - qx + ws - 1)] * wf::kLog2e;
            bm[i] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------------------------------------------
template <class L> bool win_hidden_ok(int hidden) { return hidden == L::HID_WIDE || hidden == L::HID_NARROW; }

template <class L>
bool win_supported(const swf_block_desc& d) {
    return d.attn.channels == L::C && d.attn.heads == 8 && d.attn.head_dim == L::D && d.attn.win_h == d.attn.win_w &&
           (d.attn.win_h == 8 || d.attn.win_h == 7 || d.attn.win_h == 16) && win_hidden_ok<L>(d.hidden);
}

template <class L>
size_t win_half_packed_bytes(int hidden) {
    if (!win_hidden_ok<L>(hidden)) return 0;
    return align_up(hidden == L::HID_WIDE ? L::template G<L::HID_WIDE>::p_total : L::template G<L::HID_NARROW>::p_total, 256);
}

template <class L>
size_t win_packed_bytes(const swf_block_desc& d) {
    if (!win_supported<L>(d)) return 0;
    if (d.attn.win_h != 16) return win_half_packed_bytes<L>(d.hidden);
    return align_up(d.hidden == L::HID_WIDE ? L::template G<L::HID_WIDE>::p_total16 : L::template G<L::HID_NARROW>::p_total16, 256);
}

template <class L>
int win_pack(const swf_block_desc& d, const swf_block_stream_params& px, const swf_block_stream_params& py, void* packed_x,
             void* packed_y, hipStream_t stream) {
    if (!win_supported<L>(d)) return fail(SWF_ERR_UNSUPPORTED, "%s: shape not covered", L::pack_name);
    WinPackArgs a;
    a.p[0] = px; a.p[1] = py;
    a.dst[0] = static_cast<char*>(packed_x); a.dst[1] = static_cast<char*>(packed_y);
    a.ws = d.attn.win_h;
    if (d.hidden == L::HID_WIDE) L::template pack<L::HID_WIDE>(dim3(L::PACK_GRID, 2), a, stream);
    else L::template pack<L::HID_NARROW>(dim3(L::PACK_GRID, 2), a, stream);
    return check_launch(L::pack_name);
}

// The token rows travel through 32-bit buffer descriptors: one launch covers less than 2 GB of a stream's rows.
template <class L> bool win_rows_fit(int64_t tokens) { return tokens * L::C * 4 < (int64_t(1) << 31); }

inline WinArgs win_args(const swf_block_desc& d, const void* packed_x, const void* packed_y, const float* x_in, const float* y_in,
                        float* x_out, float* y_out, int B, int H, int W) {
    WinArgs a{};
    a.in[0] = x_in; a.in[1] = y_in; a.out[0] = x_out; a.out[1] = y_out;
    a.packed[0] = static_cast<const char*>(packed_x); a.packed[1] = static_cast<const char*>(packed_y);
    a.B = B; a.H = H; a.W = W; a.shift = d.attn.shift; a.cross = d.cross;
    return a;
}

// Which instantiation a descriptor names.  The attention half ignores the MLP geometry (the wide image layout serves), the MLP
// half has no windows (WS = 8): neither instantiates the other combinations.
template <class L, int HID, int MODE, bool RAW>
int win_launch_ws(const swf_block_desc& d, const WinArgs& a, int grid, hipStream_t stream, int* route) {
    if constexpr (MODE != WIN_MLP) {
        if (d.attn.win_h != 8) return L::template launch<HID, 7, MODE, RAW>(d, a, grid, stream, route);
    }
    return L::template launch<HID, 8, MODE, RAW>(d, a, grid, stream, route);
}
template <class L, int MODE, bool RAW>
int win_launch_as(const swf_block_desc& d, const WinArgs& a, int nwin, hipStream_t stream, int* route = nullptr) {
    const int grid = std::min(nwin, L::WAVES * num_cus());   // resident workgroups per CU (register-limited)
    if constexpr (MODE != WIN_ATTN) {
        if (d.hidden != L::HID_WIDE) return win_launch_ws<L, L::HID_NARROW, MODE, RAW>(d, a, grid, stream, route);
    }
    return win_launch_ws<L, L::HID_WIDE, MODE, RAW>(d, a, grid, stream, route);
}

template <class L>
int win_launch_half(const swf_block_desc& d, int mode, int raw, const void* packed_x, const void* packed_y, const float* x_in,
                    const float* y_in, float* x_out, float* y_out, int B, int H, int W, int ntok_x, int ntok_y, hipStream_t stream) {
    const int wsd = d.attn.win_h;
    if (mode != WIN_ATTN && mode != WIN_MLP) return fail(SWF_ERR_UNSUPPORTED, "%s_half: mode %d", L::name, mode);
    if (d.attn.channels != L::C || !win_hidden_ok<L>(d.hidden)) return fail(SWF_ERR_UNSUPPORTED, "%s_half: shape not covered", L::name);
    WinArgs a = win_args(d, packed_x, packed_y, x_in, y_in, x_out, y_out, B, H, W);
    a.ntok[0] = ntok_x; a.ntok[1] = ntok_y;
    if (mode == WIN_ATTN) {
        if (!win_supported<L>(d) || wsd == 16 || H % wsd || W % wsd) return fail(SWF_ERR_UNSUPPORTED, "%s_half: shape not covered", L::name);
        if (!win_rows_fit<L>((int64_t)B * H * W)) return fail(SWF_ERR_UNSUPPORTED, "%s_half: map exceeds the 2 GB buffer window", L::name);
        const int nwin = B * (H / wsd) * (W / wsd);
        return raw ? win_launch_as<L, WIN_ATTN, true>(d, a, nwin, stream) : win_launch_as<L, WIN_ATTN, false>(d, a, nwin, stream);
    }
    const int ntok = std::max(ntok_x, ntok_y);
    if (!win_rows_fit<L>(ntok) || ntok_x <= 0) return fail(SWF_ERR_UNSUPPORTED, "%s_half: token count", L::name);
    const int nwin = (ntok + 63) / 64;
    return raw ? win_launch_as<L, WIN_MLP, true>(d, a, nwin, stream) : win_launch_as<L, WIN_MLP, false>(d, a, nwin, stream);
}

template <class L>
int win_launch(const swf_block_desc& d, const void* packed_x, const void* packed_y, const float* x_in, const float* y_in,
               float* x_out, float* y_out, int B, int H, int W, hipStream_t stream, const void* next_packed_x,
               const void* next_packed_y, size_t next_bytes, int* route) {
    const int wsd = d.attn.win_h;
    if (!win_supported<L>(d) || H % wsd || W % wsd) return fail(SWF_ERR_UNSUPPORTED, "%s: shape not covered", L::name);
    if (!win_rows_fit<L>((int64_t)B * H * W))
        return fail(SWF_ERR_UNSUPPORTED, "%s: a stream of %d x %d x %d tokens exceeds the 2 GB buffer window", L::name, B, H, W);
    WinArgs a = win_args(d, packed_x, packed_y, x_in, y_in, x_out, y_out, B, H, W);
    a.warm[0] = static_cast<const char*>(next_packed_x); a.warm[1] = static_cast<const char*>(next_packed_y);
    if (!a.warm[1]) a.warm[0] = nullptr;
    a.warm_bytes = (int)(next_bytes ? next_bytes : win_packed_bytes<L>(d));
    const int nwin = B * (H / wsd) * (W / wsd);
    if (wsd != 16) return win_launch_as<L, WIN_BLOCK, false>(d, a, nwin, stream, route);
    trace_block(route, SWF_BLOCK_WIN_W16);
    return d.hidden == L::HID_WIDE ? L::template launch16<L::HID_WIDE>(a, nwin, stream) : L::template launch16<L::HID_NARROW>(a, nwin, stream);
}

template <class L>
constexpr WinLevel win_level() {
    return {win_supported<L>, win_packed_bytes<L>, win_half_packed_bytes<L>, win_pack<L>, win_launch_half<L>, win_launch<L>};
}

}  // namespace
}  // namespace swf
