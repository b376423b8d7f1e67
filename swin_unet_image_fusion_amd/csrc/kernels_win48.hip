// Level-1 fused BasicBlock (a005:127-145) for gfx950: C = 48, 8 heads x 6 channels, 8x8 windows, hidden 192 (encoder) or 96
// (decoder).  The register-resident design of kernels_win24.hip at twice the width: a 256-thread workgroup owns one window,
// wave w the 32 tokens [32*(w&1), +32) of stream w>>1 for the whole block; activations go from MFMA accumulators to the next
// MFMA's operand in registers (weights packed with their k columns in accumulator-row order), K / V^T operand fragments are
// exchanged through lane-linear LDS images, the residual is the C operand of the projection and fc2 MFMAs.
//
// What differs from C = 24:
//  * 48 channels = two 32-row tiles (rows 48..63 are padding); a head's 6 channels + 2 spare rows are one 8-row group, so a
//    k-step of S^T = K.Q^T holds two WHOLE heads: selecting a head is a compile-time choice of two of the four fragment dwords
//    (no lane select), its O^T rows are registers 4(h&3).. of BOTH lane halves (channels 0-3 / 4-5, denominator, spare).
//  * Spare row 6 of a head is the constant 1 in V (softmax denominator), spare row 7 is 1 in K and -max in Q (S - max on the
//    matrix pipe).  Row 6 of head 0 of the normalised O (= 1) carries the projection bias.
//  * K = 48 has no spare k slot: the Q/K/V, fc1 and fc2 biases are added in the epilogues (fast-class VALU adds).
//  * The relative-position bias tile (32 registers) is loaded per window (L2 hit) instead of living in registers for the whole
//    launch: the MLP phase needs the space.
//
// Arithmetic as kernels_win24.hip: linear layers split-bf16 x3 on v_mfma_f32_32x32x16_bf16, Q.K^T and P.V on ..._f16, fp32
// LayerNorm / softmax / ELU / residual; ELU in exp2 units through v_med3 (fc1 packed with log2 e, fc2 with ln 2).
#include "win_host.h"

namespace swf {
namespace {

using namespace wf;

constexpr int W48_WAVES = 2;   // resident workgroups per CU = waves per SIMD

template <int HID_>
struct G48 {
    static constexpr int C = 48, HID = HID_, HEADS = 8, D = 6;
    static constexpr int NT1 = HID / 32, KU = HID / 16;
    static_assert(HID % 32 == 0, "hidden tiles");
    static constexpr int F_QKV = 0;                   // [q,k,v][tile 2][k-step 3][hi,lo]
    static constexpr int F_P = 36;                    // [out tile 2][k-step 4][hi,lo]
    static constexpr int F_W1 = 52;                   // [tile NT1][k-step 3][hi,lo]
    static constexpr int F_W2 = F_W1 + 6 * NT1;       // [out tile 2][k-step KU][hi,lo]
    static constexpr int NFRAG = F_W2 + 4 * KU;
    // fp32 vectors: per lane half [LN1G 24 | LN1B 24 | LN2G 24 | LN2B 24 | B2 24 | BQ 32 | BK 32 | B1 16*NT1], then BV [2 tiles][32]
    static constexpr int V_LN1G = 0, V_LN1B = 24, V_LN2G = 48, V_LN2B = 72, V_B2 = 96, V_BQ = 120, V_BK = 152, V_B1 = 184, VHF = 288;
    static_assert(V_B1 + 16 * NT1 <= VHF, "vector block");
    static constexpr int VSTREAM = 2 * VHF + 64;
    static constexpr size_t p_vec = size_t(NFRAG) * 1024;
    static constexpr size_t p_bias = (p_vec + size_t(VSTREAM) * 4 + 15) / 16 * 16;   // fp32 [query block 2][key tile 2][reg/4 4][lane 64][4]
    static constexpr size_t p_total = p_bias + size_t(2) * 2 * 16 * 64 * 4;
    // LDS: K images [stream 2][key tile 2][vch tile 2][k-step 2] x 1 KB, V^T images [stream 2][vch tile 2][pv-step 4] x 1 KB, vectors,
    // 4 KB of zeros (what the non-matching lanes of the P.V A read see: win_frag.h)
    static constexpr size_t l_k = 0, l_v = 16 * 1024, l_vec = 32 * 1024, l_zero = l_vec + size_t(2) * VSTREAM * 4, l_total = l_zero + kPvZeroBytes;
    // 16x16 windows (window48w16_kernel): bias tiles by key-tile / query-tile distance, fp32 [distance 15][reg/4 4][lane 64][4];
    // LDS of ONE stream: K images [key tile 8][vch tile 2][k-step 2] x 1 KB, V^T images [vch tile 2][pv-step 16] x 1 KB, vectors, zeros
    static constexpr size_t p_total16 = p_bias + size_t(15) * 16 * 64 * 4;
    static constexpr size_t l_k16 = 0, l_v16 = 32 * 1024, l_vec16 = 64 * 1024, l_zero16 = l_vec16 + size_t(2) * VSTREAM * 4, l_total16 = l_zero16 + kPvZeroBytes;
};

// launch modes of window48_kernel: win_level.h (WIN_BLOCK, WIN_ATTN, WIN_MLP; RAW = no LayerNorm, no residual)

// RAW modes: the un-normalised row as the operand fragments of the next linear layer
__device__ __forceinline__ void raw48(const f32x16& x0, const f32x16& x1, u32x4 (&xh)[3], u32x4 (&xl)[3]) {
    float n[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) n[i] = i < 16 ? x0[i] : x1[i - 16];
    split8(n, xh[0], xl[0]);
    split8(n + 8, xh[1], xl[1]);
    split8(n + 16, xh[2], xl[2]);
}

// LayerNorm (eps 1e-5, biased variance) of the lane's token: 24 of its 48 channels sit in this lane (tile 0 registers 0..15,
// tile 1 registers 0..7), the other 24 in lane l ^ 32.  Output: the three k-step fragments of the next linear layer.
__device__ __forceinline__ void layernorm48(const f32x16& x0, const f32x16& x1, const float* vec, int goff, int boff, u32x4 (&xh)[3], u32x4 (&xl)[3]) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += x0[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += x1[i];
    const float mean = sum_halves(s) * (1.0f / 48.0f);
    float d[24], q = 0.f;
#pragma unroll
    for (int i = 0; i < 24; ++i) {
        d[i] = (i < 16 ? x0[i] : x1[i - 16]) - mean;
        q += d[i] * d[i];
    }
    const float rstd = __builtin_amdgcn_rsqf(sum_halves(q) * (1.0f / 48.0f) + 1e-5f);
    float n[24];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const float4 g = *reinterpret_cast<const float4*>(vec + goff + 4 * a);
        const float4 b = *reinterpret_cast<const float4*>(vec + boff + 4 * a);
        n[4 * a + 0] = d[4 * a + 0] * rstd * g.x + b.x;
        n[4 * a + 1] = d[4 * a + 1] * rstd * g.y + b.y;
        n[4 * a + 2] = d[4 * a + 2] * rstd * g.z + b.z;
        n[4 * a + 3] = d[4 * a + 3] * rstd * g.w + b.w;
    }
    split8(n, xh[0], xl[0]);
    split8(n + 8, xh[1], xl[1]);
    split8(n + 16, xh[2], xl[2]);
}

// The lane's base of the P.V A read in V^T tile T (win_frag.h: mfma16_f16): lane l is row 4g + c of k-group l >> 4; a head is 8 rows,
// row groups 0 / 1 deliver its channels 0..3 (to lane half 0), row groups 2 / 3 channels 4, 5, the denominator and the spare row
// (to lane half 1): a matching lane reads slot 32 hf + 4 (g >> 1) + c of the block (the head's 8 hq and the pv-step are added as
// immediates), every other lane the zero region.  vblk: byte offset of the tile's first V^T block of the chunk, zreg: of the zeros.
__device__ __forceinline__ const u32x4* pv_src48(const char* smem, int lane, unsigned vblk, unsigned zreg) {
    const unsigned off = pv_match(lane) ? vblk + (unsigned)(((lane & 32) + ((lane >> 1) & 4) + (lane & 3)) * 16) : zreg + (unsigned)kPvZeroBase;
    return reinterpret_cast<const u32x4*>(smem + off);
}

// Attention of one wave: 32 queries x 64 keys x 8 heads.  ksrc: the stream's K operand images in LDS (+ lane); vsrc[T]: the lane's
// base of the P.V A read in V^T tile T (pv_src48);
// qf[tile][k-step]: the wave's own Q fragments; bias: relative-position bias of (stream, query block), with -inf where the shift
// mask applies (the reference assigns -1e10 to those scores: probability exactly 0).  Returns the two O^T tiles: registers 4q..4q+3 of tile T = head 4T+q:
// lane half 0 channels 0..3, lane half 1 channels 4, 5, the softmax denominator, 0.
// ONLINE (16x16 windows): the 64 keys are one chunk of a window's 256 — o is not cleared but rescaled, o = o * 2^(m_old - m_new) + t,
// with the running maximum mrun[head] kept as the f16 value the second S^T pass subtracts.
// (Signature: o stays the array reference this function always took — unlike attention24, whose single tile goes by value; mrun is
// a plain pointer, unused when !ONLINE.)
template <bool ONLINE>
__device__ __forceinline__ void attention48(const u32x4* ksrc, const u32x4* const (&vsrc)[2], const u32x4 (&qf)[2][2], const f32x16 (&bias)[2],
                                            bool half1, f32x16 (&o)[2], float* mrun = nullptr) {
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (!ONLINE) { o[0] = zero16; o[1] = zero16; }
#pragma unroll
    for (int h = 0; h < 8; ++h) {
        const int T = h >> 2, hq = h & 3, sp = hq >> 1, sub = hq & 1;
        // K fragments of (key tile, vch tile T, k-step sp): image index ((kt * 2 + T) * 2 + sp)
        const u32x4 ka0 = ksrc[((0 * 2 + T) * 2 + sp) * 64], ka1 = ksrc[((1 * 2 + T) * 2 + sp) * 64];
        // the head's 8 rows are elements 4*sub .. 4*sub+3 of both lane halves: a compile-time choice of two dwords
        u32x4 qm = {0u, 0u, 0u, 0u};
        qm[2 * sub] = qf[T][sp][2 * sub];
        qm[2 * sub + 1] = qf[T][sp][2 * sub + 1];
        // Pass 1: the row maximum, one key tile at a time (16 live score registers instead of 32).  S^T[key][query] + bias, exp2 units.
        float mx;
        {
            f32x16 s0 = mfma_f16(ka0, qm, bias[0]);
            mx = max3f(s0[0], s0[1], s0[2]);
#pragma unroll
            for (int i = 3; i < 15; i += 2) mx = max3f(mx, s0[i], s0[i + 1]);
            mx = __builtin_fmaxf(mx, s0[15]);
        }
        {
            f32x16 s1 = mfma_f16(ka1, qm, bias[1]);
#pragma unroll
            for (int i = 0; i < 16; i += 2) mx = max3f(mx, s1[i], s1[i + 1]);
        }
        mx = max_halves(mx);
        // Pass 2: S - max on the matrix pipe — the head's spare row 7 (lane half 1, element 4*sub+3) is 1 in K and -max (f16)
        // in Q — then P = exp2(.) in f16 and O^T += V^T . P^T, again one key tile (two pv-steps of 16 keys) at a time
        f16 nm = (f16)(-mx);
        float alpha = 0.f;
        if constexpr (ONLINE) {
            const float mold = mrun[h];
            nm = (f16)(-__builtin_fmaxf(mold, mx));
            const float mnew = -(float)nm;   // the shift the second pass really applies
            alpha = __builtin_amdgcn_exp2f(mold - mnew);
            mrun[h] = mnew;
        }
        qm[2 * sub + 1] |= half1 ? ((unsigned)__builtin_bit_cast(unsigned short, nm) << 16) : 0u;
        f32x4 t;   // the head's rows of the lane's query: lane half 0 channels 0..3, lane half 1 channels 4, 5, denominator, spare
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            f32x16 sc = mfma_f16(kt ? ka1 : ka0, qm, bias[kt]);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                float p[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) p[j] = __builtin_amdgcn_exp2f(sc[8 * s2 + j]);
                const u32x4 pf = pack8_f16(p);
                const u32x4 va = vsrc[T][(2 * kt + s2) * 64 + hq * 8];
                t = mfma16_f16(va, pf, (kt == 0 && s2 == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : t);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) o[T][4 * hq + j] = ONLINE ? __builtin_fmaf(o[T][4 * hq + j], alpha, t[j]) : t[j];
        __builtin_amdgcn_sched_barrier(0);   // one head at a time
    }
}

// WS = window side, 8 or 7 (the reference's default, A000_CONFIG.py:55).  A 7x7 window runs on the same 8x8 token grid, as in
// kernels_win24.hip: the 15 padding tokens load zeros and store nothing (an offset beyond the buffer descriptor's range) and
// carry -inf in the packed bias matrix as keys; the shift seam sits at WS - WS/2 = 4 for both sizes.
template <int HID, int WS, int MODE = WIN_BLOCK, bool RAW = false>
__global__ __launch_bounds__(256, W48_WAVES) void window48_kernel(WinArgs args) {
    using G = G48<HID>;
    static_assert(WS == 7 || WS == 8, "window side");
    static_assert(!RAW || MODE != WIN_BLOCK, "RAW belongs to the half-block modes");
    constexpr bool ATT = MODE != WIN_MLP, MLP = MODE != WIN_ATTN;
    __shared__ __attribute__((aligned(16))) char smem[G::l_total];
    u32x4* kimg = reinterpret_cast<u32x4*>(smem + G::l_k);   // [stream][key tile][vch tile][k-step][lane]
    u32x4* vimg = reinterpret_cast<u32x4*>(smem + G::l_v);   // [stream][vch tile][pv-step][lane]
    float* lvec = reinterpret_cast<float*>(smem + G::l_vec);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ws = wave >> 1, qb = wave & 1, r = lane & 31, hf = lane >> 5;
    const int H = args.H, W = args.W, nwx = ATT ? W / WS : 1, nwy = ATT ? H / WS : 1, npi = nwx * nwy;
    const int nwin = ATT ? args.B * npi : (max(args.ntok[0], args.ntok[1]) + 63) / 64;   // MLP half: 64 tokens of the flat list per step
    const int sh = args.shift ? WS / 2 : 0;
    const int kvs = args.cross ? 1 - ws : ws;   // the stream whose attention reads this wave's tokens as keys (a002:67-82)

    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(uniform_ptr(args.packed[ws])), 0, (int)G::p_total, 0x00020000);
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(uniform_ptr(args.packed[kvs])), 0, (int)G::p_total, 0x00020000);
    const int act_bytes = ATT ? args.B * H * W * 48 * 4 : args.ntok[ws] * 48 * 4;   // < 2^31 (launch_win48)
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(uniform_ptr(args.in[ws])), 0, act_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(args.out[ws]), 0, (MODE == WIN_BLOCK || args.out[ws]) ? act_bytes : 0, 0x00020000);
    const unsigned loff = (unsigned)lane * 16u;
    auto WF = [&](int f) { return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, loff, f * 1024, 0)); };   // own stream: Q, proj, MLP
    auto WK = [&](int f) { return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, loff, f * 1024, 0)); };   // K / V weights
    const float* vec = lvec + ws * G::VSTREAM + hf * G::VHF;       // own stream, own lane half
    const float* veck = lvec + kvs * G::VSTREAM + hf * G::VHF;     // K bias: the stream whose weights produce K
    const float* vecv = lvec + kvs * G::VSTREAM + 2 * G::VHF;      // V bias [tile][32]
    const bool half1 = hf != 0;
    const bool col_masked = half1 != (((r >> 2) & 1) != 0);
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (ATT) pv_fill_zeros<256>(smem + G::l_zero, tid);   // visible after the first window's barriers

    for (int win = blockIdx.x; win < nwin; win += gridDim.x) {
        SWF_WF_FENCE();
        const int b = win / npi, wrem = win - b * npi;
        const int wy = wrem / nwx, wx = wrem - wy * nwx;
        const int ty = 4 * qb + (r >> 3), tx = r & 7;
        int oy = wy * WS + ty + sh, ox = wx * WS + tx + sh;
        oy = oy >= H ? oy - H : oy;
        ox = ox >= W ? ox - W : ox;
        // byte offset of the lane's first float4; padding tokens of a 7x7 window point beyond the buffer (reads 0, stores dropped)
        const unsigned tokoff = [&]() -> unsigned {
            if constexpr (ATT) {
                return (WS == 8 || (ty < WS && tx < WS)) ? (unsigned)((((b * H + oy) * W + ox) * 48 + 4 * hf) * 4) : 0x80000000u;
            } else {   // flat token list; past the stream's end: out of range (reads 0, stores dropped)
                const int tok = 64 * win + 32 * qb + r;
                return tok < args.ntok[ws] ? (unsigned)((tok * 48 + 4 * hf) * 4) : 0x80000000u;
            }
        }();
        // the lane's 24 channels: tile 0 registers 4a.. = channels 8a+4hf.. (a < 4), tile 1 registers 4a.. = channels 32+8a+4hf.. (a < 2)
        auto load_rows = [&](f32x16& t0, f32x16& t1) {
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(irs, tokoff, 32 * a, 0));
                if (a < 4) { t0[4 * a] = v.x; t0[4 * a + 1] = v.y; t0[4 * a + 2] = v.z; t0[4 * a + 3] = v.w; }
                else { t1[4 * (a - 4)] = v.x; t1[4 * (a - 4) + 1] = v.y; t1[4 * (a - 4) + 2] = v.z; t1[4 * (a - 4) + 3] = v.w; }
            }
#pragma unroll
            for (int i = 8; i < 16; ++i) t1[i] = 0.f;   // rows 48..63 of every output tile have zero weights: stay zero
        };

        f32x16 res0, res1;
        if constexpr (ATT) {
        // ---- LN1, then Q (own stream's weights), K and V (weights of the stream that attends to these tokens) ----
        u32x4 qf[2][2];
        {
            // Six tile phases (Q0 Q1 K0 K1 V0 V1), 6 weight fragments each.  With two waves per SIMD nothing else hides an L2 round
            // trip, so the fragments of phase p+1 are requested before the MFMAs of phase p (double register set; the fences pin
            // the issue points, the in-order vmcnt lets phase p's data be waited for while phase p+1's stays in flight).
            u32x4 wq[2][6];
            auto req = [&](int ph, u32x4 (&dst)[6]) {
                const int m = ph >> 1, T = ph & 1;
#pragma unroll
                for (int i = 0; i < 6; ++i) dst[i] = m == 0 ? WF(G::F_QKV + ((m * 2 + T) * 3) * 2 + i) : WK(G::F_QKV + ((m * 2 + T) * 3) * 2 + i);
            };
            req(0, wq[0]);
            // the residual rows stay in registers across the attention phase: C operand of the projection
            f32x16 &x0 = res0, &x1 = res1;
            load_rows(x0, x1);
            if (win == (int)blockIdx.x) {
                // the fp32 vectors of both streams -> LDS, once per launch: requested BEHIND the first window's rows and first
                // weight fragments so that the three round trips overlap (at 512 windows a workgroup sees one or two windows:
                // its prologue is on the critical path)
                static_assert(G::VSTREAM % 4 == 0 && G::p_vec % 16 == 0, "vector sections move as 16-byte groups");
                    fill_vectors<G::VSTREAM / 4, 256>(lvec, args.packed[0] + G::p_vec, args.packed[1] + G::p_vec, tid);
                __syncthreads();
            }
            u32x4 xh[3], xl[3];
            if constexpr (RAW) raw48(x0, x1, xh, xl);
            else layernorm48(x0, x1, vec, G::V_LN1G, G::V_LN1B, xh, xl);
            float t[16];
#pragma unroll
            for (int ph = 0; ph < 6; ++ph) {
                const int m = ph >> 1, T = ph & 1;
                SWF_WF_FENCE();
                if (ph + 1 < 6) req(ph + 1, wq[(ph + 1) & 1]);
                SWF_WF_FENCE();
                const u32x4 (&w)[6] = wq[ph & 1];
                f32x16 acc = zero16;
                if (RAW && (m == 0 ? ws == 1 : ws == 0)) {
                    // (wave-uniform) RAW attention: the key / value stream has no queries, the query stream's tokens are nobody's keys;
                    // the barrier of the first K phase is every wave's
                    if (ph == 2 && win != (int)blockIdx.x) __syncthreads();
                } else if (m < 2) {
#pragma unroll
                    for (int s = 0; s < 3; ++s) acc = mma3(w[2 * s], w[2 * s + 1], xh[s], xl[s], acc);   // [virtual channel][token]
                    const float* bsrc = m == 0 ? vec + G::V_BQ : veck + G::V_BK;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 bb = *reinterpret_cast<const float4*>(bsrc + 16 * T + 4 * g);
                        t[4 * g] = acc[4 * g] + bb.x; t[4 * g + 1] = acc[4 * g + 1] + bb.y; t[4 * g + 2] = acc[4 * g + 2] + bb.z; t[4 * g + 3] = acc[4 * g + 3] + bb.w;
                    }
                    if (m == 0) {
                        qf[T][0] = pack8_f16(t);
                        qf[T][1] = pack8_f16(t + 8);
                    } else {
                        if (T == 0 && win != (int)blockIdx.x) __syncthreads();   // the attention phase of the window before has read the images
                        u32x4* kdst = kimg + (((kvs * 2 + qb) * 2 + T) * 2) * 64 + lane;
                        kdst[0] = pack8_f16(t);
                        kdst[64] = pack8_f16(t + 8);
                    }
                } else {   // V: tokens in rows (A = x fragments, B = weight fragments)
#pragma unroll
                    for (int s = 0; s < 3; ++s) acc = mma3(xh[s], xl[s], w[2 * s], w[2 * s + 1], acc);
                    const float bv = vecv[32 * T + r];
#pragma unroll
                    for (int i = 0; i < 16; ++i) t[i] = acc[i] + bv;
                    u32x4* vdst = vimg + ((kvs * 2 + T) * 4 + 2 * qb) * 64 + lane;
                    vdst[0] = pack8_f16(t);
                    vdst[64] = pack8_f16(t + 8);
                }
            }
        }
        // the bias tile of (stream, query block) is requested ahead of the barrier: its L2 round trip runs under the wait
        f32x16 bias[2];
        load_bias_tiles(wrs, loff, (int)G::p_bias, __builtin_amdgcn_readfirstlane(qb) * 2, bias);
        __syncthreads();   // K / V^T images of both streams complete
        if (RAW && ws == 1) continue;   // RAW: the key / value stream is done with this window

        // ---- attention of the wave's 32 queries, 8 heads (shift mask: kernels_win24.hip) ----
        f32x16 o[2];
        {
            const bool rowv = args.shift && wy == nwy - 1, colv = args.shift && wx == nwx - 1;
            const u32x4* ksrc = kimg + (ws * 8) * 64 + lane;
            const u32x4* const vsrc[2] = {pv_src48(smem, lane, (unsigned)(G::l_v + (ws * 8) * 1024), (unsigned)G::l_zero),
                                          pv_src48(smem, lane, (unsigned)(G::l_v + (ws * 8 + 4) * 1024), (unsigned)G::l_zero)};
            if (rowv || colv) {   // wave-uniform: the mask is a whole key tile / a whole lane, folded into the C operand once per window
                const float pen0 = ((rowv && qb == 1) || (colv && col_masked)) ? -INFINITY : 0.f;
                const float pen1 = ((rowv && qb == 0) || (colv && col_masked)) ? -INFINITY : 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) { bias[0][i] += pen0; bias[1][i] += pen1; }
            }
            attention48<false>(ksrc, vsrc, qf, bias, half1, o);
        }

        // ---- normalise (denominator: lane half 1, register 4q+2), output projection + bias + residual ----
        u32x4 wpj[16];   // all 16 projection fragments ([out tile 2][k-step 4][hi, lo]): requested here, in flight under the normalisation
        SWF_WF_FENCE();
        if constexpr (RAW) { res0 = zero16; res1 = zero16; }   // CrossAttention.forward: no residual
#pragma unroll
        for (int i = 0; i < 16; ++i) wpj[i] = WF(G::F_P + i);
        SWF_WF_FENCE();
        {
            u32x4 oh[4], ol[4];
#pragma unroll
            for (int T = 0; T < 2; ++T) {
                float t[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float lo_, den;
                    halves(o[T][4 * q + 2], lo_, den);   // den = the value of lanes 32..63
                    const float inv = __builtin_amdgcn_rcpf(den);
                    // lane half 1: register 4q+2 becomes den / den = 1 (the projection bias rides on head 0's), 4q+3 stays 0
                    t[4 * q] = o[T][4 * q] * inv; t[4 * q + 1] = o[T][4 * q + 1] * inv; t[4 * q + 2] = o[T][4 * q + 2] * inv; t[4 * q + 3] = o[T][4 * q + 3] * inv;
                }
                split8(t, oh[2 * T], ol[2 * T]);
                split8(t + 8, oh[2 * T + 1], ol[2 * T + 1]);
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                res0 = mma3(wpj[(0 * 4 + ks) * 2], wpj[(0 * 4 + ks) * 2 + 1], oh[ks], ol[ks], res0);
                res1 = mma3(wpj[(1 * 4 + ks) * 2], wpj[(1 * 4 + ks) * 2 + 1], oh[ks], ol[ks], res1);
            }
        }

        } else {   // MLP half: the rows as they are; the fp32 vectors once per launch
            load_rows(res0, res1);
            if (win == (int)blockIdx.x) {
                fill_vectors<G::VSTREAM / 4, 256>(lvec, args.packed[0] + G::p_vec, args.packed[1] + G::p_vec, tid);
                __syncthreads();
            }
        }

        // ---- LN2, MLP: fc1 tile -> ELU -> split -> two k-steps of fc2 accumulating onto the residual ----
        if constexpr (MLP) {
            // fc1 fragments of tile tI+1 and the fc2 fragments of tile tI are requested at the top of tile tI (see the Q/K/V phases)
            u32x4 w1[2][6];
            auto req1 = [&](int tI, u32x4 (&dst)[6]) {
#pragma unroll
                for (int i = 0; i < 6; ++i) dst[i] = WF(G::F_W1 + tI * 6 + i);
            };
            // fc2 fragments of a hidden tile ([out tile][k-step of the tile][hi, lo]) are requested one tile ahead as well: asked
            // for at the top of their own tile they arrived ~0.5 us after the fc1 MFMAs and ELU had finished (ablation: the six
            // MLP tiles took 17 of the launch's 50 us at two waves per SIMD, three times their issue time)
            u32x4 w2[2][2][2][2];
            auto req2 = [&](int tI, u32x4 (&dst)[2][2][2]) {
#pragma unroll
                for (int To = 0; To < 2; ++To)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        dst[To][s2][0] = WF(G::F_W2 + (To * G::KU + 2 * tI + s2) * 2);
                        dst[To][s2][1] = WF(G::F_W2 + (To * G::KU + 2 * tI + s2) * 2 + 1);
                    }
            };
            req1(0, w1[0]);
            req2(0, w2[0]);
            u32x4 xh[3], xl[3];
            if constexpr (RAW) { raw48(res0, res1, xh, xl); res0 = zero16; res1 = zero16; }   // AutoPathMLP.forward: no norm, no residual
            else layernorm48(res0, res1, vec, G::V_LN2G, G::V_LN2B, xh, xl);
#pragma unroll
            for (int tI = 0; tI < G::NT1; ++tI) {
                SWF_WF_FENCE();
                if (tI + 1 < G::NT1) { req1(tI + 1, w1[(tI + 1) & 1]); req2(tI + 1, w2[(tI + 1) & 1]); }
                SWF_WF_FENCE();
                const u32x4 (&w)[6] = w1[tI & 1];
                f32x16 acc = zero16;
#pragma unroll
                for (int s = 0; s < 3; ++s) acc = mma3(w[2 * s], w[2 * s + 1], xh[s], xl[s], acc);
                float e[16];
                elu_tile(acc, vec + G::V_B1 + 16 * tI, e);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    u32x4 hh, hl;
                    split8(e + 8 * s2, hh, hl);
                    res0 = mma3(w2[tI & 1][0][s2][0], w2[tI & 1][0][s2][1], hh, hl, res0);
                    res1 = mma3(w2[tI & 1][1][s2][0], w2[tI & 1][1][s2][1], hh, hl, res1);
                }
                __builtin_amdgcn_sched_barrier(0);   // one hidden tile at a time
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const float4 b2 = *reinterpret_cast<const float4*>(vec + G::V_B2 + 4 * a);
                if (a < 4) { res0[4 * a] += b2.x; res0[4 * a + 1] += b2.y; res0[4 * a + 2] += b2.z; res0[4 * a + 3] += b2.w; }
                else { res1[4 * (a - 4)] += b2.x; res1[4 * (a - 4) + 1] += b2.y; res1[4 * (a - 4) + 2] += b2.z; res1[4 * (a - 4) + 3] += b2.w; }
            }
        }

        // ---- store the own rows (un-shift = the same index map) ----
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const f32x4 v = a < 4 ? f32x4{res0[4 * a], res0[4 * a + 1], res0[4 * a + 2], res0[4 * a + 3]}
                                  : f32x4{res1[4 * (a - 4)], res1[4 * (a - 4) + 1], res1[4 * (a - 4) + 2], res1[4 * (a - 4) + 3]};
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ors, tokoff, 32 * a, 0);
        }
    }

    // ---- L2 warm-up of the next block's packed weights (see kernels_window.hip) ----
    if (args.warm[0]) warm_next_block<256>(args, tid);
}

// ---------------------------------------------------------------------------------------------------------------
// 16x16 windows at C = 48 (BASELINE config 5, level 1): one workgroup = (window, stream), four waves, a wave owns two of the
// eight 32-token tiles.  The K / V^T images of all 256 keys of ONE stream's attention fill 64 KB of LDS (two workgroups per CU):
// the workgroup computes them itself from the tokens its attention reads — its own stream's, or the other stream's in a cross
// block (a002:67-82: K and V of attention_x come from LN1_y(y) with attention_x's weights) — so nothing is exchanged between
// workgroups and only LN1 of those tokens is computed twice in cross blocks.  Phase A: LN1, Q (kept in registers), K, V with
// each weight-fragment set fetched once for both tiles.  Phase B per tile: online softmax over four chunks of 64 keys (the
// 8x8 kernel's attention as a chunk, running maximum kept as the f16 value the second S^T pass subtracts; bias tiles by tile
// distance; row-seam chunks skipped, column seam = register bit 2 against lane bit 3: kernels_win24.hip), projection, LN2, MLP.
template <int HID>
__global__ __launch_bounds__(256, 2) void window48w16_kernel(WinArgs args) {
    using G = G48<HID>;
    extern __shared__ __attribute__((aligned(16))) char smem48[];
    u32x4* kimg = reinterpret_cast<u32x4*>(smem48 + G::l_k16);   // [key tile][vch tile][k-step][lane]
    u32x4* vimg = reinterpret_cast<u32x4*>(smem48 + G::l_v16);   // [vch tile][pv-step][lane]
    float* lvec = reinterpret_cast<float*>(smem48 + G::l_vec16);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ws = blockIdx.y, r = lane & 31, hf = lane >> 5;
    const int H = args.H, W = args.W, nwx = W / 16, nwy = H / 16, npi = nwx * nwy;
    const int nwin = args.B * npi;
    const int sh = args.shift ? 8 : 0;
    const int src = args.cross ? 1 - ws : ws;   // the stream whose tokens this stream's attention reads as keys / values

    static_assert(G::VSTREAM % 4 == 0 && G::p_vec % 16 == 0, "vector sections move as 16-byte groups");
                    fill_vectors<G::VSTREAM / 4, 256>(lvec, args.packed[0] + G::p_vec, args.packed[1] + G::p_vec, tid);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(args.packed[ws]), 0, (int)G::p_total16, 0x00020000);
    const int act_bytes = args.B * H * W * 48 * 4;   // < 2^31 (launch_win48)
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(args.in[ws]), 0, act_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(args.in[src]), 0, act_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(args.out[ws], 0, act_bytes, 0x00020000);
    const unsigned loff = (unsigned)lane * 16u;
    auto WF = [&](int f) { return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, loff, f * 1024, 0)); };
    const float* vec = lvec + ws * G::VSTREAM + hf * G::VHF;        // own stream, own lane half (also the K bias: own weights)
    const float* vecs = lvec + src * G::VSTREAM + hf * G::VHF;      // LN1 parameters of the key / value tokens' stream
    const float* vecv = lvec + ws * G::VSTREAM + 2 * G::VHF;        // V bias [tile][32]
    const bool half1 = hf != 0;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    pv_fill_zeros<256>(smem48 + G::l_zero16, tid);
    __syncthreads();

    for (int win = blockIdx.x; win < nwin; win += gridDim.x) {
        SWF_WF_FENCE();
        const int b = win / npi, wrem = win - b * npi;
        const int wy = wrem / nwx, wx = wrem - wy * nwx;
        auto tokoff_of = [&](int j) {   // tile j = window rows 2j, 2j+1; the lane's token: row 2j + (r >> 4), column r & 15
            int oy = wy * 16 + 2 * j + (r >> 4) + sh, ox = wx * 16 + (r & 15) + sh;
            oy = oy >= H ? oy - H : oy;
            ox = ox >= W ? ox - W : ox;
            return (unsigned)((((b * H + oy) * W + ox) * 48 + 4 * hf) * 4);
        };
        auto load_rows = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned tokoff, f32x16& t0, f32x16& t1) {
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, tokoff, 32 * a, 0));
                if (a < 4) { t0[4 * a] = v.x; t0[4 * a + 1] = v.y; t0[4 * a + 2] = v.z; t0[4 * a + 3] = v.w; }
                else { t1[4 * (a - 4)] = v.x; t1[4 * (a - 4) + 1] = v.y; t1[4 * (a - 4) + 2] = v.z; t1[4 * (a - 4) + 3] = v.w; }
            }
#pragma unroll
            for (int i = 8; i < 16; ++i) t1[i] = 0.f;
        };

        // ---- phase A: LN1 of the wave's two tiles (own tokens for Q, the key / value stream's for K and V), six tile phases ----
        u32x4 qf[2][2][2];   // [tile of the wave][vch tile][k-step]
        {
            u32x4 xh[2][3], xl[2][3], kh[2][3], kl[2][3];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const unsigned tokoff = tokoff_of(2 * wave + jj);
                f32x16 x0, x1;
                load_rows(irs, tokoff, x0, x1);
                layernorm48(x0, x1, vec, G::V_LN1G, G::V_LN1B, xh[jj], xl[jj]);
                if (args.cross) {
                    load_rows(srs, tokoff, x0, x1);
                    layernorm48(x0, x1, vecs, G::V_LN1G, G::V_LN1B, kh[jj], kl[jj]);
                } else {
#pragma unroll
                    for (int s2 = 0; s2 < 3; ++s2) { kh[jj][s2] = xh[jj][s2]; kl[jj][s2] = xl[jj][s2]; }
                }
            }
            u32x4 wq[2][6];
            auto req = [&](int ph, u32x4 (&dst)[6]) {
#pragma unroll
                for (int i = 0; i < 6; ++i) dst[i] = WF(G::F_QKV + ph * 6 + i);   // [q,k,v][tile][k-step][hi,lo]
            };
            req(0, wq[0]);
#pragma unroll
            for (int ph = 0; ph < 6; ++ph) {
                const int m = ph >> 1, T = ph & 1;
                SWF_WF_FENCE();
                if (ph + 1 < 6) req(ph + 1, wq[(ph + 1) & 1]);
                SWF_WF_FENCE();
                const u32x4 (&w)[6] = wq[ph & 1];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int j = 2 * wave + jj;
                    f32x16 acc = zero16;
                    float t[16];
                    if (m < 2) {
#pragma unroll
                        for (int s2 = 0; s2 < 3; ++s2)
                            acc = m == 0 ? mma3(w[2 * s2], w[2 * s2 + 1], xh[jj][s2], xl[jj][s2], acc) : mma3(w[2 * s2], w[2 * s2 + 1], kh[jj][s2], kl[jj][s2], acc);
                        const float* bsrc = m == 0 ? vec + G::V_BQ : vec + G::V_BK;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const float4 bb = *reinterpret_cast<const float4*>(bsrc + 16 * T + 4 * g);
                            t[4 * g] = acc[4 * g] + bb.x; t[4 * g + 1] = acc[4 * g + 1] + bb.y; t[4 * g + 2] = acc[4 * g + 2] + bb.z; t[4 * g + 3] = acc[4 * g + 3] + bb.w;
                        }
                        if (m == 0) {
                            qf[jj][T][0] = pack8_f16(t);
                            qf[jj][T][1] = pack8_f16(t + 8);
                        } else {
                            u32x4* kdst = kimg + ((j * 2 + T) * 2) * 64 + lane;
                            kdst[0] = pack8_f16(t);
                            kdst[64] = pack8_f16(t + 8);
                        }
                    } else {   // V: tokens in rows (A = x fragments, B = weight fragments)
#pragma unroll
                        for (int s2 = 0; s2 < 3; ++s2) acc = mma3(kh[jj][s2], kl[jj][s2], w[2 * s2], w[2 * s2 + 1], acc);
                        const float bv = vecv[32 * T + r];
#pragma unroll
                        for (int i = 0; i < 16; ++i) t[i] = acc[i] + bv;
                        u32x4* vdst = vimg + (T * 16 + 2 * j) * 64 + lane;
                        vdst[0] = pack8_f16(t);
                        vdst[64] = pack8_f16(t + 8);
                    }
                }
            }
        }
        __syncthreads();   // K / V^T images of all 256 keys complete

        // ---- phase B ----
        const bool rowv = args.shift && wy == nwy - 1, colv = args.shift && wx == nwx - 1;
#pragma unroll 1
        for (int jj = 0; jj < 2; ++jj) {
            const int j = 2 * wave + jj;   // query tile
            const unsigned tokoff = tokoff_of(j);
            f32x16 o[2] = {zero16, zero16};
            float mrun[8];
#pragma unroll
            for (int h = 0; h < 8; ++h) mrun[h] = -INFINITY;
#pragma unroll 1
            for (int c = 0; c < 4; ++c) {
                if (rowv && ((j < 4) != (c < 2))) continue;   // keys across the row seam: probabilities exactly 0
                f32x16 bias[2];
                {
                    const int d0 = __builtin_amdgcn_readfirstlane(2 * c - j + 7);
                    load_bias_tiles(wrs, loff, (int)G::p_bias, d0, bias);
                    if (colv) col_seam16(bias, r);
                }
                // key tiles 2c, 2c + 1: 4 K fragments each, 4 pv-steps of each V^T tile (the chunk and tile offsets are part of the
                // matching lanes' base only: the zero region is one chunk of one tile)
                const u32x4* const vsrc[2] = {pv_src48(smem48, lane, (unsigned)(G::l_v16 + (4 * c) * 1024), (unsigned)G::l_zero16),
                                              pv_src48(smem48, lane, (unsigned)(G::l_v16 + (16 + 4 * c) * 1024), (unsigned)G::l_zero16)};
                attention48<true>(kimg + (2 * c) * 4 * 64 + lane, vsrc, qf[0], bias, half1, o, mrun);
            }
            // the second tile's Q fragments move up
#pragma unroll
            for (int T = 0; T < 2; ++T) { qf[0][T][0] = qf[1][T][0]; qf[0][T][1] = qf[1][T][1]; }

            // ---- normalise, output projection + bias + residual ----
            f32x16 res0, res1;
            SWF_WF_FENCE();
            load_rows(irs, tokoff, res0, res1);
            {
                u32x4 oh[4], ol[4];
#pragma unroll
                for (int T = 0; T < 2; ++T) {
                    float t[16];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float lo_, den;
                        halves(o[T][4 * q + 2], lo_, den);
                        const float inv = __builtin_amdgcn_rcpf(den);
                        t[4 * q] = o[T][4 * q] * inv; t[4 * q + 1] = o[T][4 * q + 1] * inv; t[4 * q + 2] = o[T][4 * q + 2] * inv; t[4 * q + 3] = o[T][4 * q + 3] * inv;
                    }
                    split8(t, oh[2 * T], ol[2 * T]);
                    split8(t + 8, oh[2 * T + 1], ol[2 * T + 1]);
                }
                SWF_WF_FENCE();
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    res0 = mma3(WF(G::F_P + (0 * 4 + ks) * 2), WF(G::F_P + (0 * 4 + ks) * 2 + 1), oh[ks], ol[ks], res0);
                    res1 = mma3(WF(G::F_P + (1 * 4 + ks) * 2), WF(G::F_P + (1 * 4 + ks) * 2 + 1), oh[ks], ol[ks], res1);
                }
            }
            // ---- LN2, MLP ----
            {
                u32x4 w1[2][6];
                auto req1 = [&](int tI, u32x4 (&dst)[6]) {
#pragma unroll
                    for (int i = 0; i < 6; ++i) dst[i] = WF(G::F_W1 + tI * 6 + i);
                };
                req1(0, w1[0]);
                u32x4 xh[3], xl[3];
                layernorm48(res0, res1, vec, G::V_LN2G, G::V_LN2B, xh, xl);
#pragma unroll
                for (int tI = 0; tI < G::NT1; ++tI) {
                    SWF_WF_FENCE();
                    u32x4 w2[2][2][2];
#pragma unroll
                    for (int To = 0; To < 2; ++To)
#pragma unroll
                        for (int s2 = 0; s2 < 2; ++s2) {
                            w2[To][s2][0] = WF(G::F_W2 + (To * G::KU + 2 * tI + s2) * 2);
                            w2[To][s2][1] = WF(G::F_W2 + (To * G::KU + 2 * tI + s2) * 2 + 1);
                        }
                    if (tI + 1 < G::NT1) req1(tI + 1, w1[(tI + 1) & 1]);
                    SWF_WF_FENCE();
                    const u32x4 (&w)[6] = w1[tI & 1];
                    f32x16 acc = zero16;
#pragma unroll
                    for (int s2 = 0; s2 < 3; ++s2) acc = mma3(w[2 * s2], w[2 * s2 + 1], xh[s2], xl[s2], acc);
                    float e[16];
                    elu_tile(acc, vec + G::V_B1 + 16 * tI, e);
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        u32x4 hh, hl;
                        split8(e + 8 * s2, hh, hl);
                        res0 = mma3(w2[0][s2][0], w2[0][s2][1], hh, hl, res0);
                        res1 = mma3(w2[1][s2][0], w2[1][s2][1], hh, hl, res1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    const float4 b2 = *reinterpret_cast<const float4*>(vec + G::V_B2 + 4 * a);
                    if (a < 4) { res0[4 * a] += b2.x; res0[4 * a + 1] += b2.y; res0[4 * a + 2] += b2.z; res0[4 * a + 3] += b2.w; }
                    else { res1[4 * (a - 4)] += b2.x; res1[4 * (a - 4) + 1] += b2.y; res1[4 * (a - 4) + 2] += b2.z; res1[4 * (a - 4) + 3] += b2.w; }
                }
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const f32x4 v = a < 4 ? f32x4{res0[4 * a], res0[4 * a + 1], res0[4 * a + 2], res0[4 * a + 3]}
                                      : f32x4{res1[4 * (a - 4)], res1[4 * (a - 4) + 1], res1[4 * (a - 4) + 2], res1[4 * (a - 4) + 3]};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ors, tokoff, 32 * a, 0);
            }
        }
        __syncthreads();   // every wave is done with the images: the next window may overwrite them
    }
}

// ---------------------------------------------------------------------------------------------------------------
template <int HID>
__global__ __launch_bounds__(256) void pack48_kernel(WinPackArgs a) {
    using G = G48<HID>;
    const int st = blockIdx.y;
    const swf_block_stream_params& p = a.p[st];
    char* dst = a.dst[st];
    const int gtid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
    const float qscale = kLog2e / sqrtf(6.0f);   // d^-0.5 (a001:32-34) and exp -> exp2

    for (int idx = gtid; idx < G::NFRAG * 512; idx += gsz) {
        const int f = idx >> 9, lane = (idx >> 3) & 63, e = idx & 7, r = lane & 31, hf = lane >> 5;
        float val = 0.f;
        int hl;
        if (f < G::F_P) {   // Q / K / V: row (A) or column (B) = virtual channel 32T + r = 8 * head + c; k = input channel in accumulator order
            hl = f & 1;
            const int g = f >> 1, s = g % 3, T = (g / 3) & 1, m = g / 6;
            const int k = kslot(s, hf, e), head = 4 * T + (r >> 3), c = r & 7;
            const swf_linear& l = m == 0 ? p.attn.q : m == 1 ? p.attn.k : p.attn.v;
            if (c < 6 && k < 48) {
                val = pack_wgt(l, (head * 6 + c) * 48 + k);
                if (m == 0) val *= qscale;
            }
        } else if (f < G::F_W1) {   // projection: row = output channel 32To + r; k = virtual channel of O, head 0's row 6 (= 1) carries the bias
            const int g = (f - G::F_P) >> 1, ks = g & 3, To = g >> 2;
            hl = f & 1;
            const int n = 32 * To + r, v = kslot(ks, hf, e), head = v >> 3, c = v & 7;
            if (n < 48) val = c < 6 ? pack_wgt(p.attn.proj, n * 48 + head * 6 + c) : (v == 6 ? pack_bia(p.attn.proj, n) : 0.f);
        } else if (f < G::F_W2) {   // fc1 (exp2 units): row = hidden unit
            const int g = (f - G::F_W1) >> 1, s = g % 3, tI = g / 3;
            hl = f & 1;
            const int k = kslot(s, hf, e), hid = 32 * tI + r;
            if (k < 48) val = pack_wgt(p.fc1, hid * 48 + k) * kLog2e;
        } else {   // fc2 (x ln 2): row = output channel; k = hidden unit in accumulator order
            const int g = (f - G::F_W2) >> 1, u = g % G::KU, To = g / G::KU;
            hl = f & 1;
            const int n = 32 * To + r, hid = kslot(u, hf, e);
            if (n < 48) val = pack_wgt(p.fc2, n * HID + hid) * kLn2;
        }
        const bf16 hi = (bf16)val;
        reinterpret_cast<bf16*>(dst)[idx] = hl ? (bf16)(val - (float)hi) : hi;
    }
    float* vec = reinterpret_cast<float*>(dst + G::p_vec);
    for (int i = gtid; i < G::VSTREAM; i += gsz) {
        float v = 0.f;
        if (i < 2 * G::VHF) {
            const int hf = i / G::VHF, j = i % G::VHF;
            if (j < G::V_BQ) {   // 24-channel vectors: entry k = register index (tile 0: 0..15, tile 1: 16..23)
                const int which = j / 24, k = j % 24;
                const int c = k < 16 ? rho(k, hf) : 32 + rho(k - 16, hf);
                v = which == 0 ? (p.ln1.gamma ? p.ln1.gamma[c] : 1.f) : which == 1 ? (p.ln1.beta ? p.ln1.beta[c] : 0.f)
                  : which == 2 ? (p.ln2.gamma ? p.ln2.gamma[c] : 1.f) : which == 3 ? (p.ln2.beta ? p.ln2.beta[c] : 0.f) : pack_bia(p.fc2, c);
            } else if (j < G::V_B1) {   // Q / K bias in accumulator order; K's spare row 7 is the constant 1
                const int isk = j >= G::V_BK, k = (j - (isk ? G::V_BK : G::V_BQ)), T = k >> 4, vch = 32 * T + rho(k & 15, hf);
                const int head = vch >> 3, c = vch & 7;
                if (c < 6) v = isk ? pack_bia(p.attn.k, head * 6 + c) : pack_bia(p.attn.q, head * 6 + c) * qscale;
                else if (isk && c == 7) v = 1.0f;
            } else if (j < G::V_B1 + 16 * G::NT1) {
                const int k = j - G::V_B1, hid = 32 * (k >> 4) + rho(k & 15, hf);
                v = pack_bia(p.fc1, hid) * kLog2e;
            }
        } else {   // V bias by virtual channel; spare row 6 is the constant 1 (softmax denominator)
            const int vch = i - 2 * G::VHF, head = vch >> 3, c = vch & 7;
            v = c < 6 ? pack_bia(p.attn.v, head * 6 + c) : (c == 6 ? 1.0f : 0.f);
        }
        vec[i] = v;
    }
    // relative-position bias: [query block][key tile][register / 4][lane][register % 4] (MLP half: the section is never read)
    if (p.attn.bias_table) pack_rel_bias<false>(reinterpret_cast<float*>(dst + G::p_bias), p.attn.bias_table, a.ws, gtid, gsz);
}

// The level as the shared host entries see it (win_host.h).  Static LDS; 16x16 windows: 73 KB of LDS per workgroup (dynamic),
// two workgroups per CU, grid.y = stream.
struct L48 {
    static constexpr int C = 48, D = 6, HID_WIDE = 192, HID_NARROW = 96, PACK_GRID = 64, WAVES = W48_WAVES;
    static constexpr const char *name = "win48", *pack_name = "pack_win48";
    template <int HID> using G = G48<HID>;
    template <int HID>
    static void pack(dim3 grid, const WinPackArgs& a, hipStream_t stream) { hipLaunchKernelGGL((pack48_kernel<HID>), grid, dim3(256), 0, stream, a); }
    template <int HID, int WS, int MODE, bool RAW>
    static int launch(const swf_block_desc&, const WinArgs& a, int grid, hipStream_t stream, int*) {   // one kernel: nothing to report
        hipLaunchKernelGGL((window48_kernel<HID, WS, MODE, RAW>), dim3(grid), dim3(256), 0, stream, a);
        return check_launch(MODE == WIN_BLOCK ? "window48" : "window48 (half block)");
    }
    template <int HID>
    static int launch16(const WinArgs& a, int nwin, hipStream_t stream) {
        constexpr int lds = (int)G48<HID>::l_total16;
        SWF_TRY(raise_lds_limit<&window48w16_kernel<HID>>(lds, "window48w16"));
        hipLaunchKernelGGL((window48w16_kernel<HID>), dim3(std::min(nwin, num_cus()), 2), dim3(256), lds, stream, a);
        return check_launch("window48w16");
    }
};

}  // namespace

const WinLevel& win48_level() {
    static const WinLevel level = win_level<L48>();
    return level;
}

}  // namespace swf
