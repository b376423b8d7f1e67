// The "phased" attention backward (SWF_BWD_ATTN_PHASED): exact fp32, one workgroup per (window, head, stream), one thread per query /
// key as the thread family of kernels_bwd.hip, but never more than TWO operand tiles of the (window, head) in LDS, so that the
// (256-token, d = 48) tile of level 4 of `win16` fits in the 160 KB of a CU.
//
//   phase A  thread = query i.  LDS: K and V of the head ([t][DP], zero-padded), the bias table.  Registers: the thread's own q and dO
//            rows.  Three sweeps over the keys: the row maximum; the sum of the exponentials and sum_j e_ij dP_ij (-> 1 / sum and
//            D_i = sum_j p_ij dP_ij); dS_ij = p_ij (dP_ij - D_i) and dQ_i = scale sum_j dS_ij K_j.  The three statistics stay in LDS.
//   phase B  after a barrier the two tiles are reloaded with Q and dO.  Registers: the thread's own k and v rows.  thread = key j:
//            dV_j = sum_i p_ij dO_i, dK_j = scale sum_i dS_ij Q_i from the saved statistics — in one sweep over the queries, or in
//            two (dV first: it needs p and dO only; then dK, which needs dS and Q) where one sweep would not fit the register file.
//   table    d table[offset] = sum of dS over the unmasked (query, key) pairs at that offset.  At one step i of phase B the 64 keys of
//            a wave hit 64 distinct offsets, so every wave adds its dS into a private table in LDS in program order (i ascending);
//            after a barrier the private tables are summed in wave order into dtable_partial[(window, head)], which reduce_rows
//            folds as for the thread family.  No atomics, and no order that depends on timing.
//
// Scores exactly as attn_core_kernel (kernels_generic.hip): an ascending fmaf chain over the channels, dot * scale + table[...],
// masked pairs ASSIGNED -1e10f (a001:310) with no gradient through them, the same token_of / region_of.
//
// Registers are the budget that binds, not LDS: the launch bounds follow the thread count (<= 256 threads: one wave per SIMD, the
// whole register file; <= 512: 256 VGPRs; <= 1024: 128), and phase B is split where k, v, dk and dv of DP channels would not fit.
#include "kernels_bwdattn.h"

namespace swf {
namespace {

template <int DP, int NT, bool SPLIT>
__global__ __launch_bounds__(NT) void attn_bwd_phased_kernel(AttnBwdBatch batch, int ld, int B, int H, int W, int wh, int ww, int heads,
                                                              int d, int shift, float scale) {
    static_assert(DP % 4 == 0, "rows are read as float4");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const AttnBwdProb pr = batch.p[blockIdx.z];
    const int t = wh * ww, tw = 2 * ww - 1, tsz = (2 * wh - 1) * tw;
    const int nwave = blockDim.x >> 6;
    float* T0 = smem;                    // phase A: K        phase B: Q
    float* T1 = T0 + t * DP;             // phase A: V        phase B: dO
    float* tab = T1 + t * DP;
    float* mrow = tab + tsz;             // per query: max, 1 / sum, D = sum_j p_ij dP_ij
    float* linv = mrow + t;
    float* Drow = linv + t;
    float* wtab = Drow + t;              // [waves][table entries]: each wave's own sums of dS
    const int nwx = W / ww, nwy = H / wh;
    const int win = blockIdx.x, head = blockIdx.y;
    const int b = win / (nwx * nwy), wrem = win % (nwx * nwy);
    const int wy = wrem / nwx, wx = wrem % nwx;
    const int sh = shift ? wh / 2 : 0, sw = shift ? ww / 2 : 0;
    const int tid = threadIdx.x;
    auto token_of = [&](int j) -> int64_t {
        const int sy = wy * wh + j / ww, sx = wx * ww + j % ww;
        const int oy = (sy + sh) % H, ox = (sx + sw) % W;
        return ((int64_t)b * H + oy) * W + ox;
    };
    // region_of(j) = 3 region_y(j / ww) + region_x(j % ww), the two halves kept apart for the nested (row, column) loops below
    auto region_y = [&](int y) { const int sy = wy * wh + y; return ((sy >= H - wh) + (sy >= H - wh / 2)) * 3; };
    auto region_x = [&](int x) { const int sx = wx * ww + x; return (sx >= W - ww) + (sx >= W - ww / 2); };
    auto fill = [&](const float* __restrict__ A0, const float* __restrict__ A1) {
        for (int e = tid; e < t * DP; e += blockDim.x) {
            const int j = e / DP, c = e % DP;
            float a0 = 0.f, a1 = 0.f;
            if (c < d) {
                const int64_t o = token_of(j) * ld + head * d + c;
                a0 = A0[o]; a1 = A1[o];
            }
            T0[e] = a0; T1[e] = a1;
        }
    };
    const bool live = tid < t;
    const int oy_ = tid / ww, ox_ = tid % ww;                       // the thread's own token inside the window (query in A, key in B)
    const int64_t own = live ? token_of(tid) * ld + head * d : 0;
    const int rown = shift ? region_y(oy_) + region_x(ox_) : 0;
    // the thread's own row of `src` in registers, zeros beyond head_dim (every load is in bounds and unconditional: channel 0 stands in)
    auto own_row = [&](const float* __restrict__ src, float (&r)[DP]) {
#pragma unroll
        for (int c = 0; c < DP; ++c) {
            const float x = src[own + (c < d ? c : 0)];
            r[c] = (live && c < d) ? x : 0.f;
        }
    };
    const int tbase = (wh - 1) * tw + (ww - 1);                     // table[(jy - iy + wh - 1) * tw + (jx - ix + ww - 1)]

    for (int i = tid; i < tsz; i += blockDim.x) tab[i] = pr.bias_table[i];
    for (int i = tid; i < nwave * tsz; i += blockDim.x) wtab[i] = 0.f;
    fill(pr.K, pr.V);
    // ---- phase A, thread = query i ----
    {
        float q[DP], g[DP];
        own_row(pr.Q, q);
        own_row(pr.dO, g);
        __syncthreads();
        if (live) {
            const int i = tid, toff = tbase - oy_ * tw - ox_;
            auto score = [&](int j, int jy, int jx, int ry) -> float {   // exactly attn_core_kernel's score(i, j)
                const float4* kr = reinterpret_cast<const float4*>(T0 + j * DP);
                float dot = 0.f;
#pragma unroll
                for (int c = 0; c < DP / 4; ++c) {
                    const float4 kk = kr[c];
                    dot = fmaf(q[4 * c], kk.x, dot); dot = fmaf(q[4 * c + 1], kk.y, dot);
                    dot = fmaf(q[4 * c + 2], kk.z, dot); dot = fmaf(q[4 * c + 3], kk.w, dot);
                }
                float s = dot * scale + tab[toff + jy * tw + jx];
                if (shift && ry + region_x(jx) != rown) s = -1e10f;
                return s;
            };
            auto dP = [&](int j) -> float {
                const float4* vr = reinterpret_cast<const float4*>(T1 + j * DP);
                float dot = 0.f;
#pragma unroll
                for (int c = 0; c < DP / 4; ++c) {
                    const float4 vv = vr[c];
                    dot = fmaf(g[4 * c], vv.x, dot); dot = fmaf(g[4 * c + 1], vv.y, dot);
                    dot = fmaf(g[4 * c + 2], vv.z, dot); dot = fmaf(g[4 * c + 3], vv.w, dot);
                }
                return dot;
            };
            float mx = -INFINITY;
            for (int jy = 0, j = 0; jy < wh; ++jy) {
                const int ry = shift ? region_y(jy) : 0;
                for (int jx = 0; jx < ww; ++jx, ++j) mx = fmaxf(mx, score(j, jy, jx, ry));
            }
            float l = 0.f, Dn = 0.f;
            for (int jy = 0, j = 0; jy < wh; ++jy) {
                const int ry = shift ? region_y(jy) : 0;
                for (int jx = 0; jx < ww; ++jx, ++j) {
                    const float e = expf(score(j, jy, jx, ry) - mx);
                    l += e;
                    Dn = fmaf(e, dP(j), Dn);
                }
            }
            const float inv = 1.0f / l, D = Dn * inv;
            mrow[i] = mx; linv[i] = inv; Drow[i] = D;
            float dq[DP];
#pragma unroll
            for (int c = 0; c < DP; ++c) dq[c] = 0.f;
            for (int jy = 0, j = 0; jy < wh; ++jy) {
                const int ry = shift ? region_y(jy) : 0;
                for (int jx = 0; jx < ww; ++jx, ++j) {
                    // the masked scores were ASSIGNED the constant -1e10 (a001:310): no gradient flows through them (their p is 0 anyway)
                    const float p = expf(score(j, jy, jx, ry) - mx) * inv, ds = p * (dP(j) - D);
                    const float4* kr = reinterpret_cast<const float4*>(T0 + j * DP);
#pragma unroll
                    for (int c = 0; c < DP / 4; ++c) {
                        const float4 kk = kr[c];
                        dq[4 * c] = fmaf(ds, kk.x, dq[4 * c]); dq[4 * c + 1] = fmaf(ds, kk.y, dq[4 * c + 1]);
                        dq[4 * c + 2] = fmaf(ds, kk.z, dq[4 * c + 2]); dq[4 * c + 3] = fmaf(ds, kk.w, dq[4 * c + 3]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < DP; ++c)
                if (c < d) pr.dQ[own + c] = dq[c] * scale;
        }
    }
    __syncthreads();   // every query is done with K and V; the statistics are written
    fill(pr.Q, pr.dO);
    // ---- phase B, thread = key j ----
    {
        float k[DP];
        own_row(pr.K, k);
        __syncthreads();
        if (live) {
            const int toff = tbase + oy_ * tw + ox_;
            float* wt = wtab + (tid >> 6) * tsz;
            // p_ij from the saved statistics of query i; `masked` as the forward assigned it
            auto prob = [&](int i, int iy, int ix, int ry, bool& masked) -> float {
                const float4* qr = reinterpret_cast<const float4*>(T0 + i * DP);
                float dot = 0.f;
#pragma unroll
                for (int c = 0; c < DP / 4; ++c) {
                    const float4 qq = qr[c];
                    dot = fmaf(qq.x, k[4 * c], dot); dot = fmaf(qq.y, k[4 * c + 1], dot);
                    dot = fmaf(qq.z, k[4 * c + 2], dot); dot = fmaf(qq.w, k[4 * c + 3], dot);
                }
                float s = dot * scale + tab[toff - iy * tw - ix];
                masked = shift && ry + region_x(ix) != rown;
                if (masked) s = -1e10f;
                return expf(s - mrow[i]) * linv[i];
            };
            auto add_dv = [&](float (&dv)[DP], float p, int i) {
                const float4* gr = reinterpret_cast<const float4*>(T1 + i * DP);
#pragma unroll
                for (int c = 0; c < DP / 4; ++c) {
                    const float4 gg = gr[c];
                    dv[4 * c] = fmaf(p, gg.x, dv[4 * c]); dv[4 * c + 1] = fmaf(p, gg.y, dv[4 * c + 1]);
                    dv[4 * c + 2] = fmaf(p, gg.z, dv[4 * c + 2]); dv[4 * c + 3] = fmaf(p, gg.w, dv[4 * c + 3]);
                }
            };
            // dS_ij, added to dk and to the wave's own table partial (one key of the wave per offset at a given i; the waves of a
            // workgroup never share a partial, and the LDS operations of one wave complete in program order)
            auto add_dk = [&](float (&dk)[DP], const float (&v)[DP], float p, bool masked, int i, int iy, int ix) {
                const float4* gr = reinterpret_cast<const float4*>(T1 + i * DP);
                float dp = 0.f;
#pragma unroll
                for (int c = 0; c < DP / 4; ++c) {
                    const float4 gg = gr[c];
                    dp = fmaf(gg.x, v[4 * c], dp); dp = fmaf(gg.y, v[4 * c + 1], dp);
                    dp = fmaf(gg.z, v[4 * c + 2], dp); dp = fmaf(gg.w, v[4 * c + 3], dp);
                }
                const float ds = masked ? 0.f : p * (dp - Drow[i]);
                const float4* qr = reinterpret_cast<const float4*>(T0 + i * DP);
#pragma unroll
                for (int c = 0; c < DP / 4; ++c) {
                    const float4 qq = qr[c];
                    dk[4 * c] = fmaf(ds, qq.x, dk[4 * c]); dk[4 * c + 1] = fmaf(ds, qq.y, dk[4 * c + 1]);
                    dk[4 * c + 2] = fmaf(ds, qq.z, dk[4 * c + 2]); dk[4 * c + 3] = fmaf(ds, qq.w, dk[4 * c + 3]);
                }
                float* slot = wt + (toff - iy * tw - ix);
                *slot += ds;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the next step's read of the partial stays behind this write
                __builtin_amdgcn_wave_barrier();
            };
            if constexpr (!SPLIT) {
                float v[DP], dk[DP], dv[DP];
                own_row(pr.V, v);
#pragma unroll
                for (int c = 0; c < DP; ++c) { dk[c] = 0.f; dv[c] = 0.f; }
                for (int iy = 0, i = 0; iy < wh; ++iy) {
                    const int ry = shift ? region_y(iy) : 0;
                    for (int ix = 0; ix < ww; ++ix, ++i) {
                        bool masked;
                        const float p = prob(i, iy, ix, ry, masked);
                        add_dv(dv, p, i);
                        add_dk(dk, v, p, masked, i, iy, ix);
                    }
                }
#pragma unroll
                for (int c = 0; c < DP; ++c)
                    if (c < d) { pr.dK[own + c] = dk[c] * scale; pr.dV[own + c] = dv[c]; }
            } else {
                {   // dV needs p and dO only
                    float dv[DP];
#pragma unroll
                    for (int c = 0; c < DP; ++c) dv[c] = 0.f;
                    for (int iy = 0, i = 0; iy < wh; ++iy) {
                        const int ry = shift ? region_y(iy) : 0;
                        for (int ix = 0; ix < ww; ++ix, ++i) {
                            bool masked;
                            add_dv(dv, prob(i, iy, ix, ry, masked), i);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < DP; ++c)
                        if (c < d) pr.dV[own + c] = dv[c];
                }
                {   // dK needs dS and Q
                    float v[DP], dk[DP];
                    own_row(pr.V, v);
#pragma unroll
                    for (int c = 0; c < DP; ++c) dk[c] = 0.f;
                    for (int iy = 0, i = 0; iy < wh; ++iy) {
                        const int ry = shift ? region_y(iy) : 0;
                        for (int ix = 0; ix < ww; ++ix, ++i) {
                            bool masked;
                            const float p = prob(i, iy, ix, ry, masked);
                            add_dk(dk, v, p, masked, i, iy, ix);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < DP; ++c)
                        if (c < d) pr.dK[own + c] = dk[c] * scale;
                }
            }
        }
    }
    __syncthreads();
    // ---- the table gradient of the (window, head): the waves' partials in wave order ----
    float* dt = pr.dtable_partial + ((int64_t)win * heads + head) * tsz;
    for (int e = tid; e < tsz; e += blockDim.x) {
        float acc = 0.f;
        for (int w = 0; w < nwave; ++w) acc += wtab[w * tsz + e];
        dt[e] = acc;
    }
}

// phase B in two sweeps where k, v, dk and dv (4 DP floats) and the temporaries would not fit the VGPRs the launch bounds leave.
// (Resource remarks, DESIGN 6c: no scratch in any instantiation a shipped configuration or a test reaches; (64, 512) and (32, 1024) —
// windows of 257 .. ~300 tokens at head_dim > 48, 513 .. ~600 tokens at head_dim 17 .. 32 — keep 264 B / 132 B a lane of
// loop-invariant addresses there.)
constexpr bool phased_split(int dp, int nt) { return nt <= 512 ? dp > 32 : dp > 16; }
template <int DP, int NT>
int launch_phased_t(const AttnBwdBatch& batch, int nprob, int ld, int B, int H, int W, int wh, int ww, int heads, int d, int shift,
                    size_t lds, hipStream_t stream) {
    constexpr auto kernel = &attn_bwd_phased_kernel<DP, NT, phased_split(DP, NT)>;
    if (lds > 64 * 1024) SWF_TRY((raise_lds_limit<kernel>((int)kAttnBwdLdsMax, "attn_bwd (phased)")));
    const dim3 grid(B * (H / wh) * (W / ww), heads, nprob);
    hipLaunchKernelGGL(kernel, grid, dim3(cdiv(wh * ww, 64) * 64), lds, stream, batch, ld, B, H, W, wh, ww, heads, d, shift,
                       1.0f / sqrtf((float)d));
    return check_launch("attn_bwd (phased)");
}

}  // namespace

int attn_bwd_phased_width(int d) { return d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : d <= 48 ? 48 : d <= 64 ? 64 : 0; }

size_t attn_bwd_lds_phased(int wh, int ww, int dp) {
    const size_t t = (size_t)wh * ww, tsz = (size_t)(2 * wh - 1) * (2 * ww - 1), nwave = (t + 63) / 64;
    return (2 * t * dp + tsz + 3 * t + nwave * tsz) * sizeof(float);
}

int check_attn_bwd_phased_shape(const char* what, int wh, int ww, int d) {
    const int t = wh * ww, dp = attn_bwd_phased_width(d);
    if (!dp) return fail(SWF_ERR_UNSUPPORTED, "%s: attention backward: head_dim %d > 64", what, d);
    if (cdiv(t, 64) * 64 > 1024) return fail(SWF_ERR_UNSUPPORTED, "%s: attention backward: window of %d tokens > 1024", what, t);
    const size_t lds = attn_bwd_lds_phased(wh, ww, dp);
    if (lds > kAttnBwdLdsMax)
        return fail(SWF_ERR_UNSUPPORTED, "%s: phased attention backward tile (t=%d, d=%d) needs %zu B of LDS (at most %zu B)", what, t, d, lds,
                    kAttnBwdLdsMax);
    return SWF_OK;
}

int launch_attn_bwd_phased(const AttnBwdBatch& batch, int nprob, int ld, int B, int H, int W, int wh, int ww, int heads, int d, int shift,
                           swf_bwd_route* route, hipStream_t stream) {
    SWF_TRY(check_attn_bwd_phased_shape("attn_bwd", wh, ww, d));
    const int dp = attn_bwd_phased_width(d), threads = cdiv(wh * ww, 64) * 64;
    const size_t lds = attn_bwd_lds_phased(wh, ww, dp);
    if (route) route->attention = SWF_BWD_ATTN_RAN_PHASED;
#define SWF_PH(DP, NT) return launch_phased_t<DP, NT>(batch, nprob, ld, B, H, W, wh, ww, heads, d, shift, lds, stream)
#define SWF_PH_NT(DP)                        \
    do {                                     \
        if (threads <= 256) SWF_PH(DP, 256); \
        if (threads <= 512) SWF_PH(DP, 512); \
    } while (0)
    // (more than 512 threads leave 128 VGPRs and, under the LDS limit, at most 32 padded channels)
    if (dp == 4) { SWF_PH_NT(4); SWF_PH(4, 1024); }
    if (dp == 8) { SWF_PH_NT(8); SWF_PH(8, 1024); }
    if (dp == 16) { SWF_PH_NT(16); SWF_PH(16, 1024); }
    if (dp == 32) { SWF_PH_NT(32); SWF_PH(32, 1024); }
    if (dp == 48) SWF_PH_NT(48);
    if (dp == 64) SWF_PH_NT(64);
#undef SWF_PH_NT
#undef SWF_PH
    return fail(SWF_ERR_UNSUPPORTED, "attention backward (phased): no kernel for %d threads at %d padded channels", threads, dp);
}

}  // namespace swf
