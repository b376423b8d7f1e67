// C-ABI entry points of libswinfuse: argument checks, workspace carving and the composition
// of kernels into the reference's units (WindowAttention, BasicBlock halves, SelfAndCrossBlockPair,
// PatchMergingAndLinearLayer + MyPadding, final head, MyModel.forward).
#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "kernels_generic.h"
#include <cstdlib>
#include "kernels_window.h"
#include "kernels_bwd.h"
#include "kernels_dropout.h"
#include "kernels_loss.h"
#include "kernels_fidelity.h"
#include "kernels_structure.h"
#include "kernels_perception.h"
#include "kernels_comparative.h"
#include "kernels_feature.h"
#include "kernels_metrics.h"
#include "metric_frag.h"
#include "kernels_optim.h"
#include "kernels_flat.h"
#include "kernels_deep.h"
#include "kernels_patch.h"
#include "kernels_patchrr.h"
#include "kernels_deeppatch.h"
#include "kernels_mlp.h"
#include "kernels_qkvattn.h"
#include "kernels_attnproj.h"

namespace swf {

char* err_buf() {
    static thread_local char buf[512] = "";
    return buf;
}
int fail(int status, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return status;
}

static int check_attn_desc(const swf_attn_desc* d, int B, int H, int W) {
    if (!d) return fail(SWF_ERR_NULL, "desc is NULL");
    if (d->channels <= 0 || d->heads <= 0 || d->head_dim <= 0 || d->win_h <= 0 || d->win_w <= 0)
        return fail(SWF_ERR_BAD_SHAPE, "non-positive attention dims");
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "empty batch or map (%d,%d,%d)", B, H, W);
    if (H % d->win_h || W % d->win_w)
        return fail(SWF_ERR_BAD_SHAPE, "map %dx%d is not a multiple of the window %dx%d", H, W, d->win_h, d->win_w);
    return SWF_OK;
}

// room for the split-K partials of the largest fast-tier GEMM of a unit
static int64_t splitk_need(int K, int64_t nprob_m_n) {
    const int sk = gemm_splitk_for(K);
    return sk > 1 ? sk * nprob_m_n : 0;
}

// ---- generic composition -----------------------------------------------------------------
// Q/K/V projections (three GEMM problems per stream in one launch), attention core, output
// projection (+ residual).  qsrc/ksrc/vsrc are [N][C] token-major inputs per stream.
struct AttnBufs { float *qkv[2][3], *o[2], *sk, *bias16; int64_t sk_floats; };
static AttnBufs carve_attention(Carver& ws, const swf_attn_desc& d, int nstream, int64_t N, int fast) {
    const int C = d.channels, HD = d.heads * d.head_dim;
    AttnBufs b{};
    for (int s = 0; s < nstream; ++s) {
        for (int i = 0; i < 3; ++i) b.qkv[s][i] = ws.floats(N * HD);
        b.o[s] = ws.floats(N * HD);
    }
    b.sk_floats = fast ? std::max(splitk_need(C, 3 * nstream * N * HD), splitk_need(HD, nstream * N * C)) : 0;
    b.sk = fast ? ws.floats(b.sk_floats) : nullptr;
    const bool win16 = fast && attn_core_mfma16_supported(d.win_h, d.win_w, d.head_dim);
    b.bias16 = win16 ? ws.floats((int64_t)attn_core_mfma16_scratch_floats(nstream)) : nullptr;
    return b;
}

static int attention_generic(const swf_attn_desc& d, int nstream, const swf_attn_params* const* prm,
                             const float* const* qsrc, const float* const* ksrc, const float* const* vsrc,
                             const float* const* residual, float* const* out, int B, int H, int W, const AttnBufs& bufs,
                             hipStream_t stream, int fast = 0, const swf_norm* const* qnorm = nullptr,
                             const swf_norm* const* kvnorm = nullptr) {
    // qnorm / kvnorm non-null: q/k/v sources are PRE-LayerNorm tensors and the projections run with the
    // LayerNorm prologue (fast tier only)
    const int64_t N = (int64_t)B * H * W;
    const int C = d.channels, HD = d.heads * d.head_dim;
    GemmBatch gb{};
    gb.scratch = bufs.sk; gb.scratch_floats = bufs.sk_floats;
    for (int s = 0; s < nstream; ++s) {
        const swf_linear* lin[3] = {&prm[s]->q, &prm[s]->k, &prm[s]->v};
        const float* src[3] = {qsrc[s], ksrc[s], vsrc[s]};
        for (int i = 0; i < 3; ++i) gb.p[s * 3 + i] = GemmProb{src[i], lin[i]->weight, lin[i]->bias, nullptr, bufs.qkv[s][i]};
    }
    if (qnorm) {
        LnGemmBatch lb{};
        for (int s = 0; s < nstream; ++s) {
            const swf_linear* lin[3] = {&prm[s]->q, &prm[s]->k, &prm[s]->v};
            const float* src[3] = {qsrc[s], ksrc[s], vsrc[s]};
            const swf_norm* nrm[3] = {qnorm[s], kvnorm[s], kvnorm[s]};
            for (int i = 0; i < 3; ++i) lb.p[s * 3 + i] = LnGemmProb{src[i], nrm[i]->gamma, nrm[i]->beta, lin[i]->weight, lin[i]->bias, bufs.qkv[s][i]};
        }
        SWF_TRY(launch_lngemm_bf16x3(lb, nstream * 3, (int)N, HD, C, 0, stream));
    } else {
        SWF_TRY(launch_gemm(fast, gb, nstream * 3, (int)N, HD, C, C, HD, 0, stream));
    }
    if (bufs.bias16) {   // 16x16 windows
        const float* qq[2] = {bufs.qkv[0][0], bufs.qkv[1][0]};
        const float* kk[2] = {bufs.qkv[0][1], bufs.qkv[1][1]};
        const float* vv[2] = {bufs.qkv[0][2], bufs.qkv[1][2]};
        const float* tt[2] = {prm[0]->bias_table, nstream == 2 ? prm[1]->bias_table : nullptr};
        SWF_TRY(launch_attn_core_mfma16(qq, kk, vv, bufs.o, tt, nstream, HD, HD, HD, HD, B, H, W, d.heads, d.head_dim, d.shift, bufs.bias16, stream));
    } else if (fast && attn_core_mfma_supported(d.win_h, d.win_w, d.head_dim)) {
        const float* qq[2] = {bufs.qkv[0][0], bufs.qkv[1][0]};
        const float* kk[2] = {bufs.qkv[0][1], bufs.qkv[1][1]};
        const float* vv[2] = {bufs.qkv[0][2], bufs.qkv[1][2]};
        const float* tt[2] = {prm[0]->bias_table, nstream == 2 ? prm[1]->bias_table : nullptr};
        SWF_TRY(launch_attn_core_mfma(qq, kk, vv, bufs.o, tt, nstream, HD, HD, HD, HD, B, H, W, d.heads, d.head_dim, d.shift, stream, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, d.win_h));
    } else {
        AttnCoreBatch ab{};
        for (int s = 0; s < nstream; ++s) ab.p[s] = AttnCoreProb{bufs.qkv[s][0], bufs.qkv[s][1], bufs.qkv[s][2], bufs.o[s], prm[s]->bias_table};
        SWF_TRY(launch_attn_core(ab, nstream, HD, HD, HD, HD, B, H, W, d.win_h, d.win_w, d.heads, d.head_dim, d.shift, stream));
    }
    GemmBatch pb{};
    pb.scratch = bufs.sk; pb.scratch_floats = bufs.sk_floats;
    for (int s = 0; s < nstream; ++s)
        pb.p[s] = GemmProb{bufs.o[s], prm[s]->proj.weight, prm[s]->proj.bias, residual ? residual[s] : nullptr, out[s]};
    SWF_TRY(launch_gemm(fast, pb, nstream, (int)N, C, HD, HD, C, 0, stream));
    return SWF_OK;
}

// precision is not an argument of the stand-alone query: the larger of both tiers
static size_t attention_generic_ws(const swf_attn_desc& d, int nstream, int B, int H, int W) {
    Carver exact = Carver::measure(), fast = Carver::measure();
    carve_attention(exact, d, nstream, (int64_t)B * H * W, 0);
    carve_attention(fast, d, nstream, (int64_t)B * H * W, 1);
    return std::max(exact.bytes(), fast.bytes());
}

static int check_stream_params(const swf_block_stream_params* p, const char* which, bool need_attn, bool need_mlp) {
    if (!p) return fail(SWF_ERR_NULL, "%s params are NULL", which);
    if (need_attn && (!p->ln1.gamma || !p->ln1.beta || !p->attn.q.weight || !p->attn.k.weight || !p->attn.v.weight ||
                      !p->attn.proj.weight || !p->attn.bias_table))
        return fail(SWF_ERR_NULL, "%s: attention half has a NULL weight", which);
    if (need_mlp && (!p->ln2.gamma || !p->ln2.beta || !p->fc1.weight || !p->fc2.weight))
        return fail(SWF_ERR_NULL, "%s: MLP half has a NULL weight", which);
    return SWF_OK;
}

// attention half: the LayerNorm output rows (unless the fast tier folds LN1 into the projection GEMMs), then attention_generic's buffers
struct AttnHalfBufs { float* xn[2]; AttnBufs a; };
static AttnHalfBufs carve_attn_half(Carver& ws, const swf_block_desc& d, int nstream, int64_t N) {
    const int fast = d.precision == SWF_PREC_FAST;
    AttnHalfBufs b{};
    if (!(fast && lngemm_supported(d.attn.channels)))
        for (int s = 0; s < nstream; ++s) b.xn[s] = ws.floats(N * d.attn.channels);
    b.a = carve_attention(ws, d.attn, nstream, N, fast);
    return b;
}

static int attn_halfblock_generic(const swf_block_desc* desc, const swf_block_stream_params* px,
                                  const swf_block_stream_params* py, const float* x_in, const float* y_in, float* x_out,
                                  float* y_out, int B, int H, int W, Carver& ws, hipStream_t stream) {
    const int nstream = py ? 2 : 1;
    const int64_t N = (int64_t)B * H * W;
    const int C = desc->attn.channels;
    const bool cross = desc->cross && nstream == 2;   // single path ignores cross (a002:83)
    const int fast = desc->precision == SWF_PREC_FAST;
    const swf_attn_params* prm[2] = {&px->attn, py ? &py->attn : nullptr};
    const float* res[2] = {x_in, y_in};
    float* out[2] = {x_out, y_out};
    const AttnHalfBufs bufs = carve_attn_half(ws, *desc, nstream, N);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "attention half-block workspace too small (need %zu B)", ws.bytes());
    if (fast && lngemm_supported(C)) {
        // LayerNorm folded into the projection GEMMs: K and V of stream s read the OTHER stream's tokens in a
        // cross block, normalised with that stream's LayerNorm (a004:29-38 then a002:67-82)
        const float* raw[2] = {x_in, y_in};
        const swf_norm* nrm[2] = {&px->ln1, py ? &py->ln1 : nullptr};
        const float* qsrc[2] = {raw[0], raw[1]};
        const float* kvsrc[2] = {cross ? raw[1] : raw[0], cross ? raw[0] : raw[1]};
        const swf_norm* kvn[2] = {cross ? nrm[1] : nrm[0], cross ? nrm[0] : nrm[1]};
        return attention_generic(desc->attn, nstream, prm, qsrc, kvsrc, kvsrc, res, out, B, H, W, bufs.a, stream, fast, nrm, kvn);
    }
    float* const* xn = bufs.xn;
    LnBatch lb{};
    lb.p[0] = LnProb{x_in, xn[0], px->ln1.gamma, px->ln1.beta};
    if (nstream == 2) lb.p[1] = LnProb{y_in, xn[1], py->ln1.gamma, py->ln1.beta};
    SWF_TRY(launch_layernorm(lb, nstream, N, C, 0, stream));
    const float* qsrc[2] = {xn[0], xn[1]};
    const float* kvsrc[2] = {cross ? xn[1] : xn[0], cross ? xn[0] : xn[1]};
    return attention_generic(desc->attn, nstream, prm, qsrc, kvsrc, kvsrc, res, out, B, H, W, bufs.a, stream, fast);
}

struct MlpHalfBufs { float *xn[2], *hb[2], *sk; int64_t sk_floats; };
static MlpHalfBufs carve_mlp_half(Carver& ws, const swf_block_desc& d, int nstream, int64_t N) {
    const int C = d.attn.channels, hid = d.hidden;
    const int fast = d.precision == SWF_PREC_FAST;
    MlpHalfBufs b{};
    if (!(fast && lngemm_supported(C)))
        for (int s = 0; s < nstream; ++s) b.xn[s] = ws.floats(N * C);
    for (int s = 0; s < nstream; ++s) b.hb[s] = ws.floats(N * hid);
    b.sk_floats = fast ? std::max(splitk_need(C, nstream * N * hid), splitk_need(hid, nstream * N * C)) : 0;
    b.sk = fast ? ws.floats(b.sk_floats) : nullptr;
    return b;
}

static int mlp_halfblock_generic(const swf_block_desc* desc, const swf_block_stream_params* px,
                                 const swf_block_stream_params* py, const float* x_in, const float* y_in, float* x_out,
                                 float* y_out, int B, int H, int W, Carver& ws, hipStream_t stream) {
    const int nstream = py ? 2 : 1;
    const int64_t N = (int64_t)B * H * W;
    const int C = desc->attn.channels, hid = desc->hidden;
    const int fast = desc->precision == SWF_PREC_FAST;
    const bool fold_ln = fast && lngemm_supported(C);
    const MlpHalfBufs bufs = carve_mlp_half(ws, *desc, nstream, N);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "MLP half-block workspace too small (need %zu B)", ws.bytes());
    const swf_block_stream_params* pp[2] = {px, py};
    const float* res[2] = {x_in, y_in};
    float* out[2] = {x_out, y_out};
    GemmBatch g2{};
    g2.scratch = bufs.sk; g2.scratch_floats = bufs.sk_floats;
    for (int s = 0; s < nstream; ++s) g2.p[s] = GemmProb{bufs.hb[s], pp[s]->fc2.weight, pp[s]->fc2.bias, res[s], out[s]};
    if (fold_ln) {
        LnGemmBatch l1{};
        for (int s = 0; s < nstream; ++s) l1.p[s] = LnGemmProb{res[s], pp[s]->ln2.gamma, pp[s]->ln2.beta, pp[s]->fc1.weight, pp[s]->fc1.bias, bufs.hb[s]};
        SWF_TRY(launch_lngemm_bf16x3(l1, nstream, (int)N, hid, C, Act(desc->act), stream));
    } else {
        LnBatch lb{};
        lb.p[0] = LnProb{x_in, bufs.xn[0], px->ln2.gamma, px->ln2.beta};
        if (nstream == 2) lb.p[1] = LnProb{y_in, bufs.xn[1], py->ln2.gamma, py->ln2.beta};
        SWF_TRY(launch_layernorm(lb, nstream, N, C, 0, stream));
        GemmBatch g1{};
        g1.scratch = bufs.sk; g1.scratch_floats = bufs.sk_floats;
        for (int s = 0; s < nstream; ++s) g1.p[s] = GemmProb{bufs.xn[s], pp[s]->fc1.weight, pp[s]->fc1.bias, nullptr, bufs.hb[s]};
        SWF_TRY(launch_gemm(fast, g1, nstream, (int)N, hid, C, C, hid, Act(desc->act), stream));
    }
    SWF_TRY(launch_gemm(fast, g2, nstream, (int)N, C, hid, hid, C, 0, stream));
    return SWF_OK;
}

// ---- deep-level composition (fast tier, C >= 128): pre-split bf16 planes between the units ----------
// LN1 -> planes | Q/K/V GEMMs -> fp32 | MFMA attention core -> planes | proj GEMM (+x) | LN2 -> planes |
// fc1 GEMM + ELU -> planes | fc2 GEMM (+x, split-K when hidden >= 1024).  `packed_*`: pre-split weight images
// (pack_deep_block) or nullptr, in which case they are derived into the workspace on every call.
// The LN1 planes of a deep-level block sit at the START of its workspace, at offsets that depend on the token count and C only:
// whoever runs before the block on the same workspace (the previous block's MLP reduce, the previous stage's last block, the
// patch-merging kernel) can leave them there and say so through `ln1_ready`.
static void deep_ln1_planes(Carver& ws, int64_t N, int C, int nstream, bf16_raw** hi, bf16_raw** lo) {
    for (int s = 0; s < nstream; ++s) {
        hi[s] = reinterpret_cast<bf16_raw*>(ws.floats(N * C / 2));
        lo[s] = reinterpret_cast<bf16_raw*>(ws.floats(N * C / 2));
    }
}

// Every buffer of deep_block_impl.  `fused_mlp`: the fused MLP kernel runs (its hidden splits may need more reduce scratch than the GEMMs).
struct DeepBufs {
    bf16_raw *xn_hi[2], *xn_lo[2], *o_hi[2], *o_lo[2], *h_hi[2], *h_lo[2];
    bf16_raw* qkv[2][3];   // Q (bf16, pre-scaled), K (bf16), V (fp16): the attention core's operand formats
    void* wbuf[2];         // the packed weight images when the caller has none
    float *sk, *part[2][2], *x1[2];
    int64_t sk_floats;
};
static DeepBufs carve_deep_block(Carver& ws, const swf_block_desc& d, int nstream, int64_t N, bool fused_mlp) {
    const int C = d.attn.channels, HD = d.attn.heads * d.attn.head_dim, hid = d.hidden;
    auto planes = [&](int64_t n) { return reinterpret_cast<bf16_raw*>(ws.floats(n / 2)); };
    DeepBufs b{};
    deep_ln1_planes(ws, N, C, nstream, b.xn_hi, b.xn_lo);
    for (int s = 0; s < nstream; ++s) {
        b.wbuf[s] = ws.floats((int64_t)deep_block_packed_bytes(d) / 4);
        for (int i = 0; i < 3; ++i) b.qkv[s][i] = planes(N * HD);
        b.o_hi[s] = planes(N * HD); b.o_lo[s] = planes(N * HD);
        b.h_hi[s] = planes(N * hid); b.h_lo[s] = planes(N * hid);
    }
    int64_t skn = std::max((int64_t)gemm_sp_splitk_for(HD, SP_EPI_F32), (int64_t)gemm_sp_splitk_for(hid, SP_EPI_F32));
    if (fused_mlp) skn = std::max(skn, (int64_t)mlp_fused_splits(C, hid));
    b.sk_floats = skn > 1 ? skn * nstream * N * C : 0;
    b.sk = ws.floats(b.sk_floats);
    // Output projection folded into its neighbours (C = 192 levels): qkv_attn writes the two head-group partial sums of
    // O . Wp^T, the fused MLP kernel's prologue adds x + bias + both and normalises — no projection GEMM launch, O never
    // reaches HBM.  (Carved last, and by shape alone, so the LN1 planes keep their offsets from block to block.)
    if (qkvattn_supported(d) && mlp_fused_supported(C, hid) && HD == C)
        for (int s = 0; s < nstream; ++s) { b.part[0][s] = ws.floats(N * C); b.part[1][s] = ws.floats(N * C); b.x1[s] = ws.floats(N * C); }
    return b;
}
// with and without the fused MLP kernel (SWF_NO_FUSED_MLP, token count)
static size_t deep_block_ws(const swf_block_desc* d, int nstream, int B, int H, int W) {
    if (!deep_block_supported(*d)) return 0;
    Carver plain = Carver::measure(), fused = Carver::measure();
    carve_deep_block(plain, *d, nstream, (int64_t)B * H * W, false);
    carve_deep_block(fused, *d, nstream, (int64_t)B * H * W, mlp_fused_supported(d->attn.channels, d->hidden));
    return std::max(plain.bytes(), fused.bytes());
}

static size_t block_generic_ws(const swf_block_desc* d, int nstream, int B, int H, int W) {
    Carver a = Carver::measure(), m = Carver::measure();
    carve_attn_half(a, *d, nstream, (int64_t)B * H * W);
    carve_mlp_half(m, *d, nstream, (int64_t)B * H * W);
    return std::max(std::max(a.bytes(), m.bytes()), deep_block_ws(d, nstream, B, H, W));
}

static int deep_block_impl(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                           const float* x_in, const float* y_in, float* x_out, float* y_out, int B, int H, int W,
                           Carver& ws, hipStream_t stream, const void* packed_x, const void* packed_y,
                           const swf_block_stream_params* const* next_p = nullptr, bool* ln1_ready = nullptr, int* route = nullptr) {
    // `route` (or nullptr): every branch that launches ORs its flag in (swf_block_route)
    // `next_p`: stream parameters of the block that runs next on the same workspace with the same shapes (or nullptr).  When the
    // fused MLP's reduce kernel can, it also writes that block's LN1 planes; `*ln1_ready` reports it, and on entry says whether the
    // previous block did the same for this one (the planes sit at the same workspace offsets: the carve depends on shapes only).
    const bool ln1_given = ln1_ready && *ln1_ready;
    if (ln1_ready) *ln1_ready = false;
    const int nstream = py ? 2 : 1;
    const int64_t N = (int64_t)B * H * W;
    const int C = desc->attn.channels, HD = desc->attn.heads * desc->attn.head_dim, hid = desc->hidden;
    const bool cross = desc->cross && nstream == 2;
    const swf_block_stream_params* pp[2] = {px, py};
    const float* xin[2] = {x_in, y_in};
    float* xout[2] = {x_out, y_out};
    const void* pk[2] = {packed_x, packed_y};
    static const bool no_fused_mlp = debug_env("SWF_NO_FUSED_MLP") != nullptr;   // A/B switch
    const bool fused_mlp = !no_fused_mlp && mlp_fused_supported(C, hid) && N <= INT32_MAX / 2;
    const DeepBufs b = carve_deep_block(ws, *desc, nstream, N, fused_mlp);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "deep block workspace too small (need %zu B)", ws.bytes());
    static const bool no_qkvattn = debug_env("SWF_NO_QKVATTN") != nullptr;     // A/B switches
    static const bool no_projfuse = debug_env("SWF_NO_PROJFUSE") != nullptr;
    const bool fused_attn_shape = !no_qkvattn && qkvattn_supported(*desc) && N <= INT32_MAX / 256;
    // Measured: +0.5 % on the step at B=16 256x256 (16x16 maps at this level), -1.7 % at 512x512 — the extra rows the MLP prologue
    // pulls per workgroup only pay while its grid under-fills the chip.  The rule looks at the map size, never at the batch, so
    // batch shards keep taking the same path (bit-identical rows across shard sizes).
    const bool proj_fused = fused_attn_shape && fused_mlp && !no_projfuse && HD == C && (int64_t)H * W <= 256;
    DeepWeights wv[2];
    trace_block(route, SWF_BLOCK_ROUTE_DEEP);
    if (pk[0] && (nstream == 1 || pk[1])) trace_block(route, SWF_BLOCK_PREPACKED);
    for (int s = 0; s < nstream; ++s) {
        if (!pk[s]) { SWF_TRY(pack_deep_block(*desc, *pp[s], b.wbuf[s], stream)); pk[s] = b.wbuf[s]; }
        wv[s] = deep_block_views(*desc, pk[s]);
    }
    // attention half (a004:29-38 around a002:58-82)
    if (!ln1_given) {
        LnBatch l1{};
        for (int s = 0; s < nstream; ++s) l1.p[s] = LnProb{xin[s], nullptr, pp[s]->ln1.gamma, pp[s]->ln1.beta, b.xn_hi[s], b.xn_lo[s]};
        SWF_TRY(launch_layernorm(l1, nstream, N, C, 0, stream));
    } else {
        trace_block(route, SWF_BLOCK_LN1_GIVEN);
    }
    const bool fused_attn = fused_attn_shape && wv[0].qa && (nstream == 1 || wv[1].qa);
    const bool fold_proj = proj_fused && fused_attn && pp[0]->attn.proj.bias && (nstream == 1 || pp[1]->attn.proj.bias);
    if (fused_attn) {   // Q/K/V projections + window attention (+ output projection partials) in one launch
        QkvAttnArgs qa{};
        for (int s = 0; s < nstream; ++s) {
            qa.packed[s] = wv[s].qa; qa.xn_hi[s] = b.xn_hi[s]; qa.xn_lo[s] = b.xn_lo[s]; qa.o_hi[s] = b.o_hi[s]; qa.o_lo[s] = b.o_lo[s];
            if (fold_proj) { qa.part[0][s] = b.part[0][s]; qa.part[1][s] = b.part[1][s]; }
        }
        qa.B = B; qa.H = H; qa.W = W; qa.shift = desc->attn.shift; qa.cross = cross;
        SWF_TRY(launch_qkvattn(*desc, qa, nstream, stream));
        trace_block(route, SWF_BLOCK_DEEP_QKVATTN | (fold_proj ? SWF_BLOCK_DEEP_FOLD_PROJ : 0));
    }
    SpGemmBatch gq{};
    for (int s = 0; s < nstream; ++s) {
        const int kvs = cross ? 1 - s : s;   // K and V of stream s read the other stream's normalised tokens in a cross block
        const swf_linear* lin[3] = {&pp[s]->attn.q, &pp[s]->attn.k, &pp[s]->attn.v};
        const bf16_raw* wh[3] = {wv[s].q_hi, wv[s].k_hi, wv[s].v_hi};
        const bf16_raw* wl[3] = {wv[s].q_lo, wv[s].k_lo, wv[s].v_lo};
        for (int i = 0; i < 3; ++i) {
            const int src = i == 0 ? s : kvs;
            gq.p[s * 3 + i] = SpGemmProb{b.xn_hi[src], b.xn_lo[src], wh[i], wl[i], lin[i]->bias, nullptr, nullptr, b.qkv[s][i], nullptr};
        }
    }
    gq.qscale = 1.4426950408889634f / std::sqrt((float)desc->attn.head_dim);   // d^-0.5 (a001:32-34) and exp -> exp2
    const bool deep_qkv = !fused_attn && HD == C && deep_qkv_supported(*desc) && wv[0].qkvf_hi && (nstream == 1 || wv[1].qkvf_hi);
    if (deep_qkv) {   // level 4: the three projections of both streams in one launch of the rows-times-fragment-major-weights kernel
        DeepQkvArgs dq{};
        for (int s = 0; s < nstream; ++s) {
            dq.xn_hi[s] = b.xn_hi[s]; dq.xn_lo[s] = b.xn_lo[s]; dq.w_hi[s] = wv[s].qkvf_hi; dq.w_lo[s] = wv[s].qkvf_lo;
            dq.bias[s][0] = pp[s]->attn.q.bias; dq.bias[s][1] = pp[s]->attn.k.bias; dq.bias[s][2] = pp[s]->attn.v.bias;
            for (int i = 0; i < 3; ++i) dq.out[s][i] = b.qkv[s][i];
        }
        dq.qscale = gq.qscale; dq.cross = cross; dq.M = (int)N; dq.C = C; dq.schedule = desc->schedule;
        SWF_TRY(launch_deep_qkv(dq, nstream, stream));
        trace_block(route, SWF_BLOCK_DEEP_QKV);
    }
    if (!fused_attn && !deep_qkv) SWF_TRY(launch_gemm_sp(gq, 3 * nstream, (int)N, HD, C, HD, SP_EPI_QKV16, stream));
    // level 4 (C = 384): attention core + output projection + residual in one launch
    const bool attn_proj = !fused_attn && HD == C && attnproj_supported(*desc) && wv[0].pf_hi && (nstream == 1 || wv[1].pf_hi);
    if (attn_proj) {
        AttnProjArgs ap{};
        for (int s = 0; s < nstream; ++s) {
            ap.q[s] = b.qkv[s][0]; ap.k[s] = b.qkv[s][1]; ap.v[s] = b.qkv[s][2];
            ap.wp_hi[s] = wv[s].pf_hi; ap.wp_lo[s] = wv[s].pf_lo; ap.pbias[s] = pp[s]->attn.proj.bias; ap.table[s] = pp[s]->attn.bias_table;
            ap.res[s] = xin[s]; ap.out[s] = xout[s];
        }
        ap.B = B; ap.H = H; ap.W = W; ap.shift = desc->attn.shift;
        SWF_TRY(launch_attnproj(*desc, ap, nstream, stream));
        trace_block(route, SWF_BLOCK_DEEP_ATTNPROJ);
    }
    if (!fused_attn && !attn_proj) {
        const bf16_raw* qq[2] = {b.qkv[0][0], b.qkv[1][0]};
        const bf16_raw* kk[2] = {b.qkv[0][1], b.qkv[1][1]};
        const bf16_raw* vv[2] = {b.qkv[0][2], b.qkv[1][2]};
        const float* tt[2] = {pp[0]->attn.bias_table, nstream == 2 ? pp[1]->attn.bias_table : nullptr};
        if (desc->attn.win_h == 16) {
            SWF_TRY(launch_attn_core_mfma16(nullptr, nullptr, nullptr, nullptr, tt, nstream, HD, HD, HD, HD, B, H, W, desc->attn.heads,
                                            desc->attn.head_dim, desc->attn.shift, nullptr, stream, b.o_hi, b.o_lo, qq, kk, vv));
            trace_block(route, SWF_BLOCK_DEEP_CORE16);
        } else
            SWF_TRY(launch_attn_core_mfma(nullptr, nullptr, nullptr, nullptr, tt, nstream, HD, HD, HD, HD, B, H, W, desc->attn.heads,
                                          desc->attn.head_dim, desc->attn.shift, stream, b.o_hi, b.o_lo, qq, kk, vv, desc->attn.win_h));
    }
    SpGemmBatch gp{};
    gp.scratch = b.sk; gp.scratch_floats = b.sk_floats;
    for (int s = 0; s < nstream; ++s)
        gp.p[s] = SpGemmProb{b.o_hi[s], b.o_lo[s], wv[s].p_hi, wv[s].p_lo, pp[s]->attn.proj.bias, xin[s], xout[s], nullptr, nullptr};
    const bool deep_proj = !fold_proj && !attn_proj && HD == C && deep_proj_supported(*desc) && wv[0].pf_hi && (nstream == 1 || wv[1].pf_hi);
    if (deep_proj) {   // rows x fragment-major Wproj (+ bias + residual) instead of the plane GEMM
        DeepProjArgs dp{};
        for (int s = 0; s < nstream; ++s) {
            dp.o_hi[s] = b.o_hi[s]; dp.o_lo[s] = b.o_lo[s]; dp.w_hi[s] = wv[s].pf_hi; dp.w_lo[s] = wv[s].pf_lo;
            dp.bias[s] = pp[s]->attn.proj.bias; dp.res[s] = xin[s]; dp.out[s] = xout[s];
        }
        dp.M = (int)N; dp.C = C;
        SWF_TRY(launch_deep_proj(dp, nstream, stream));
        trace_block(route, SWF_BLOCK_DEEP_PROJ);
    }
    if (!fold_proj && !attn_proj && !deep_proj) SWF_TRY(launch_gemm_sp(gp, nstream, (int)N, C, HD, C, SP_EPI_F32, stream));
    // MLP half (a004:29-38 around a003:46-50)
    if (fused_mlp) {   // LN2 + fc1 + ELU + fc2 + residual in one launch (+ a fixed-order reduce over the hidden splits)
        MlpFusedDesc md{};
        for (int s = 0; s < nstream; ++s) {
            md.x[s] = fold_proj ? xin[s] : xout[s]; md.out[s] = xout[s]; md.gamma[s] = pp[s]->ln2.gamma; md.beta[s] = pp[s]->ln2.beta;
            if (fold_proj) { md.part0[s] = b.part[0][s]; md.part1[s] = b.part[1][s]; md.pbias[s] = pp[s]->attn.proj.bias; md.x1[s] = b.x1[s]; }
            md.w1_hi[s] = wv[s].w1f_hi; md.w1_lo[s] = wv[s].w1f_lo; md.w2_hi[s] = wv[s].w2f_hi; md.w2_lo[s] = wv[s].w2f_lo;
            md.b1[s] = pp[s]->fc1.bias; md.b2[s] = pp[s]->fc2.bias;
        }
        md.scratch = b.sk; md.scratch_floats = b.sk_floats; md.M = (int)N; md.C = C; md.HID = hid; md.schedule = desc->schedule;
        const bool ln_next = next_p && ln1_ready && next_p[0] && (nstream == 1 || next_p[1]) && mlp_fused_writes_ln(C, hid);
        if (ln_next)
            for (int s = 0; s < nstream; ++s) {
                md.ln_gamma[s] = next_p[s]->ln1.gamma; md.ln_beta[s] = next_p[s]->ln1.beta; md.ln_hi[s] = b.xn_hi[s]; md.ln_lo[s] = b.xn_lo[s];
            }
        trace_block(route, SWF_BLOCK_MLP_FUSED);
        SWF_TRY(launch_mlp_fused(md, nstream, stream, route));
        if (ln_next) { *ln1_ready = true; trace_block(route, SWF_BLOCK_LN1_WRITTEN); }
        return SWF_OK;
    }
    LnBatch l2{};
    for (int s = 0; s < nstream; ++s) l2.p[s] = LnProb{xout[s], nullptr, pp[s]->ln2.gamma, pp[s]->ln2.beta, b.xn_hi[s], b.xn_lo[s]};
    SWF_TRY(launch_layernorm(l2, nstream, N, C, 0, stream));
    SpGemmBatch g1{};
    for (int s = 0; s < nstream; ++s)
        g1.p[s] = SpGemmProb{b.xn_hi[s], b.xn_lo[s], wv[s].w1_hi, wv[s].w1_lo, pp[s]->fc1.bias, nullptr, nullptr, b.h_hi[s], b.h_lo[s]};
    SWF_TRY(launch_gemm_sp(g1, nstream, (int)N, hid, C, hid, SP_EPI_ELU_SPLIT, stream));
    SpGemmBatch g2{};
    g2.scratch = b.sk; g2.scratch_floats = b.sk_floats;
    for (int s = 0; s < nstream; ++s)
        g2.p[s] = SpGemmProb{b.h_hi[s], b.h_lo[s], wv[s].w2_hi, wv[s].w2_lo, pp[s]->fc2.bias, xout[s], xout[s], nullptr, nullptr};
    return launch_gemm_sp(g2, nstream, (int)N, C, hid, C, SP_EPI_F32, stream);
}

// bytes of the pre-packed weight image of ONE stream of a block (fused window kernel or deep-level GEMMs); 0 = none
static size_t block_packed_bytes(const swf_block_desc& d) {
    const size_t pb = window_block_packed_bytes(d);
    return pb ? pb : deep_block_packed_bytes(d);
}

static int check_block(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                       const float* x_in, const float* y_in, float* x_out, float* y_out, int B, int H, int W,
                       bool attn, bool mlp) {
    if (!desc) return fail(SWF_ERR_NULL, "desc is NULL");
    SWF_TRY(check_attn_desc(&desc->attn, B, H, W));
    if (mlp && desc->hidden <= 0) return fail(SWF_ERR_BAD_SHAPE, "hidden must be positive");
    SWF_TRY(check_stream_params(px, "x-stream", attn, mlp));
    if (!x_in || !x_out) return fail(SWF_ERR_NULL, "x tensors are NULL");
    if (py) {
        SWF_TRY(check_stream_params(py, "y-stream", attn, mlp));
        if (!y_in || !y_out) return fail(SWF_ERR_NULL, "y tensors are NULL with dual-path params");
    }
    return check_activation(desc->act, "block");
}

// Fused window-block route: the packed weight images of both streams (callers without pre-packed ones), then two temporary output maps
// (`tmp_out`) for a kernel that cannot run a cross block in place (window_block_out_of_place): basic_block_impl copies them to the
// outputs, block_pair4_impl ping-pongs its two cross blocks through them.
struct WindowBufs { char* packed; float *ox, *oy; };
static WindowBufs carve_window_block(Carver& ws, const swf_block_desc& d, int64_t N, bool prepacked, bool tmp_out) {
    WindowBufs b{};
    if (!prepacked) b.packed = reinterpret_cast<char*>(ws.floats((int64_t)(2 * window_block_packed_bytes(d) / 4)));
    if (tmp_out) {
        b.ox = ws.floats(2 * N * d.attn.channels);
        b.oy = b.ox ? b.ox + N * d.attn.channels : nullptr;
    }
    return b;
}
// pre-packed or not, in place or not: the route with both is the largest
static size_t window_block_ws(const swf_block_desc& d, int B, int H, int W) {
    if (!window_block_supported(d, B, H, W)) return 0;
    size_t need = 0;
    for (int route = 0; route < 4; ++route) {
        if ((route & 2) && !window_block_out_of_place(d)) continue;
        Carver m = Carver::measure();
        carve_window_block(m, d, (int64_t)B * H * W, (route & 1) != 0, (route & 2) != 0);
        need = std::max(need, m.bytes());
    }
    return need;
}

static int basic_block_impl(const swf_block_desc* desc, const swf_block_stream_params* px,
                            const swf_block_stream_params* py, const float* x_in, const float* y_in, float* x_out,
                            float* y_out, int B, int H, int W, void* workspace, size_t workspace_bytes,
                            hipStream_t stream, const void* prepacked_x = nullptr, const void* prepacked_y = nullptr,
                            const void* next_x = nullptr, const void* next_y = nullptr, size_t next_bytes = 0,
                            const swf_block_stream_params* const* next_p = nullptr, bool* ln1_ready = nullptr, int* route = nullptr) {
    // next_p / ln1_ready: see deep_block_impl; every other path ignores the planes and leaves *ln1_ready false
    // route (or nullptr; the caller zeroes it): the family and the flags of what ran, set where it is launched (swf_block_route)
    // The fused families keep ELU(alpha = 1) inside their kernels and packed images: any other activation is one more thing they do not
    // cover, and the block takes the generic family at its precision.
    const bool fused_act = act_is_default(desc->act);
    if (fused_act && desc->precision == SWF_PREC_FAST && py && window_block_supported(*desc, B, H, W)) {
        if (ln1_ready) *ln1_ready = false;
        const bool prepacked = prepacked_x && prepacked_y;   // model path: weights were packed once (swf_model_pack_weights)
        const size_t pb = window_block_packed_bytes(*desc);
        // a kernel whose workgroups read one stream while others write it (kernels_window.h) gets temporary outputs when called in place
        const size_t map_bytes = (size_t)B * H * W * desc->attn.channels * 4;
        const bool via_tmp = window_block_out_of_place(*desc) && desc->cross && (x_in == x_out || y_in == y_out || x_in == y_out || y_in == x_out);
        Carver ws(workspace, workspace_bytes);
        const WindowBufs bufs = carve_window_block(ws, *desc, (int64_t)B * H * W, prepacked, via_tmp);
        if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "fused block workspace too small (need %zu B)", ws.bytes());
        char* w = bufs.packed;
        float *ox = via_tmp ? bufs.ox : x_out, *oy = via_tmp ? bufs.oy : y_out;
        trace_block(route, SWF_BLOCK_ROUTE_WINDOW);
        if (prepacked) {
            SWF_TRY(launch_window_block(*desc, prepacked_x, prepacked_y, x_in, y_in, ox, oy, B, H, W, stream, next_x, next_y, next_bytes, route));
            trace_block(route, SWF_BLOCK_PREPACKED);
        } else {   // block-level entry: pack this block's weights into the workspace, then one fused launch
            SWF_TRY(pack_window_block(*desc, *px, *py, w, w + pb, stream));
            SWF_TRY(launch_window_block(*desc, w, w + pb, x_in, y_in, ox, oy, B, H, W, stream, nullptr, nullptr, 0, route));
        }
        if (via_tmp) {
            trace_block(route, SWF_BLOCK_VIA_TMP);
            if (hipMemcpyAsync(x_out, ox, map_bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
                hipMemcpyAsync(y_out, oy, map_bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess)
                return fail(SWF_ERR_HIP, "fused block: copy of the temporary outputs failed");
        }
        return SWF_OK;
    }
    auto aligned16 = [](const swf_block_stream_params* p) {
        if (!p) return true;
        const void* v[] = {p->ln1.gamma, p->ln1.beta, p->ln2.gamma, p->ln2.beta, p->attn.q.weight, p->attn.k.weight, p->attn.v.weight,
                           p->attn.proj.weight, p->fc1.weight, p->fc2.weight, p->attn.q.bias, p->attn.k.bias, p->attn.v.bias,
                           p->attn.proj.bias, p->fc1.bias, p->fc2.bias};
        uintptr_t bits = 0;
        for (const void* q : v) bits |= reinterpret_cast<uintptr_t>(q);
        return bits % 16 == 0;
    };
    const uintptr_t tbits = reinterpret_cast<uintptr_t>(x_in) | reinterpret_cast<uintptr_t>(y_in) | reinterpret_cast<uintptr_t>(x_out) |
                            reinterpret_cast<uintptr_t>(y_out);
    static const bool no_deep = debug_env("SWF_NO_DEEP") != nullptr;   // A/B switch for tools/profile_block.py
    if (fused_act && deep_block_supported(*desc) && !no_deep && tbits % 16 == 0 && aligned16(px) && aligned16(py)) {
        Carver ws(workspace, workspace_bytes);
        return deep_block_impl(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, ws, stream, prepacked_x, prepacked_y, next_p, ln1_ready, route);
    }
    if (ln1_ready) *ln1_ready = false;
    trace_block(route, SWF_BLOCK_ROUTE_GENERIC);
    {
        Carver ws(workspace, workspace_bytes);
        SWF_TRY(attn_halfblock_generic(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, ws, stream));
    }
    Carver ws(workspace, workspace_bytes);
    return mlp_halfblock_generic(desc, px, py, x_out, y_out, x_out, y_out, B, H, W, ws, stream);
}

// ---- patch layers -------------------------------------------------------------------------
static int pad_amount(int len, int mult) { return (mult - len % mult) % mult; }

static int merge_shapes(int H, int W, int mh, int mw, int wh, int ww, int* Hm, int* Wm, int* Ho, int* Wo) {
    if (H <= 0 || W <= 0 || mh <= 0 || mw <= 0 || wh <= 0 || ww <= 0) return fail(SWF_ERR_BAD_SHAPE, "non-positive size");
    const int ph = pad_amount(H, mh), pw = pad_amount(W, mw);
    // F.pad(reflect) requires pad < dim (a006:128 raises RuntimeError otherwise)
    if (ph >= H || pw >= W) return fail(SWF_ERR_PAD, "reflect pad (%d,%d) >= map (%d,%d) before merging", ph, pw, H, W);
    *Hm = (H + ph) / mh;
    *Wm = (W + pw) / mw;
    const int qh = pad_amount(*Hm, wh), qw = pad_amount(*Wm, ww);
    if (qh >= *Hm || qw >= *Wm)
        return fail(SWF_ERR_PAD, "Padding size should be less than the corresponding input dimension: pad (%d,%d) on a %dx%d map",
                    qh, qw, *Hm, *Wm);
    *Ho = *Hm + qh;
    *Wo = *Wm + qw;
    return SWF_OK;
}

// Packed image of ONE stream of a patch layer for the fast-tier kernels that need one: the register-resident kernel's, or the deep-level
// kernel's where that one does not cover the shape (0 bytes: neither covers it).  The model's pack and the stand-alone tier-selectable
// entries (swf_patch_*_fwd_prec) size and write their images here.
static size_t patch_image_bytes(int decoder, int Cin, int Cout, int mh, int mw) {
    const size_t rr = patch_rr_packed_bytes(decoder, Cin, Cout, mh, mw);
    return rr ? rr : deep_patch_packed_bytes(decoder, Cin, Cout, mh, mw);
}
static int pack_patch_image(int decoder, int Cin, int Cout, int mh, int mw, const swf_patch_params& p, void* dst, hipStream_t stream) {
    if (patch_rr_packed_bytes(decoder, Cin, Cout, mh, mw))
        return pack_patch_rr(decoder, Cin, Cout, mh, mw, p.conv.weight, p.conv.bias, p.ln.gamma, p.ln.beta, dst, stream);
    return pack_deep_patch(decoder, Cin, Cout, mh, mw, p.conv.weight, dst, stream);
}

// What the two impls report to a caller that asks (swf_patch_*_fwd_prec): the route that ran (swf_patch_route), set in the branch
// that runs it, and the LN1 planes that route wrote (nullptr: none).
struct PatchTrace { int route; bf16_raw *ln_hi[2], *ln_lo[2]; };
static void trace_route(PatchTrace* t, int route) { if (t) t->route = route; }

// Deep-level patch kernels: the LN1 planes of the block that runs next on this workspace (`with_ln`; at its start: deep_ln1_planes), then,
// for the column-sliced route, `row_floats` conv rows per stream (0: the whole-row route, which keeps its rows on chip).
struct DeepPatchBufs { bf16_raw *ln_hi[2], *ln_lo[2]; float* zr[2]; };
static DeepPatchBufs carve_deep_patch(Carver& ws, int nstream, bool with_ln, int64_t N_ln, int C_ln, int64_t row_floats) {
    DeepPatchBufs b{};
    if (with_ln) deep_ln1_planes(ws, N_ln, C_ln, nstream, b.ln_hi, b.ln_lo);
    for (int s = 0; s < nstream && row_floats; ++s) b.zr[s] = ws.floats(row_floats);
    return b;
}
// the kernel's LayerNorm epilogue for the block `blk` (nullptr: none)
static const DeepPatchExtra* deep_patch_ln(DeepPatchExtra& ex, const DeepPatchBufs& b, const swf_block_stream_params* const* blk, int nstream) {
    if (!blk) return nullptr;
    for (int s = 0; s < nstream; ++s) {
        ex.ln_gamma[s] = blk[s]->ln1.gamma; ex.ln_beta[s] = blk[s]->ln1.beta; ex.ln_hi[s] = b.ln_hi[s]; ex.ln_lo[s] = b.ln_lo[s];
    }
    return &ex;
}

// generic routes: gathered patches and conv rows (merge) / cropped input, conv rows and their LayerNorm (unmerge), split-K partials
struct PatchBufs { float *a[2], *z[2], *zn[2], *sk; int64_t sk_floats; };
static PatchBufs carve_merge_generic(Carver& ws, int nstream, int64_t N, int K, int Cout, int fast) {
    PatchBufs b{};
    for (int s = 0; s < nstream; ++s) { b.a[s] = ws.floats(N * K); b.z[s] = ws.floats(N * Cout); }
    b.sk_floats = fast ? splitk_need(K, nstream * N * Cout) : 0;
    b.sk = fast ? ws.floats(b.sk_floats) : nullptr;
    return b;
}
static PatchBufs carve_unmerge_generic(Carver& ws, int nstream, int64_t N, int Cin, int Kz, bool need_crop, int fast) {
    PatchBufs b{};
    for (int s = 0; s < nstream; ++s) {
        if (need_crop) b.a[s] = ws.floats(N * Cin);
        b.z[s] = ws.floats(N * Kz);
        b.zn[s] = ws.floats(N * Kz);
    }
    b.sk_floats = fast ? splitk_need(Cin, nstream * N * Kz) : 0;
    b.sk = fast ? ws.floats(b.sk_floats) : nullptr;
    return b;
}

static int patch_merge_impl(const swf_patch_params* const* p, int nstream, const float* const* in, float* const* out,
                            int B, int H, int W, int Cin, int Cout, int mh, int mw, int wh, int ww, void* workspace,
                            size_t workspace_bytes, hipStream_t stream, int fast = 0, const void* const* prr = nullptr,
                            const swf_block_stream_params* const* first_blk = nullptr, bool* ln1_ready = nullptr,
                            PatchTrace* trace = nullptr, const swf_activation& act = {}) {
    // act: a non-default activation takes the generic route at the requested precision (the fused kernels hold ELU(alpha = 1))
    // prr: per-stream packed images of the register-resident kernel (pack_patch_rr; the model path has them) or nullptr
    // first_blk / ln1_ready: the parameters of the deep-level block that runs next on this workspace; when the whole-row deep patch
    // kernel runs, it also leaves that block's LN1 planes (deep_ln1_planes) and sets *ln1_ready
    if (ln1_ready) *ln1_ready = false;
    int Hm, Wm, Ho, Wo;
    SWF_TRY(merge_shapes(H, W, mh, mw, wh, ww, &Hm, &Wm, &Ho, &Wo));
    const int64_t N = (int64_t)B * Ho * Wo;
    const int K = mh * mw * Cin;
    static const bool no_fused = debug_env("SWF_NO_FUSED_PATCH") != nullptr;   // A/B switches
    static const bool no_prr = debug_env("SWF_NO_PATCH_RR") != nullptr;
    const bool fused_act = act_is_default(act);
    const bool use_prr = fused_act && fast && !no_fused && !no_prr && prr && nstream == 2 && patch_rr_supported(0, Cin, Cout, mh, mw) &&
                         (int64_t)B * H * W * Cin < (int64_t(1) << 31);
    const bool use_dp = fused_act && fast && !no_fused && !use_prr && prr && deep_patch_supported(0, Cin, Cout, mh, mw) && (int64_t)B * H * W * Cin < (int64_t(1) << 31);
    if (use_prr || use_dp || (fused_act && fast && !no_fused && patch_fused_supported(K, Cout))) {   // one launch: gather -> conv -> LN -> ELU
        PatchFusedDesc d{};
        for (int s = 0; s < nstream; ++s) {
            d.in[s] = in[s]; d.out[s] = out[s]; d.skip[s] = nullptr;
            d.w[s] = p[s]->conv.weight; d.bias[s] = p[s]->conv.bias; d.gamma[s] = p[s]->ln.gamma; d.beta[s] = p[s]->ln.beta;
        }
        d.decoder = 0; d.B = B; d.H = H; d.W = W; d.Cin = Cin; d.mh = mh; d.mw = mw; d.Hm = Hm; d.Wm = Wm; d.Ho = Ho; d.Wo = Wo;
        d.K = K; d.N = Cout; d.Cout = Cout; d.M = N;
        if (use_prr) { trace_route(trace, SWF_PATCH_ROUTE_RR); return launch_patch_rr(d, prr, nstream, stream); }
        if (use_dp) {
            // column slices: conv rows into the workspace, then LayerNorm + ELU (+ the next block's LN1) as a second launch; else whole rows
            const bool sliced = deep_patch_raw(0, Cin, Cout, mh, mw);
            const bool with_ln = first_blk && ln1_ready && first_blk[0] && (nstream == 1 || first_blk[1]) && (sliced || workspace);
            Carver wz(workspace, workspace_bytes);
            const DeepPatchBufs b = carve_deep_patch(wz, nstream, with_ln, N, Cout, sliced ? N * Cout : 0);
            if (!wz.ok()) return fail(SWF_ERR_WORKSPACE, "patch-merge workspace too small (need %zu B)", wz.bytes());
            DeepPatchExtra ex{};
            const DeepPatchExtra* ln = deep_patch_ln(ex, b, with_ln ? first_blk : nullptr, nstream);
            trace_route(trace, sliced ? SWF_PATCH_ROUTE_DEEP_SLICED : SWF_PATCH_ROUTE_DEEP_ROW);
            if (sliced) {
                SWF_TRY(launch_deep_patch(d, prr, nstream, stream, b.zr));
                SWF_TRY(launch_deep_patch_finish(d, b.zr, nstream, stream, ln));
            } else {
                SWF_TRY(launch_deep_patch(d, prr, nstream, stream, nullptr, ln));
            }
            if (with_ln) *ln1_ready = true;
            if (with_ln && trace) for (int s = 0; s < nstream; ++s) { trace->ln_hi[s] = b.ln_hi[s]; trace->ln_lo[s] = b.ln_lo[s]; }
            return SWF_OK;
        }
        trace_route(trace, SWF_PATCH_ROUTE_FUSED);
        return launch_patch_fused(d, nstream, stream);
    }
    trace_route(trace, SWF_PATCH_ROUTE_GENERIC);
    Carver ws(workspace, workspace_bytes);
    const PatchBufs bufs = carve_merge_generic(ws, nstream, N, K, Cout, fast);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "patch-merge workspace too small (need %zu B)", ws.bytes());
    float* const *a = bufs.a, *const *z = bufs.z;
    PtrPair pp{};
    GemmBatch gb{};
    gb.scratch = bufs.sk; gb.scratch_floats = bufs.sk_floats;
    LnBatch lb{};
    for (int s = 0; s < nstream; ++s) {
        pp.in[s] = in[s]; pp.out[s] = a[s];
        gb.p[s] = GemmProb{a[s], p[s]->conv.weight, p[s]->conv.bias, nullptr, z[s]};
        lb.p[s] = LnProb{z[s], out[s], p[s]->ln.gamma, p[s]->ln.beta};
    }
    SWF_TRY(launch_merge_gather(pp, nstream, B, H, W, Cin, mh, mw, Hm, Wm, Ho, Wo, stream));
    SWF_TRY(launch_gemm(fast, gb, nstream, (int)N, Cout, K, K, Cout, 0, stream));
    return launch_layernorm(lb, nstream, N, Cout, Act(act), stream);
}

static int unmerge_shapes(int Hp, int Wp, int Hm, int Wm, int mh, int mw, int Hout, int Wout) {
    if (Hm <= 0 || Wm <= 0 || Hm > Hp || Wm > Wp) return fail(SWF_ERR_BAD_SHAPE, "crop %dx%d of %dx%d", Hm, Wm, Hp, Wp);
    if (Hout <= 0 || Wout <= 0 || Hout > Hm * mh || Wout > Wm * mw)
        return fail(SWF_ERR_BAD_SHAPE, "output %dx%d larger than the unmerged map %dx%d", Hout, Wout, Hm * mh, Wm * mw);
    return SWF_OK;
}

static int patch_unmerge_impl(const swf_patch_params* const* p, int nstream, const float* const* in,
                              const float* const* skip, float* const* out, int B, int Hp, int Wp, int Hm, int Wm, int Cin,
                              int Cout, int mh, int mw, int Hout, int Wout, void* workspace, size_t workspace_bytes,
                              hipStream_t stream, int fast = 0, const void* const* prr = nullptr, const char* warm = nullptr,
                              size_t warm_pb = 0, bool* warmed = nullptr, const swf_block_stream_params* const* next_blk = nullptr,
                              bool* ln1_ready = nullptr, PatchTrace* trace = nullptr, const swf_activation& act = {}) {
    // act: as patch_merge_impl
    // next_blk / ln1_ready: the first block of the decoder stage that runs next (a deep-level stage on this workspace): the
    // column-sliced layer's second launch also leaves that block's LN1 planes (deep_ln1_planes over the output pixels)
    if (ln1_ready) *ln1_ready = false;
    // warm / warm_pb: packed images (x, then y at + warm_pb) of the block that runs next; the whole-row deep patch kernel touches them
    // at its end and sets *warmed (the caller otherwise spends a launch on it)
    if (warmed) *warmed = false;
    SWF_TRY(unmerge_shapes(Hp, Wp, Hm, Wm, mh, mw, Hout, Wout));
    const int64_t N = (int64_t)B * Hm * Wm;
    const int Kz = mh * mw * Cout;
    const bool need_crop = (Hm != Hp) || (Wm != Wp);
    static const bool no_fused = debug_env("SWF_NO_FUSED_PATCH") != nullptr;   // A/B switches
    static const bool no_prr = debug_env("SWF_NO_PATCH_RR") != nullptr;
    const bool fused_act = act_is_default(act);
    const bool use_prr = fused_act && fast && !no_fused && !no_prr && prr && nstream == 2 && patch_rr_supported(1, Cin, Cout, mh, mw) &&
                         (int64_t)B * Hp * Wp * Cin < (int64_t(1) << 31);
    const bool use_dp = fused_act && fast && !no_fused && !use_prr && prr && deep_patch_supported(1, Cin, Cout, mh, mw) && (int64_t)B * Hp * Wp * Cin < (int64_t(1) << 31);
    if (use_prr || use_dp || (fused_act && fast && !no_fused && patch_fused_supported(Cin, Kz))) {   // one launch: crop -> conv -> LN -> scatter -> ELU (+ skip)
        PatchFusedDesc d{};
        for (int s = 0; s < nstream; ++s) {
            d.in[s] = in[s]; d.out[s] = out[s]; d.skip[s] = skip ? skip[s] : nullptr;
            d.w[s] = p[s]->conv.weight; d.bias[s] = p[s]->conv.bias; d.gamma[s] = p[s]->ln.gamma; d.beta[s] = p[s]->ln.beta;
        }
        d.decoder = 1; d.B = B; d.H = Hp; d.W = Wp; d.Cin = Cin; d.mh = mh; d.mw = mw; d.Hm = Hm; d.Wm = Wm; d.Ho = Hout; d.Wo = Wout;
        d.K = Cin; d.N = Kz; d.Cout = Cout; d.M = N;
        if (use_prr) { trace_route(trace, SWF_PATCH_ROUTE_RR); return launch_patch_rr(d, prr, nstream, stream); }
        if (use_dp && deep_patch_raw(1, Cin, Cout, mh, mw)) {   // conv over column slices, then LayerNorm + scatter + ELU (+ skip) (+ the next block's LN1)
            const bool with_ln = next_blk && ln1_ready && next_blk[0] && (nstream == 1 || next_blk[1]);
            Carver wz(workspace, workspace_bytes);
            const DeepPatchBufs b = carve_deep_patch(wz, nstream, with_ln, (int64_t)B * Hout * Wout, Cout, N * Kz);
            if (!wz.ok()) return fail(SWF_ERR_WORKSPACE, "patch-unmerge workspace too small (need %zu B)", wz.bytes());
            DeepPatchExtra ex{};
            trace_route(trace, SWF_PATCH_ROUTE_DEEP_SLICED);
            SWF_TRY(launch_deep_patch(d, prr, nstream, stream, b.zr));
            SWF_TRY(launch_deep_patch_finish(d, b.zr, nstream, stream, deep_patch_ln(ex, b, with_ln ? next_blk : nullptr, nstream)));
            if (with_ln) *ln1_ready = true;
            if (with_ln && trace) for (int s = 0; s < nstream; ++s) { trace->ln_hi[s] = b.ln_hi[s]; trace->ln_lo[s] = b.ln_lo[s]; }
            return SWF_OK;
        }
        if (use_dp) {   // whole rows: no workspace
            trace_route(trace, SWF_PATCH_ROUTE_DEEP_ROW);
            DeepPatchExtra ex{};
            if (warm && warm_pb && nstream == 2) { ex.warm[0] = warm; ex.warm[1] = warm + warm_pb; ex.warm_bytes = warm_pb; }
            SWF_TRY(launch_deep_patch(d, prr, nstream, stream, nullptr, ex.warm[0] ? &ex : nullptr));
            if (warmed && ex.warm[0]) *warmed = true;
            return SWF_OK;
        }
        trace_route(trace, SWF_PATCH_ROUTE_FUSED);
        return launch_patch_fused(d, nstream, stream);
    }
    trace_route(trace, SWF_PATCH_ROUTE_GENERIC);
    Carver ws(workspace, workspace_bytes);
    const PatchBufs bufs = carve_unmerge_generic(ws, nstream, N, Cin, Kz, need_crop, fast);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "patch-unmerge workspace too small (need %zu B)", ws.bytes());
    float* const *cr = bufs.a, *const *z = bufs.z, *const *zn = bufs.zn;
    PtrPair cp{}, sp{};
    GemmBatch gb{};
    gb.scratch = bufs.sk; gb.scratch_floats = bufs.sk_floats;
    LnBatch lb{};
    for (int s = 0; s < nstream; ++s) {
        cp.in[s] = in[s]; cp.out[s] = cr[s];
        gb.p[s] = GemmProb{need_crop ? cr[s] : in[s], p[s]->conv.weight, p[s]->conv.bias, nullptr, z[s]};
        lb.p[s] = LnProb{z[s], zn[s], p[s]->ln.gamma, p[s]->ln.beta};
        sp.in[s] = zn[s]; sp.out[s] = out[s]; sp.aux[s] = skip ? skip[s] : nullptr;
    }
    if (need_crop) SWF_TRY(launch_crop(cp, nstream, B, Hp, Wp, Hm, Wm, Cin, stream));
    SWF_TRY(launch_gemm(fast, gb, nstream, (int)N, Kz, Cin, Cin, Kz, 0, stream));
    if (ln_unmerge_scatter_supported(lb, sp, nstream, Cout, mh, mw))   // LN + depth-to-space + ELU (+ skip) in one launch
        return launch_ln_unmerge_scatter(lb, sp, nstream, B, Hm, Wm, Cout, mh, mw, Hout, Wout, stream, Act(act));
    SWF_TRY(launch_layernorm(lb, nstream, N, Kz, 0, stream));
    return launch_unmerge_scatter(sp, nstream, B, Hm, Wm, Cout, mh, mw, Hout, Wout, stream, Act(act));
}

// Every route of the two impls that the shape admits: the generic one in both tiers, and the deep-level kernels with the LN1 planes of
// the block behind them (the single-launch fused and register-resident kernels take no workspace).
static size_t merge_ws(int nstream, int B, int H, int W, int Cin, int Cout, int mh, int mw, int wh, int ww) {
    int Hm, Wm, Ho, Wo;
    if (Cin <= 0 || Cout <= 0 || merge_shapes(H, W, mh, mw, wh, ww, &Hm, &Wm, &Ho, &Wo) != SWF_OK) return 0;
    const int64_t N = (int64_t)B * Ho * Wo;
    Carver exact = Carver::measure(), fast = Carver::measure(), deep = Carver::measure();
    carve_merge_generic(exact, nstream, N, mh * mw * Cin, Cout, 0);
    carve_merge_generic(fast, nstream, N, mh * mw * Cin, Cout, 1);
    if (deep_patch_supported(0, Cin, Cout, mh, mw)) carve_deep_patch(deep, nstream, true, N, Cout, deep_patch_raw(0, Cin, Cout, mh, mw) ? N * Cout : 0);
    return std::max(std::max(exact.bytes(), fast.bytes()), deep.bytes());
}
static size_t unmerge_ws(int nstream, int B, int Hp, int Wp, int Hm, int Wm, int Cin, int Cout, int mh, int mw, int Hout, int Wout) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || mh <= 0 || mw <= 0 || Hm <= 0 || Wm <= 0 || Hm > Hp || Wm > Wp) return 0;
    const int64_t N = (int64_t)B * Hm * Wm;
    const int Kz = mh * mw * Cout;
    Carver exact = Carver::measure(), fast = Carver::measure(), deep = Carver::measure();
    carve_unmerge_generic(exact, nstream, N, Cin, Kz, Hm != Hp || Wm != Wp, 0);
    carve_unmerge_generic(fast, nstream, N, Cin, Kz, Hm != Hp || Wm != Wp, 1);
    if (deep_patch_supported(1, Cin, Cout, mh, mw) && deep_patch_raw(1, Cin, Cout, mh, mw))
        carve_deep_patch(deep, nstream, true, (int64_t)B * Hout * Wout, Cout, N * Kz);
    return std::max(std::max(exact.bytes(), fast.bytes()), deep.bytes());
}
// The stand-alone query does not know the crop (Hm x Wm of Hp x Wp) nor the output size: the maximum over the three crops that can be
// the largest, each measured with its whole unmerged map as output.  Every buffer of the unmerge carves is a multiple of Hm * Wm, and
// only a real crop adds the cropped copy, so the largest need is either no crop or the crop by one row or one column; a carve that
// stops being monotone in the kept map has to widen this list (tests/test_workspace_host.py probes other crops against it).  The
// stand-alone entry has no packed images and never takes the deep routes; they are measured all the same.
static size_t unmerge_ws_any_crop(int nstream, int B, int Hp, int Wp, int Cin, int Cout, int mh, int mw) {
    size_t need = 0;
    const int crops[3][2] = {{Hp, Wp}, {Hp - 1, Wp}, {Hp, Wp - 1}};
    for (const auto& c : crops) need = std::max(need, unmerge_ws(nstream, B, Hp, Wp, c[0], c[1], Cin, Cout, mh, mw, c[0] * mh, c[1] * mw));
    return need;
}

// ---- model layout ---------------------------------------------------------------------------
struct BlockOff { int64_t ln1g, ln1b, wq, bq, wk, bk, wv, bv, wp, bp, table, ln2g, ln2b, w1, b1, w2, b2; };
struct PatchOff { int64_t w, b, g, bt; };
struct ParamEntry { std::string name; int64_t offset, numel; };
struct ModelLayout {
    swf_model_desc desc;
    std::vector<ParamEntry> entries;
    int64_t total = 0;
    BlockOff enc_blk[SWF_MAX_LEVELS][4][2], dec_blk[SWF_MAX_LEVELS][4][2];
    PatchOff enc_patch[SWF_MAX_LEVELS][2], dec_patch[SWF_MAX_LEVELS][2];
    int64_t h_c1w, h_c1b, h_g, h_b, h_m, h_v, h_c2w, h_c2b;

    int64_t add(const std::string& name, int64_t numel) {
        const int64_t off = total;
        entries.push_back({name, off, numel});
        total += (numel + 3) / 4 * 4;   // keep every tensor 16-byte aligned
        return off;
    }
    void add_blocks(const std::string& prefix, int C, int heads, int hd, int hidden, int wh, int ww, BlockOff (*dst)[2]) {
        static const char* grp[2] = {"self_att_block.", "cross_att_block."};
        static const char* blk[2] = {"normal_window_block.", "shifted_window_block."};
        for (int g = 0; g < 2; ++g)
            for (int k = 0; k < 2; ++k)
                for (int s = 0; s < 2; ++s) {
                    const std::string p = prefix + grp[g] + blk[k];
                    const std::string st = s == 0 ? "x" : "y";
                    const std::string nl = s == 0 ? "norm_layer_1." : "norm_layer_2.";
                    const std::string wa = p + "auto_path_win_att.window_attention_" + st + ".";
                    const std::string ml = p + "auto_path_mlp.mlp_" + st;
                    BlockOff& o = dst[g * 2 + k][s];
                    const int HD = heads * hd;
                    o.ln1g = add(p + "stage_1." + nl + "weight", C);
                    o.ln1b = add(p + "stage_1." + nl + "bias", C);
                    o.wq = add(wa + "q_for_heads.weight", (int64_t)HD * C); o.bq = add(wa + "q_for_heads.bias", HD);
                    o.wk = add(wa + "k_for_heads.weight", (int64_t)HD * C); o.bk = add(wa + "k_for_heads.bias", HD);
                    o.wv = add(wa + "v_for_heads.weight", (int64_t)HD * C); o.bv = add(wa + "v_for_heads.bias", HD);
                    o.wp = add(wa + "linear_projection.weight", (int64_t)C * HD); o.bp = add(wa + "linear_projection.bias", C);
                    o.table = add(wa + "relative_position_bias_table", (int64_t)(2 * wh - 1) * (2 * ww - 1));
                    o.ln2g = add(p + "stage_2." + nl + "weight", C);
                    o.ln2b = add(p + "stage_2." + nl + "bias", C);
                    o.w1 = add(ml + "_1.weight", (int64_t)hidden * C); o.b1 = add(ml + "_1.bias", hidden);
                    o.w2 = add(ml + "_2.weight", (int64_t)C * hidden); o.b2 = add(ml + "_2.bias", C);
                }
    }
    void add_patch(const std::string& prefix, int cin, int cout, PatchOff* dst) {
        for (int s = 0; s < 2; ++s) {
            const std::string st = s == 0 ? "x" : "y";
            dst[s].w = add(prefix + "mlp_layer_" + st + ".weight", (int64_t)cin * cout);
            dst[s].b = add(prefix + "mlp_layer_" + st + ".bias", cout);
            dst[s].g = add(prefix + "layer_norm_" + st + ".weight", cout);
            dst[s].bt = add(prefix + "layer_norm_" + st + ".bias", cout);
        }
    }
    void build(const swf_model_desc& d) {
        desc = d;
        const int mm = d.merge_h * d.merge_w;
        for (int s = 0; s < d.levels; ++s) {   // encoder: [pad2, merge(.1), padW, blocks(.3)] (a013:302-311)
            const std::string e = "encoder_list." + std::to_string(s) + ".";
            add_patch(e + "1.", d.in_dims[s] * mm, d.out_dims[s], enc_patch[s]);
            add_blocks(e + "3.", d.out_dims[s], d.heads, d.head_dim[s], d.out_dims[s] * d.mlp_ratio, d.win_h, d.win_w, enc_blk[s]);
        }
        for (int j = 0; j < d.levels; ++j) {   // decoder j serves level L-1-j, module order reversed (a013:313-314)
            const int lvl = d.levels - 1 - j;
            const std::string e = "decoder_list." + std::to_string(j) + ".";
            add_blocks(e + "0.", d.out_dims[lvl], d.heads, d.head_dim[lvl], d.in_dims[lvl] * d.mlp_ratio, d.win_h, d.win_w, dec_blk[j]);
            add_patch(e + "2.", d.out_dims[lvl], d.in_dims[lvl] * mm, dec_patch[j]);
        }
        const int k2 = d.head_ksize * d.head_ksize;
        h_c1w = add("final_layer.0.weight", 2 * 2 * k2); h_c1b = add("final_layer.0.bias", 2);
        h_g = add("final_layer.1.weight", 2); h_b = add("final_layer.1.bias", 2);
        h_m = add("final_layer.1.running_mean", 2); h_v = add("final_layer.1.running_var", 2);
        h_c2w = add("final_layer.3.weight", 2 * k2); h_c2b = add("final_layer.3.bias", 1);
    }
};

static int check_model_desc(const swf_model_desc* d) {
    if (!d) return fail(SWF_ERR_NULL, "model desc is NULL");
    if (d->levels <= 0 || d->levels > SWF_MAX_LEVELS) return fail(SWF_ERR_BAD_SHAPE, "levels %d outside 1..%d", d->levels, SWF_MAX_LEVELS);
    if (d->heads <= 0 || d->mlp_ratio <= 0 || d->win_h <= 0 || d->win_w <= 0 || d->merge_h <= 0 || d->merge_w <= 0)
        return fail(SWF_ERR_BAD_SHAPE, "non-positive model dims");
    if (d->head_ksize <= 0 || d->head_ksize % 2 == 0) return fail(SWF_ERR_UNSUPPORTED, "final conv kernel must be odd");
    for (int s = 0; s < d->levels; ++s) {
        if (d->in_dims[s] <= 0 || d->out_dims[s] <= 0 || d->head_dim[s] <= 0) return fail(SWF_ERR_BAD_SHAPE, "non-positive dims at level %d", s);
        if (s > 0 && d->in_dims[s] != d->out_dims[s - 1])
            return fail(SWF_ERR_BAD_SHAPE, "in_dims[%d]=%d != out_dims[%d]=%d", s, d->in_dims[s], s - 1, d->out_dims[s - 1]);
    }
    if (d->in_dims[0] != 1) return fail(SWF_ERR_UNSUPPORTED, "in_dims[0] must be 1 (single-channel IR / Y inputs, final head takes 2 channels)");
    return check_activation(d->act, "model");
}

// Layouts are cached per descriptor; the key is a canonical copy (unused levels and struct padding
// zeroed) so that callers need not zero-initialise the struct.
static swf_model_desc canonical_desc(const swf_model_desc* d) {
    swf_model_desc c;
    std::memset(&c, 0, sizeof(c));
    c.levels = d->levels;
    for (int s = 0; s < d->levels; ++s) { c.in_dims[s] = d->in_dims[s]; c.out_dims[s] = d->out_dims[s]; c.head_dim[s] = d->head_dim[s]; }
    c.heads = d->heads; c.mlp_ratio = d->mlp_ratio;
    c.win_h = d->win_h; c.win_w = d->win_w; c.merge_h = d->merge_h; c.merge_w = d->merge_w;
    c.head_ksize = d->head_ksize;
    c.precision = 0;   // the parameter layout depends on neither the arithmetic mode nor the activation
    return c;
}

static const ModelLayout* get_layout(const swf_model_desc* d_in) {
    const swf_model_desc canon = canonical_desc(d_in);
    const swf_model_desc* d = &canon;
    static std::mutex mu;
    static std::vector<ModelLayout*> cache;
    std::lock_guard<std::mutex> lock(mu);
    for (ModelLayout* l : cache)
        if (std::memcmp(&l->desc, d, sizeof(*d)) == 0) return l;
    ModelLayout* l = new ModelLayout();
    l->build(*d);
    cache.push_back(l);
    return l;
}

static swf_block_stream_params make_stream_params(const float* a, const BlockOff& o) {
    swf_block_stream_params p;
    p.ln1 = {a + o.ln1g, a + o.ln1b};
    p.attn.q = {a + o.wq, a + o.bq}; p.attn.k = {a + o.wk, a + o.bk}; p.attn.v = {a + o.wv, a + o.bv};
    p.attn.proj = {a + o.wp, a + o.bp}; p.attn.bias_table = a + o.table;
    p.ln2 = {a + o.ln2g, a + o.ln2b};
    p.fc1 = {a + o.w1, a + o.b1}; p.fc2 = {a + o.w2, a + o.b2};
    return p;
}

struct LevelShape { int Hin, Win, Hm, Wm, Ho, Wo; };

static int model_shapes(const swf_model_desc* d, int H, int W, LevelShape* ls) {
    int h = H, w = W;
    for (int s = 0; s < d->levels; ++s) {
        ls[s].Hin = h; ls[s].Win = w;
        SWF_TRY(merge_shapes(h, w, d->merge_h, d->merge_w, d->win_h, d->win_w, &ls[s].Hm, &ls[s].Wm, &ls[s].Ho, &ls[s].Wo));
        h = ls[s].Ho; w = ls[s].Wo;
    }
    if (d->head_ksize / 2 >= H || d->head_ksize / 2 >= W) return fail(SWF_ERR_PAD, "final conv reflect pad >= image");
    return SWF_OK;
}

static swf_block_desc level_block_desc(const swf_model_desc* d, int lvl, bool encoder) {
    swf_block_desc b;
    b.attn.channels = d->out_dims[lvl];
    b.attn.heads = d->heads;
    b.attn.head_dim = d->head_dim[lvl];
    b.attn.win_h = d->win_h; b.attn.win_w = d->win_w;
    b.attn.shift = 0;
    b.hidden = (encoder ? d->out_dims[lvl] : d->in_dims[lvl]) * d->mlp_ratio;
    b.cross = 0;
    b.precision = d->precision;
    b.schedule = d->schedule;
    b.act = d->act;
    return b;
}

// `packed`: nullptr, or the 8 packed weight images of the stage laid out [block 0..3][stream x,y] at a
// stride of window_block_packed_bytes(desc)
static int block_pair4_impl(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                            const float* x_in, const float* y_in, float* x_out, float* y_out, int B, int H, int W,
                            void* workspace, size_t workspace_bytes, hipStream_t stream, const char* packed = nullptr,
                            const char* after = nullptr, size_t after_pb = 0, int32_t* equal_flags = nullptr,
                            const swf_block_stream_params* const* stage_next = nullptr, bool* ln1_io = nullptr, int32_t* routes = nullptr) {
    // `routes` (host, 4 entries, or nullptr): the swf_block_route of each block
    // `stage_next` / `ln1_io` (deep levels): the first block's parameters of the stage that runs next on the same workspace with the
    // same map (the decoder stage behind the deepest encoder stage), so that this stage's last MLP reduce leaves that block's LN1
    // planes; *ln1_io says on entry whether this stage's first block finds its planes in place, on return whether the next does
    // `equal_flags` (device, 2 entries pre-set to 1, or nullptr): cleared when the inputs of the stage's two cross blocks
    // differ somewhere — the reference's first-forward check `(x == y).all()` (a005:111-118)
    // `after`: packed images (x, then y at + after_pb) of the first block of the NEXT stage when that is a fused-kernel stage
    // too: the last block of this stage warms them
    const float* xi = x_in;
    const float* yi = y_in;
    const size_t pb = packed ? block_packed_bytes(*desc) : 0;
    bool ln1_ready = ln1_io ? *ln1_io : false;   // deep levels: block i's MLP reduce also writes block i+1's LN1 planes
    // Kernels that cannot run a cross block in place (window_block_out_of_place): the two cross blocks ping-pong through two
    // temporary maps of carve_window_block (block 2: maps -> temporaries, block 3: temporaries -> outputs) instead of
    // each going through basic_block_impl's temporary-and-copy route
    float *tx = nullptr, *ty = nullptr;
    size_t ws_left = workspace_bytes;
    {
        swf_block_desc dc = *desc;
        dc.cross = 1;
        if (act_is_default(dc.act) && desc->precision == SWF_PREC_FAST && py && window_block_supported(dc, B, H, W) && window_block_out_of_place(dc)) {
            Carver ws(workspace, workspace_bytes);
            const WindowBufs bufs = carve_window_block(ws, dc, (int64_t)B * H * W, packed != nullptr, true);
            if (workspace && ws.ok()) {   // (otherwise each cross block takes basic_block_impl's temporary-and-copy route, or fails there)
                tx = bufs.ox; ty = bufs.oy;
                // The blocks themselves get what lies before the maps, i.e. room for their packed images and nothing else.  That is
                // all they carve: window_block_supported ignores cross and shift, so all four blocks of the stage take the fused route,
                // none of them in place.  A block that could fall back to the deep or generic route here would have to be measured in.
                ws_left = reinterpret_cast<char*>(tx) - static_cast<char*>(workspace);
            }
        }
    }
    for (int i = 0; i < 4; ++i) {
        swf_block_desc d = *desc;
        d.cross = i >= 2;          // self pair first, then cross pair (a012:72-73)
        d.attn.shift = i & 1;      // normal window, then shifted window (a009:102-105)
        const void* pkx = (packed && pb) ? packed + (size_t)(2 * i) * pb : nullptr;
        const void* pky = (packed && pb) ? packed + (size_t)(2 * i + 1) * pb : nullptr;
        const void* nkx = (packed && pb && i < 3) ? packed + (size_t)(2 * i + 2) * pb : (i == 3 ? after : nullptr);   // next block: warmed in L2
        const void* nky = (packed && pb && i < 3) ? packed + (size_t)(2 * i + 3) * pb : (i == 3 && after ? after + after_pb : nullptr);
        const swf_block_stream_params* nxt[2] = {i < 3 ? &px[i + 1] : nullptr, (i < 3 && py) ? &py[i + 1] : nullptr};
        const bool chain_out = i == 3 && stage_next && stage_next[0] && (!py || stage_next[1]);
        if (chain_out) { nxt[0] = stage_next[0]; nxt[1] = py ? stage_next[1] : nullptr; }
        if (equal_flags && d.cross && py)
            SWF_TRY(launch_all_equal(xi, yi, (int64_t)B * H * W * desc->attn.channels, equal_flags + (i - 2), stream));
        float* xo = (tx && i == 2) ? tx : x_out;
        float* yo = (tx && i == 2) ? ty : y_out;
        int route = 0;
        SWF_TRY(basic_block_impl(&d, &px[i], py ? &py[i] : nullptr, xi, yi, xo, yo, B, H, W, workspace, tx ? ws_left : workspace_bytes, stream, pkx, pky,
                                 nkx, nky, i == 3 ? after_pb : 0, (i < 3 || chain_out) ? nxt : nullptr, &ln1_ready, routes ? &route : nullptr));
        if (tx && i >= 2) trace_block(&route, SWF_BLOCK_VIA_TMP);   // block 2 wrote the temporaries, block 3 read them
        if (routes) routes[i] = route;
        xi = xo; yi = yo;
    }
    if (ln1_io) *ln1_io = ln1_ready;
    return SWF_OK;
}

// byte offset of each stage's packed images inside the model-level packed buffer (encoder stages first)
struct PackedPlan {
    size_t enc[SWF_MAX_LEVELS], dec[SWF_MAX_LEVELS], total;
    bool enc_on[SWF_MAX_LEVELS], dec_on[SWF_MAX_LEVELS];
    // patch layers (register-resident kernel, or the deep-level kernel where that one does not cover the shape): two per-stream
    // images of penc_b / pdec_b bytes each, 0 = layer not covered
    size_t penc[SWF_MAX_LEVELS], pdec[SWF_MAX_LEVELS], penc_b[SWF_MAX_LEVELS], pdec_b[SWF_MAX_LEVELS];
};
static PackedPlan packed_plan(const swf_model_desc* d) {
    PackedPlan p{};
    size_t off = 0;
    for (int s = 0; s < d->levels; ++s) {
        swf_block_desc be = level_block_desc(d, s, true);
        be.precision = SWF_PREC_FAST;
        const size_t pb = block_packed_bytes(be);
        p.enc_on[s] = pb > 0; p.enc[s] = off; off += 8 * pb;
    }
    for (int j = 0; j < d->levels; ++j) {
        swf_block_desc bd = level_block_desc(d, d->levels - 1 - j, false);
        bd.precision = SWF_PREC_FAST;
        const size_t pb = block_packed_bytes(bd);
        p.dec_on[j] = pb > 0; p.dec[j] = off; off += 8 * pb;
    }
    for (int s = 0; s < d->levels; ++s) {
        p.penc_b[s] = patch_image_bytes(0, d->in_dims[s], d->out_dims[s], d->merge_h, d->merge_w);
        p.penc[s] = off; off += 2 * p.penc_b[s];
    }
    for (int j = 0; j < d->levels; ++j) {
        const int lvl = d->levels - 1 - j;
        p.pdec_b[j] = patch_image_bytes(1, d->out_dims[lvl], d->in_dims[lvl], d->merge_h, d->merge_w);
        p.pdec[j] = off; off += 2 * p.pdec_b[j];
    }
    p.total = off;
    return p;
}

}  // namespace swf

using namespace swf;

extern "C" {

int swf_version(void) { return SWF_VERSION_MAJOR * 1000 + SWF_VERSION_MINOR; }
const char* swf_last_error_string(void) { return err_buf(); }
const char* swf_status_string(int status) {
    switch (status) {
        case SWF_OK: return "ok";
        case SWF_ERR_NULL: return "null pointer";
        case SWF_ERR_BAD_SHAPE: return "bad shape";
        case SWF_ERR_PAD: return "reflect padding >= dimension";
        case SWF_ERR_UNSUPPORTED: return "unsupported configuration";
        case SWF_ERR_WORKSPACE: return "workspace too small";
        case SWF_ERR_HIP: return "HIP error";
        default: return "unknown status";
    }
}

// ---- fast tier of the stand-alone module entries at level-0 width (C = 24): the block kernel with the other half compiled out ----
// (levels 0-2: C = 24 / 48 / 96, 8 heads of C / 8, 8x8 or 7x7 windows; hidden widths of the encoder / decoder blocks)
// the packed images of both streams of a half-block kernel (0 bytes where no kernel covers the width)
static char* carve_window_half(Carver& ws, int C, int hid) { return reinterpret_cast<char*>(ws.floats((int64_t)(2 * window_half_packed_bytes(C, hid) / 4))); }
// ... at the start of a workspace, or nullptr when it has no room for them (the caller then takes its generic route)
static char* window_half_images(void* workspace, size_t workspace_bytes, int C, int hid) {
    Carver ws(workspace, workspace_bytes);
    char* pk = carve_window_half(ws, C, hid);
    return ws.ok() ? pk : nullptr;
}
static size_t window_half_ws(int C, int hid) {
    Carver m = Carver::measure();
    carve_window_half(m, C, hid);
    return m.bytes();
}
static bool half_attn_shape(const swf_attn_desc& a, int H, int W) {
    return (a.channels == 24 || a.channels == 48 || a.channels == 96) && a.heads == 8 && a.head_dim * 8 == a.channels && a.win_h == a.win_w &&
           (a.win_h == 8 || a.win_h == 7) && H % a.win_h == 0 && W % a.win_w == 0;
}
static int half_attn_hidden(int C) { return 4 * C; }   // the attention half runs on the wide-MLP image layout (fc sections unused)

// MLP half on window24 / window48 / window96_kernel <HID, 8, MLP half, raw>: tokens as flat lists.  Dual path: one list per stream.  Single path: the one
// list is split between the kernel's two stream slots (same weights).  SWF_ERR_UNSUPPORTED = shape not covered (the caller falls back).
static int mlp_half24(int C, int hid, int raw, const swf_block_stream_params* px, const swf_block_stream_params* py, const float* x_in,
                      const float* y_in, float* x_out, float* y_out, int64_t N, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const size_t pb = window_half_packed_bytes(C, hid);
    char* pk = window_half_images(workspace, workspace_bytes, C, hid);
    if (!pb || N <= 0 || N * C * 4 >= (int64_t(1) << 31) || !pk) return SWF_ERR_UNSUPPORTED;
    swf_block_desc bd{};
    bd.attn = swf_attn_desc{C, 8, C / 8, 8, 8, 0};
    bd.hidden = hid; bd.cross = 0; bd.precision = SWF_PREC_FAST;
    swf_block_stream_params sx = *px, sy = py ? *py : *px;
    sx.attn = swf_attn_params{}; sy.attn = swf_attn_params{};
    sx.ln1 = sy.ln1 = swf_norm{nullptr, nullptr};
    if (raw) sx.ln2 = sy.ln2 = swf_norm{nullptr, nullptr};
    SWF_TRY(pack_window_half(bd, sx, sy, pk, pb, stream));
    if (py) return launch_window_half(bd, WIN_MLP, raw, pk, pb, x_in, y_in, x_out, y_out, 1, 1, 1, (int)N, (int)N, stream);
    const int64_t n0 = std::min<int64_t>(N, ((N + 1) / 2 + 63) / 64 * 64);
    return launch_window_half(bd, WIN_MLP, raw, pk, pb, x_in, x_in + n0 * C, x_out, x_out + n0 * C, 1, 1, 1, (int)n0, (int)(N - n0), stream);
}

size_t swf_window_attention_workspace_bytes(const swf_attn_desc* desc, int32_t B, int32_t H, int32_t W) {
    if (!desc || B <= 0 || H <= 0 || W <= 0) return 0;
    return std::max(attention_generic_ws(*desc, 1, B, H, W), window_half_ws(desc->channels, half_attn_hidden(desc->channels)));
}

static int window_attention_impl(const swf_attn_desc* desc, int precision, const swf_attn_params* p, const float* q, const float* k,
                                 const float* v, const float* residual, float* out, int32_t B, int32_t H, int32_t W,
                                 void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_attn_desc(desc, B, H, W));
    if (precision != SWF_PREC_FP32 && precision != SWF_PREC_FAST) return fail(SWF_ERR_BAD_SHAPE, "window_attention: unknown precision %d", precision);
    if (!p || !q || !k || !v || !out) return fail(SWF_ERR_NULL, "window_attention: NULL tensor or params");
    if (!p->q.weight || !p->k.weight || !p->v.weight || !p->proj.weight || !p->bias_table)
        return fail(SWF_ERR_NULL, "window_attention: NULL weight");
    const int hid_a = half_attn_hidden(desc->channels);
    const size_t pbh = window_half_packed_bytes(desc->channels, hid_a);
    char* pk = window_half_images(workspace, workspace_bytes, desc->channels, hid_a);
    if (precision == SWF_PREC_FAST && k == v && !residual && half_attn_shape(*desc, H, W) && (int64_t)B * H * W * desc->channels * 4 < (int64_t(1) << 31) &&
        pbh && pk && out != q && out != k) {
        // window24/48_kernel<.., attention half, RAW>: stream 0 = the queries and the output, stream 1 = the key / value tensor
        swf_block_desc bd{*desc, hid_a, 1, SWF_PREC_FAST};
        swf_block_stream_params sp{};
        sp.attn = *p;
        SWF_TRY(pack_window_half(bd, sp, sp, pk, pbh, as_stream(stream)));
        return launch_window_half(bd, WIN_ATTN, 1, pk, pbh, q, k, out, nullptr, B, H, W, 0, 0, as_stream(stream));
    }
    Carver ws(workspace, workspace_bytes);
    const swf_attn_params* prm[2] = {p, nullptr};
    const float* qs[2] = {q, nullptr};
    const float* ks[2] = {k, nullptr};
    const float* vs[2] = {v, nullptr};
    const float* rs[2] = {residual, nullptr};
    float* os[2] = {out, nullptr};
    const int fast = precision == SWF_PREC_FAST ? 1 : 0;
    const AttnBufs bufs = carve_attention(ws, *desc, 1, (int64_t)B * H * W, fast);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "attention workspace too small (need %zu B)", ws.bytes());
    return attention_generic(*desc, 1, prm, qs, ks, vs, residual ? rs : nullptr, os, B, H, W, bufs, as_stream(stream), fast);
}

int swf_window_attention_fwd(const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k,
                             const float* v, const float* residual, float* out, int32_t B, int32_t H, int32_t W,
                             void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return window_attention_impl(desc, SWF_PREC_FP32, p, q, k, v, residual, out, B, H, W, workspace, workspace_bytes, stream);
}

int swf_window_attention_fwd_prec(const swf_attn_desc* desc, int32_t precision, const swf_attn_params* p, const float* q, const float* k,
                                  const float* v, const float* residual, float* out, int32_t B, int32_t H, int32_t W,
                                  void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return window_attention_impl(desc, precision, p, q, k, v, residual, out, B, H, W, workspace, workspace_bytes, stream);
}

size_t swf_basic_block_workspace_bytes(const swf_block_desc* desc, int32_t B, int32_t H, int32_t W) {
    if (!desc || B <= 0 || H <= 0 || W <= 0) return 0;
    return std::max(std::max(block_generic_ws(desc, 2, B, H, W), window_block_ws(*desc, B, H, W)),
                    std::max(window_half_ws(desc->attn.channels, half_attn_hidden(desc->attn.channels)), window_half_ws(desc->attn.channels, desc->hidden)));
}

int swf_attn_halfblock_fwd(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                           const float* x_in, const float* y_in, float* x_out, float* y_out, int32_t B, int32_t H, int32_t W,
                           void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_block(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, true, false));
    const int hid_a = half_attn_hidden(desc->attn.channels);
    const size_t pbh = window_half_packed_bytes(desc->attn.channels, hid_a);
    char* pk = window_half_images(workspace, workspace_bytes, desc->attn.channels, hid_a);
    if (desc->precision == SWF_PREC_FAST && half_attn_shape(desc->attn, H, W) && (int64_t)B * H * W * desc->attn.channels * 4 < (int64_t(1) << 31) &&
        pbh && pk) {
        // window24/48_kernel<.., attention half>: LN1 + Q/K/V + attention + projection + residual of both streams in one launch.  A single-path
        // block runs its stream as stream 0; stream 1 mirrors it with its stores dropped.
        swf_block_desc bd = *desc;
        bd.hidden = hid_a;
        bd.cross = desc->cross && py;   // a single path ignores cross (a002:83)
        swf_block_stream_params sx = *px, sy = py ? *py : *px;
        sx.fc1 = sx.fc2 = swf_linear{nullptr, nullptr}; sy.fc1 = sy.fc2 = swf_linear{nullptr, nullptr};
        sx.ln2 = sy.ln2 = swf_norm{nullptr, nullptr};
        SWF_TRY(pack_window_half(bd, sx, sy, pk, pbh, as_stream(stream)));
        return launch_window_half(bd, WIN_ATTN, 0, pk, pbh, x_in, py ? y_in : x_in, x_out, py ? y_out : nullptr, B, H, W, 0, 0, as_stream(stream));
    }
    Carver ws(workspace, workspace_bytes);
    return attn_halfblock_generic(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, ws, as_stream(stream));
}

int swf_mlp_halfblock_fwd(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                          const float* x_in, const float* y_in, float* x_out, float* y_out, int32_t B, int32_t H, int32_t W,
                          void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_block(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, false, true));
    if (desc->precision == SWF_PREC_FAST && act_is_default(desc->act)) {
        const int st = mlp_half24(desc->attn.channels, desc->hidden, 0, px, py, x_in, y_in, x_out, y_out, (int64_t)B * H * W, workspace, workspace_bytes,
                                  as_stream(stream));
        if (st != SWF_ERR_UNSUPPORTED) return st;
    }
    Carver ws(workspace, workspace_bytes);
    return mlp_halfblock_generic(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, ws, as_stream(stream));
}

// generic MLP: the hidden activations, then the scratch of the two linear layers (they run one after the other)
struct MlpBufs { float *hid, *rest; size_t rest_bytes; };
static MlpBufs carve_mlp(Carver& ws, int32_t precision, int64_t tokens, int32_t channels, int32_t hidden) {
    MlpBufs b{};
    b.hid = ws.floats(tokens * hidden);
    b.rest_bytes = std::max(swf_linear_workspace_bytes(precision, tokens, channels, hidden), swf_linear_workspace_bytes(precision, tokens, hidden, channels));
    b.rest = ws.floats((int64_t)(b.rest_bytes / 4));
    return b;
}

size_t swf_mlp_workspace_bytes(int32_t precision, int64_t tokens, int32_t channels, int32_t hidden) {
    if (tokens <= 0 || channels <= 0 || hidden <= 0) return 0;
    Carver m = Carver::measure();
    carve_mlp(m, precision, tokens, channels, hidden);
    return std::max(m.bytes(), window_half_ws(channels, hidden));
}

int swf_mlp_fwd_act(const swf_activation* act_, int32_t precision, const swf_block_stream_params* px, const swf_block_stream_params* py,
                    const float* x_in, const float* y_in, float* x_out, float* y_out, int64_t tokens, int32_t channels, int32_t hidden,
                    void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    const swf_activation act = act_or_default(act_);
    if (precision != SWF_PREC_FP32 && precision != SWF_PREC_FAST) return fail(SWF_ERR_BAD_SHAPE, "mlp: unknown precision %d", precision);
    if (!px || !px->fc1.weight || !px->fc2.weight || !x_in || !x_out) return fail(SWF_ERR_NULL, "mlp: NULL argument");
    if (py && (!py->fc1.weight || !py->fc2.weight || !y_in || !y_out)) return fail(SWF_ERR_NULL, "mlp: NULL y-stream argument");
    if (tokens <= 0 || tokens > INT32_MAX || channels <= 0 || hidden <= 0) return fail(SWF_ERR_BAD_SHAPE, "mlp: bad sizes");
    SWF_TRY(check_activation(act, "mlp"));
    if (precision == SWF_PREC_FAST && act_is_default(act)) {
        const int st = mlp_half24(channels, hidden, 1, px, py, x_in, y_in, x_out, y_out, tokens, workspace, workspace_bytes, as_stream(stream));
        if (st != SWF_ERR_UNSUPPORTED) return st;
    }
    // two linear layers per stream through the hidden activations in the workspace
    Carver ws(workspace, workspace_bytes);
    const MlpBufs bufs = carve_mlp(ws, precision, tokens, channels, hidden);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "mlp: workspace too small (need %zu B)", ws.bytes());
    float *hid = bufs.hid, *rest = bufs.rest;
    const size_t rest_bytes = bufs.rest_bytes;
    const swf_block_stream_params* pp[2] = {px, py};
    const float* in[2] = {x_in, y_in};
    float* out[2] = {x_out, y_out};
    for (int s = 0; s < (py ? 2 : 1); ++s) {
        SWF_TRY(swf_linear_fwd_prec_act(&act, &pp[s]->fc1, precision, in[s], nullptr, hid, tokens, channels, hidden, 1, rest, rest_bytes, stream));
        SWF_TRY(swf_linear_fwd_prec(&pp[s]->fc2, precision, hid, nullptr, out[s], tokens, hidden, channels, 0, rest, rest_bytes, stream));
    }
    return SWF_OK;
}
int swf_mlp_fwd(int32_t precision, const swf_block_stream_params* px, const swf_block_stream_params* py, const float* x_in, const float* y_in,
                float* x_out, float* y_out, int64_t tokens, int32_t channels, int32_t hidden, void* workspace, size_t workspace_bytes,
                swf_stream_t stream) {
    return swf_mlp_fwd_act(nullptr, precision, px, py, x_in, y_in, x_out, y_out, tokens, channels, hidden, workspace, workspace_bytes, stream);
}

int swf_basic_block_fwd(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                        const float* x_in, const float* y_in, float* x_out, float* y_out, int32_t B, int32_t H, int32_t W,
                        void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_block(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, true, true));
    return basic_block_impl(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, workspace, workspace_bytes, as_stream(stream));
}

int swf_basic_block_fwd_route(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                              const float* x_in, const float* y_in, float* x_out, float* y_out, int32_t B, int32_t H, int32_t W,
                              int32_t* route, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_block(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, true, true));
    int r = 0;
    SWF_TRY(basic_block_impl(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, workspace, workspace_bytes, as_stream(stream), nullptr, nullptr,
                             nullptr, nullptr, 0, nullptr, nullptr, &r));
    if (route) *route = r;
    return SWF_OK;
}

size_t swf_basic_block_packed_bytes(const swf_block_desc* desc) {
    if (!desc || desc->precision != SWF_PREC_FAST || !act_is_default(desc->act)) return 0;
    return 2 * window_block_packed_bytes(*desc);
}

int swf_basic_block_pack(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                         void* packed, size_t packed_bytes, swf_stream_t stream) {
    if (!desc) return fail(SWF_ERR_NULL, "desc is NULL");
    SWF_TRY(check_stream_params(px, "x-stream", true, true));
    SWF_TRY(check_stream_params(py, "y-stream", true, true));
    const size_t pb = window_block_packed_bytes(*desc);
    if (pb == 0 || desc->precision != SWF_PREC_FAST || !act_is_default(desc->act))
        return fail(SWF_ERR_UNSUPPORTED, "no fused kernel for C=%d hidden=%d activation kind %d", desc->attn.channels, desc->hidden, desc->act.kind);
    if (!packed || packed_bytes < 2 * pb) return fail(SWF_ERR_WORKSPACE, "packed buffer too small (need %zu B)", 2 * pb);
    return pack_window_block(*desc, *px, *py, packed, static_cast<char*>(packed) + pb, as_stream(stream));
}

int swf_basic_block_fwd_packed(const swf_block_desc* desc, const void* packed, const float* x_in, const float* y_in,
                               float* x_out, float* y_out, int32_t B, int32_t H, int32_t W, swf_stream_t stream) {
    if (!desc || !packed || !x_in || !y_in || !x_out || !y_out) return fail(SWF_ERR_NULL, "basic_block_fwd_packed: NULL argument");
    SWF_TRY(check_attn_desc(&desc->attn, B, H, W));
    if (!window_block_supported(*desc, B, H, W) || !act_is_default(desc->act)) return fail(SWF_ERR_UNSUPPORTED, "no fused kernel for this block shape and activation");
    const size_t pb = window_block_packed_bytes(*desc);
    return launch_window_block(*desc, packed, static_cast<const char*>(packed) + pb, x_in, y_in, x_out, y_out, B, H, W, as_stream(stream));
}

size_t swf_basic_block_bwd_workspace_bytes(const swf_block_desc* desc, int32_t B, int32_t H, int32_t W) {
    if (!desc || B <= 0 || H <= 0 || W <= 0) return 0;
    return basic_block_bwd_ws(*desc, 2, B, H, W);
}

size_t swf_window_attention_bwd_workspace_bytes(const swf_attn_desc* desc, int32_t B, int32_t H, int32_t W) {
    if (!desc || B <= 0 || H <= 0 || W <= 0 || desc->win_h <= 0 || desc->win_w <= 0 || desc->channels <= 0 || desc->heads <= 0 || desc->head_dim <= 0) return 0;
    return window_attention_bwd_ws(*desc, B, H, W);
}

size_t swf_mlp_bwd_workspace_bytes(int64_t tokens, int32_t channels, int32_t hidden) {
    if (tokens <= 0 || channels <= 0 || hidden <= 0) return 0;
    return mlp_bwd_ws(tokens, channels, hidden);
}

// ---- dropout (training side) --------------------------------------------------------------------------------------------------------
static bool drop_ratio_ok(float p) { return p >= 0.f && p <= 1.f; }   // false for NaN
static int check_dropout(const swf_dropout* drop, const char* what) {
    if (!drop) return fail(SWF_ERR_NULL, "%s: drop is NULL", what);
    if (!drop_ratio_ok(drop->attn_p) || !drop_ratio_ok(drop->proj_p) || !drop_ratio_ok(drop->mlp_p))
        return fail(SWF_ERR_BAD_SHAPE, "%s: dropout ratios must lie in [0, 1] (got %g, %g, %g)", what, drop->attn_p, drop->proj_p, drop->mlp_p);
    return SWF_OK;
}

int swf_dropout_mask(uint64_t seed, int32_t stream_id, int32_t site, int64_t count, float p, float* out, swf_stream_t stream) {
    if (!out) return fail(SWF_ERR_NULL, "dropout_mask: out is NULL");
    if (count <= 0 || stream_id < 0 || site < 0 || site > 3) return fail(SWF_ERR_BAD_SHAPE, "dropout_mask: bad count, stream or site");
    if (!drop_ratio_ok(p)) return fail(SWF_ERR_BAD_SHAPE, "dropout_mask: p = %g outside [0, 1]", p);
    return launch_dropout_mask(out, count, drop_site(seed, stream_id, site, p), as_stream(stream));
}

size_t swf_basic_block_drop_workspace_bytes(const swf_block_desc* desc, int32_t B, int32_t H, int32_t W) {
    if (!desc || B <= 0 || H <= 0 || W <= 0) return 0;
    return basic_block_drop_ws(*desc, 2, B, H, W);
}

int swf_basic_block_fwd_drop(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                             const float* x_in, const float* y_in, float* x_out, float* y_out, int32_t B, int32_t H, int32_t W,
                             const swf_dropout* drop, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_block(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, true, true));
    SWF_TRY(check_dropout(drop, "basic_block_fwd_drop"));
    return basic_block_fwd_drop(*desc, px, py, x_in, y_in, x_out, y_out, B, H, W, *drop, workspace, workspace_bytes, as_stream(stream));
}

size_t swf_window_attention_drop_workspace_bytes(const swf_attn_desc* desc, int32_t B, int32_t H, int32_t W) {
    if (!desc || B <= 0 || H <= 0 || W <= 0 || desc->win_h <= 0 || desc->win_w <= 0 || desc->channels <= 0 || desc->heads <= 0 || desc->head_dim <= 0) return 0;
    return window_attention_drop_ws(*desc, B, H, W);
}

static int check_attn_drop_args(const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k, const float* v,
                                const swf_dropout* drop, int32_t stream_id, int32_t B, int32_t H, int32_t W, const char* what) {
    if (!desc || !p || !q || !k || !v) return fail(SWF_ERR_NULL, "%s: NULL argument", what);
    if (!p->q.weight || !p->k.weight || !p->v.weight || !p->proj.weight || !p->bias_table) return fail(SWF_ERR_NULL, "%s: NULL parameter", what);
    SWF_TRY(check_attn_desc(desc, B, H, W));
    if (stream_id < 0) return fail(SWF_ERR_BAD_SHAPE, "%s: negative stream id", what);
    return check_dropout(drop, what);
}

int swf_window_attention_fwd_drop(const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k, const float* v,
                                  const float* residual, float* out, int32_t B, int32_t H, int32_t W, const swf_dropout* drop,
                                  int32_t stream_id, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_attn_drop_args(desc, p, q, k, v, drop, stream_id, B, H, W, "window_attention_fwd_drop"));
    if (!out) return fail(SWF_ERR_NULL, "window_attention_fwd_drop: out is NULL");
    return window_attention_fwd_drop(*desc, *p, q, k, v, residual, out, B, H, W, *drop, stream_id, workspace, workspace_bytes, as_stream(stream));
}

size_t swf_mlp_drop_workspace_bytes(int64_t tokens, int32_t channels, int32_t hidden) {
    if (tokens <= 0 || channels <= 0 || hidden <= 0) return 0;
    return mlp_drop_ws(tokens, channels, hidden);
}

int swf_mlp_fwd_drop_act(const swf_activation* act_, const swf_linear* fc1, const swf_linear* fc2, const float* x, float* out, int64_t tokens,
                         int32_t channels, int32_t hidden, const swf_dropout* drop, int32_t stream_id, void* workspace, size_t workspace_bytes,
                         swf_stream_t stream) {
    if (!fc1 || !fc2 || !fc1->weight || !fc2->weight || !x || !out) return fail(SWF_ERR_NULL, "mlp_fwd_drop: NULL argument");
    if (tokens <= 0 || channels <= 0 || hidden <= 0 || stream_id < 0) return fail(SWF_ERR_BAD_SHAPE, "mlp_fwd_drop: bad sizes");
    SWF_TRY(check_dropout(drop, "mlp_fwd_drop"));
    const swf_activation act = act_or_default(act_);
    SWF_TRY(check_activation(act, "mlp_fwd_drop"));
    return mlp_fwd_drop(*fc1, *fc2, x, out, tokens, channels, hidden, *drop, stream_id, workspace, workspace_bytes, as_stream(stream), act);
}
int swf_mlp_fwd_drop(const swf_linear* fc1, const swf_linear* fc2, const float* x, float* out, int64_t tokens, int32_t channels,
                     int32_t hidden, const swf_dropout* drop, int32_t stream_id, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return swf_mlp_fwd_drop_act(nullptr, fc1, fc2, x, out, tokens, channels, hidden, drop, stream_id, workspace, workspace_bytes, stream);
}

// ---- kernel families of the backward (swf_bwd_options / swf_bwd_route) -----------------------------------------------------------------
// options -> the internal tier; the route is zeroed here and filled by the branches that launch
static int bwd_tier(const swf_bwd_options* opt, swf_bwd_route* route, const char* what, BwdTier* tier) {
    const int gemm = opt ? opt->gemm : SWF_BWD_GEMM_FMA, attn = opt ? opt->attention : SWF_BWD_ATTN_THREAD;
    if (gemm != SWF_BWD_GEMM_FMA && gemm != SWF_BWD_GEMM_MFMA) return fail(SWF_ERR_UNSUPPORTED, "%s: unknown gradient-GEMM family %d", what, gemm);
    if (attn != SWF_BWD_ATTN_THREAD && attn != SWF_BWD_ATTN_PHASED) return fail(SWF_ERR_UNSUPPORTED, "%s: unknown attention-backward family %d", what, attn);
    if (route) *route = swf_bwd_route{};
    *tier = BwdTier{gemm, route, attn};
    return SWF_OK;
}

size_t swf_attention_bwd_lds_bytes(int32_t family, int32_t win_h, int32_t win_w, int32_t head_dim) {
    return attn_bwd_lds_bytes(family, win_h, win_w, head_dim);
}

// One implementation behind the plain, the *_drop and the *_opt entry of each unit.  what: the entry's name in error texts;
// need_drop: the *_drop entries require their masks (the others take NULL for none).
static int block_bwd_entry(const char* what, bool need_drop, const swf_block_desc* desc, const swf_block_stream_params* px,
                           const swf_block_stream_params* py, const float* x_in, const float* y_in, const float* gx_out, const float* gy_out,
                           float* gx_in, float* gy_in, const swf_block_stream_grads* gpx, const swf_block_stream_grads* gpy, int32_t B, int32_t H,
                           int32_t W, const swf_dropout* drop, const swf_bwd_options* opt, swf_bwd_route* route, void* workspace,
                           size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_block(desc, px, py, x_in, y_in, gx_in, gy_in, B, H, W, true, true));
    if (!gx_out || (py && !gy_out)) return fail(SWF_ERR_NULL, "%s: NULL output gradient", what);
    if (need_drop || drop) SWF_TRY(check_dropout(drop, what));
    BwdTier tier;
    SWF_TRY(bwd_tier(opt, route, what, &tier));
    if (drop)
        return basic_block_bwd_drop(*desc, px, py, x_in, y_in, gx_out, gy_out, gx_in, gy_in, gpx, gpy, B, H, W, *drop, workspace, workspace_bytes,
                                    as_stream(stream), tier);
    return basic_block_bwd(*desc, px, py, x_in, y_in, gx_out, gy_out, gx_in, gy_in, gpx, gpy, B, H, W, workspace, workspace_bytes,
                           as_stream(stream), tier);
}
int swf_basic_block_bwd(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py, const float* x_in,
                        const float* y_in, const float* gx_out, const float* gy_out, float* gx_in, float* gy_in, const swf_block_stream_grads* gpx,
                        const swf_block_stream_grads* gpy, int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes,
                        swf_stream_t stream) {
    return block_bwd_entry("basic_block_bwd", false, desc, px, py, x_in, y_in, gx_out, gy_out, gx_in, gy_in, gpx, gpy, B, H, W, nullptr, nullptr,
                           nullptr, workspace, workspace_bytes, stream);
}
int swf_basic_block_bwd_drop(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                             const float* x_in, const float* y_in, const float* gx_out, const float* gy_out, float* gx_in, float* gy_in,
                             const swf_block_stream_grads* gpx, const swf_block_stream_grads* gpy, int32_t B, int32_t H, int32_t W,
                             const swf_dropout* drop, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return block_bwd_entry("basic_block_bwd_drop", true, desc, px, py, x_in, y_in, gx_out, gy_out, gx_in, gy_in, gpx, gpy, B, H, W, drop, nullptr,
                           nullptr, workspace, workspace_bytes, stream);
}
int swf_basic_block_bwd_opt(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                            const float* x_in, const float* y_in, const float* gx_out, const float* gy_out, float* gx_in, float* gy_in,
                            const swf_block_stream_grads* gpx, const swf_block_stream_grads* gpy, int32_t B, int32_t H, int32_t W,
                            const swf_dropout* drop, const swf_bwd_options* opt, swf_bwd_route* route, void* workspace,
                            size_t workspace_bytes, swf_stream_t stream) {
    return block_bwd_entry("basic_block_bwd_opt", false, desc, px, py, x_in, y_in, gx_out, gy_out, gx_in, gy_in, gpx, gpy, B, H, W, drop, opt,
                           route, workspace, workspace_bytes, stream);
}

static int attention_bwd_entry(const char* what, bool need_drop, const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k,
                               const float* v, const float* gout, float* gq, float* gk, float* gv, const swf_attn_grads* gp, int32_t B, int32_t H,
                               int32_t W, const swf_dropout* drop, int32_t stream_id, const swf_bwd_options* opt, swf_bwd_route* route,
                               void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    if (!desc || !p || !q || !k || !v) return fail(SWF_ERR_NULL, "%s: NULL argument", what);
    if (!p->q.weight || !p->k.weight || !p->v.weight || !p->proj.weight || !p->bias_table) return fail(SWF_ERR_NULL, "%s: NULL parameter", what);
    SWF_TRY(check_attn_desc(desc, B, H, W));
    if (stream_id < 0) return fail(SWF_ERR_BAD_SHAPE, "%s: negative stream id", what);
    if (need_drop || drop) SWF_TRY(check_dropout(drop, what));
    if (!gout || !gq || !gk || !gv) return fail(SWF_ERR_NULL, "%s: NULL gradient", what);
    if (gq == gk || gq == gv || gk == gv) return fail(SWF_ERR_UNSUPPORTED, "%s: gq, gk, gv must be three buffers", what);
    BwdTier tier;
    SWF_TRY(bwd_tier(opt, route, what, &tier));
    if (drop)
        return window_attention_bwd_drop(*desc, *p, q, k, v, gout, gq, gk, gv, gp, B, H, W, *drop, stream_id, workspace, workspace_bytes,
                                         as_stream(stream), tier);
    return window_attention_bwd(*desc, *p, q, k, v, gout, gq, gk, gv, gp, B, H, W, workspace, workspace_bytes, as_stream(stream), tier);
}
int swf_window_attention_bwd(const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k, const float* v, const float* gout,
                             float* gq, float* gk, float* gv, const swf_attn_grads* gp, int32_t B, int32_t H, int32_t W, void* workspace,
                             size_t workspace_bytes, swf_stream_t stream) {
    return attention_bwd_entry("window_attention_bwd", false, desc, p, q, k, v, gout, gq, gk, gv, gp, B, H, W, nullptr, 0, nullptr, nullptr,
                               workspace, workspace_bytes, stream);
}
int swf_window_attention_bwd_drop(const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k, const float* v,
                                  const float* gout, float* gq, float* gk, float* gv, const swf_attn_grads* gp, int32_t B, int32_t H,
                                  int32_t W, const swf_dropout* drop, int32_t stream_id, void* workspace, size_t workspace_bytes,
                                  swf_stream_t stream) {
    return attention_bwd_entry("window_attention_bwd_drop", true, desc, p, q, k, v, gout, gq, gk, gv, gp, B, H, W, drop, stream_id, nullptr,
                               nullptr, workspace, workspace_bytes, stream);
}
int swf_window_attention_bwd_opt(const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k, const float* v,
                                 const float* gout, float* gq, float* gk, float* gv, const swf_attn_grads* gp, int32_t B, int32_t H,
                                 int32_t W, const swf_dropout* drop, int32_t stream_id, const swf_bwd_options* opt, swf_bwd_route* route,
                                 void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return attention_bwd_entry("window_attention_bwd_opt", false, desc, p, q, k, v, gout, gq, gk, gv, gp, B, H, W, drop, stream_id, opt, route,
                               workspace, workspace_bytes, stream);
}

static int mlp_bwd_entry(const char* what, bool need_drop, const swf_linear* fc1, const swf_linear* fc2, const float* x, const float* gout, float* gx,
                         const swf_linear_grad* gfc1, const swf_linear_grad* gfc2, int64_t tokens, int32_t channels, int32_t hidden,
                         const swf_dropout* drop, int32_t stream_id, const swf_bwd_options* opt, swf_bwd_route* route, void* workspace,
                         size_t workspace_bytes, swf_stream_t stream, const swf_activation* act_ = nullptr) {
    const swf_activation act = act_or_default(act_);
    if (!fc1 || !fc2 || !fc1->weight || !fc2->weight || !x || !gout || !gx) return fail(SWF_ERR_NULL, "%s: NULL argument", what);
    if (tokens <= 0 || channels <= 0 || hidden <= 0 || stream_id < 0) return fail(SWF_ERR_BAD_SHAPE, "%s: bad sizes", what);
    if (need_drop || drop) SWF_TRY(check_dropout(drop, what));
    SWF_TRY(check_activation(act, what));
    BwdTier tier;
    SWF_TRY(bwd_tier(opt, route, what, &tier));
    if (drop)
        return mlp_bwd_drop(*fc1, *fc2, x, gout, gx, gfc1, gfc2, tokens, channels, hidden, *drop, stream_id, workspace, workspace_bytes,
                            as_stream(stream), tier, act);
    return mlp_bwd(*fc1, *fc2, x, gout, gx, gfc1, gfc2, tokens, channels, hidden, workspace, workspace_bytes, as_stream(stream), tier, act);
}
int swf_mlp_bwd_opt_act(const swf_activation* act, const swf_linear* fc1, const swf_linear* fc2, const float* x, const float* gout, float* gx,
                        const swf_linear_grad* gfc1, const swf_linear_grad* gfc2, int64_t tokens, int32_t channels, int32_t hidden,
                        const swf_dropout* drop, int32_t stream_id, const swf_bwd_options* opt, swf_bwd_route* route, void* workspace,
                        size_t workspace_bytes, swf_stream_t stream) {
    return mlp_bwd_entry("mlp_bwd_opt", false, fc1, fc2, x, gout, gx, gfc1, gfc2, tokens, channels, hidden, drop, stream_id, opt, route, workspace,
                         workspace_bytes, stream, act);
}
int swf_mlp_bwd(const swf_linear* fc1, const swf_linear* fc2, const float* x, const float* gout, float* gx, const swf_linear_grad* gfc1,
                const swf_linear_grad* gfc2, int64_t tokens, int32_t channels, int32_t hidden, void* workspace, size_t workspace_bytes,
                swf_stream_t stream) {
    return mlp_bwd_entry("mlp_bwd", false, fc1, fc2, x, gout, gx, gfc1, gfc2, tokens, channels, hidden, nullptr, 0, nullptr, nullptr, workspace,
                         workspace_bytes, stream);
}
int swf_mlp_bwd_drop(const swf_linear* fc1, const swf_linear* fc2, const float* x, const float* gout, float* gx,
                     const swf_linear_grad* gfc1, const swf_linear_grad* gfc2, int64_t tokens, int32_t channels, int32_t hidden,
                     const swf_dropout* drop, int32_t stream_id, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return mlp_bwd_entry("mlp_bwd_drop", true, fc1, fc2, x, gout, gx, gfc1, gfc2, tokens, channels, hidden, drop, stream_id, nullptr, nullptr,
                         workspace, workspace_bytes, stream);
}
int swf_mlp_bwd_opt(const swf_linear* fc1, const swf_linear* fc2, const float* x, const float* gout, float* gx, const swf_linear_grad* gfc1,
                    const swf_linear_grad* gfc2, int64_t tokens, int32_t channels, int32_t hidden, const swf_dropout* drop, int32_t stream_id,
                    const swf_bwd_options* opt, swf_bwd_route* route, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return mlp_bwd_entry("mlp_bwd_opt", false, fc1, fc2, x, gout, gx, gfc1, gfc2, tokens, channels, hidden, drop, stream_id, opt, route, workspace,
                         workspace_bytes, stream);
}

size_t swf_linear_bwd_workspace_bytes(int64_t M, int32_t N, int32_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return linear_bwd_ws(M, N, K);
}

int swf_linear_bwd(const float* x, const float* weight, const float* gout, float* gx, float* gw, float* gb, int64_t M, int32_t N, int32_t K,
                   int32_t accumulate, const swf_bwd_options* opt, swf_bwd_route* route, void* workspace, size_t workspace_bytes,
                   swf_stream_t stream) {
    if (!x || !weight || !gout) return fail(SWF_ERR_NULL, "linear_bwd: NULL tensor");
    if (M <= 0 || N <= 0 || K <= 0) return fail(SWF_ERR_BAD_SHAPE, "linear_bwd: bad sizes");
    BwdTier tier;
    SWF_TRY(bwd_tier(opt, route, "linear_bwd", &tier));
    return linear_bwd(x, weight, gout, gx, gw, gb, M, N, K, accumulate, workspace, workspace_bytes, as_stream(stream), tier);
}

size_t swf_layernorm_bwd_workspace_bytes(int64_t tokens, int32_t C) {
    if (tokens <= 0 || C <= 0) return 0;
    return layernorm_bwd_ws(tokens, C);
}

int swf_layernorm_bwd(const swf_norm* ln, const float* x, const float* gout, float* gx, const swf_norm_grad* gp, int64_t tokens, int32_t C,
                      void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    if (!ln || !ln->gamma || !ln->beta || !x || !gout || !gx) return fail(SWF_ERR_NULL, "layernorm_bwd: NULL argument");
    if (tokens <= 0 || C <= 0) return fail(SWF_ERR_BAD_SHAPE, "layernorm_bwd: bad sizes");
    return layernorm_bwd(*ln, x, gout, gx, gp, tokens, C, workspace, workspace_bytes, as_stream(stream));
}

size_t swf_patch_layer_bwd_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t encoder) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || merge_h <= 0 || merge_w <= 0) return 0;
    return patch_bwd_ws(B, H, W, Cin, Cout, merge_h, merge_w, encoder);
}

int swf_patch_layer_bwd_opt_act(const swf_activation* act_, const swf_patch_params* p, const float* in, const float* gout, float* gin,
                                const swf_patch_grads* gp, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t merge_h,
                                int32_t merge_w, int32_t encoder, const swf_bwd_options* opt, swf_bwd_route* route, void* workspace,
                                size_t workspace_bytes, swf_stream_t stream) {
    const swf_activation act = act_or_default(act_);
    if (!p || !p->conv.weight || !p->ln.gamma || !p->ln.beta || !in || !gout || !gin) return fail(SWF_ERR_NULL, "patch_layer_bwd: NULL argument");
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || merge_h <= 0 || merge_w <= 0) return fail(SWF_ERR_BAD_SHAPE, "patch_layer_bwd: bad sizes");
    SWF_TRY(check_activation(act, "patch_layer_bwd"));
    BwdTier tier;
    SWF_TRY(bwd_tier(opt, route, "patch_layer_bwd", &tier));
    return patch_bwd(*p, in, gout, gin, gp, B, H, W, Cin, Cout, merge_h, merge_w, encoder, workspace, workspace_bytes, as_stream(stream), tier, act);
}
int swf_patch_layer_bwd_opt(const swf_patch_params* p, const float* in, const float* gout, float* gin, const swf_patch_grads* gp, int32_t B,
                            int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t encoder,
                            const swf_bwd_options* opt, swf_bwd_route* route, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return swf_patch_layer_bwd_opt_act(nullptr, p, in, gout, gin, gp, B, H, W, Cin, Cout, merge_h, merge_w, encoder, opt, route, workspace,
                                       workspace_bytes, stream);
}

int swf_patch_layer_bwd(const swf_patch_params* p, const float* in, const float* gout, float* gin, const swf_patch_grads* gp, int32_t B, int32_t H,
                        int32_t W, int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t encoder, void* workspace,
                        size_t workspace_bytes, swf_stream_t stream) {
    return swf_patch_layer_bwd_opt(p, in, gout, gin, gp, B, H, W, Cin, Cout, merge_h, merge_w, encoder, nullptr, nullptr, workspace, workspace_bytes,
                                   stream);
}

int swf_reflect_pad_bwd(const float* gout, float* gin, int32_t B, int32_t H, int32_t W, int32_t C, int32_t pad_h, int32_t pad_w, swf_stream_t stream) {
    if (!gout || !gin) return fail(SWF_ERR_NULL, "reflect_pad_bwd: NULL tensor");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(SWF_ERR_BAD_SHAPE, "reflect_pad_bwd: empty tensor");
    return reflect_pad_bwd(gout, gin, B, H, W, C, pad_h, pad_w, as_stream(stream));
}

size_t swf_final_head_bwd_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t ksize) {
    if (B <= 0 || H <= 0 || W <= 0 || ksize <= 0) return 0;
    return head_bwd_ws(B, H, W, ksize);
}

int swf_final_head_batch_stats(const swf_head_params* p, const float* x, const float* y, float* mean, float* var, float* running_mean,
                               float* running_var, float momentum, int32_t B, int32_t H, int32_t W, int32_t ksize, void* workspace,
                               size_t workspace_bytes, swf_stream_t stream) {
    if (!p || !p->conv1_w || !x || !y || !mean || !var) return fail(SWF_ERR_NULL, "final_head_batch_stats: NULL argument");
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "final_head_batch_stats: empty tensor");
    return head_batch_stats(*p, x, y, mean, var, running_mean, running_var, momentum, B, H, W, ksize, workspace, workspace_bytes, as_stream(stream));
}

int swf_final_head_bwd_act(const swf_activation* act_, const swf_head_params* p, const float* x, const float* y, const float* gout, float* gx,
                           float* gy, const swf_head_grads* gp, int32_t B, int32_t H, int32_t W, int32_t ksize, int32_t batch_stats,
                           void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    const swf_activation act = act_or_default(act_);
    if (!p || !p->conv1_w || !p->conv2_w || !p->bn_gamma || !p->bn_beta || !p->bn_mean || !p->bn_var || !x || !y || !gout || !gx || !gy)
        return fail(SWF_ERR_NULL, "final_head_bwd: NULL argument");
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "final_head_bwd: empty tensor");
    SWF_TRY(check_activation(act, "final_head_bwd"));
    return head_bwd(*p, x, y, gout, gx, gy, gp, B, H, W, ksize, batch_stats, workspace, workspace_bytes, as_stream(stream), act);
}
int swf_final_head_bwd(const swf_head_params* p, const float* x, const float* y, const float* gout, float* gx, float* gy, const swf_head_grads* gp,
                       int32_t B, int32_t H, int32_t W, int32_t ksize, int32_t batch_stats, void* workspace, size_t workspace_bytes,
                       swf_stream_t stream) {
    return swf_final_head_bwd_act(nullptr, p, x, y, gout, gx, gy, gp, B, H, W, ksize, batch_stats, workspace, workspace_bytes, stream);
}

// The head's BatchNorm over a batch that spans several calls or ranks: the entries above, split where the per-channel sums exist.
int swf_final_head_stats_pass(const swf_head_params* p, const float* x, const float* y, int32_t pass, const float* mean, float* sums_out,
                              int32_t B, int32_t H, int32_t W, int32_t ksize, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    if (!p || !p->conv1_w || !x || !y || !sums_out) return fail(SWF_ERR_NULL, "final_head_stats_pass: NULL argument");
    if (pass != 0 && pass != 1) return fail(SWF_ERR_BAD_SHAPE, "final_head_stats_pass: pass %d is neither 0 nor 1", pass);
    if (pass == 1 && !mean) return fail(SWF_ERR_NULL, "final_head_stats_pass: pass 1 needs the mean");
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "final_head_stats_pass: empty tensor");
    return head_stats_pass(*p, x, y, pass, mean, sums_out, B, H, W, ksize, workspace, workspace_bytes, as_stream(stream));
}

int swf_final_head_stats_finish(const float* sums, size_t sums_bytes, int64_t count, int32_t pass, float* mean, float* var, float* running_mean,
                                float* running_var, float momentum, swf_stream_t stream) {
    if (!sums || !mean || (pass == 1 && !var)) return fail(SWF_ERR_NULL, "final_head_stats_finish: NULL argument");
    if (pass != 0 && pass != 1) return fail(SWF_ERR_BAD_SHAPE, "final_head_stats_finish: pass %d is neither 0 nor 1", pass);
    if (count <= 0) return fail(SWF_ERR_BAD_SHAPE, "final_head_stats_finish: a batch of %lld elements", (long long)count);
    if (sums_bytes < 2 * sizeof(float))
        return fail(SWF_ERR_WORKSPACE, "final_head_stats_finish: sums buffer of %zu bytes, %zu needed", sums_bytes, 2 * sizeof(float));
    return head_stats_finish(sums, count, pass, mean, var, running_mean, running_var, momentum, as_stream(stream));
}

int swf_final_head_bwd_sums_act(const swf_activation* act_, const swf_head_params* p, const float* x, const float* y, const float* gout,
                                float* sums_out, int32_t B, int32_t H, int32_t W, int32_t ksize, void* workspace, size_t workspace_bytes,
                                swf_stream_t stream) {
    const swf_activation act = act_or_default(act_);
    if (!p || !p->conv1_w || !p->conv2_w || !p->bn_gamma || !p->bn_beta || !p->bn_mean || !p->bn_var || !x || !y || !gout || !sums_out)
        return fail(SWF_ERR_NULL, "final_head_bwd_sums: NULL argument");
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "final_head_bwd_sums: empty tensor");
    SWF_TRY(check_activation(act, "final_head_bwd_sums"));
    return head_bwd_sums(*p, x, y, gout, sums_out, B, H, W, ksize, workspace, workspace_bytes, as_stream(stream), act);
}
int swf_final_head_bwd_sums(const swf_head_params* p, const float* x, const float* y, const float* gout, float* sums_out, int32_t B, int32_t H,
                            int32_t W, int32_t ksize, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return swf_final_head_bwd_sums_act(nullptr, p, x, y, gout, sums_out, B, H, W, ksize, workspace, workspace_bytes, stream);
}

int swf_final_head_bwd_synced_act(const swf_activation* act_, const swf_head_params* p, const float* x, const float* y, const float* gout,
                                  const float* sums, int64_t count, float* gx, float* gy, const swf_head_grads* gp, int32_t B, int32_t H,
                                  int32_t W, int32_t ksize, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    const swf_activation act = act_or_default(act_);
    if (!p || !p->conv1_w || !p->conv2_w || !p->bn_gamma || !p->bn_beta || !p->bn_mean || !p->bn_var || !x || !y || !gout || !sums || !gx || !gy)
        return fail(SWF_ERR_NULL, "final_head_bwd_synced: NULL argument");
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "final_head_bwd_synced: empty tensor");
    if (count < (int64_t)B * H * W)
        return fail(SWF_ERR_BAD_SHAPE, "final_head_bwd_synced: a whole batch of %lld elements is smaller than this call's %lld", (long long)count,
                    (long long)B * H * W);
    SWF_TRY(check_activation(act, "final_head_bwd_synced"));
    return head_bwd_apply(*p, x, y, gout, sums, count, gx, gy, gp, B, H, W, ksize, workspace, workspace_bytes, as_stream(stream), act);
}
int swf_final_head_bwd_synced(const swf_head_params* p, const float* x, const float* y, const float* gout, const float* sums, int64_t count,
                              float* gx, float* gy, const swf_head_grads* gp, int32_t B, int32_t H, int32_t W, int32_t ksize, void* workspace,
                              size_t workspace_bytes, swf_stream_t stream) {
    return swf_final_head_bwd_synced_act(nullptr, p, x, y, gout, sums, count, gx, gy, gp, B, H, W, ksize, workspace, workspace_bytes, stream);
}

int swf_add_fwd(const float* a, const float* b, float* out, int64_t count, swf_stream_t stream) {
    if (!a || !b || !out) return fail(SWF_ERR_NULL, "add: NULL tensor");
    if (count <= 0) return fail(SWF_ERR_BAD_SHAPE, "add: empty tensor");
    return add_tensors(a, b, out, count, as_stream(stream));
}

int swf_block_pair4_fwd(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                        const float* x_in, const float* y_in, float* x_out, float* y_out, int32_t B, int32_t H, int32_t W,
                        void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    if (!px) return fail(SWF_ERR_NULL, "block params are NULL");
    for (int i = 0; i < 4; ++i)
        SWF_TRY(check_block(desc, &px[i], py ? &py[i] : nullptr, x_in, y_in, x_out, y_out, B, H, W, true, true));
    return block_pair4_impl(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, workspace, workspace_bytes, as_stream(stream));
}

// ---- one stage as the model runs it: images packed at the front of the workspace, then block_pair4_impl on the rest ----------------
// Bytes of ONE image of the stage (0: this shape, tier and stream count run without images).  The window kernels need two streams.
static size_t stage_image_bytes(const swf_block_desc& d, int nstream) {
    if (d.precision != SWF_PREC_FAST || !act_is_default(d.act)) return 0;
    if (window_block_packed_bytes(d)) return nstream == 2 ? window_block_packed_bytes(d) : 0;
    return deep_block_packed_bytes(d);
}
// What block_pair4_impl and its four blocks carve when they run from images: a window-kernel stage only the two temporary maps of a
// kernel that cannot run a cross block in place; every other stage what its largest block needs.
static size_t stage_inner_ws(const swf_block_desc& d, int nstream, int B, int H, int W) {
    if (act_is_default(d.act) && d.precision == SWF_PREC_FAST && nstream == 2 && window_block_supported(d, B, H, W)) {
        Carver m = Carver::measure();
        carve_window_block(m, d, (int64_t)B * H * W, true, window_block_out_of_place(d));
        return m.bytes();
    }
    return block_generic_ws(&d, nstream, B, H, W);
}
struct StageBufs { char* packed; void* inner; size_t inner_bytes; };
static StageBufs carve_block_stage(Carver& ws, const swf_block_desc& d, int nstream, int B, int H, int W) {
    StageBufs b{};
    const size_t image = stage_image_bytes(d, nstream);
    if (image) b.packed = reinterpret_cast<char*>(ws.floats((int64_t)(8 * image / 4)));
    b.inner_bytes = stage_inner_ws(d, nstream, B, H, W);
    b.inner = ws.floats((int64_t)(b.inner_bytes / 4));
    return b;
}
static bool stage_precision_ok(const swf_block_desc* d) { return d && (d->precision == SWF_PREC_FP32 || d->precision == SWF_PREC_FAST); }

size_t swf_block_stage_prec_workspace_bytes(const swf_block_desc* desc, int32_t dual, int32_t B, int32_t H, int32_t W) {
    if (!stage_precision_ok(desc) || desc->hidden <= 0 || check_attn_desc(&desc->attn, B, H, W) != SWF_OK) return 0;
    Carver m = Carver::measure();
    carve_block_stage(m, *desc, dual ? 2 : 1, B, H, W);
    return m.bytes();
}

int swf_block_stage_fwd_prec(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                             const float* x_in, const float* y_in, float* x_out, float* y_out, int32_t B, int32_t H, int32_t W,
                             const swf_patch_ln1* ln1_x, const swf_patch_ln1* ln1_y, int32_t* route, void* workspace, size_t workspace_bytes,
                             swf_stream_t stream_) {
    if (!px) return fail(SWF_ERR_NULL, "block_stage_prec: block params are NULL");
    for (int i = 0; i < 4; ++i)
        SWF_TRY(check_block(desc, &px[i], py ? &py[i] : nullptr, x_in, y_in, x_out, y_out, B, H, W, true, true));
    if (!stage_precision_ok(desc)) return fail(SWF_ERR_BAD_SHAPE, "block_stage_prec: unknown precision %d", desc->precision);
    if (ln1_y && !py) return fail(SWF_ERR_NULL, "block_stage_prec: LN1 planes of a y stream that is not there");
    if (ln1_x ? (py && !ln1_y) : ln1_y != nullptr) return fail(SWF_ERR_NULL, "block_stage_prec: LN1 planes are asked for every stream or for none");
    for (const swf_patch_ln1* l : {ln1_x, ln1_y})
        if (l && (!l->ln.gamma || !l->ln.beta || !l->hi || !l->lo)) return fail(SWF_ERR_NULL, "block_stage_prec: NULL pointer in swf_patch_ln1");
    const int nstream = py ? 2 : 1;
    Carver ws(workspace, workspace_bytes);
    const StageBufs bufs = carve_block_stage(ws, *desc, nstream, B, H, W);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "block_stage_prec: workspace too small (need %zu B)", ws.bytes());
    hipStream_t stream = as_stream(stream_);
    if (bufs.packed) {   // [block 0..3][stream x, y], as swf_model_pack_weights lays a stage out
        const size_t pb = stage_image_bytes(*desc, nstream);
        for (int i = 0; i < 4; ++i) {
            char* dst = bufs.packed + (size_t)(2 * i) * pb;
            if (window_block_packed_bytes(*desc)) {
                SWF_TRY(pack_window_block(*desc, px[i], py[i], dst, dst + pb, stream));
            } else {
                SWF_TRY(pack_deep_block(*desc, px[i], dst, stream));
                if (py) SWF_TRY(pack_deep_block(*desc, py[i], dst + pb, stream));
            }
        }
    }
    const swf_patch_ln1* ln[2] = {ln1_x, ln1_y};
    swf_block_stream_params nb[2] = {};   // the first block of the stage behind this one: only its LN1 is read
    const swf_block_stream_params* nbp[2] = {&nb[0], nstream == 2 ? &nb[1] : nullptr};
    for (int s = 0; s < nstream && ln[0]; ++s) nb[s].ln1 = ln[s]->ln;
    bool ln1_io = false;
    int32_t r[4] = {0, 0, 0, 0};
    SWF_TRY(block_pair4_impl(desc, px, py, x_in, y_in, x_out, y_out, B, H, W, bufs.inner, bufs.inner_bytes, stream, bufs.packed, nullptr, 0, nullptr,
                             ln[0] ? nbp : nullptr, &ln1_io, r));
    if (ln[0] && ln1_io) {   // the planes lie where the next block on this workspace would look for them
        bf16_raw *hi[2], *lo[2];
        Carver at(bufs.inner, bufs.inner_bytes);
        deep_ln1_planes(at, (int64_t)B * H * W, desc->attn.channels, nstream, hi, lo);
        const size_t plane_bytes = (size_t)B * H * W * desc->attn.channels * sizeof(bf16_raw);
        for (int s = 0; s < nstream; ++s)
            if (hipMemcpyAsync(ln[s]->hi, hi[s], plane_bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
                hipMemcpyAsync(ln[s]->lo, lo[s], plane_bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess)
                return fail(SWF_ERR_HIP, "block_stage_prec: copy of the LN1 planes failed");
    }
    if (route) std::copy(r, r + 4, route);
    return SWF_OK;
}

int swf_merge_out_shape(int32_t H, int32_t W, int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w, int32_t* Hm,
                        int32_t* Wm, int32_t* Ho, int32_t* Wo) {
    if (!Hm || !Wm || !Ho || !Wo) return fail(SWF_ERR_NULL, "output pointer is NULL");
    return merge_shapes(H, W, merge_h, merge_w, win_h, win_w, Hm, Wm, Ho, Wo);
}

size_t swf_patch_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t merge_h,
                                 int32_t merge_w, int32_t win_h, int32_t win_w, int32_t encoder) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    if (encoder) return merge_ws(1, B, H, W, Cin, Cout, merge_h, merge_w, win_h, win_w);
    return unmerge_ws_any_crop(1, B, H, W, Cin, Cout, merge_h, merge_w);
}

int swf_patch_merge_fwd_act(const swf_activation* act_, const swf_patch_params* p, const float* in, float* out, int32_t B, int32_t H, int32_t W,
                            int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w, void* workspace,
                            size_t workspace_bytes, swf_stream_t stream) {
    if (!p || !in || !out || !p->conv.weight || !p->ln.gamma || !p->ln.beta) return fail(SWF_ERR_NULL, "patch_merge: NULL argument");
    if (B <= 0 || Cin <= 0 || Cout <= 0) return fail(SWF_ERR_BAD_SHAPE, "patch_merge: non-positive dims");
    const swf_activation act = act_or_default(act_);
    SWF_TRY(check_activation(act, "patch_merge"));
    const swf_patch_params* pp[2] = {p, nullptr};
    const float* ins[2] = {in, nullptr};
    float* outs[2] = {out, nullptr};
    return patch_merge_impl(pp, 1, ins, outs, B, H, W, Cin, Cout, merge_h, merge_w, win_h, win_w, workspace, workspace_bytes,
                            as_stream(stream), 0, nullptr, nullptr, nullptr, nullptr, act);
}
int swf_patch_merge_fwd(const swf_patch_params* p, const float* in, float* out, int32_t B, int32_t H, int32_t W, int32_t Cin,
                        int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w, void* workspace,
                        size_t workspace_bytes, swf_stream_t stream) {
    return swf_patch_merge_fwd_act(nullptr, p, in, out, B, H, W, Cin, Cout, merge_h, merge_w, win_h, win_w, workspace, workspace_bytes, stream);
}

int swf_patch_unmerge_fwd_act(const swf_activation* act_, const swf_patch_params* p, const float* in, const float* skip, float* out, int32_t B,
                              int32_t Hp, int32_t Wp, int32_t Hm, int32_t Wm, int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w,
                              int32_t Hout, int32_t Wout, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    if (!p || !in || !out || !p->conv.weight || !p->ln.gamma || !p->ln.beta) return fail(SWF_ERR_NULL, "patch_unmerge: NULL argument");
    if (B <= 0 || Cin <= 0 || Cout <= 0 || merge_h <= 0 || merge_w <= 0) return fail(SWF_ERR_BAD_SHAPE, "patch_unmerge: non-positive dims");
    const swf_activation act = act_or_default(act_);
    SWF_TRY(check_activation(act, "patch_unmerge"));
    const swf_patch_params* pp[2] = {p, nullptr};
    const float* ins[2] = {in, nullptr};
    const float* sk[2] = {skip, nullptr};
    float* outs[2] = {out, nullptr};
    return patch_unmerge_impl(pp, 1, ins, skip ? sk : nullptr, outs, B, Hp, Wp, Hm, Wm, Cin, Cout, merge_h, merge_w, Hout, Wout,
                              workspace, workspace_bytes, as_stream(stream), 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, act);
}
int swf_patch_unmerge_fwd(const swf_patch_params* p, const float* in, const float* skip, float* out, int32_t B, int32_t Hp,
                          int32_t Wp, int32_t Hm, int32_t Wm, int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w,
                          int32_t Hout, int32_t Wout, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return swf_patch_unmerge_fwd_act(nullptr, p, in, skip, out, B, Hp, Wp, Hm, Wm, Cin, Cout, merge_h, merge_w, Hout, Wout, workspace,
                                     workspace_bytes, stream);
}

// ---- the pair of patch layers of one stage with the arithmetic tier as an argument -------------------------------------------------
// The fast tier's packed images (one per stream, where a kernel of this shape takes one), then the room of the impl behind the entry.
struct PatchPrecBufs { void* packed[2]; void* inner; size_t inner_bytes; };
static PatchPrecBufs carve_patch_prec(Carver& ws, int nstream, size_t image_bytes, size_t inner_bytes) {
    PatchPrecBufs b{};
    for (int s = 0; s < nstream && image_bytes; ++s) b.packed[s] = ws.floats((int64_t)(image_bytes / 4));
    b.inner = ws.floats((int64_t)(inner_bytes / 4));
    b.inner_bytes = inner_bytes;
    return b;
}

static int check_patch_prec(const char* what, int32_t precision, const swf_patch_params* px, const swf_patch_params* py, const float* x_in,
                            const float* y_in, float* x_out, float* y_out, const swf_patch_ln1* ln1_x, const swf_patch_ln1* ln1_y,
                            int B, int Cin, int Cout, int mh, int mw) {
    if (precision != SWF_PREC_FP32 && precision != SWF_PREC_FAST) return fail(SWF_ERR_BAD_SHAPE, "%s: unknown precision %d", what, precision);
    if (!px || !x_in || !x_out || !px->conv.weight || !px->ln.gamma || !px->ln.beta) return fail(SWF_ERR_NULL, "%s: NULL x-stream argument", what);
    if (py && (!y_in || !y_out || !py->conv.weight || !py->ln.gamma || !py->ln.beta))
        return fail(SWF_ERR_NULL, "%s: NULL y-stream argument with dual-path params", what);
    if (ln1_y && !py) return fail(SWF_ERR_NULL, "%s: LN1 planes of a y stream that is not there", what);
    if (ln1_x ? (py && !ln1_y) : ln1_y != nullptr) return fail(SWF_ERR_NULL, "%s: LN1 planes are asked for every stream or for none", what);
    for (const swf_patch_ln1* l : {ln1_x, ln1_y})
        if (l && (!l->ln.gamma || !l->ln.beta || !l->hi || !l->lo)) return fail(SWF_ERR_NULL, "%s: NULL pointer in swf_patch_ln1", what);
    if (B <= 0 || Cin <= 0 || Cout <= 0 || mh <= 0 || mw <= 0) return fail(SWF_ERR_BAD_SHAPE, "%s: non-positive dims", what);
    return SWF_OK;
}

// After the impl: the planes its route wrote go to the caller's buffers, and the route code says whether there were any.
static int finish_patch_prec(const char* what, const PatchTrace& tr, const swf_patch_ln1* const* ln, int nstream, size_t plane_bytes,
                             int32_t* route, hipStream_t stream) {
    const bool planes = ln[0] && tr.ln_hi[0];
    for (int s = 0; s < nstream && planes; ++s)
        if (hipMemcpyAsync(ln[s]->hi, tr.ln_hi[s], plane_bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
            hipMemcpyAsync(ln[s]->lo, tr.ln_lo[s], plane_bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return fail(SWF_ERR_HIP, "%s: copy of the LN1 planes failed", what);
    if (route) *route = tr.route | (planes ? SWF_PATCH_ROUTE_LN1 : 0);
    return SWF_OK;
}

static size_t merge_prec_ws(int32_t precision, int nstream, int B, int H, int W, int Cin, int Cout, int mh, int mw, int wh, int ww) {
    Carver m = Carver::measure();
    carve_patch_prec(m, nstream, precision == SWF_PREC_FAST ? patch_image_bytes(0, Cin, Cout, mh, mw) : 0,
                     merge_ws(nstream, B, H, W, Cin, Cout, mh, mw, wh, ww));
    return m.bytes();
}
static size_t unmerge_prec_ws(int32_t precision, int nstream, int B, int Hp, int Wp, int Hm, int Wm, int Cin, int Cout, int mh, int mw,
                              int Hout, int Wout) {
    Carver m = Carver::measure();
    carve_patch_prec(m, nstream, precision == SWF_PREC_FAST ? patch_image_bytes(1, Cin, Cout, mh, mw) : 0,
                     unmerge_ws(nstream, B, Hp, Wp, Hm, Wm, Cin, Cout, mh, mw, Hout, Wout));
    return m.bytes();
}

size_t swf_patch_merge_prec_workspace_bytes(int32_t precision, int32_t dual, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                            int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w) {
    int Hm, Wm, Ho, Wo;
    if ((precision != SWF_PREC_FP32 && precision != SWF_PREC_FAST) || B <= 0 || Cin <= 0 || Cout <= 0 ||
        merge_shapes(H, W, merge_h, merge_w, win_h, win_w, &Hm, &Wm, &Ho, &Wo) != SWF_OK)
        return 0;
    return merge_prec_ws(precision, dual ? 2 : 1, B, H, W, Cin, Cout, merge_h, merge_w, win_h, win_w);
}

size_t swf_patch_unmerge_prec_workspace_bytes(int32_t precision, int32_t dual, int32_t B, int32_t Hp, int32_t Wp, int32_t Hm, int32_t Wm,
                                              int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t Hout, int32_t Wout) {
    if ((precision != SWF_PREC_FP32 && precision != SWF_PREC_FAST) || B <= 0 || Cin <= 0 || Cout <= 0 || merge_h <= 0 || merge_w <= 0 ||
        unmerge_shapes(Hp, Wp, Hm, Wm, merge_h, merge_w, Hout, Wout) != SWF_OK)
        return 0;
    return unmerge_prec_ws(precision, dual ? 2 : 1, B, Hp, Wp, Hm, Wm, Cin, Cout, merge_h, merge_w, Hout, Wout);
}

int swf_patch_merge_fwd_prec_act(const swf_activation* act_, int32_t precision, const swf_patch_params* px, const swf_patch_params* py,
                                 const float* x_in, const float* y_in, float* x_out, float* y_out, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                 int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w, const swf_patch_ln1* ln1_x,
                                 const swf_patch_ln1* ln1_y, int32_t* route, void* workspace, size_t workspace_bytes, swf_stream_t stream_) {
    SWF_TRY(check_patch_prec("patch_merge_prec", precision, px, py, x_in, y_in, x_out, y_out, ln1_x, ln1_y, B, Cin, Cout, merge_h, merge_w));
    int Hm, Wm, Ho, Wo;
    SWF_TRY(merge_shapes(H, W, merge_h, merge_w, win_h, win_w, &Hm, &Wm, &Ho, &Wo));
    const swf_activation act = act_or_default(act_);
    SWF_TRY(check_activation(act, "patch_merge_prec"));
    const int nstream = py ? 2 : 1, fast = precision == SWF_PREC_FAST;
    const size_t image = fast ? patch_image_bytes(0, Cin, Cout, merge_h, merge_w) : 0;
    Carver ws(workspace, workspace_bytes);
    const PatchPrecBufs bufs = carve_patch_prec(ws, nstream, image, merge_ws(nstream, B, H, W, Cin, Cout, merge_h, merge_w, win_h, win_w));
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "patch_merge_prec: workspace too small (need %zu B)", ws.bytes());
    hipStream_t stream = as_stream(stream_);
    const swf_patch_params* pp[2] = {px, py};
    const float* ins[2] = {x_in, y_in};
    float* outs[2] = {x_out, y_out};
    const swf_patch_ln1* ln[2] = {ln1_x, ln1_y};
    swf_block_stream_params blk[2] = {};   // the block behind the layer: only its LN1 is read
    const swf_block_stream_params* blkp[2] = {&blk[0], &blk[1]};
    for (int s = 0; s < nstream; ++s) {
        if (image) SWF_TRY(pack_patch_image(0, Cin, Cout, merge_h, merge_w, *pp[s], bufs.packed[s], stream));
        if (ln[0]) blk[s].ln1 = ln[s]->ln;
    }
    bool ln1_ready = false;
    PatchTrace tr{};
    SWF_TRY(patch_merge_impl(pp, nstream, ins, outs, B, H, W, Cin, Cout, merge_h, merge_w, win_h, win_w, bufs.inner, bufs.inner_bytes, stream,
                             fast, image ? bufs.packed : nullptr, ln[0] ? blkp : nullptr, ln[0] ? &ln1_ready : nullptr, &tr, act));
    return finish_patch_prec("patch_merge_prec", tr, ln, nstream, (size_t)B * Ho * Wo * Cout * sizeof(bf16_raw), route, stream);
}
int swf_patch_merge_fwd_prec(int32_t precision, const swf_patch_params* px, const swf_patch_params* py, const float* x_in, const float* y_in,
                             float* x_out, float* y_out, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t merge_h,
                             int32_t merge_w, int32_t win_h, int32_t win_w, const swf_patch_ln1* ln1_x, const swf_patch_ln1* ln1_y,
                             int32_t* route, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return swf_patch_merge_fwd_prec_act(nullptr, precision, px, py, x_in, y_in, x_out, y_out, B, H, W, Cin, Cout, merge_h, merge_w, win_h, win_w,
                                        ln1_x, ln1_y, route, workspace, workspace_bytes, stream);
}

int swf_patch_unmerge_fwd_prec_act(const swf_activation* act_, int32_t precision, const swf_patch_params* px, const swf_patch_params* py,
                                   const float* x_in, const float* y_in, const float* x_skip, const float* y_skip, float* x_out, float* y_out,
                                   int32_t B, int32_t Hp, int32_t Wp, int32_t Hm, int32_t Wm, int32_t Cin, int32_t Cout, int32_t merge_h,
                                   int32_t merge_w, int32_t Hout, int32_t Wout, const swf_patch_ln1* ln1_x, const swf_patch_ln1* ln1_y,
                                   int32_t* route, void* workspace, size_t workspace_bytes, swf_stream_t stream_) {
    const swf_activation act = act_or_default(act_);
    SWF_TRY(check_patch_prec("patch_unmerge_prec", precision, px, py, x_in, y_in, x_out, y_out, ln1_x, ln1_y, B, Cin, Cout, merge_h, merge_w));
    if (py && (x_skip != nullptr) != (y_skip != nullptr)) return fail(SWF_ERR_NULL, "patch_unmerge_prec: skip is given for every stream or for none");
    SWF_TRY(unmerge_shapes(Hp, Wp, Hm, Wm, merge_h, merge_w, Hout, Wout));
    SWF_TRY(check_activation(act, "patch_unmerge_prec"));
    const int nstream = py ? 2 : 1, fast = precision == SWF_PREC_FAST;
    const size_t image = fast ? patch_image_bytes(1, Cin, Cout, merge_h, merge_w) : 0;
    Carver ws(workspace, workspace_bytes);
    const PatchPrecBufs bufs = carve_patch_prec(ws, nstream, image, unmerge_ws(nstream, B, Hp, Wp, Hm, Wm, Cin, Cout, merge_h, merge_w, Hout, Wout));
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "patch_unmerge_prec: workspace too small (need %zu B)", ws.bytes());
    hipStream_t stream = as_stream(stream_);
    const swf_patch_params* pp[2] = {px, py};
    const float* ins[2] = {x_in, y_in};
    const float* sk[2] = {x_skip, y_skip};
    float* outs[2] = {x_out, y_out};
    const swf_patch_ln1* ln[2] = {ln1_x, ln1_y};
    swf_block_stream_params blk[2] = {};   // the block behind the layer: only its LN1 is read
    const swf_block_stream_params* blkp[2] = {&blk[0], &blk[1]};
    for (int s = 0; s < nstream; ++s) {
        if (image) SWF_TRY(pack_patch_image(1, Cin, Cout, merge_h, merge_w, *pp[s], bufs.packed[s], stream));
        if (ln[0]) blk[s].ln1 = ln[s]->ln;
    }
    bool ln1_ready = false;
    PatchTrace tr{};
    SWF_TRY(patch_unmerge_impl(pp, nstream, ins, x_skip ? sk : nullptr, outs, B, Hp, Wp, Hm, Wm, Cin, Cout, merge_h, merge_w, Hout, Wout,
                               bufs.inner, bufs.inner_bytes, stream, fast, image ? bufs.packed : nullptr, nullptr, 0, nullptr,
                               ln[0] ? blkp : nullptr, ln[0] ? &ln1_ready : nullptr, &tr, act));
    return finish_patch_prec("patch_unmerge_prec", tr, ln, nstream, (size_t)B * Hout * Wout * Cout * sizeof(bf16_raw), route, stream);
}
int swf_patch_unmerge_fwd_prec(int32_t precision, const swf_patch_params* px, const swf_patch_params* py, const float* x_in,
                               const float* y_in, const float* x_skip, const float* y_skip, float* x_out, float* y_out, int32_t B, int32_t Hp,
                               int32_t Wp, int32_t Hm, int32_t Wm, int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t Hout,
                               int32_t Wout, const swf_patch_ln1* ln1_x, const swf_patch_ln1* ln1_y, int32_t* route, void* workspace,
                               size_t workspace_bytes, swf_stream_t stream) {
    return swf_patch_unmerge_fwd_prec_act(nullptr, precision, px, py, x_in, y_in, x_skip, y_skip, x_out, y_out, B, Hp, Wp, Hm, Wm, Cin, Cout,
                                          merge_h, merge_w, Hout, Wout, ln1_x, ln1_y, route, workspace, workspace_bytes, stream);
}

static float* carve_head_fwd(Carver& ws, int B, int H, int W) { return ws.floats((int64_t)B * H * W * 2); }   // conv1's two channels

int swf_final_head_fwd_act(const swf_activation* act_, const swf_head_params* p, const float* x, const float* y, float* out, int32_t B, int32_t H,
                           int32_t W, int32_t ksize, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    const swf_activation act = act_or_default(act_);
    if (!p || !x || !y || !out) return fail(SWF_ERR_NULL, "final_head: NULL argument");
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "final_head: empty tensor");
    if (ksize <= 0 || ksize % 2 == 0) return fail(SWF_ERR_UNSUPPORTED, "final_head: even kernel size %d", ksize);
    if (ksize / 2 >= H || ksize / 2 >= W) return fail(SWF_ERR_PAD, "final_head: reflect pad %d >= map %dx%d", ksize / 2, H, W);
    SWF_TRY(check_activation(act, "final_head"));
    Carver ws(workspace, workspace_bytes);
    float* tmp = carve_head_fwd(ws, B, H, W);
    // no size query: swinfuse.h documents 2*B*H*W floats, so exactly that many bytes are enough, aligned or not
    if (!workspace || ws.used > workspace_bytes) return fail(SWF_ERR_WORKSPACE, "final_head workspace too small (need %zu B)", ws.used);
    return launch_head(x, y, tmp, out, *p, B, H, W, ksize, as_stream(stream), Act(act));
}
int swf_final_head_fwd(const swf_head_params* p, const float* x, const float* y, float* out, int32_t B, int32_t H, int32_t W,
                       int32_t ksize, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return swf_final_head_fwd_act(nullptr, p, x, y, out, B, H, W, ksize, workspace, workspace_bytes, stream);
}

// `act` (0 / 1) says whether the activation `fn` is applied at all
static Act linear_act(int act, const swf_activation& fn) { return act ? Act(fn) : Act(0); }

int swf_linear_fwd_act(const swf_activation* act_fn, const swf_linear* lin, const float* in, const float* residual, float* out, int64_t tokens,
                       int32_t n_in, int32_t n_out, int32_t act, swf_stream_t stream) {
    const swf_activation fn = act_or_default(act_fn);
    if (!lin || !lin->weight || !in || !out) return fail(SWF_ERR_NULL, "linear: NULL argument");
    if (tokens <= 0 || tokens > INT32_MAX || n_in <= 0 || n_out <= 0) return fail(SWF_ERR_BAD_SHAPE, "linear: bad sizes");
    if (act != 0 && act != 1) return fail(SWF_ERR_UNSUPPORTED, "linear: activation %d", act);
    SWF_TRY(check_activation(fn, "linear"));
    GemmBatch gb{};
    gb.p[0] = GemmProb{in, lin->weight, lin->bias, residual, out};
    return launch_gemm_f32(gb, 1, (int)tokens, n_out, n_in, n_in, n_out, linear_act(act, fn), as_stream(stream));
}
int swf_linear_fwd(const swf_linear* lin, const float* in, const float* residual, float* out, int64_t tokens, int32_t n_in,
                   int32_t n_out, int32_t act, swf_stream_t stream) {
    return swf_linear_fwd_act(nullptr, lin, in, residual, out, tokens, n_in, n_out, act, stream);
}

static GemmBatch carve_linear(Carver& ws, int64_t tokens, int32_t n_in, int32_t n_out) {   // fast tier: the split-K partials
    GemmBatch gb{};
    gb.scratch_floats = splitk_need(n_in, tokens * n_out);
    gb.scratch = ws.floats(gb.scratch_floats);
    return gb;
}

size_t swf_linear_workspace_bytes(int32_t precision, int64_t tokens, int32_t n_in, int32_t n_out) {
    if (precision != SWF_PREC_FAST || tokens <= 0 || n_in <= 0 || n_out <= 0) return 0;
    Carver m = Carver::measure();
    carve_linear(m, tokens, n_in, n_out);
    return m.bytes();
}

int swf_linear_fwd_prec_act(const swf_activation* act_fn, const swf_linear* lin, int32_t precision, const float* in, const float* residual,
                            float* out, int64_t tokens, int32_t n_in, int32_t n_out, int32_t act, void* workspace, size_t workspace_bytes,
                            swf_stream_t stream) {
    if (precision == SWF_PREC_FP32) return swf_linear_fwd_act(act_fn, lin, in, residual, out, tokens, n_in, n_out, act, stream);
    const swf_activation fn = act_or_default(act_fn);
    if (precision != SWF_PREC_FAST) return fail(SWF_ERR_BAD_SHAPE, "linear: unknown precision %d", precision);
    if (!lin || !lin->weight || !in || !out) return fail(SWF_ERR_NULL, "linear: NULL argument");
    if (tokens <= 0 || tokens > INT32_MAX || n_in <= 0 || n_out <= 0) return fail(SWF_ERR_BAD_SHAPE, "linear: bad sizes");
    if (act != 0 && act != 1) return fail(SWF_ERR_UNSUPPORTED, "linear: activation %d", act);
    SWF_TRY(check_activation(fn, "linear"));
    Carver ws(workspace, workspace_bytes);
    GemmBatch gb = carve_linear(ws, tokens, n_in, n_out);
    if (!ws.ok()) return fail(SWF_ERR_WORKSPACE, "linear: workspace too small (need %zu B)", ws.bytes());
    gb.p[0] = GemmProb{in, lin->weight, lin->bias, residual, out};
    return launch_gemm_bf16x3(gb, 1, (int)tokens, n_out, n_in, n_in, n_out, linear_act(act, fn), as_stream(stream));
}
int swf_linear_fwd_prec(const swf_linear* lin, int32_t precision, const float* in, const float* residual, float* out, int64_t tokens,
                        int32_t n_in, int32_t n_out, int32_t act, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return swf_linear_fwd_prec_act(nullptr, lin, precision, in, residual, out, tokens, n_in, n_out, act, workspace, workspace_bytes, stream);
}

int swf_layernorm_fwd_act(const swf_activation* act_, const swf_norm* ln, const float* in, float* out, int64_t tokens, int32_t C, int32_t elu,
                          swf_stream_t stream) {
    const swf_activation act = act_or_default(act_);
    if (!ln || !ln->gamma || !ln->beta || !in || !out) return fail(SWF_ERR_NULL, "layernorm: NULL argument");
    if (tokens <= 0 || C <= 0) return fail(SWF_ERR_BAD_SHAPE, "layernorm: bad sizes");
    SWF_TRY(check_activation(act, "layernorm"));
    LnBatch lb{};
    lb.p[0] = LnProb{in, out, ln->gamma, ln->beta};
    return launch_layernorm(lb, 1, tokens, C, linear_act(elu, act), as_stream(stream));
}
int swf_layernorm_fwd(const swf_norm* ln, const float* in, float* out, int64_t tokens, int32_t C, int32_t elu, swf_stream_t stream) {
    return swf_layernorm_fwd_act(nullptr, ln, in, out, tokens, C, elu, stream);
}

int swf_reflect_pad_fwd(const float* in, float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t pad_h, int32_t pad_w,
                        swf_stream_t stream) {
    if (!in || !out) return fail(SWF_ERR_NULL, "reflect_pad: NULL tensor");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || pad_h < 0 || pad_w < 0) return fail(SWF_ERR_BAD_SHAPE, "reflect_pad: bad sizes");
    if (pad_h >= H || pad_w >= W)
        return fail(SWF_ERR_PAD, "Padding size should be less than the corresponding input dimension: pad (%d,%d) on a %dx%d map", pad_h, pad_w, H, W);
    return launch_reflect_pad(in, out, B, H, W, C, pad_h, pad_w, as_stream(stream));
}

int swf_crop_fwd(const float* in, float* out, int32_t B, int32_t Hp, int32_t Wp, int32_t H, int32_t W, int32_t C, swf_stream_t stream) {
    if (!in || !out) return fail(SWF_ERR_NULL, "crop: NULL tensor");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || H > Hp || W > Wp) return fail(SWF_ERR_BAD_SHAPE, "crop: bad sizes");
    PtrPair pp{};
    pp.in[0] = in; pp.out[0] = out;
    return launch_crop(pp, 1, B, Hp, Wp, H, W, C, as_stream(stream));
}

int swf_nchw_to_nhwc(const float* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, swf_stream_t stream) {
    if (!in || !out) return fail(SWF_ERR_NULL, "layout: NULL tensor");
    return launch_nchw_to_nhwc(in, out, B, C, H, W, as_stream(stream));
}
int swf_nhwc_to_nchw(const float* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, swf_stream_t stream) {
    if (!in || !out) return fail(SWF_ERR_NULL, "layout: NULL tensor");
    return launch_nhwc_to_nchw(in, out, B, C, H, W, as_stream(stream));
}

// ---- model ------------------------------------------------------------------------------------
int32_t swf_model_param_count(const swf_model_desc* desc) {
    if (check_model_desc(desc) != SWF_OK) return -1;
    return (int32_t)get_layout(desc)->entries.size();
}
int64_t swf_model_arena_elems(const swf_model_desc* desc) {
    if (check_model_desc(desc) != SWF_OK) return -1;
    return get_layout(desc)->total;
}
int swf_model_param_info(const swf_model_desc* desc, int32_t index, char* name_buf, size_t name_buf_len, int64_t* offset_elems,
                         int64_t* numel) {
    SWF_TRY(check_model_desc(desc));
    const ModelLayout* l = get_layout(desc);
    if (index < 0 || index >= (int32_t)l->entries.size()) return fail(SWF_ERR_BAD_SHAPE, "param index %d out of range", index);
    const ParamEntry& e = l->entries[index];
    if (name_buf && name_buf_len) {
        if (e.name.size() + 1 > name_buf_len) return fail(SWF_ERR_WORKSPACE, "name buffer too small (%zu needed)", e.name.size() + 1);
        std::memcpy(name_buf, e.name.c_str(), e.name.size() + 1);
    }
    if (offset_elems) *offset_elems = e.offset;
    if (numel) *numel = e.numel;
    return SWF_OK;
}

// workspace layout: per level two activation maps (x, y), two full-resolution decoder outputs,
// then one scratch region shared by every unit: the largest of their measured needs.
static size_t model_scratch_bytes(const swf_model_desc* d, int B, const LevelShape* ls) {
    size_t scratch = 0;
    for (int s = 0; s < d->levels; ++s) {
        swf_block_desc be = level_block_desc(d, s, true), bd = level_block_desc(d, s, false);
        scratch = std::max(scratch, std::max(block_generic_ws(&be, 2, B, ls[s].Ho, ls[s].Wo), block_generic_ws(&bd, 2, B, ls[s].Ho, ls[s].Wo)));
        scratch = std::max(scratch, std::max(window_block_ws(be, B, ls[s].Ho, ls[s].Wo), window_block_ws(bd, B, ls[s].Ho, ls[s].Wo)));
        scratch = std::max(scratch, merge_ws(2, B, ls[s].Hin, ls[s].Win, d->in_dims[s], d->out_dims[s], d->merge_h, d->merge_w, d->win_h, d->win_w));
        scratch = std::max(scratch, unmerge_ws(2, B, ls[s].Ho, ls[s].Wo, ls[s].Hm, ls[s].Wm, d->out_dims[s], d->in_dims[s], d->merge_h, d->merge_w,
                                               ls[s].Hin, ls[s].Win));
    }
    Carver head = Carver::measure();
    carve_head_fwd(head, B, ls[0].Hin, ls[0].Win);
    return std::max(scratch, head.bytes());
}
struct ModelBufs { float *act[SWF_MAX_LEVELS][2], *full[2], *scratch; size_t scratch_bytes; };
static ModelBufs carve_model(Carver& ws, const swf_model_desc* d, int B, int H, int W, const LevelShape* ls) {
    ModelBufs b{};
    for (int s = 0; s < d->levels; ++s)
        for (int t = 0; t < 2; ++t) b.act[s][t] = ws.floats((int64_t)B * ls[s].Ho * ls[s].Wo * d->out_dims[s]);
    for (int t = 0; t < 2; ++t) b.full[t] = ws.floats((int64_t)B * H * W * d->in_dims[0]);
    b.scratch_bytes = model_scratch_bytes(d, B, ls);
    b.scratch = ws.floats((int64_t)(b.scratch_bytes / 4));
    return b;
}

size_t swf_model_workspace_bytes(const swf_model_desc* desc, int32_t B, int32_t H, int32_t W) {
    if (check_model_desc(desc) != SWF_OK || B <= 0) return 0;
    LevelShape ls[SWF_MAX_LEVELS];
    if (model_shapes(desc, H, W, ls) != SWF_OK) return 0;
    Carver m = Carver::measure();
    carve_model(m, desc, B, H, W, ls);
    return m.bytes();
}

size_t swf_model_packed_bytes(const swf_model_desc* desc) {
    if (check_model_desc(desc) != SWF_OK || !act_is_default(desc->act)) return 0;   // (no image is read for another activation)
    return packed_plan(desc).total;
}

int swf_model_pack_weights(const swf_model_desc* desc, const float* arena, void* packed, size_t packed_bytes, swf_stream_t stream_) {
    SWF_TRY(check_model_desc(desc));
    if (!arena) return fail(SWF_ERR_NULL, "model_pack_weights: NULL arena");
    const PackedPlan plan = packed_plan(desc);
    if (plan.total == 0 || !act_is_default(desc->act)) return SWF_OK;
    if (!packed || packed_bytes < plan.total) return fail(SWF_ERR_WORKSPACE, "packed buffer too small (need %zu B)", plan.total);
    const ModelLayout* L = get_layout(desc);
    hipStream_t stream = as_stream(stream_);
    char* base = static_cast<char*>(packed);
    for (int pass = 0; pass < 2; ++pass)
        for (int k = 0; k < desc->levels; ++k) {
            const bool enc = pass == 0;
            if (!(enc ? plan.enc_on[k] : plan.dec_on[k])) continue;
            swf_block_desc bd = level_block_desc(desc, enc ? k : desc->levels - 1 - k, enc);
            bd.precision = SWF_PREC_FAST;
            const size_t pb = block_packed_bytes(bd);
            const bool fused = window_block_packed_bytes(bd) > 0;
            char* dst = base + (enc ? plan.enc[k] : plan.dec[k]);
            for (int i = 0; i < 4; ++i) {
                const swf_block_stream_params px = make_stream_params(arena, enc ? L->enc_blk[k][i][0] : L->dec_blk[k][i][0]);
                const swf_block_stream_params py = make_stream_params(arena, enc ? L->enc_blk[k][i][1] : L->dec_blk[k][i][1]);
                if (fused) {
                    SWF_TRY(pack_window_block(bd, px, py, dst + (size_t)(2 * i) * pb, dst + (size_t)(2 * i + 1) * pb, stream));
                } else {
                    SWF_TRY(pack_deep_block(bd, px, dst + (size_t)(2 * i) * pb, stream));
                    SWF_TRY(pack_deep_block(bd, py, dst + (size_t)(2 * i + 1) * pb, stream));
                }
            }
        }
    for (int k = 0; k < desc->levels; ++k) {   // patch layers of the register-resident kernel
        const int lvl = desc->levels - 1 - k;
        for (int st = 0; st < 2; ++st) {
            if (plan.penc_b[k]) {
                const PatchOff& o = L->enc_patch[k][st];
                SWF_TRY(pack_patch_image(0, desc->in_dims[k], desc->out_dims[k], desc->merge_h, desc->merge_w,
                                         swf_patch_params{{arena + o.w, arena + o.b}, {arena + o.g, arena + o.bt}},
                                         base + plan.penc[k] + st * plan.penc_b[k], stream));
            }
            if (plan.pdec_b[k]) {
                const PatchOff& o = L->dec_patch[k][st];
                SWF_TRY(pack_patch_image(1, desc->out_dims[lvl], desc->in_dims[lvl], desc->merge_h, desc->merge_w,
                                         swf_patch_params{{arena + o.w, arena + o.b}, {arena + o.g, arena + o.bt}},
                                         base + plan.pdec[k] + st * plan.pdec_b[k], stream));
            }
        }
    }
    return SWF_OK;
}

static int model_forward_impl(const swf_model_desc* desc, const float* arena, const char* packed, const float* ir, const float* vis, float* out,
                              int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream_,
                              int32_t* equal_flags = nullptr, hipEvent_t* marks = nullptr) {
    // marks (swf_model_forward_profiled): 4 * levels + 2 events, recorded on the stream at the start and after every segment
    SWF_TRY(check_model_desc(desc));
    const PackedPlan plan = packed_plan(desc);
    if (!act_is_default(desc->act)) packed = nullptr;   // every level runs the generic family: the images are not read
    if (!arena || !ir || !vis || !out) return fail(SWF_ERR_NULL, "model_forward: NULL tensor");
    if (B <= 0) return fail(SWF_ERR_BAD_SHAPE, "model_forward: empty batch");
    LevelShape ls[SWF_MAX_LEVELS];
    SWF_TRY(model_shapes(desc, H, W, ls));
    const ModelLayout* L = get_layout(desc);
    hipStream_t stream = as_stream(stream_);
    const int n = desc->levels;
    Carver ws(workspace, workspace_bytes);
    const ModelBufs bufs = carve_model(ws, desc, B, H, W, ls);
    if (!workspace || !ws.ok()) return fail(SWF_ERR_WORKSPACE, "model workspace too small: have %zu B, need %zu B", workspace_bytes, ws.bytes());

    auto patch_params = [&](const PatchOff& o) { return swf_patch_params{{arena + o.w, arena + o.b}, {arena + o.g, arena + o.bt}}; };

    int nmark = 0;
    auto mark = [&]() -> int {
        if (marks && hipEventRecord(marks[nmark++], stream) != hipSuccess) return fail(SWF_ERR_HIP, "model_forward: hipEventRecord failed");
        return SWF_OK;
    };
    SWF_TRY(mark());
    // encoder (a013:215-220)
    const float* cur[2] = {ir, vis};
    bool ln1_carry = false;   // deep levels: the LN1 planes of the next block to run are in place (deep_ln1_planes)
    swf_block_stream_params dpx0 = make_stream_params(arena, L->dec_blk[0][0][0]), dpy0 = make_stream_params(arena, L->dec_blk[0][0][1]);
    const swf_block_stream_params* dec_first[2] = {&dpx0, &dpy0};   // first block of the decoder stage that follows the deepest encoder stage
    for (int s = 0; s < n; ++s) {
        swf_patch_params pm[2] = {patch_params(L->enc_patch[s][0]), patch_params(L->enc_patch[s][1])};
        const swf_patch_params* pmp[2] = {&pm[0], &pm[1]};
        const void* prr_enc[2] = {packed ? packed + plan.penc[s] : nullptr, packed ? packed + plan.penc[s] + plan.penc_b[s] : nullptr};
        swf_block_stream_params px[4], py[4];
        for (int i = 0; i < 4; ++i) { px[i] = make_stream_params(arena, L->enc_blk[s][i][0]); py[i] = make_stream_params(arena, L->enc_blk[s][i][1]); }
        swf_block_desc bd = level_block_desc(desc, s, true);
        const swf_block_stream_params* first_blk[2] = {&px[0], &py[0]};
        const bool deep_stage = packed && desc->precision == SWF_PREC_FAST && window_block_packed_bytes(bd) == 0 && deep_block_supported(bd);
        ln1_carry = false;
        SWF_TRY(patch_merge_impl(pmp, 2, cur, bufs.act[s], B, ls[s].Hin, ls[s].Win, desc->in_dims[s], desc->out_dims[s], desc->merge_h,
                                 desc->merge_w, desc->win_h, desc->win_w, bufs.scratch, bufs.scratch_bytes, stream, desc->precision == SWF_PREC_FAST,
                                 (packed && plan.penc_b[s]) ? prr_enc : nullptr, deep_stage ? first_blk : nullptr, deep_stage ? &ln1_carry : nullptr,
                                 nullptr, desc->act));
        SWF_TRY(mark());
        // the first block of the next fused-kernel stage is warmed by this stage's last block
        const char* after = nullptr;
        size_t after_pb = 0;
        if (packed && s + 1 < n) {
            swf_block_desc nb = level_block_desc(desc, s + 1, true);
            if (window_block_packed_bytes(nb) && plan.enc_on[s + 1]) { after = packed + plan.enc[s + 1]; after_pb = window_block_packed_bytes(nb); }
        }
        // the deepest stage hands the LN1 planes of the decoder's first block (same level, same map, same workspace) to it
        const bool chain = deep_stage && s == n - 1;
        SWF_TRY(block_pair4_impl(&bd, px, py, bufs.act[s][0], bufs.act[s][1], bufs.act[s][0], bufs.act[s][1], B, ls[s].Ho, ls[s].Wo, bufs.scratch, bufs.scratch_bytes, stream,
                                 (packed && plan.enc_on[s]) ? packed + plan.enc[s] : nullptr, after, after_pb,
                                 equal_flags ? equal_flags + 2 * s : nullptr, chain ? dec_first : nullptr, deep_stage ? &ln1_carry : nullptr));
        if (!chain) ln1_carry = false;
        SWF_TRY(mark());
        cur[0] = bufs.act[s][0]; cur[1] = bufs.act[s][1];
    }
    // decoder (a013:221-227): the skip add of stage j+1 is folded into stage j's unmerge epilogue,
    // written in place over the encoder activation of the level below.
    for (int j = 0; j < n; ++j) {
        const int lvl = n - 1 - j;
        swf_block_stream_params px[4], py[4];
        for (int i = 0; i < 4; ++i) { px[i] = make_stream_params(arena, L->dec_blk[j][i][0]); py[i] = make_stream_params(arena, L->dec_blk[j][i][1]); }
        swf_block_desc bd = level_block_desc(desc, lvl, false);
        const char* after = nullptr;
        size_t after_pb = 0;
        if (packed && j + 1 < n) {
            swf_block_desc nb = level_block_desc(desc, n - 2 - j, false);
            if (window_block_packed_bytes(nb) && plan.dec_on[j + 1]) { after = packed + plan.dec[j + 1]; after_pb = window_block_packed_bytes(nb); }
        }
        bool ln1_in = ln1_carry;   // planes left by the deepest encoder stage (j == 0) or by the unmerge layer of the stage before
        SWF_TRY(block_pair4_impl(&bd, px, py, bufs.act[lvl][0], bufs.act[lvl][1], bufs.act[lvl][0], bufs.act[lvl][1], B, ls[lvl].Ho, ls[lvl].Wo, bufs.scratch, bufs.scratch_bytes, stream,
                                 (packed && plan.dec_on[j]) ? packed + plan.dec[j] : nullptr, after, after_pb,
                                 equal_flags ? equal_flags + 2 * (n + j) : nullptr, nullptr, &ln1_in));
        SWF_TRY(mark());
        // a deep-level stage cannot warm its successor from inside a block kernel: its patch layer does it (or one small launch)
        const bool warm_next = after && window_block_packed_bytes(bd) == 0;
        bool warmed = false;
        // the next decoder stage, when it is a deep-level one, finds its first block's LN1 planes written by this stage's unmerge layer
        swf_block_stream_params npx0{}, npy0{};
        bool next_deep = false;
        if (packed && desc->precision == SWF_PREC_FAST && j + 1 < n) {
            swf_block_desc nb = level_block_desc(desc, n - 2 - j, false);
            nb.precision = SWF_PREC_FAST;
            next_deep = window_block_packed_bytes(nb) == 0 && deep_block_supported(nb);
            if (next_deep) { npx0 = make_stream_params(arena, L->dec_blk[j + 1][0][0]); npy0 = make_stream_params(arena, L->dec_blk[j + 1][0][1]); }
        }
        const swf_block_stream_params* next_first[2] = {&npx0, &npy0};
        ln1_carry = false;
        swf_patch_params pm[2] = {patch_params(L->dec_patch[j][0]), patch_params(L->dec_patch[j][1])};
        const swf_patch_params* pmp[2] = {&pm[0], &pm[1]};
        const float* ins[2] = {bufs.act[lvl][0], bufs.act[lvl][1]};
        const float* skip[2] = {lvl > 0 ? bufs.act[lvl - 1][0] : nullptr, lvl > 0 ? bufs.act[lvl - 1][1] : nullptr};
        float* outs[2] = {lvl > 0 ? bufs.act[lvl - 1][0] : bufs.full[0], lvl > 0 ? bufs.act[lvl - 1][1] : bufs.full[1]};
        const void* prr_dec[2] = {packed ? packed + plan.pdec[j] : nullptr, packed ? packed + plan.pdec[j] + plan.pdec_b[j] : nullptr};
        SWF_TRY(patch_unmerge_impl(pmp, 2, ins, lvl > 0 ? skip : nullptr, outs, B, ls[lvl].Ho, ls[lvl].Wo, ls[lvl].Hm, ls[lvl].Wm,
                                   desc->out_dims[lvl], desc->in_dims[lvl], desc->merge_h, desc->merge_w, ls[lvl].Hin, ls[lvl].Win,
                                   bufs.scratch, bufs.scratch_bytes, stream, desc->precision == SWF_PREC_FAST, (packed && plan.pdec_b[j]) ? prr_dec : nullptr,
                                   warm_next ? after : nullptr, warm_next ? after_pb : 0, &warmed, next_deep ? next_first : nullptr,
                                   next_deep ? &ln1_carry : nullptr, nullptr, desc->act));
        if (warm_next && !warmed) SWF_TRY(launch_l2_warm(after, 2 * after_pb, stream));
        SWF_TRY(mark());
    }
    swf_head_params hp{arena + L->h_c1w, arena + L->h_c1b, arena + L->h_g, arena + L->h_b, arena + L->h_m, arena + L->h_v,
                       arena + L->h_c2w, arena + L->h_c2b};
    Carver hw(bufs.scratch, bufs.scratch_bytes);
    float* tmp = carve_head_fwd(hw, B, H, W);
    SWF_TRY(launch_head(bufs.full[0], bufs.full[1], tmp, out, hp, B, H, W, desc->head_ksize, stream, Act(desc->act)));
    return mark();
}

int swf_model_forward(const swf_model_desc* desc, const float* arena, const float* ir, const float* vis, float* out,
                      int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return model_forward_impl(desc, arena, nullptr, ir, vis, out, B, H, W, workspace, workspace_bytes, stream);
}

int swf_model_forward_packed(const swf_model_desc* desc, const float* arena, const void* packed, const float* ir, const float* vis,
                             float* out, int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return model_forward_impl(desc, arena, static_cast<const char*>(packed), ir, vis, out, B, H, W, workspace, workspace_bytes, stream);
}

int swf_model_forward_checked(const swf_model_desc* desc, const float* arena, const void* packed, const float* ir, const float* vis,
                              float* out, int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes,
                              int32_t* cross_equal_flags, swf_stream_t stream) {
    if (!cross_equal_flags) return fail(SWF_ERR_NULL, "model_forward_checked: NULL flags");
    if (check_model_desc(desc) != SWF_OK) return SWF_ERR_BAD_SHAPE;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(cross_equal_flags), 1, (size_t)4 * desc->levels, as_stream(stream));
    if (e != hipSuccess) return fail(SWF_ERR_HIP, "model_forward_checked: memset: %s", hipGetErrorString(e));
    return model_forward_impl(desc, arena, static_cast<const char*>(packed), ir, vis, out, B, H, W, workspace, workspace_bytes, stream,
                              cross_equal_flags);
}

int swf_model_forward_profiled(const swf_model_desc* desc, const float* arena, const void* packed, const float* ir, const float* vis,
                               float* out, int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, float* seg_ms,
                               int32_t seg_count, swf_stream_t stream) {
    if (!seg_ms) return fail(SWF_ERR_NULL, "model_forward_profiled: NULL seg_ms");
    if (check_model_desc(desc) != SWF_OK) return SWF_ERR_BAD_SHAPE;
    const int nseg = 4 * desc->levels + 1;
    if (seg_count < nseg) return fail(SWF_ERR_BAD_SHAPE, "model_forward_profiled: seg_ms holds %d values, need %d", seg_count, nseg);
    hipEvent_t ev[4 * SWF_MAX_LEVELS + 2];
    int made = 0, st = SWF_OK;
    for (; made < nseg + 1; ++made)
        if (hipEventCreate(&ev[made]) != hipSuccess) { st = fail(SWF_ERR_HIP, "model_forward_profiled: hipEventCreate failed"); break; }
    if (st == SWF_OK)
        st = model_forward_impl(desc, arena, static_cast<const char*>(packed), ir, vis, out, B, H, W, workspace, workspace_bytes, stream, nullptr, ev);
    if (st == SWF_OK && hipStreamSynchronize(as_stream(stream)) != hipSuccess) st = fail(SWF_ERR_HIP, "model_forward_profiled: synchronize failed");
    for (int i = 0; st == SWF_OK && i < nseg; ++i)
        if (hipEventElapsedTime(&seg_ms[i], ev[i], ev[i + 1]) != hipSuccess) st = fail(SWF_ERR_HIP, "model_forward_profiled: hipEventElapsedTime failed");
    for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]);
    return st;
}

int swf_tensors_equal(const float* a, const float* b, int64_t count, int32_t* flag, swf_stream_t stream) {
    if (!flag) return fail(SWF_ERR_NULL, "tensors_equal: NULL flag");
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(flag), 1, 1, as_stream(stream));
    if (e != hipSuccess) return fail(SWF_ERR_HIP, "tensors_equal: memset: %s", hipGetErrorString(e));
    return launch_all_equal(a, b, count, flag, as_stream(stream));
}

// a008 MyLoss.  Every argument check comes before the first HIP call.
static int check_fusion_loss(const swf_loss_desc* desc, int32_t B, int32_t H, int32_t W) {
    if (!desc) return fail(SWF_ERR_NULL, "fusion_loss: NULL descriptor");
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "fusion_loss: empty tensor (B=%d H=%d W=%d)", B, H, W);
    if (desc->ssim_mode != 0 && desc->ssim_mode != 1)
        return fail(SWF_ERR_UNSUPPORTED, "fusion_loss: ssim_mode %d (0 = MS-SSIM + L1, 1 = single-scale SSIM)", desc->ssim_mode);
    if (desc->ssim_mode == 1 && (H < 6 || W < 6))
        return fail(SWF_ERR_PAD, "fusion_loss: the 11-tap SSIM window reflects 5 pixels, the map is %dx%d", H, W);
    return SWF_OK;
}

size_t swf_fusion_loss_workspace_bytes(const swf_loss_desc* desc, int32_t B, int32_t H, int32_t W, int32_t with_grad) {
    if (check_fusion_loss(desc, B, H, W) != SWF_OK) return 0;
    return fusion_loss_workspace_bytes(*desc, B, H, W, with_grad != 0);
}

int swf_fusion_loss(const swf_loss_desc* desc, const float* fusion, const float* ir, const float* vis, float* terms, float* grad_fusion,
                    int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    if (!desc || !fusion || !ir || !vis || !terms) return fail(SWF_ERR_NULL, "fusion_loss: NULL descriptor, image or terms");
    SWF_TRY(check_fusion_loss(desc, B, H, W));
    SWF_TRY(need_workspace("fusion_loss", workspace, workspace_bytes, fusion_loss_workspace_bytes(*desc, B, H, W, grad_fusion != nullptr)));
    return fusion_loss(*desc, fusion, ir, vis, terms, grad_fusion, B, H, W, workspace, workspace_bytes, as_stream(stream));
}

// The three evaluation calls: fusion-quality metrics; VIF and Nabf; SSIM, MS-SSIM and the Piella / Cvejic / Yang indices.  Every
// argument check comes before the first HIP call.  `holds` is what of the kernels the shape message says the shape exceeds.
static int check_metric_shape(const char* name, const char* holds, int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "%s: empty tensor (B=%d H=%d W=%d)", name, B, H, W);
    if (!metric_shape_ok(B, H, W))
        return fail(SWF_ERR_BAD_SHAPE, "%s: B=%d H=%d W=%d exceeds the kernels' %s (H W <= 2^30, B <= 65535)", name, B, H, W, holds);
    return SWF_OK;
}

// NULL check -> shape -> the descriptor's own check, if it has one -> workspace -> call.  A call that carves nothing needs no workspace
// (fusion_structure under 7 pixels in an axis: no window).
extern "C++" template <class DESC>
static int metric_call(const char* name, const char* holds, int (*check_desc)(const DESC&), size_t (*bytes)(int, int, int),
                       int (*run)(const DESC&, const float*, const float*, const float*, double*, int, int, int, void*, size_t, hipStream_t),
                       const DESC* desc, const float* fusion, const float* ir, const float* vis, double* out, int32_t B, int32_t H,
                       int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    if (!desc || !fusion || !ir || !vis || !out) return fail(SWF_ERR_NULL, "%s: NULL descriptor, image or output", name);
    SWF_TRY(check_metric_shape(name, holds, B, H, W));
    if (check_desc) SWF_TRY(check_desc(*desc));
    const size_t need = bytes(B, H, W);
    if (need > 0) SWF_TRY(need_workspace(name, workspace, workspace_bytes, need));
    return run(*desc, fusion, ir, vis, out, B, H, W, workspace, workspace_bytes, as_stream(stream));
}

size_t swf_fusion_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return check_metric_shape("fusion_metrics", "counters", B, H, W) == SWF_OK ? fusion_metrics_workspace_bytes(B, H, W) : 0;
}

int swf_fusion_metrics(const swf_metrics_desc* desc, const float* fusion, const float* ir, const float* vis, double* out,
                       int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return metric_call<swf_metrics_desc>("fusion_metrics", "counters", nullptr, fusion_metrics_workspace_bytes, fusion_metrics, desc, fusion,
                                         ir, vis, out, B, H, W, workspace, workspace_bytes, stream);
}

size_t swf_fusion_fidelity_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return check_metric_shape("fusion_fidelity", "grids", B, H, W) == SWF_OK ? fusion_fidelity_workspace_bytes(B, H, W) : 0;
}

int swf_fusion_fidelity(const swf_fidelity_desc* desc, const float* fusion, const float* ir, const float* vis, double* out,
                        int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return metric_call<swf_fidelity_desc>("fusion_fidelity", "grids", nullptr, fusion_fidelity_workspace_bytes, fusion_fidelity, desc, fusion,
                                          ir, vis, out, B, H, W, workspace, workspace_bytes, stream);
}

size_t swf_fusion_structure_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return check_metric_shape("fusion_structure", "grids", B, H, W) == SWF_OK ? fusion_structure_workspace_bytes(B, H, W) : 0;
}

static int check_structure_desc(const swf_structure_desc& d) {
    if (!std::isfinite(d.K1) || !std::isfinite(d.K2) || !std::isfinite(d.alpha) || !std::isfinite(d.Ty) || d.K1 <= 0.0 || d.K2 <= 0.0 ||
        d.alpha < 0.0)
        return fail(SWF_ERR_BAD_SHAPE, "fusion_structure: constants K1=%g K2=%g alpha=%g Ty=%g (finite, K1 > 0, K2 > 0, alpha >= 0)", d.K1,
                    d.K2, d.alpha, d.Ty);
    return SWF_OK;
}

int swf_fusion_structure(const swf_structure_desc* desc, const float* fusion, const float* ir, const float* vis, double* out,
                         int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    return metric_call<swf_structure_desc>("fusion_structure", "grids", check_structure_desc, fusion_structure_workspace_bytes,
                                           fusion_structure, desc, fusion, ir, vis, out, B, H, W, workspace, workspace_bytes, stream);
}

// The perception call's shape check: its transforms are dense, so what it holds is narrower than the other calls' and is its own status.
static int check_perception_shape(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "fusion_perception: empty tensor (B=%d H=%d W=%d)", B, H, W);
    if (!perception_shape_ok(B, H, W))
        return fail(SWF_ERR_UNSUPPORTED, "fusion_perception: B=%d H=%d W=%d exceeds the int32 indices of the dense transforms "
                    "(H, W <= 16384, B <= 13107)", B, H, W);
    return SWF_OK;
}

size_t swf_fusion_perception_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return check_perception_shape(B, H, W) == SWF_OK ? fusion_perception_workspace_bytes(B, H, W) : 0;
}

static int check_perception_desc(const swf_perception_desc& d) {
    const double v[7] = {d.f0, d.f1, d.a, d.p, d.q, d.Z, d.alpha};
    bool ok = d.f0 > 0.0 && d.f1 > 0.0 && d.Z > 0.0 && d.p >= 0.0 && d.q >= 0.0 && d.alpha >= 0.0;
    for (double x : v) ok = ok && std::isfinite(x);
    if (!ok)
        return fail(SWF_ERR_BAD_SHAPE, "fusion_perception: constants f0=%g f1=%g a=%g p=%g q=%g Z=%g alpha=%g (finite, f0 > 0, f1 > 0, "
                    "Z > 0, p >= 0, q >= 0, alpha >= 0)", d.f0, d.f1, d.a, d.p, d.q, d.Z, d.alpha);
    return SWF_OK;
}

int swf_fusion_perception(const swf_perception_desc* desc, const float* fusion, const float* ir, const float* vis, double* out,
                          int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    if (!desc || !fusion || !ir || !vis || !out) return fail(SWF_ERR_NULL, "fusion_perception: NULL descriptor, image or output");
    SWF_TRY(check_perception_shape(B, H, W));
    SWF_TRY(check_perception_desc(*desc));
    SWF_TRY(need_workspace("fusion_perception", workspace, workspace_bytes, fusion_perception_workspace_bytes(B, H, W)));
    return fusion_perception(*desc, fusion, ir, vis, out, B, H, W, workspace, workspace_bytes, as_stream(stream));
}

// The comparative-study call: dense transforms too, 24 planes per image.
static int check_comparative_shape(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "fusion_comparative: empty tensor (B=%d H=%d W=%d)", B, H, W);
    if (!comparative_shape_ok(B, H, W))
        return fail(SWF_ERR_UNSUPPORTED, "fusion_comparative: B=%d H=%d W=%d exceeds the int32 indices of the dense transforms "
                    "(H, W <= 16384, B <= 2730)", B, H, W);
    return SWF_OK;
}

size_t swf_fusion_comparative_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return check_comparative_shape(B, H, W) == SWF_OK ? fusion_comparative_workspace_bytes(B, H, W) : 0;
}

static int check_comparative_desc(const swf_comparative_desc& d) {
    const double v[14] = {d.q, d.alpha1, d.alpha2, d.min_wavelength, d.mult, d.sigma_onf, d.k, d.cutoff, d.g, d.eps, d.C, d.ep, d.eM, d.em};
    bool ok = d.q > 0.0 && d.q != 1.0 && d.mult > 1.0 && d.sigma_onf > 0.0 && d.sigma_onf < 1.0 && d.min_wavelength >= 2.0 && d.eps > 0.0 &&
              d.C > 0.0 && d.alpha1 >= 0.0 && d.alpha2 >= 0.0 && d.ep >= 0.0 && d.eM >= 0.0 && d.em >= 0.0;
    for (double x : v) ok = ok && std::isfinite(x);
    if (!ok)
        return fail(SWF_ERR_BAD_SHAPE, "fusion_comparative: constants q=%g alpha1=%g alpha2=%g min_wavelength=%g mult=%g sigma_onf=%g k=%g "
                    "cutoff=%g g=%g eps=%g C=%g ep=%g eM=%g em=%g (finite, q > 0, q != 1, mult > 1, 0 < sigma_onf < 1, min_wavelength >= 2, "
                    "eps > 0, C > 0, exponents >= 0)", d.q, d.alpha1, d.alpha2, d.min_wavelength, d.mult, d.sigma_onf, d.k, d.cutoff, d.g,
                    d.eps, d.C, d.ep, d.eM, d.em);
    return SWF_OK;
}

int swf_fusion_comparative(const swf_comparative_desc* desc, const float* fusion, const float* ir, const float* vis, double* out,
                           int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    if (!desc || !fusion || !ir || !vis || !out) return fail(SWF_ERR_NULL, "fusion_comparative: NULL descriptor, image or output");
    SWF_TRY(check_comparative_shape(B, H, W));
    SWF_TRY(check_comparative_desc(*desc));
    SWF_TRY(need_workspace("fusion_comparative", workspace, workspace_bytes, fusion_comparative_workspace_bytes(B, H, W)));
    return fusion_comparative(*desc, fusion, ir, vis, out, B, H, W, workspace, workspace_bytes, as_stream(stream));
}

// The feature-mutual-information call: dense DCT matrices, three transform planes per image.
static int check_feature_shape(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "fusion_feature: empty tensor (B=%d H=%d W=%d)", B, H, W);
    if (!feature_shape_ok(B, H, W))
        return fail(SWF_ERR_UNSUPPORTED, "fusion_feature: B=%d H=%d W=%d exceeds the int32 indices of the dense transforms "
                    "(H, W <= 16384, H W <= 2^30, B <= 21845)", B, H, W);
    return SWF_OK;
}

size_t swf_fusion_feature_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return check_feature_shape(B, H, W) == SWF_OK ? fusion_feature_workspace_bytes(B, H, W) : 0;
}

static int check_feature_desc(const swf_feature_desc& d) {
    if (!(d.window == 3.0 || d.window == 5.0) || !std::isfinite(d.dct_step) || !(d.dct_step > 0.0))
        return fail(SWF_ERR_BAD_SHAPE, "fusion_feature: constants window=%g dct_step=%g (window 3 or 5, dct_step finite and > 0)", d.window,
                    d.dct_step);
    return SWF_OK;
}

int swf_fusion_feature(const swf_feature_desc* desc, const float* fusion, const float* ir, const float* vis, double* out, int32_t B,
                       int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    if (!desc || !fusion || !ir || !vis || !out) return fail(SWF_ERR_NULL, "fusion_feature: NULL descriptor, image or output");
    SWF_TRY(check_feature_shape(B, H, W));
    SWF_TRY(check_feature_desc(*desc));
    SWF_TRY(need_workspace("fusion_feature", workspace, workspace_bytes, fusion_feature_workspace_bytes(B, H, W)));
    return fusion_feature(*desc, fusion, ir, vis, out, B, H, W, workspace, workspace_bytes, as_stream(stream));
}

// torch.optim.Adam over a table of tensors.  Every argument check, the table's own rows included, comes before the first HIP call.
static int64_t adam_max_chunks(int32_t n_tensors, int64_t total_elems) { return total_elems / kAdamChunk + n_tensors; }

size_t swf_adam_table_bytes(int32_t n_tensors, int64_t total_elems) {
    if (n_tensors <= 0 || total_elems < n_tensors || adam_max_chunks(n_tensors, total_elems) > INT32_MAX) return 0;
    return adam_layout(n_tensors, adam_max_chunks(n_tensors, total_elems)).total_bytes;
}

int swf_adam_table_fill(void* table_host, size_t table_bytes, int32_t n_tensors, const void* const* param, const void* const* grad,
                        const void* const* exp_avg, const void* const* exp_avg_sq, const int64_t* numel, const float* step_size,
                        const float* bc2_sqrt) {
    if (!table_host || !param || !grad || !exp_avg || !exp_avg_sq || !numel || !step_size || !bc2_sqrt)
        return fail(SWF_ERR_NULL, "adam_table_fill: NULL table or array");
    if (n_tensors <= 0) return fail(SWF_ERR_BAD_SHAPE, "adam_table_fill: %d tensors", n_tensors);
    int64_t n_chunks = 0;
    for (int32_t i = 0; i < n_tensors; ++i) {
        if (!param[i] || !grad[i] || !exp_avg[i] || !exp_avg_sq[i]) return fail(SWF_ERR_NULL, "adam_table_fill: tensor %d has a NULL pointer", i);
        if (numel[i] <= 0) return fail(SWF_ERR_BAD_SHAPE, "adam_table_fill: tensor %d has %lld elements", i, (long long)numel[i]);
        n_chunks += cdiv64(numel[i], kAdamChunk);
    }
    if (n_chunks > INT32_MAX) return fail(SWF_ERR_UNSUPPORTED, "adam_table_fill: %lld chunks", (long long)n_chunks);
    const AdamLayout lay = adam_layout(n_tensors, n_chunks);
    if (table_bytes < lay.total_bytes)
        return fail(SWF_ERR_WORKSPACE, "adam_table_fill: table of %zu bytes, %zu needed", table_bytes, lay.total_bytes);
    swf_adam_tensor* rows = static_cast<swf_adam_tensor*>(table_host);
    int32_t* map = reinterpret_cast<int32_t*>(static_cast<char*>(table_host) + lay.map_off);
    int32_t c = 0;
    for (int32_t i = 0; i < n_tensors; ++i) {
        swf_adam_tensor r;
        r.param = static_cast<float*>(const_cast<void*>(param[i]));
        r.grad = static_cast<const float*>(grad[i]);
        r.exp_avg = static_cast<float*>(const_cast<void*>(exp_avg[i]));
        r.exp_avg_sq = static_cast<float*>(const_cast<void*>(exp_avg_sq[i]));
        r.numel = numel[i];
        r.step_size = step_size[i];
        r.bc2_sqrt = bc2_sqrt[i];
        r.first_chunk = c;
        r.reserved = 0;
        rows[i] = r;
        for (int64_t k = cdiv64(numel[i], kAdamChunk); k > 0; --k) map[c++] = i;
    }
    return SWF_OK;
}

// Validate a filled host table against the buffer size, -> the number of chunks.  Reads host memory only.
// `flat` (swf_tensors_gather / _scatter): only `param`, the destination, must be set in every row; the moments are not read.
static int check_adam_table(const char* who, const void* table_host, void* table_device, size_t table_bytes, int32_t n_tensors,
                            int64_t* n_chunks_out, bool flat = false) {
    if (!table_host || !table_device) return fail(SWF_ERR_NULL, "%s: NULL table", who);
    if (n_tensors <= 0) return fail(SWF_ERR_BAD_SHAPE, "%s: %d tensors", who, n_tensors);
    if (table_bytes < (size_t)n_tensors * sizeof(swf_adam_tensor))
        return fail(SWF_ERR_WORKSPACE, "%s: table of %zu bytes cannot hold %d rows", who, table_bytes, n_tensors);
    const swf_adam_tensor* rows = static_cast<const swf_adam_tensor*>(table_host);
    int64_t c = 0;
    for (int32_t i = 0; i < n_tensors; ++i) {
        const swf_adam_tensor& r = rows[i];
        if (!r.param || (!flat && (!r.grad || !r.exp_avg || !r.exp_avg_sq))) return fail(SWF_ERR_NULL, "%s: row %d has a NULL pointer", who, i);
        if (r.numel <= 0 || r.first_chunk != c)
            return fail(SWF_ERR_BAD_SHAPE, "%s: row %d is not what swf_adam_table_fill writes (numel %lld, first chunk %d, expected %lld)", who, i,
                        (long long)r.numel, r.first_chunk, (long long)c);
        c += cdiv64(r.numel, kAdamChunk);
        if (c > INT32_MAX) return fail(SWF_ERR_UNSUPPORTED, "%s: too many chunks", who);
    }
    const AdamLayout lay = adam_layout(n_tensors, c);
    if (table_bytes < lay.total_bytes) return fail(SWF_ERR_WORKSPACE, "%s: table of %zu bytes, %zu needed", who, table_bytes, lay.total_bytes);
    const int32_t* map = reinterpret_cast<const int32_t*>(static_cast<const char*>(table_host) + lay.map_off);
    for (int64_t k = 0; k < c; ++k)   // the kernels index the rows with these: keep them inside the table
        if (map[k] < 0 || map[k] >= n_tensors || k < rows[map[k]].first_chunk ||
            k >= rows[map[k]].first_chunk + cdiv64(rows[map[k]].numel, kAdamChunk))
            return fail(SWF_ERR_BAD_SHAPE, "%s: chunk %lld maps to row %d, which does not cover it", who, (long long)k, map[k]);
    *n_chunks_out = c;
    return SWF_OK;
}

int swf_adam_grad_norm(double max_grad_norm, const void* table_pinned_host, void* table_device, size_t table_bytes, int32_t n_tensors,
                       float* norm_out_device, swf_stream_t stream) {
    if (!norm_out_device) return fail(SWF_ERR_NULL, "adam_grad_norm: NULL norm_out_device");
    if (!(max_grad_norm > 0)) return fail(SWF_ERR_BAD_SHAPE, "adam_grad_norm: max_grad_norm %g is not positive", max_grad_norm);
    int64_t n_chunks = 0;
    SWF_TRY(check_adam_table("adam_grad_norm", table_pinned_host, table_device, table_bytes, n_tensors, &n_chunks));
    AdamTable t;
    SWF_TRY(upload_adam_table("adam_grad_norm", table_pinned_host, table_device, n_tensors, n_chunks, as_stream(stream), &t));
    return launch_gradnorm(t.rows, t.map, t.n_chunks, t.partials, (float)max_grad_norm, norm_out_device, as_stream(stream));
}

int swf_adam_step(const swf_adam_desc* desc, const void* table_pinned_host, void* table_device, size_t table_bytes, int32_t n_tensors,
                  float* norm_out_device, swf_stream_t stream) {
    if (!desc) return fail(SWF_ERR_NULL, "adam_step: NULL descriptor");
    if (!(desc->beta1 >= 0 && desc->beta1 < 1 && desc->beta2 >= 0 && desc->beta2 < 1 && desc->eps >= 0 && desc->weight_decay >= 0))
        return fail(SWF_ERR_UNSUPPORTED, "adam_step: betas (%g, %g) must lie in [0, 1), eps %g and weight_decay %g must not be negative",
                    desc->beta1, desc->beta2, desc->eps, desc->weight_decay);
    const bool clip = desc->max_grad_norm > 0;
    if (clip && !norm_out_device) return fail(SWF_ERR_NULL, "adam_step: clipping is on and norm_out_device is NULL");
    int64_t n_chunks = 0;
    SWF_TRY(check_adam_table("adam_step", table_pinned_host, table_device, table_bytes, n_tensors, &n_chunks));
    AdamTable t;
    SWF_TRY(upload_adam_table("adam_step", table_pinned_host, table_device, n_tensors, n_chunks, as_stream(stream), &t));
    if (clip && !desc->norm_ready)
        SWF_TRY(launch_gradnorm(t.rows, t.map, t.n_chunks, t.partials, (float)desc->max_grad_norm, norm_out_device, as_stream(stream)));
    return launch_adam_multi(t.rows, t.map, t.n_chunks, *desc, clip ? norm_out_device : nullptr, as_stream(stream));
}

// Gather / scatter of a tensor list (kernels_flat.hip) over the optimiser's table.  The flat side of every row must be the unpadded
// running-sum segment of `flat`, so nothing outside flat[0, flat_elems) is touched; all of it is checked on the host before the upload.
static int tensors_flat(const char* who, bool gather, const void* table_pinned_host, void* table_device, size_t table_bytes, int32_t n_tensors,
                        float* flat, int64_t flat_elems, float scale, hipStream_t stream) {
    if (!flat) return fail(SWF_ERR_NULL, "%s: NULL flat buffer", who);
    int64_t n_chunks = 0;
    SWF_TRY(check_adam_table(who, table_pinned_host, table_device, table_bytes, n_tensors, &n_chunks, true));
    const swf_adam_tensor* rows = static_cast<const swf_adam_tensor*>(table_pinned_host);
    int64_t off = 0;
    for (int32_t i = 0; i < n_tensors; ++i) {
        const float* seg = gather ? rows[i].param : rows[i].grad;
        if (!gather && !seg) return fail(SWF_ERR_NULL, "%s: row %d has no source segment", who, i);
        if (seg != flat + off)
            return fail(SWF_ERR_BAD_SHAPE, "%s: row %d does not address element %lld of the flat buffer (segments are consecutive and unpadded)", who, i,
                        (long long)off);
        off += rows[i].numel;
    }
    if (off > flat_elems) return fail(SWF_ERR_BAD_SHAPE, "%s: %lld elements in a flat buffer of %lld", who, (long long)off, (long long)flat_elems);
    AdamTable t;
    SWF_TRY(upload_adam_table(who, table_pinned_host, table_device, n_tensors, n_chunks, stream, &t));
    return launch_tensors_copy(t.rows, t.map, t.n_chunks, scale, gather ? 1 : 0, stream);
}

int swf_tensors_gather(const void* table_pinned_host, void* table_device, size_t table_bytes, int32_t n_tensors, float* flat, int64_t flat_elems,
                       float scale, swf_stream_t stream) {
    return tensors_flat("tensors_gather", true, table_pinned_host, table_device, table_bytes, n_tensors, flat, flat_elems, scale, as_stream(stream));
}

int swf_tensors_scatter(const void* table_pinned_host, void* table_device, size_t table_bytes, int32_t n_tensors, const float* flat,
                        int64_t flat_elems, swf_stream_t stream) {
    return tensors_flat("tensors_scatter", false, table_pinned_host, table_device, table_bytes, n_tensors, const_cast<float*>(flat), flat_elems, 1.f,
                        as_stream(stream));
}

}  // extern "C"
