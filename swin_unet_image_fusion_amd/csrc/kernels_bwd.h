// Backward of one BasicBlock in exact fp32 (kernels_bwd.hip): SURVEY.md section 8(f) rank 4, first stage.
#pragma once
#include "swf_common.h"

namespace swf {

// The activation (swf_activation; the block entries read desc.act, the others take it as their last argument, zero = ELU(alpha = 1)): the
// default kind takes ELU' from the activation's OUTPUT as it always did; every other kind recomputes the PRE-activation u into the hidden
// buffer, multiplies the hidden gradient by act'(u), and then turns u into act(u) in place for the weight gradient that needs it, so no
// workspace depends on the activation.
// The kernel family of a backward call (swf_bwd_options) and where it reports what it launched (may be NULL).  Every entry below that
// runs gradient GEMMs takes one last; the default is the scalar-FMA family with no report.  `attn` is read by the entries that reach the
// attention core (basic_block_bwd*, window_attention_bwd*); the others ignore it.
struct BwdTier {
    int gemm = SWF_BWD_GEMM_FMA;
    swf_bwd_route* route = nullptr;
    int attn = SWF_BWD_ATTN_THREAD;
};

size_t attn_bwd_lds_bytes(int family, int wh, int ww, int d);
size_t basic_block_bwd_ws(const swf_block_desc& d, int nstream, int B, int H, int W);
int basic_block_bwd(const swf_block_desc& d, const swf_block_stream_params* px, const swf_block_stream_params* py, const float* x_in,
                    const float* y_in, const float* gx_out, const float* gy_out, float* gx_in, float* gy_in, const swf_block_stream_grads* gx,
                    const swf_block_stream_grads* gy, int B, int H, int W, void* workspace, size_t workspace_bytes, hipStream_t stream, const BwdTier& tier = {});

// the inner modules on their own: WindowAttention (a001), one MLP stream (a003), one LayerNorm (a004)
size_t window_attention_bwd_ws(const swf_attn_desc& d, int B, int H, int W);
int window_attention_bwd(const swf_attn_desc& d, const swf_attn_params& p, const float* q_in, const float* k_in, const float* v_in, const float* gout,
                         float* gq, float* gk, float* gv, const swf_attn_grads* gp, int B, int H, int W, void* workspace, size_t workspace_bytes,
                         hipStream_t stream, const BwdTier& tier = {});
size_t mlp_bwd_ws(int64_t N, int C, int hid);
int mlp_bwd(const swf_linear& fc1, const swf_linear& fc2, const float* x, const float* gout, float* gx, const swf_linear_grad* g1, const swf_linear_grad* g2,
            int64_t N, int C, int hid, void* workspace, size_t workspace_bytes, hipStream_t stream, const BwdTier& tier = {}, const swf_activation& act = {});
size_t layernorm_bwd_ws(int64_t N, int C);
int layernorm_bwd(const swf_norm& ln, const float* x, const float* gout, float* gx, const swf_norm_grad* gp, int64_t N, int C, void* workspace,
                  size_t workspace_bytes, hipStream_t stream);

// dropout in training mode (swf_dropout; masks: kernels_dropout.h), exact fp32.  The block entries share basic_block_drop_ws (both streams),
// the WindowAttention entries window_attention_drop_ws, the MLP entries mlp_drop_ws.
size_t basic_block_drop_ws(const swf_block_desc& d, int nstream, int B, int H, int W);
int basic_block_fwd_drop(const swf_block_desc& d, const swf_block_stream_params* px, const swf_block_stream_params* py, const float* x_in,
                         const float* y_in, float* x_out, float* y_out, int B, int H, int W, const swf_dropout& drop, void* workspace,
                         size_t workspace_bytes, hipStream_t stream);
int basic_block_bwd_drop(const swf_block_desc& d, const swf_block_stream_params* px, const swf_block_stream_params* py, const float* x_in,
                         const float* y_in, const float* gx_out, const float* gy_out, float* gx_in, float* gy_in, const swf_block_stream_grads* gx,
                         const swf_block_stream_grads* gy, int B, int H, int W, const swf_dropout& drop, void* workspace, size_t workspace_bytes,
                         hipStream_t stream, const BwdTier& tier = {});
size_t window_attention_drop_ws(const swf_attn_desc& d, int B, int H, int W);
int window_attention_fwd_drop(const swf_attn_desc& d, const swf_attn_params& p, const float* q_in, const float* k_in, const float* v_in,
                              const float* residual, float* out, int B, int H, int W, const swf_dropout& drop, int stream_id, void* workspace,
                              size_t workspace_bytes, hipStream_t stream);
int window_attention_bwd_drop(const swf_attn_desc& d, const swf_attn_params& p, const float* q_in, const float* k_in, const float* v_in,
                              const float* gout, float* gq, float* gk, float* gv, const swf_attn_grads* gp, int B, int H, int W,
                              const swf_dropout& drop, int stream_id, void* workspace, size_t workspace_bytes, hipStream_t stream, const BwdTier& tier = {});
size_t mlp_drop_ws(int64_t N, int C, int hid);
int mlp_fwd_drop(const swf_linear& fc1, const swf_linear& fc2, const float* x, float* out, int64_t N, int C, int hid, const swf_dropout& drop,
                 int stream_id, void* workspace, size_t workspace_bytes, hipStream_t stream, const swf_activation& act = {});
int mlp_bwd_drop(const swf_linear& fc1, const swf_linear& fc2, const float* x, const float* gout, float* gx, const swf_linear_grad* g1,
                 const swf_linear_grad* g2, int64_t N, int C, int hid, const swf_dropout& drop, int stream_id, void* workspace, size_t workspace_bytes,
                 hipStream_t stream, const BwdTier& tier = {}, const swf_activation& act = {});

// one linear layer y = x W^T + b, x [M][K], W [N][K], gout [M][N]: gx (+)= gout . W, gw = gout^T . x, gb = column sums of gout (any of
// the three may be NULL); the per-layer seam of the two gradient-GEMM families
size_t linear_bwd_ws(int64_t M, int N, int K);
int linear_bwd(const float* x, const float* w, const float* gout, float* gx, float* gw, float* gb, int64_t M, int N, int K, int accumulate,
               void* workspace, size_t workspace_bytes, hipStream_t stream, const BwdTier& tier = {});

// PatchMergingAndLinearLayer (one stream; H x W = the layer's input map), reflect pad, elementwise add
size_t patch_bwd_ws(int B, int H, int W, int Cin, int Cout, int mh, int mw, int encoder);
int patch_bwd(const swf_patch_params& p, const float* in, const float* gout, float* gin, const swf_patch_grads* gp, int B, int H, int W, int Cin,
              int Cout, int mh, int mw, int encoder, void* workspace, size_t workspace_bytes, hipStream_t stream, const BwdTier& tier = {}, const swf_activation& act = {});
int reflect_pad_bwd(const float* g, float* dx, int B, int H, int W, int C, int ph, int pw, hipStream_t stream);
int add_tensors(const float* a, const float* b, float* out, int64_t n, hipStream_t stream);

// final head (BatchNorm in eval mode)
size_t head_bwd_ws(int B, int H, int W, int ks);
int head_bwd(const swf_head_params& p, const float* x, const float* y, const float* gout, float* gx, float* gy, const swf_head_grads* gp, int B,
             int H, int W, int ks, int batch_stats, void* workspace, size_t workspace_bytes, hipStream_t stream, const swf_activation& act = {});
// batch mean / biased variance of conv1's two output channels (BatchNorm2d in training mode, a013:133) + the running-statistics update
int head_batch_stats(const swf_head_params& p, const float* x, const float* y, float* mean, float* var, float* running_mean, float* running_var,
                     float momentum, int B, int H, int W, int ks, void* workspace, size_t workspace_bytes, hipStream_t stream);
// The same over a batch that is spread over several calls (or ranks): one pass stopped at its two per-channel sums (device), and the
// finish over sums the caller has added up, with the element count of the whole batch.
int head_stats_pass(const swf_head_params& p, const float* x, const float* y, int pass, const float* mean, float* sums_out, int B, int H, int W,
                    int ks, void* workspace, size_t workspace_bytes, hipStream_t stream);
int head_stats_finish(const float* sums, int64_t count, int pass, float* mean, float* var, float* running_mean, float* running_var,
                      float momentum, hipStream_t stream);
// head_bwd with batch statistics in two phases: the four sums (dt2 xhat [2], dt2 [2]) of this call's batch -> sums_out (device); then the
// backward proper with k1, k2 from the sums of the whole batch (device) over n_global elements per channel.  No state is kept between them.
int head_bwd_sums(const swf_head_params& p, const float* x, const float* y, const float* gout, float* sums_out, int B, int H, int W, int ks,
                  void* workspace, size_t workspace_bytes, hipStream_t stream, const swf_activation& act = {});
int head_bwd_apply(const swf_head_params& p, const float* x, const float* y, const float* gout, const float* sums, int64_t n_global, float* gx,
                   float* gy, const swf_head_grads* gp, int B, int H, int W, int ks, void* workspace, size_t workspace_bytes, hipStream_t stream, const swf_activation& act = {});

}  // namespace swf
