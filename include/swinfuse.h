/*
 * swinfuse.h — C-ABI of the MI355X (gfx950) Swin-UNet image-fusion forward library.
 *
 * The reference (RainbowZL0/swin-unet-image-fusion) has no FFI layer: its boundary is the
 * Python nn.Module API.  This header is the boundary a maintainer binds underneath that API
 * (ctypes stub in INTEGRATION.md).  Each entry point names the reference interface it
 * replaces (file:line relative to the reference root).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.
 *  - All tensors are DEVICE pointers, fp32, **NHWC** ("token-major": [B][H][W][C]) unless a
 *    function says NCHW.  (B,1,H,W) NCHW and NHWC coincide, so the whole-model entry takes the
 *    reference's input/output tensors as they are.
 *  - The library never allocates, frees or retains device memory: weights and workspaces are
 *    borrowed for the duration of a call.  Workspace sizes come from the
 *    *_workspace_bytes queries.
 *  - Every function enqueues on the caller's stream (hipStream_t passed as void*), never
 *    synchronises, and is safe to capture into a hipGraph.
 *  - Return value: 0 = SWF_OK, negative = swf_status.  Nothing throws or aborts.
 *    swf_last_error_string() gives a thread-local description of the last failure.
 *  - The inference forward (eval(): dropout is the identity, BatchNorm uses its running statistics) is the hot path; the
 *    training side adds exact-fp32 backward entries (*_bwd), the head's batch statistics and dropout (*_drop, swf_dropout_mask).
 */
#ifndef SWINFUSE_H
#define SWINFUSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWF_VERSION_MAJOR 0
#define SWF_VERSION_MINOR 1

typedef void* swf_stream_t; /* hipStream_t */

typedef enum swf_status {
    SWF_OK = 0,
    SWF_ERR_NULL = -1,        /* required pointer is NULL */
    SWF_ERR_BAD_SHAPE = -2,   /* sizes inconsistent (e.g. map not a multiple of the window; einops error in the reference) */
    SWF_ERR_PAD = -3,         /* reflect pad >= dimension (torch RuntimeError at a006_PaddingOperation.py:128) */
    SWF_ERR_UNSUPPORTED = -4, /* configuration outside what the kernels cover */
    SWF_ERR_WORKSPACE = -5,   /* workspace too small */
    SWF_ERR_HIP = -6          /* a HIP launch failed */
} swf_status;

/* Arithmetic mode of the window-attention contractions and linear layers.
 *  FP32 : every contraction in exact fp32 (f32-input MFMA == fmaf chain; VALU attention).
 *  FAST : fused window kernels — linear layers as split-bf16 (bf16x3, fp32-grade) MFMA,
 *         QK^T in f16 MFMA, P.V in fp16 MFMA; LayerNorm statistics, softmax, residual
 *         stream and all accumulators stay fp32.  Shapes the fused kernels do not cover
 *         fall back to FP32 kernels (never to the host). */
typedef enum swf_precision { SWF_PREC_FP32 = 0, SWF_PREC_FAST = 1 } swf_precision;

/* The pointwise activation of the MLPs (a003), of the patch merge / un-merge layers (a011:230-237) and of the fusion head (a013:134):
 * the reference's MLP_ACTIVATION_FUNC, as torch.nn defines each.  A zero-initialised descriptor is ELU(alpha = 1), the reference's
 * configured default, with `param` ignored.  param: alpha of SWF_ACT_ELU, negative_slope of SWF_ACT_LEAKY_RELU (any finite value),
 * ignored by the other kinds.  An unknown kind or a non-finite parameter that is read: SWF_ERR_UNSUPPORTED before anything is launched
 * and before the workspace is looked at.
 * Only the default kind runs the fused fast-tier kernels (they keep ELU in exp2 units inside their packed weight images).  Under
 * SWF_PREC_FAST every other kind takes the generic family at that precision: split-bf16 GEMMs with the activation in their epilogue,
 * the f16 MFMA attention core, the unfused patch path; block routes report SWF_BLOCK_ROUTE_GENERIC, patch routes
 * SWF_PATCH_ROUTE_GENERIC.  The backward takes act' from the recomputed pre-activation; for the default kind it is unchanged. */
typedef enum swf_act_kind {
    SWF_ACT_ELU1 = 0,        /* nn.ELU(alpha = 1) */
    SWF_ACT_ELU = 1,         /* nn.ELU(alpha = param) */
    SWF_ACT_RELU = 2,        /* nn.ReLU */
    SWF_ACT_LEAKY_RELU = 3,  /* nn.LeakyReLU(negative_slope = param) */
    SWF_ACT_GELU = 4,        /* nn.GELU(approximate = "none"), erff */
    SWF_ACT_GELU_TANH = 5,   /* nn.GELU(approximate = "tanh"), tanhf */
    SWF_ACT_SILU = 6         /* nn.SiLU: v / (1 + expf(-v)) */
} swf_act_kind;
typedef struct swf_activation { int32_t kind; float param; } swf_activation;

typedef struct swf_linear { const float* weight; /* [out][in] row-major (nn.Linear / 1x1 Conv2d) */
                            const float* bias;   /* [out] or NULL */ } swf_linear;
typedef struct swf_norm   { const float* gamma; const float* beta; } swf_norm; /* LayerNorm over C, eps 1e-5 */

/* ---- WindowAttention (a001_WindowAttention.py:9-20 ctor, :448-474 forward) ---------------- */
typedef struct swf_attn_desc {
    int32_t channels;      /* in_out_dims */
    int32_t heads;         /* num_heads */
    int32_t head_dim;      /* dims_per_head (heads*head_dim need not equal channels) */
    int32_t win_h, win_w;  /* window_size */
    int32_t shift;         /* use_cyclic_shift: roll by (-win_h/2,-win_w/2), mask = -1e10 (a001:217-315) */
} swf_attn_desc;

typedef struct swf_attn_params {
    swf_linear q, k, v;        /* q_for_heads / k_for_heads / v_for_heads: [heads*head_dim][channels] */
    swf_linear proj;           /* linear_projection: [channels][heads*head_dim] */
    const float* bias_table;   /* relative_position_bias_table [(2*win_h-1)][(2*win_w-1)], shared by all heads (a001:72-82) */
} swf_attn_params;

/* out = WindowAttention(q, k, v) [+ residual if non-NULL].  q,k,v,out,residual: [B][H][W][C].
 * H,W must be multiples of the window (SWF_ERR_BAD_SHAPE otherwise). */
int swf_window_attention_fwd(const swf_attn_desc* desc, const swf_attn_params* p,
                             const float* q, const float* k, const float* v, const float* residual,
                             float* out, int32_t B, int32_t H, int32_t W,
                             void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* The same with the arithmetic mode as an argument (swf_precision): SWF_PREC_FAST runs the four projections as split-bf16 MFMA
 * GEMMs and QK^T / P.V on the f16 MFMA attention core (same workspace query); swf_window_attention_fwd == SWF_PREC_FP32. */
int swf_window_attention_fwd_prec(const swf_attn_desc* desc, int32_t precision, const swf_attn_params* p,
                                  const float* q, const float* k, const float* v, const float* residual,
                                  float* out, int32_t B, int32_t H, int32_t W,
                                  void* workspace, size_t workspace_bytes, swf_stream_t stream);
size_t swf_window_attention_workspace_bytes(const swf_attn_desc* desc, int32_t B, int32_t H, int32_t W);

/* ---- BasicBlock (a005_BasicBlock.py:127-145) and its two halves ---------------------------- */
/* Which kernel shapes the fast tier picks where it has a choice (same arithmetic, results differ in the last bits):
 * LATENCY (default): shortest single forward — eight waves per window at level 2, 32-token MLP tiles at level 3;
 * THROUGHPUT: least CU-time per forward, for callers that keep several forwards in flight on separate streams
 * (ShardedFusion lanes) — four waves per window at level 2, two windows per CU: two resident workgroups on maps of more windows
 * than CUs, one 512-thread workgroup of two windows (same bits) on maps of up to 2 x CUs windows; 64-token MLP tiles. */
typedef enum swf_schedule { SWF_SCHED_LATENCY = 0, SWF_SCHED_THROUGHPUT = 1 } swf_schedule;

typedef struct swf_block_desc {
    swf_attn_desc attn;
    int32_t hidden;        /* mlp_hidden_dims */
    int32_t cross;         /* use_cross_attr: x'=WA_x(q=x,k=y,v=y), y'=WA_y(q=y,k=x,v=x) (a002_AutoPathWinAtt.py:67-82) */
    int32_t precision;     /* swf_precision */
    int32_t schedule;      /* swf_schedule */
    swf_activation act;    /* mlp_activation_func between fc1 and fc2; zero = ELU(alpha = 1) */
} swf_block_desc;

typedef struct swf_block_stream_params {   /* one modality stream of one BasicBlock */
    swf_norm ln1;              /* stage_1.norm_layer_{1|2}  (a004_AddAndLayerNormWithOtherModule.py:16-18) */
    swf_attn_params attn;      /* auto_path_win_att.window_attention_{x|y} */
    swf_norm ln2;              /* stage_2.norm_layer_{1|2} */
    swf_linear fc1, fc2;       /* auto_path_mlp.mlp_{x|y}_1 [hidden][C], mlp_{x|y}_2 [C][hidden]; the activation between them (a003_AutoPathMLP.py:21-44) is the descriptor's or the entry's swf_activation */
} swf_block_stream_params;

/* stage_1 of a BasicBlock for both streams: out = in + Attention(LN(in), ...) (a004:29-38 with
 * other_module = AutoPathWinAtt a002:58-82).  py / y_* may be NULL for a single-path block. */
int swf_attn_halfblock_fwd(const swf_block_desc* desc, const swf_block_stream_params* px,
                           const swf_block_stream_params* py,
                           const float* x_in, const float* y_in, float* x_out, float* y_out,
                           int32_t B, int32_t H, int32_t W,
                           void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* stage_2: out = in + MLP(LN(in)) per stream (a004:29-38 with other_module = AutoPathMLP a003:46-50). */
int swf_mlp_halfblock_fwd(const swf_block_desc* desc, const swf_block_stream_params* px,
                          const swf_block_stream_params* py,
                          const float* x_in, const float* y_in, float* x_out, float* y_out,
                          int32_t B, int32_t H, int32_t W,
                          void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* whole BasicBlock.forward(x, y) (a005:127-145); x_out/y_out may alias x_in/y_in. */
int swf_basic_block_fwd(const swf_block_desc* desc, const swf_block_stream_params* px,
                        const swf_block_stream_params* py,
                        const float* x_in, const float* y_in, float* x_out, float* y_out,
                        int32_t B, int32_t H, int32_t W,
                        void* workspace, size_t workspace_bytes, swf_stream_t stream);
size_t swf_basic_block_workspace_bytes(const swf_block_desc* desc, int32_t B, int32_t H, int32_t W);

/* Which kernels a block ran: a family in the low byte, OR-ed with the flags of every choice the dispatch made inside that family.  The
 * code is put together by the branches that launch (never recomputed beside them), so that a caller can tell the kernel it means to run
 * from a fallback: every fallback of the fast tier is more accurate than the kernel it replaces, and no number would show it. */
typedef enum swf_block_route {
    SWF_BLOCK_ROUTE_GENERIC = 0,           /* family: attention half and MLP half composed from separate launches (exact tier; fast tier where no fused kernel covers the block) */
    SWF_BLOCK_ROUTE_WINDOW = 1,            /* family: one launch of a register-resident window kernel (C = 24 / 48 / 96, two streams) */
    SWF_BLOCK_ROUTE_DEEP = 2,              /* family: deep-level composition over split-bf16 planes (C >= 128) */
    SWF_BLOCK_ROUTE_FAMILY_MASK = 0xff,
    /* window family */
    SWF_BLOCK_WIN_X8 = 0x100,              /* C = 96, 8x8 / 7x7 windows: the eight-waves-per-window kernel (absent: four waves per window) */
    SWF_BLOCK_WIN_W16 = 0x200,             /* the level's 16x16-window kernel */
    SWF_BLOCK_VIA_TMP = 0x400,             /* the outputs went through temporary maps: copied back (an in-place cross block of a kernel that cannot run
                                              in place), or the ping-pong of a stage's two cross blocks */
    SWF_BLOCK_PREPACKED = 0x800,           /* window and deep family: the weight images came from the caller, nothing was packed in the call */
    /* deep family, attention and projection (none of the first four: Q/K/V as plane GEMMs, the 8x8 / 7x7 attention core, the projection as a plane GEMM) */
    SWF_BLOCK_DEEP_QKVATTN = 0x1000,       /* Q/K/V projections + window attention in one launch (C = 192) */
    SWF_BLOCK_DEEP_FOLD_PROJ = 0x2000,     /* ... which also left the projection's partial sums: the fused MLP's prologue finishes the attention half */
    SWF_BLOCK_DEEP_QKV = 0x4000,           /* the three projections of every stream in one launch over fragment-major weights */
    SWF_BLOCK_DEEP_ATTNPROJ = 0x8000,      /* attention core + output projection + residual in one launch (C = 384) */
    SWF_BLOCK_DEEP_PROJ = 0x10000,         /* output projection over fragment-major weights (+ bias + residual) */
    SWF_BLOCK_DEEP_CORE16 = 0x20000,       /* the 16x16-window attention core */
    /* deep family, MLP (no SWF_BLOCK_MLP_FUSED: LayerNorm, fc1 and fc2 as separate launches) */
    SWF_BLOCK_MLP_FUSED = 0x40000,         /* LN2 + fc1 + ELU + fc2 + residual in one launch, with exactly one of the three tile variants: */
    SWF_BLOCK_MLP_TOK32 = 0x80000,         /*   32-token tiles, six waves (C = 192, latency schedule) */
    SWF_BLOCK_MLP_TOK64 = 0x100000,        /*   64-token tiles, four waves */
    SWF_BLOCK_MLP_WIDE8 = 0x200000,        /*   64-token tiles, eight waves on one 256-wide hidden chunk (C = 384) */
    SWF_BLOCK_MLP_SPLIT = 0x400000,        /* the hidden width was split over workgroups and a reduce launch summed the parts */
    /* deep family, LN1 hand-off between blocks that share a workspace */
    SWF_BLOCK_LN1_GIVEN = 0x800000,        /* the block found its LN1 planes in place: no LayerNorm launch */
    SWF_BLOCK_LN1_WRITTEN = 0x1000000      /* the block's MLP also wrote the LN1 planes of the block that runs next */
} swf_block_route;
/* swf_basic_block_fwd that also reports the route: *route (host int32, may be NULL) is written when the call succeeds.  Same workspace
 * query; desc->schedule is honoured as everywhere. */
int swf_basic_block_fwd_route(const swf_block_desc* desc, const swf_block_stream_params* px,
                              const swf_block_stream_params* py,
                              const float* x_in, const float* y_in, float* x_out, float* y_out,
                              int32_t B, int32_t H, int32_t W, int32_t* route,
                              void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* Block-level pre-pack for callers that run the same block many times (fast tier): derive the fused kernel's
 * weight images once into a caller-owned buffer of swf_basic_block_packed_bytes(desc) bytes (0 = this shape has no
 * fused kernel; use swf_basic_block_fwd), then launch with swf_basic_block_fwd_packed — exactly one kernel. */
size_t swf_basic_block_packed_bytes(const swf_block_desc* desc);
int swf_basic_block_pack(const swf_block_desc* desc, const swf_block_stream_params* px,
                         const swf_block_stream_params* py, void* packed, size_t packed_bytes, swf_stream_t stream);
int swf_basic_block_fwd_packed(const swf_block_desc* desc, const void* packed,
                               const float* x_in, const float* y_in, float* x_out, float* y_out,
                               int32_t B, int32_t H, int32_t W, swf_stream_t stream);

/* ---- training side, first stage: backward of one BasicBlock ------------------------------------------------
 * What torch.autograd computes for a005_BasicBlock.py:127-145 inside the reference's training step (a016_train.py:150-196), in
 * exact fp32.  The forward intermediates are recomputed from the block's inputs, so nothing has to be saved by the forward call.
 * gx_out / gy_out: dL/d(block outputs); gx_in / gy_in: dL/d(block inputs) (written); gpx / gpy: where the parameter gradients go —
 * the same fields as swf_block_stream_params, every non-NULL pointer is OVERWRITTEN with the gradient of that tensor (NULL = not
 * wanted).  py / y_* / gpy NULL for a single-path block.  Sums over tokens run in a fixed order (no atomics): bit-reproducible. */
typedef struct swf_linear_grad { float* weight; float* bias; } swf_linear_grad;
typedef struct swf_norm_grad { float* gamma; float* beta; } swf_norm_grad;
typedef struct swf_attn_grads { swf_linear_grad q, k, v, proj; float* bias_table; } swf_attn_grads;
typedef struct swf_block_stream_grads {
    swf_norm_grad ln1; swf_attn_grads attn; swf_norm_grad ln2; swf_linear_grad fc1, fc2;
} swf_block_stream_grads;
typedef struct swf_patch_grads { swf_linear_grad conv; swf_norm_grad ln; } swf_patch_grads;
size_t swf_basic_block_bwd_workspace_bytes(const swf_block_desc* desc, int32_t B, int32_t H, int32_t W);
int swf_basic_block_bwd(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                        const float* x_in, const float* y_in, const float* gx_out, const float* gy_out,
                        float* gx_in, float* gy_in, const swf_block_stream_grads* gpx, const swf_block_stream_grads* gpy,
                        int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* The inner modules on their own under autograd (a caller that keeps the reference's BasicBlock and swaps only a001 / a003 / a004):
 * exact fp32, forward intermediates recomputed, fixed-order sums.  Gradient pointers as above (NULL = not wanted).
 * WindowAttention.forward (a001:448-474): q / k / v [B][H][W][C]; gq / gk / gv are three separate buffers — where one tensor was passed
 * as more than one of q, k, v the caller adds them (torch.autograd does).
 * A (window, head_dim) whose attention backward tile fits neither kernel's LDS (16 x 16 windows at head_dim > 32: 262.8 KB against
 * 160 KB) is refused by the block and the attention entries with SWF_ERR_UNSUPPORTED before anything is launched, like a short
 * workspace: no gradient buffer and no byte of the workspace is written.  The exact-tier forward accepts that shape. */
size_t swf_window_attention_bwd_workspace_bytes(const swf_attn_desc* desc, int32_t B, int32_t H, int32_t W);
int swf_window_attention_bwd(const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k, const float* v,
                             const float* gout, float* gq, float* gk, float* gv, const swf_attn_grads* gp,
                             int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* one stream of AutoPathMLP.forward (a003:46-50): out = fc2(ELU(fc1(x))), x [tokens][channels] */
size_t swf_mlp_bwd_workspace_bytes(int64_t tokens, int32_t channels, int32_t hidden);
int swf_mlp_bwd(const swf_linear* fc1, const swf_linear* fc2, const float* x, const float* gout, float* gx,
                const swf_linear_grad* gfc1, const swf_linear_grad* gfc2, int64_t tokens, int32_t channels, int32_t hidden,
                void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* my_layer_norm (a004:54-72) */
size_t swf_layernorm_bwd_workspace_bytes(int64_t tokens, int32_t C);
int swf_layernorm_bwd(const swf_norm* ln, const float* x, const float* gout, float* gx, const swf_norm_grad* gp,
                      int64_t tokens, int32_t C, void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- training side: dropout (attention_drop_ratio, linear_after_att_drop_ratio, mlp_drop_ratio; a005:22-27, a013:29-33) ------------
 * Inverted dropout, x * mask / (1 - p), at the reference's four points of one stream of a block:
 *   site 0  the attention output values P.V before the projection (a001:351-354)       [tokens][heads*head_dim]
 *   site 1  the projection output before the residual add (a001:412-414)              [tokens][channels]
 *   site 2  the MLP hidden activation after ELU, before fc2 (a003:25-31, dropout_*_1)  [tokens][hidden]
 *   site 3  the fc2 output before the residual add (a003:25-31, dropout_*_2)           [tokens][channels]
 * The mask is a function of (seed, stream, site, element index) only: element i = token * width + channel, token = the row in the
 * image-order NHWC layout ((b * H + h) * W + w of the unshifted map), so it does not depend on tiling, window partition or cyclic
 * shift.  r = word (i % 4) of Philox4x32-10 with key {seed & 0xffffffff, seed >> 32} and counter {(i / 4) & 0xffffffff, (i / 4) >> 32,
 * site, stream}; the element is kept iff (r >> 8) * 2^-24 >= p and then multiplied by 1 / (1 - p) computed in fp32, else it becomes 0
 * (p = 1 drops everything).  stream: 0 = the x stream, 1 = the y stream of a dual-path block.
 * The *_drop entries run the exact fp32 tier whatever desc->precision says (the fused fast kernels have no masks), and their backward
 * recomputes the forward with the same seed, so nothing is kept between the two calls.  A site with p = 0 applies no mask. */
typedef struct swf_dropout {
    uint64_t seed;
    float attn_p;   /* site 0: attention_drop_ratio */
    float proj_p;   /* site 1: linear_after_att_drop_ratio */
    float mlp_p;    /* sites 2 and 3: mlp_drop_ratio */
} swf_dropout;
/* out[i] = the factor the kernels apply to element i (0 or 1 / (1 - p)), i < count: the documented way to reproduce a mask. */
int swf_dropout_mask(uint64_t seed, int32_t stream_id, int32_t site, int64_t count, float p, float* out, swf_stream_t stream);
/* BasicBlock.forward / its backward with dropout; arguments as swf_basic_block_fwd / swf_basic_block_bwd, both with the workspace of
 * swf_basic_block_drop_workspace_bytes.  x_out / y_out may alias x_in / y_in. */
size_t swf_basic_block_drop_workspace_bytes(const swf_block_desc* desc, int32_t B, int32_t H, int32_t W);
int swf_basic_block_fwd_drop(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                             const float* x_in, const float* y_in, float* x_out, float* y_out, int32_t B, int32_t H, int32_t W,
                             const swf_dropout* drop, void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_basic_block_bwd_drop(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                             const float* x_in, const float* y_in, const float* gx_out, const float* gy_out, float* gx_in, float* gy_in,
                             const swf_block_stream_grads* gpx, const swf_block_stream_grads* gpy, int32_t B, int32_t H, int32_t W,
                             const swf_dropout* drop, void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* WindowAttention on its own (sites 0 and 1 of mask stream stream_id; drop->mlp_p is ignored): forward as swf_window_attention_fwd
 * (residual may be NULL), backward as swf_window_attention_bwd; workspace of swf_window_attention_drop_workspace_bytes. */
size_t swf_window_attention_drop_workspace_bytes(const swf_attn_desc* desc, int32_t B, int32_t H, int32_t W);
int swf_window_attention_fwd_drop(const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k, const float* v,
                                  const float* residual, float* out, int32_t B, int32_t H, int32_t W, const swf_dropout* drop,
                                  int32_t stream_id, void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_window_attention_bwd_drop(const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k, const float* v,
                                  const float* gout, float* gq, float* gk, float* gv, const swf_attn_grads* gp, int32_t B, int32_t H,
                                  int32_t W, const swf_dropout* drop, int32_t stream_id, void* workspace, size_t workspace_bytes,
                                  swf_stream_t stream);
/* One stream of AutoPathMLP (sites 2 and 3 of mask stream stream_id): out = d3(fc2(d2(ELU(fc1(x))))), x / out [tokens][channels];
 * backward as swf_mlp_bwd; workspace of swf_mlp_drop_workspace_bytes. */
size_t swf_mlp_drop_workspace_bytes(int64_t tokens, int32_t channels, int32_t hidden);
int swf_mlp_fwd_drop(const swf_linear* fc1, const swf_linear* fc2, const float* x, float* out, int64_t tokens, int32_t channels,
                     int32_t hidden, const swf_dropout* drop, int32_t stream_id, void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_mlp_bwd_drop(const swf_linear* fc1, const swf_linear* fc2, const float* x, const float* gout, float* gx,
                     const swf_linear_grad* gfc1, const swf_linear_grad* gfc2, int64_t tokens, int32_t channels, int32_t hidden,
                     const swf_dropout* drop, int32_t stream_id, void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- training side: kernel families of the exact-fp32 backward ---------------------------------------------------------------------
 * The gradient GEMMs of every backward entry (dX = dY . W and dW = dY^T . X, the latter per 256-token chunk + a fixed reduction tree)
 * exist in two families that return THE SAME BITS: both keep one accumulator per output element, start it at zero and take the
 * reduction index in ascending order with one rounding per product.  SWF_BWD_GEMM_FMA: LDS-tiled scalar fmaf, 4 x 4 outputs per
 * thread (what the entries above run).  SWF_BWD_GEMM_MFMA: the same chains on the matrix cores (v_mfma_f32_16x16x4_f32, an fmaf
 * chain in hardware), 16-byte loads where the pointers and row lengths allow.
 * The attention core has two families, both exact fp32 with one thread per query / key, no atomics and fixed summation orders.
 * SWF_BWD_ATTN_THREAD (the default): Q, K, V and dO of a (window, head) in LDS at once, the probability tile beside them where it
 * fits (RAN_RESIDENT) or rebuilt by every pass (RAN_RECOMPUTE); it refuses a tile whose four operand tiles pass 160 KB — 256 tokens at
 * head_dim 33 .. 64, level 4 of 16 x 16 windows.  SWF_BWD_ATTN_PHASED (opt-in): two operand tiles at a time — K and V while every query
 * takes its softmax statistics and dQ, then Q and dO while every key takes dK and dV — and the table gradient through one private
 * partial per wave; it runs at EVERY shape it can hold (RAN_PHASED) and refuses only head_dim > 64, more than 1024 tokens or an LDS
 * need of its own past 160 KB (swf_attention_bwd_lds_bytes).  Its results agree with the thread family's to rounding, not bit for bit.
 * Codes 1 and 2 are refused: 1 is kept for a matrix-core kernel, 2 so that the codes of swf_bwd_attn and swf_bwd_attn_ran that name
 * the phased kernel are the same.  Any other code: SWF_ERR_UNSUPPORTED.  All-zero options are the entries above.
 * swf_mlp_bwd_opt, swf_patch_layer_bwd_opt and swf_linear_bwd have no attention core: they validate `attention` like the others
 * (0 or 3, anything else is refused), then ignore it and report SWF_BWD_ATTN_RAN_NONE, so one options struct serves a whole model. */
typedef enum swf_bwd_gemm { SWF_BWD_GEMM_FMA = 0, SWF_BWD_GEMM_MFMA = 1 } swf_bwd_gemm;
typedef enum swf_bwd_attn { SWF_BWD_ATTN_THREAD = 0, SWF_BWD_ATTN_PHASED = 3 } swf_bwd_attn;
typedef struct swf_bwd_options { int32_t gemm; int32_t attention; } swf_bwd_options;
/* What a backward call launched, written by the branches that launch (host memory, zeroed by the call first; may be NULL): the number
 * of dX and dW launches per family — a call never mixes them, so a caller can tell the family it asked for from a fallback — and the
 * attention-core kernel. */
typedef enum swf_bwd_attn_ran {
    SWF_BWD_ATTN_RAN_NONE = 0,        /* the entry has no attention core */
    SWF_BWD_ATTN_RAN_RESIDENT = 1,    /* thread family, probability tile of the (window, head) resident in LDS */
    SWF_BWD_ATTN_RAN_RECOMPUTE = 2,   /* thread family, every pass rebuilds its scores (windows whose tile does not fit: 16 x 16) */
    SWF_BWD_ATTN_RAN_PHASED = 3       /* phased family: K and V in LDS for dQ, then Q and dO for dK and dV */
} swf_bwd_attn_ran;
typedef struct swf_bwd_route { int32_t dx_fma, dx_mfma, dw_fma, dw_mfma; int32_t attention; } swf_bwd_route;
/* Dynamic LDS in bytes of the attention-backward kernel that `family` (swf_bwd_attn) launches for one (window, head) of
 * win_h x win_w tokens at head_dim channels; 0 where the family refuses the tile or the code is unknown.  Host only, no GPU needed. */
size_t swf_attention_bwd_lds_bytes(int32_t family, int32_t win_h, int32_t win_w, int32_t head_dim);
/* The backward entries with the family as an argument: arguments, results and workspace as swf_basic_block_bwd /
 * swf_window_attention_bwd / swf_mlp_bwd / swf_patch_layer_bwd, plus drop (NULL: no dropout, the workspace query of the plain entry;
 * non-NULL: as the *_bwd_drop entry with its workspace query and, for the inner modules, its mask stream stream_id), the options
 * (NULL = all zero) and the route (NULL = not wanted). */
int swf_basic_block_bwd_opt(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                            const float* x_in, const float* y_in, const float* gx_out, const float* gy_out, float* gx_in, float* gy_in,
                            const swf_block_stream_grads* gpx, const swf_block_stream_grads* gpy, int32_t B, int32_t H, int32_t W,
                            const swf_dropout* drop, const swf_bwd_options* opt, swf_bwd_route* route,
                            void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_window_attention_bwd_opt(const swf_attn_desc* desc, const swf_attn_params* p, const float* q, const float* k, const float* v,
                                 const float* gout, float* gq, float* gk, float* gv, const swf_attn_grads* gp, int32_t B, int32_t H,
                                 int32_t W, const swf_dropout* drop, int32_t stream_id, const swf_bwd_options* opt, swf_bwd_route* route,
                                 void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_mlp_bwd_opt(const swf_linear* fc1, const swf_linear* fc2, const float* x, const float* gout, float* gx,
                    const swf_linear_grad* gfc1, const swf_linear_grad* gfc2, int64_t tokens, int32_t channels, int32_t hidden,
                    const swf_dropout* drop, int32_t stream_id, const swf_bwd_options* opt, swf_bwd_route* route,
                    void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* The per-layer seam of the two families: one linear layer y = x W^T + b on its own, x [M][K], W [N][K], gout = dL/dy [M][N], any
 * M, N, K >= 1 and any 4-byte-aligned pointers.  gx [M][K] = gout . W (accumulate != 0: added to gx), gw [N][K] = gout^T . x,
 * gb [N] = column sums of gout; each of the three may be NULL.  The workspace is the weight-gradient scratch, sized as the block
 * entries size it for the same layer (not read when gw and gb are NULL). */
size_t swf_linear_bwd_workspace_bytes(int64_t M, int32_t N, int32_t K);
int swf_linear_bwd(const float* x, const float* weight, const float* gout, float* gx, float* gw, float* gb,
                   int64_t M, int32_t N, int32_t K, int32_t accumulate, const swf_bwd_options* opt, swf_bwd_route* route,
                   void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* SelfAndCrossBlockPair.forward (a012_SelfAndCrossBlockPair.py:70-78): four BasicBlocks in the
 * order self/normal, self/shifted, cross/normal, cross/shifted (a009:90-109).  `desc` gives the
 * shared dims; shift/cross flags inside it are ignored.  px[4], py[4]. */
int swf_block_pair4_fwd(const swf_block_desc* desc, const swf_block_stream_params* px,
                        const swf_block_stream_params* py,
                        const float* x_in, const float* y_in, float* x_out, float* y_out,
                        int32_t B, int32_t H, int32_t W,
                        void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- PatchMergingAndLinearLayer (a011_PatchOperation.py:244-264) + MyPadding (a006:167-187) -- */
typedef struct swf_patch_params { swf_linear conv; /* mlp_layer_{x|y}: 1x1 conv */ swf_norm ln; /* layer_norm_{x|y} */ } swf_patch_params;

/* Encoder stage front: reflect-pad in (H,W) bottom/right to a multiple of (merge_h,merge_w)
 * (a006:122-131), space-to-depth with channel order (ph*merge_w+pw)*Cin+c (a011:87-93), 1x1 conv
 * 4Cin->Cout, LayerNorm(Cout), ELU (a011:236-239), then reflect-pad the merged map to a multiple
 * of (win_h,win_w).  in: [B][H][W][Cin]; out: [B][Ho][Wo][Cout] with Ho,Wo from swf_merge_out_shape.
 * SWF_ERR_PAD when a reflect pad is >= the dimension it pads (the reference raises RuntimeError). */
int swf_patch_merge_fwd(const swf_patch_params* p, const float* in, float* out,
                        int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                        int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w,
                        void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_merge_out_shape(int32_t H, int32_t W, int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w,
                        int32_t* Hm, int32_t* Wm, int32_t* Ho, int32_t* Wo);

/* Decoder stage back: crop the window padding (in is [B][Hp][Wp][Cin], valid part Hm x Wm,
 * a006:143-146), 1x1 conv Cin->mh*mw*Cout, LayerNorm over mh*mw*Cout, depth-to-space (a011:111-117),
 * ELU (order a011:241), crop to (Hout,Wout) (undo of the merge padding), then optionally add
 * `skip` [B][Hout][Wout][Cout] (the U-Net skip add that precedes the next decoder stage,
 * a013_ModelDefinition.py:222-225). */
int swf_patch_unmerge_fwd(const swf_patch_params* p, const float* in, const float* skip, float* out,
                          int32_t B, int32_t Hp, int32_t Wp, int32_t Hm, int32_t Wm, int32_t Cin, int32_t Cout,
                          int32_t merge_h, int32_t merge_w, int32_t Hout, int32_t Wout,
                          void* workspace, size_t workspace_bytes, swf_stream_t stream);
size_t swf_patch_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                 int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w, int32_t encoder);

/* The pair of patch layers of one stage (both modality streams) with the arithmetic mode as an argument.  SWF_PREC_FP32 is
 * swf_patch_merge_fwd / swf_patch_unmerge_fwd per stream.  SWF_PREC_FAST packs the weight images this shape admits into the workspace
 * (per call: these entries are for tests and tools, not the hot path) and then takes the route the whole-model forward takes for the
 * layer, through the same dispatch; *route (host int32, may be NULL) says which kernel that was, so that a caller can tell the kernel it
 * means to run from a fallback.  py / y_* NULL = one stream (size queries: dual = 0).  Geometry arguments as the single-stream entries above. */
typedef enum swf_patch_route {
    SWF_PATCH_ROUTE_GENERIC = 0,      /* gather / crop, GEMM (fast tier: split-bf16, split-K for deep K), LayerNorm, scatter as separate launches */
    SWF_PATCH_ROUTE_FUSED = 1,        /* one launch, conv operands staged through LDS */
    SWF_PATCH_ROUTE_RR = 2,           /* one launch, register-resident (two streams, levels 0-2) */
    SWF_PATCH_ROUTE_DEEP_ROW = 3,     /* deep level, whole rows: one launch */
    SWF_PATCH_ROUTE_DEEP_SLICED = 4,  /* deep level, conv over column slices, then the finishing launch */
    SWF_PATCH_ROUTE_LN1 = 0x100       /* flag, OR-ed in: the LN1 planes asked for were written (absent: the route has none, buffers untouched) */
} swf_patch_route;
/* Optional: the LN1 of the block that runs behind the layer, as the deep-level kernels leave it for that block: LayerNorm(out) with
 * `ln` as split-bf16 planes hi / lo, caller-owned uint16 [rows][Cout], rows = the pixels of `out`; value = float(hi) + float(lo).
 * Written by the encoder whole-row route and by both column-sliced routes (SWF_PATCH_ROUTE_LN1 in *route).  For every stream or none. */
typedef struct swf_patch_ln1 { swf_norm ln; uint16_t* hi; uint16_t* lo; } swf_patch_ln1;
size_t swf_patch_merge_prec_workspace_bytes(int32_t precision, int32_t dual, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                            int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w);
int swf_patch_merge_fwd_prec(int32_t precision, const swf_patch_params* px, const swf_patch_params* py,
                             const float* x_in, const float* y_in, float* x_out, float* y_out,
                             int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                             int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w,
                             const swf_patch_ln1* ln1_x, const swf_patch_ln1* ln1_y, int32_t* route,
                             void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* Unlike swf_patch_workspace_bytes this query knows the crop and the output size. */
size_t swf_patch_unmerge_prec_workspace_bytes(int32_t precision, int32_t dual, int32_t B, int32_t Hp, int32_t Wp, int32_t Hm, int32_t Wm,
                                              int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t Hout, int32_t Wout);
int swf_patch_unmerge_fwd_prec(int32_t precision, const swf_patch_params* px, const swf_patch_params* py,
                               const float* x_in, const float* y_in, const float* x_skip, const float* y_skip,
                               float* x_out, float* y_out,
                               int32_t B, int32_t Hp, int32_t Wp, int32_t Hm, int32_t Wm, int32_t Cin, int32_t Cout,
                               int32_t merge_h, int32_t merge_w, int32_t Hout, int32_t Wout,
                               const swf_patch_ln1* ln1_x, const swf_patch_ln1* ln1_y, int32_t* route,
                               void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* One SelfAndCrossBlockPair stage as the whole-model forward runs it (arguments as swf_block_pair4_fwd; desc carries precision and
 * schedule).  Under SWF_PREC_FAST the images this shape admits (eight, [block][stream]) are packed at the front of the workspace, per call
 * (this entry is for tests and tools, not the hot path), and the stage then runs from them through the same code as the model's: each
 * block warms the next block's images, at the deep levels each block's MLP leaves the next block's LN1 planes, and the two cross blocks
 * of a 16x16-window kernel ping-pong through temporary maps.  route: host int32[4], one swf_block_route per block, or NULL.
 * ln1_x / ln1_y (for every stream or none; reuse of swf_patch_ln1): the LN1 of the first block of a stage that would run next on the
 * same map.  Where the last block's route carries SWF_BLOCK_LN1_WRITTEN its MLP wrote LayerNorm(out) with `ln` as split-bf16 planes
 * and they were copied to hi / lo (uint16 [B*H*W][C]); without the flag the buffers are untouched.  x_out / y_out may alias the
 * inputs.  The query takes dual = 0 for py == NULL. */
size_t swf_block_stage_prec_workspace_bytes(const swf_block_desc* desc, int32_t dual, int32_t B, int32_t H, int32_t W);
int swf_block_stage_fwd_prec(const swf_block_desc* desc, const swf_block_stream_params* px, const swf_block_stream_params* py,
                             const float* x_in, const float* y_in, float* x_out, float* y_out,
                             int32_t B, int32_t H, int32_t W,
                             const swf_patch_ln1* ln1_x, const swf_patch_ln1* ln1_y, int32_t* route,
                             void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- final fusion head (a013:126-152): cat -> conv kxk reflect -> BatchNorm2d(eval) -> ELU -> conv kxk reflect */
typedef struct swf_head_params {
    const float* conv1_w; const float* conv1_b;   /* final_layer.0: [2][2][k][k], [2] */
    const float* bn_gamma; const float* bn_beta; const float* bn_mean; const float* bn_var; /* final_layer.1, eps 1e-5 */
    const float* conv2_w; const float* conv2_b;   /* final_layer.3: [1][2][k][k], [1] */
} swf_head_params;
/* x,y,out: [B][H][W] (single channel).  tmp workspace: 2*B*H*W floats. */
int swf_final_head_fwd(const swf_head_params* p, const float* x, const float* y, float* out,
                       int32_t B, int32_t H, int32_t W, int32_t ksize,
                       void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* Backward of the final head with BatchNorm in eval mode (running statistics: a per-channel affine map).  gout: dL/d(out) [B][H][W];
 * gx / gy: dL/d(x), dL/d(y); gp: parameter gradients (overwritten; NULL pointers skipped; the running statistics have none).  Reads
 * the eight BatchNorm scalars back to the host: synchronises the stream once. */
typedef struct swf_head_grads {
    float* conv1_w; float* conv1_b; float* bn_gamma; float* bn_beta; float* conv2_w; float* conv2_b;
} swf_head_grads;
size_t swf_final_head_bwd_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t ksize);
/* batch_stats != 0: p->bn_mean / bn_var hold the BATCH statistics of this forward (training-mode BatchNorm, as the reference trains:
 * a016:137 model.train()), and the normalisation's own gradient is included. */
int swf_final_head_bwd(const swf_head_params* p, const float* x, const float* y, const float* gout, float* gx, float* gy,
                       const swf_head_grads* gp, int32_t B, int32_t H, int32_t W, int32_t ksize, int32_t batch_stats,
                       void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* Training-mode BatchNorm2d of the head (a013:133 under model.train()): the batch mean and biased variance of conv1(cat(x, y)) per
 * channel -> mean[2], var[2] (device; pass them as bn_mean / bn_var of swf_final_head_fwd / _bwd), and, when non-NULL,
 * running = (1 - momentum) running + momentum (mean, unbiased variance) as nn.BatchNorm2d does.  Workspace: swf_final_head_bwd's. */
int swf_final_head_batch_stats(const swf_head_params* p, const float* x, const float* y, float* mean, float* var,
                               float* running_mean, float* running_var, float momentum,
                               int32_t B, int32_t H, int32_t W, int32_t ksize,
                               void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* The same BatchNorm over a batch that is SPREAD over several calls or ranks (data-parallel training): the two entries above split at
 * the per-channel sums, which the caller adds up (an all-reduce SUM) between the calls.  All sums live in device memory; nothing is
 * kept in the workspace from one call to the next.  Workspace of the three entries that take one: swf_final_head_bwd's.
 *   forward:   stats_pass(0) -> add -> stats_finish(0) writes mean;  stats_pass(1, mean) -> add -> stats_finish(1) writes var and running
 *   backward:  bwd_sums -> add -> bwd_synced
 * swf_final_head_stats_pass: ONE pass over this call's batch; sums_out[2] <- sum of t (pass 0) or of (t - mean)^2 (pass 1, mean[2] from
 * the caller), t = conv1(cat(x, y)). */
int swf_final_head_stats_pass(const swf_head_params* p, const float* x, const float* y, int32_t pass, const float* mean, float* sums_out,
                              int32_t B, int32_t H, int32_t W, int32_t ksize,
                              void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* sums[2] over a batch of `count` elements per channel in all (sums_bytes: the size of that buffer, at least 8; SWF_ERR_WORKSPACE
 * otherwise): pass 0 writes mean = sums / count; pass 1 writes the biased var = sums / count and, where non-NULL, moves the running
 * statistics by `momentum` towards mean[2] and the unbiased variance sums / (count - 1), as swf_final_head_batch_stats does. */
int swf_final_head_stats_finish(const float* sums, size_t sums_bytes, int64_t count, int32_t pass, float* mean, float* var,
                                float* running_mean, float* running_var, float momentum, swf_stream_t stream);
/* The two halves of swf_final_head_bwd with batch_stats != 0.  bwd_sums: sums_out[4] <- sum of dt2 xhat [2], sum of dt2 [2] over this
 * call's batch (p->bn_mean / bn_var: the statistics of the WHOLE batch).  bwd_synced: the backward with the normalisation's gradient
 * formed from sums[4] (device) of the whole batch and its `count` elements per channel; gx, gy and the parameter gradients are this
 * call's batch's. */
int swf_final_head_bwd_sums(const swf_head_params* p, const float* x, const float* y, const float* gout, float* sums_out,
                            int32_t B, int32_t H, int32_t W, int32_t ksize,
                            void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_final_head_bwd_synced(const swf_head_params* p, const float* x, const float* y, const float* gout, const float* sums, int64_t count,
                              float* gx, float* gy, const swf_head_grads* gp, int32_t B, int32_t H, int32_t W, int32_t ksize,
                              void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- training side, second stage: patch layers, padding, skip add ------------------------------------------------------------ */
/* Backward of one stream of PatchMergingAndLinearLayer (a011:244-264) as the module runs it (no padding inside: MyPadding is its own
 * module).  H x W = the layer's INPUT map: encoder the full map (divisible by the merging size), decoder the merged map.  in: the
 * forward input [B][H][W][Cin]; gout: dL/d(output) (encoder [B][H/mh][W/mw][Cout], decoder [B][H*mh][W*mw][Cout]); gin: dL/d(input);
 * gp: parameter gradients (overwritten; NULL pointers skipped). */
size_t swf_patch_layer_bwd_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w,
                                           int32_t encoder);
int swf_patch_layer_bwd(const swf_patch_params* p, const float* in, const float* gout, float* gin, const swf_patch_grads* gp,
                        int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t encoder,
                        void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* ... with the family of its gradient GEMMs as an argument (swf_bwd_options above; the layer has no dropout) */
int swf_patch_layer_bwd_opt(const swf_patch_params* p, const float* in, const float* gout, float* gin, const swf_patch_grads* gp,
                            int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t merge_h, int32_t merge_w, int32_t encoder,
                            const swf_bwd_options* opt, swf_bwd_route* route,
                            void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* Adjoint of swf_reflect_pad_fwd (MyPadding encoder side, a006:122-131): gout [B][H+pad_h][W+pad_w][C] -> gin [B][H][W][C]. */
int swf_reflect_pad_bwd(const float* gout, float* gin, int32_t B, int32_t H, int32_t W, int32_t C, int32_t pad_h, int32_t pad_w,
                        swf_stream_t stream);
/* out = a + b (the decoder's skip connection, a013:222-225, when the stages run as separate modules under autograd). */
int swf_add_fwd(const float* a, const float* b, float* out, int64_t count, swf_stream_t stream);

/* AutoPathMLP.forward (a003_AutoPathMLP.py:46-50) on NHWC tokens: out = fc2(ELU(fc1(in))) per stream, no norm, no residual
 * (px / py: only fc1 and fc2 are read; py / y_* NULL for a single path).  SWF_PREC_FAST runs the level-0 width (24 channels,
 * hidden 96 or 4) as ONE launch of the fused block kernel's MLP half, other shapes as split-bf16 GEMMs. */
size_t swf_mlp_workspace_bytes(int32_t precision, int64_t tokens, int32_t channels, int32_t hidden);
int swf_mlp_fwd(int32_t precision, const swf_block_stream_params* px, const swf_block_stream_params* py,
                const float* x_in, const float* y_in, float* x_out, float* y_out,
                int64_t tokens, int32_t channels, int32_t hidden,
                void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- token-level pieces used by the inner reference modules ------------------------------------ */
/* out[tokens][n_out] = act(in[tokens][n_in] . W^T + b) (+ residual); act 0 = none, 1 = the activation: ELU(alpha = 1) here, the
 * swf_activation argument in swf_linear_fwd_act / swf_linear_fwd_prec_act.
 * nn.Linear (a001:42-61) and 1x1 nn.Conv2d on NHWC tokens (a003:21-22, a011:60-63).  Exact fp32. */
int swf_linear_fwd(const swf_linear* lin, const float* in, const float* residual, float* out,
                   int64_t tokens, int32_t n_in, int32_t n_out, int32_t act, swf_stream_t stream);
/* The same with the arithmetic mode as an argument: SWF_PREC_FAST = split-bf16 (bf16x3) MFMA, fp32 accumulate (deterministic
 * split-K for deep K: workspace from swf_linear_workspace_bytes, 0 for SWF_PREC_FP32). */
size_t swf_linear_workspace_bytes(int32_t precision, int64_t tokens, int32_t n_in, int32_t n_out);
int swf_linear_fwd_prec(const swf_linear* lin, int32_t precision, const float* in, const float* residual, float* out,
                        int64_t tokens, int32_t n_in, int32_t n_out, int32_t act,
                        void* workspace, size_t workspace_bytes, swf_stream_t stream);
/* my_layer_norm (a004:54-72): LayerNorm over C of [tokens][C], eps 1e-5; elu != 0 applies the activation after: ELU(alpha = 1) here,
 * the swf_activation argument in swf_layernorm_fwd_act. */
int swf_layernorm_fwd(const swf_norm* ln, const float* in, float* out, int64_t tokens, int32_t C, int32_t elu,
                      swf_stream_t stream);
/* MyPadding encoder side (a006:122-131): reflect-pad bottom/right by (pad_h,pad_w); [B][H][W][C] ->
 * [B][H+pad_h][W+pad_w][C].  An NCHW tensor is passed as B*C maps with C=1.  SWF_ERR_PAD if pad >= dim. */
int swf_reflect_pad_fwd(const float* in, float* out, int32_t B, int32_t H, int32_t W, int32_t C,
                        int32_t pad_h, int32_t pad_w, swf_stream_t stream);
/* MyPadding decoder side (a006:133-146): top-left crop [B][Hp][Wp][C] -> [B][H][W][C]. */
int swf_crop_fwd(const float* in, float* out, int32_t B, int32_t Hp, int32_t Wp, int32_t H, int32_t W, int32_t C,
                 swf_stream_t stream);

/* ---- the entries without a descriptor, with the activation as an argument ----------------------------------------------------------
 * swf_<entry>_act(act, ...) is swf_<entry>(...) with `act` (NULL = the zero descriptor = ELU(alpha = 1)) in place of ELU: the same
 * arguments in the same order behind it, the same workspace query (no workspace depends on the activation: the backward keeps either
 * the pre-activation or the activation in the one hidden buffer it always had), the same results for a default descriptor bit for bit.
 * The entries above are these with act = NULL.  Under SWF_PREC_FAST a non-default activation takes the generic family (swf_activation). */
int swf_mlp_fwd_act(const swf_activation* act, int32_t precision, const swf_block_stream_params* px, const swf_block_stream_params* py,
                    const float* x_in, const float* y_in, float* x_out, float* y_out,
                    int64_t tokens, int32_t channels, int32_t hidden,
                    void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_mlp_fwd_drop_act(const swf_activation* act, const swf_linear* fc1, const swf_linear* fc2, const float* x, float* out, int64_t tokens,
                         int32_t channels, int32_t hidden, const swf_dropout* drop, int32_t stream_id,
                         void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_mlp_bwd_opt_act(const swf_activation* act, const swf_linear* fc1, const swf_linear* fc2, const float* x, const float* gout, float* gx,
                        const swf_linear_grad* gfc1, const swf_linear_grad* gfc2, int64_t tokens, int32_t channels, int32_t hidden,
                        const swf_dropout* drop, int32_t stream_id, const swf_bwd_options* opt, swf_bwd_route* route,
                        void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_patch_merge_fwd_act(const swf_activation* act, const swf_patch_params* p, const float* in, float* out,
                            int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                            int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w,
                            void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_patch_unmerge_fwd_act(const swf_activation* act, const swf_patch_params* p, const float* in, const float* skip, float* out,
                              int32_t B, int32_t Hp, int32_t Wp, int32_t Hm, int32_t Wm, int32_t Cin, int32_t Cout,
                              int32_t merge_h, int32_t merge_w, int32_t Hout, int32_t Wout,
                              void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_patch_merge_fwd_prec_act(const swf_activation* act, int32_t precision, const swf_patch_params* px, const swf_patch_params* py,
                                 const float* x_in, const float* y_in, float* x_out, float* y_out,
                                 int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                 int32_t merge_h, int32_t merge_w, int32_t win_h, int32_t win_w,
                                 const swf_patch_ln1* ln1_x, const swf_patch_ln1* ln1_y, int32_t* route,
                                 void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_patch_unmerge_fwd_prec_act(const swf_activation* act, int32_t precision, const swf_patch_params* px, const swf_patch_params* py,
                                   const float* x_in, const float* y_in, const float* x_skip, const float* y_skip,
                                   float* x_out, float* y_out,
                                   int32_t B, int32_t Hp, int32_t Wp, int32_t Hm, int32_t Wm, int32_t Cin, int32_t Cout,
                                   int32_t merge_h, int32_t merge_w, int32_t Hout, int32_t Wout,
                                   const swf_patch_ln1* ln1_x, const swf_patch_ln1* ln1_y, int32_t* route,
                                   void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_patch_layer_bwd_opt_act(const swf_activation* act, const swf_patch_params* p, const float* in, const float* gout, float* gin,
                                const swf_patch_grads* gp, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                int32_t merge_h, int32_t merge_w, int32_t encoder, const swf_bwd_options* opt, swf_bwd_route* route,
                                void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_final_head_fwd_act(const swf_activation* act, const swf_head_params* p, const float* x, const float* y, float* out,
                           int32_t B, int32_t H, int32_t W, int32_t ksize,
                           void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_final_head_bwd_act(const swf_activation* act, const swf_head_params* p, const float* x, const float* y, const float* gout,
                           float* gx, float* gy, const swf_head_grads* gp, int32_t B, int32_t H, int32_t W, int32_t ksize,
                           int32_t batch_stats, void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_final_head_bwd_sums_act(const swf_activation* act, const swf_head_params* p, const float* x, const float* y, const float* gout,
                                float* sums_out, int32_t B, int32_t H, int32_t W, int32_t ksize,
                                void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_final_head_bwd_synced_act(const swf_activation* act, const swf_head_params* p, const float* x, const float* y, const float* gout,
                                  const float* sums, int64_t count, float* gx, float* gy, const swf_head_grads* gp,
                                  int32_t B, int32_t H, int32_t W, int32_t ksize,
                                  void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_linear_fwd_act(const swf_activation* act_fn, const swf_linear* lin, const float* in, const float* residual, float* out,
                       int64_t tokens, int32_t n_in, int32_t n_out, int32_t act, swf_stream_t stream);
int swf_linear_fwd_prec_act(const swf_activation* act_fn, const swf_linear* lin, int32_t precision, const float* in, const float* residual,
                            float* out, int64_t tokens, int32_t n_in, int32_t n_out, int32_t act,
                            void* workspace, size_t workspace_bytes, swf_stream_t stream);
int swf_layernorm_fwd_act(const swf_activation* act, const swf_norm* ln, const float* in, float* out, int64_t tokens, int32_t C, int32_t elu,
                          swf_stream_t stream);

/* ---- layout helpers for the NCHW module API (a007_utils.py:7-26 are the reference's permutes) */
int swf_nchw_to_nhwc(const float* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, swf_stream_t stream);
int swf_nhwc_to_nchw(const float* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, swf_stream_t stream);

/* ---- whole model: MyModel.forward(in_x, in_y) (a013:209-230) -------------------------------- */
#define SWF_MAX_LEVELS 8
typedef struct swf_model_desc {
    int32_t levels;                      /* len(in_dims_list) */
    int32_t in_dims[SWF_MAX_LEVELS];     /* in_dims_list  (a013:22) */
    int32_t out_dims[SWF_MAX_LEVELS];    /* out_dims_list (a013:23) */
    int32_t heads;                       /* att_num_heads */
    int32_t head_dim[SWF_MAX_LEVELS];    /* floor(out_dims[j]*att_dims_per_head_ratio) (a013:174,191) */
    int32_t mlp_ratio;                   /* mlp_hidden_dims_ratio: encoder hidden = out_dims[j]*ratio (a013:177), decoder hidden = in_dims[j]*ratio (a013:196) */
    int32_t win_h, win_w, merge_h, merge_w;
    int32_t head_ksize;                  /* final_conv_layer_kernel_size */
    int32_t precision;                   /* swf_precision */
    int32_t schedule;                    /* swf_schedule */
    swf_activation act;                  /* mlp_activation_func of every block, patch layer and the head; zero = ELU(alpha = 1) */
} swf_model_desc;

/* The weights live in ONE fp32 device arena whose layout the library defines.  Parameter i has
 * the reference's canonical state_dict key (e.g.
 * "encoder_list.0.3.self_att_block.normal_window_block.auto_path_win_att.window_attention_x.q_for_heads.weight"),
 * an element offset into the arena and an element count; the host copies each tensor there once. */
int32_t swf_model_param_count(const swf_model_desc* desc);
int swf_model_param_info(const swf_model_desc* desc, int32_t index, char* name_buf, size_t name_buf_len,
                         int64_t* offset_elems, int64_t* numel);
int64_t swf_model_arena_elems(const swf_model_desc* desc);
size_t swf_model_workspace_bytes(const swf_model_desc* desc, int32_t B, int32_t H, int32_t W);
/* ir, vis, out: [B][1][H][W] == [B][H][W][1] fp32.  out is NOT clamped (callers clamp: a016:153, a017:83). */
int swf_model_forward(const swf_model_desc* desc, const float* arena, const float* ir, const float* vis,
                      float* out, int32_t B, int32_t H, int32_t W,
                      void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* Optional: derive the fused kernels' weight images (split-bf16, pre-scaled Wq, masked bias matrices) ONCE
 * instead of per call.  `packed` is a caller-owned device buffer of swf_model_packed_bytes(desc) bytes
 * (0 when no level of this model uses a fused kernel); repack after the arena changes. */
size_t swf_model_packed_bytes(const swf_model_desc* desc);
int swf_model_pack_weights(const swf_model_desc* desc, const float* arena, void* packed, size_t packed_bytes,
                           swf_stream_t stream);
int swf_model_forward_packed(const swf_model_desc* desc, const float* arena, const void* packed,
                             const float* ir, const float* vis, float* out, int32_t B, int32_t H, int32_t W,
                             void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* First-forward variant: additionally reports, per cross-attention block, whether its two input streams were identical
 * everywhere — the condition on which the reference prints a message and calls exit() on a model's first forward
 * (a005_BasicBlock.py:98-118, `(x == y).all()`).  cross_equal_flags: device int32[4 * levels], index
 * 2*stage + {0: plain-window cross block, 1: shifted-window cross block}, stages = encoder 0..levels-1 then decoder
 * 0..levels-1; 1 = identical inputs, 0 = inputs differ.  `packed` may be NULL (weights are then packed per call).  The
 * caller reads the flags back after synchronising and raises; the forward itself always completes. */
int swf_model_forward_checked(const swf_model_desc* desc, const float* arena, const void* packed,
                              const float* ir, const float* vis, float* out, int32_t B, int32_t H, int32_t W,
                              void* workspace, size_t workspace_bytes, int32_t* cross_equal_flags, swf_stream_t stream);
/* Measurement entry (bench.py's per-level roofline): swf_model_forward_packed with HIP events recorded on `stream` between
 * the stages of a013:209-230.  Unlike every other entry it SYNCHRONISES the stream (and so cannot be graph-captured), then
 * writes the elapsed milliseconds of the 4 * levels + 1 segments to the host array seg_ms: for s = 0 .. levels-1
 * [2s] = the patch-merging layer of encoder stage s (a011), [2s + 1] = its four BasicBlocks (a012); for j = 0 .. levels-1
 * [2 levels + 2j] = the four BasicBlocks of decoder stage j (level levels-1-j), [2 levels + 2j + 1] = its un-merging layer (with
 * the skip add); [4 levels] = the final head (a013:126-152).  seg_count = capacity of seg_ms. */
int swf_model_forward_profiled(const swf_model_desc* desc, const float* arena, const void* packed,
                               const float* ir, const float* vis, float* out, int32_t B, int32_t H, int32_t W,
                               void* workspace, size_t workspace_bytes, float* seg_ms, int32_t seg_count, swf_stream_t stream);
/* *flag (device int32) = 1 if a[i] == b[i] for every i < count, else 0 (torch semantics: NaN != NaN).  The first-call
 * test of BasicBlock / SelfAndCrossBlockPair (a005:111-113) without a device->host copy of the tensors. */
int swf_tensors_equal(const float* a, const float* b, int64_t count, int32_t* flag, swf_stream_t stream);

/* ---- colour-space steps either side of the model in the reference's inference script ------
 * a015_dataset.py:73-93 / a017_test.py:68,83-88.  OpenCV's 8-bit fixed-point BGR->YCrCb and float YCrCb->RGB,
 * restated from its published formulas (cv2 itself is not available to this build). */
/* bgr [B][H][W][3] uint8 (cv2.imread layout) -> y [B][1][H][W], crcb [B][2][H][W], float32 = uint8/255 */
int swf_bgr8_to_ycrcb_fwd(const uint8_t* bgr, float* y, float* crcb, int32_t B, int32_t H, int32_t W, swf_stream_t stream);
/* IR gray uint8 -> float32 / 255 (v2.ToDtype(scale=True), a015:57-60) */
int swf_gray8_to_unit_fwd(const uint8_t* gray, float* out, int64_t count, swf_stream_t stream);
/* fused_y [B][1][H][W] (unclamped model output), crcb [B][2][H][W] -> clamp(Y,0,1), YCrCb->RGB:
 * rgb_f [B][3][H][W] float32 (may be NULL) and/or rgb8 [B][H][W][3] uint8 quantised like torchvision save_image */
int swf_ycrcb_to_rgb_fwd(const float* fused_y, const float* crcb, float* rgb_f, uint8_t* rgb8,
                         int32_t B, int32_t H, int32_t W, swf_stream_t stream);

/* ---- baseline JPEG encoder: the last line of the reference's test loop, save_image(fus, "..._MKX_SELF.jpg") (a017:112-114) ---------
 * Baseline sequential DCT (SOF0), 8 bits, from RGB [B][H][W][3] (three components in JFIF YCbCr, chroma 4:2:0 or 4:4:4) or gray
 * [B][H][W] (one component).  The files are decoded by Pillow; the bytes are this format's, not libjpeg's: PARITY WITH libjpeg's
 * STREAM IS NOT CLAIMED.  The format, all integer arithmetic:
 *   tables   Annex K luminance / chrominance quantisation tables scaled as libjpeg scales them: s = 5000 / q (integer) for q < 50,
 *            else 200 - 2 q; t = clamp((base s + 50) / 100, 1, 255).  The four Annex K.3 Huffman tables.
 *   colour   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *            Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16; 4:2:0 chroma (a + b + c + d + 2) >> 2 over each 2 x 2.
 *            Partial MCUs at the right and bottom edges replicate the edge pixels of the input before the colour transform.
 *   DCT      level shift -128; C13[u][x] = round(8192 alpha(u) cos((2x + 1) u pi / 16)), alpha(0) = sqrt(1/8), else sqrt(2/8);
 *            rows t = (sum_x C13[u][x] s[x] + 1024) >> 11, then columns c = (sum_y C13[v][y] t[y] + 16384) >> 15;
 *            quantised sign(c) ((|c| + (Q >> 1)) / Q).
 *   entropy  zig-zag scan, DC differences, (run, size) codes with ZRL and EOB, 0xFF -> 0xFF00, as the standard prescribes.
 *   stream   the MCU is 16 x 16 in 4:2:0 (Y00 Y01 Y10 Y11 Cb Cr) and 8 x 8 otherwise.  The restart interval is one MCU row (DRI's Ri =
 *            the MCUs per row): every MCU row starts from zero DC predictors, is padded to a byte with 1-bits and is followed by
 *            RSTm, m = row index mod 8, the last one by EOI instead.
 *   header   SOI, APP0 JFIF 1.01 (no units, density 1:1), DQT (luminance; then chrominance, each its own segment), SOF0, DHT (DC0,
 *            AC0; then DC1, AC1, each its own segment), DRI, SOS; gray carries the luminance tables only.  629 bytes with three
 *            components, 334 with one.
 * swf_jpeg_header_bytes / swf_jpeg_header / swf_jpeg_capacity_bytes / swf_jpeg_workspace_bytes are host-only. */
enum { SWF_JPEG_444 = 0, SWF_JPEG_420 = 1 };
typedef struct swf_jpeg_desc {
    int32_t channels;      /* 1 (gray) or 3 (RGB) */
    int32_t subsampling;   /* SWF_JPEG_444 or SWF_JPEG_420; one channel takes SWF_JPEG_444 only */
    int32_t quality;       /* 1..100 */
} swf_jpeg_desc;
/* Bytes of the header; 0 for a descriptor the encoder would refuse. */
size_t swf_jpeg_header_bytes(const swf_jpeg_desc* desc);
/* host_out[0 .. swf_jpeg_header_bytes) <- the header of an H x W image.  SWF_ERR_BAD_SHAPE for a bad descriptor or H, W < 1,
 * SWF_ERR_UNSUPPORTED for H or W > 65535, SWF_ERR_WORKSPACE for n below the header's size. */
int swf_jpeg_header(const swf_jpeg_desc* desc, int32_t H, int32_t W, uint8_t* host_out, size_t n);
/* The most bytes one image's stream can take: the header, and per MCU row 2 marker bytes and twice its worst bytes before stuffing,
 * ceil(blocks per row (20 + 63 * 26) / 8) (a block is at most a 20-bit DC symbol and 63 AC symbols of 16 + 10 bits, and stuffing at
 * most doubles a byte).  0 for what the encoder would refuse. */
size_t swf_jpeg_capacity_bytes(const swf_jpeg_desc* desc, int32_t H, int32_t W);
/* Bytes of workspace swf_jpeg_encode needs (the carve of kernels_jpeg.hip run without memory): per image the zig-zagged int16
 * coefficients and one int32 bit count per block, one int32 byte count per MCU row, and the rows' staged streams.  0 for what the
 * encoder would refuse. */
size_t swf_jpeg_workspace_bytes(const swf_jpeg_desc* desc, int32_t B, int32_t H, int32_t W);
/* pixels: device [B][H][W][channels] uint8.  header_dev: the bytes of swf_jpeg_header on the device (a caller encodes many batches
 * of one shape with one upload), or NULL: the kernels then write the header from their constant tables.  out: device
 * [B][capacity], capacity >= swf_jpeg_capacity_bytes; out[b][0 .. lengths[b]) <- the file of image b, and no byte of out[b] at or
 * after lengths[b] is written.  lengths: device int32 [B].  Three launches (coefficients, entropy coding per MCU row, packing); no
 * allocation, no copy to the host and no synchronisation, so the call can be captured into a hipGraph on one stream.  The bytes of
 * an image depend on that image alone: not on B, the rest of the batch, an earlier use of the workspace, or timing.
 * SWF_ERR_BAD_SHAPE for B, H or W < 1, quality outside 1..100, channels not 1 or 3, 4:2:0 with one channel or an unknown
 * subsampling; SWF_ERR_UNSUPPORTED for H or W > 65535, B H W > 2^31 - 1 or swf_jpeg_capacity_bytes > 2^31 - 1 (lengths is int32);
 * SWF_ERR_WORKSPACE for a workspace or a capacity below the queries; all before anything is launched. */
int swf_jpeg_encode(const swf_jpeg_desc* desc, const uint8_t* pixels, const uint8_t* header_dev, uint8_t* out, size_t capacity,
                    int32_t* lengths, int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- PNG encoder: the same loop with lossless files, so that the 8-bit levels the fusion metrics are defined on are stored exactly ----
 * 8-bit gray [B][H][W] (colour type 0) or RGB [B][H][W][3] (colour type 2), not interlaced.  Every conforming decoder returns the input
 * pixels.  THE BYTES ARE NOT libpng's OR Pillow's; claimed is only that, and that the filtered stream below is a function of the pixels:
 *   file     signature, IHDR, ONE IDAT, IEND; no other chunk.  The IDAT is a zlib stream: header 0x78 0x01, deflate blocks, Adler-32.
 *   filter   per row the five PNG filters (None, Sub, Up, Average floor((a + b) / 2), Paeth with ties in the order a, b, c) of the
 *            unfiltered bytes channels to the left and one row up, zero outside the image; the row takes the filter with the smallest
 *            sum of min(x, 256 - x) over its filtered bytes, ties to the lowest filter number (libpng's heuristic).  The stream is
 *            every row's filter byte followed by its filtered bytes.
 *   blocks   rows_per_block rows of the stream make one deflate block (the last one what is left); BFINAL on the last block only.
 *   tokens   literals and matches at distance 1 only (no dictionary search): in a block, every maximal stretch of bytes that repeat
 *            their predecessor (which may lie in the block before, never before the stream) is cut into chunks of 258 from its start;
 *            a chunk of 3 or more is one match, a shorter one literals.  Each block ends with the end-of-block symbol.
 *   codes    per block a Huffman code over its literal/length histogram, limited to 15 bits and complete (Kraft sum 1): Huffman's
 *            lengths where they fit, else lengths cut to the limit and repaired from the limit's level; least frequent symbols take the
 *            longest codes, ties by symbol number.  The distance code gives symbols 0 and 1 one bit each (no decoder sees a one-code
 *            tree).  The header codes the lengths with 16, 17 and 18 as zlib does, the code-length code limited to 7 bits the same way.
 *            A block takes the fixed code instead where that is smaller.  No stored blocks.
 *   sums     Adler-32 and the IDAT's CRC-32 are combined from per-row and per-1024-byte values; no lane walks a whole stream.
 * swf_png_capacity_bytes and swf_png_workspace_bytes are host-only. */
typedef struct swf_png_desc {
    int32_t channels;         /* 1 (gray) or 3 (RGB) */
    int32_t rows_per_block;   /* rows of the image per deflate block; 0 = the default, 16 */
    int32_t reserved;         /* 0 */
} swf_png_desc;
/* The most bytes one image's file can take, proved, not measured: 63 bytes of framing (signature 8, IHDR 25, IDAT's length, type and
 * CRC 12, zlib's header 2 and Adler-32 4, IEND 12), and per block at most 17 + 3 * 19 + 7 * (286 + 30) header bits (every length coded
 * by itself costs at most the code-length code's 7 bits, and a repeat symbol stands for three lengths or more in at most 7 + 7), 15
 * bits per stream byte (no code is longer; a match covers three bytes or more in at most 15 + 5 + 1) and 15 for the end-of-block symbol;
 * the fixed code is taken only where it is smaller.  0 for what the encoder would refuse. */
size_t swf_png_capacity_bytes(const swf_png_desc* desc, int32_t H, int32_t W);
/* Bytes of workspace swf_png_encode needs (the carve of kernels_png.hip run without memory): per image the filtered stream, one
 * 16-bit token per stream byte, two Adler sums per row, and per block its code table, header, size and bit offset.  0 for what the
 * encoder would refuse. */
size_t swf_png_workspace_bytes(const swf_png_desc* desc, int32_t B, int32_t H, int32_t W);
/* pixels: device [B][H][W][channels] uint8.  out: device [B][capacity], capacity >= swf_png_capacity_bytes; out[b][0 .. lengths[b]) <-
 * the file of image b; nothing outside out[b][0 .. capacity), lengths and the workspace is written.  lengths: device int32 [B].  Six
 * launches (filter, tokens and codes, framing, emit, CRC segments, CRC); no allocation, no copy to the host and no synchronisation,
 * so the call can be captured into a hipGraph on one stream.  The bytes of an image depend on that image and the descriptor alone: not
 * on B, the rest of the batch, an earlier use of the workspace, or timing.
 * SWF_ERR_NULL for a NULL pointer; SWF_ERR_BAD_SHAPE for B, H or W < 1, channels not 1 or 3, rows_per_block < 0 or reserved != 0;
 * SWF_ERR_UNSUPPORTED for B H W channels, B times the stream or swf_png_capacity_bytes > 2^31 - 1 (lengths is int32) or a block of more
 * than 2^22 stream bytes; SWF_ERR_WORKSPACE for a workspace or a capacity below the queries; all before anything is launched. */
int swf_png_encode(const swf_png_desc* desc, const uint8_t* pixels, uint8_t* out, size_t capacity, int32_t* lengths, int32_t B, int32_t H,
                   int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- baseline JPEG decoder: the input end of the same loop, many files per call ----------------------------------------------------
 * Pixels equal to Pillow's on libjpeg-turbo (Image.open(...).convert(mode)), bit for bit: libjpeg's default decode path is three
 * integer-only pieces, restated here from the published format and the published libjpeg sources.
 *   scope    baseline sequential DCT (SOF0), 8-bit samples, ONE interleaved scan holding all components; one component (its sampling
 *            factors are read as 1 x 1) or three with chroma 1 x 1 and luma 1 x 1, 2 x 1 or 2 x 2 (4:4:4, 4:2:2, 4:2:0); up to four
 *            8-bit quantisation tables and four DC and four AC Huffman tables, arbitrary; any DRI; any APPn / COM; JFIF YCbCr assumed.
 *   parse    host only.  SWF_ERR_UNSUPPORTED (a caller falls back to another decoder): any other SOFn, DAC, precision not 8, 16-bit DQT,
 *            2 or 4 or more components, other sampling, a scan that does not hold every component in frame order or is not Ss 0 Se 63
 *            Ah Al 0, a marker other than EOI behind the scan (several scans), an Adobe APP14 segment with transform 0, components
 *            named 'R' 'G' 'B' without a JFIF segment, H or W of 0, a file of 2^32 bytes or more.  SWF_ERR_BAD_SHAPE (broken): no SOI, a
 *            segment running past the file, SOS before SOF, two SOFs, a table the scan or frame names but no segment defined, a DHT
 *            with more than 256 values, over-subscribed code lengths or a DC symbol above 15, restart markers out of the order RST0 ..
 *            RST7, RST0 .., or a number of restart intervals other than ceil(MCUs / Ri) (1 for Ri = 0).
 *   entropy  one lane per restart interval: bytes [begin, end) of the file, 0xFF00 -> 0xFF, the data ending at the first 0xFF that
 *            is followed by anything else or by nothing; DC predictors from zero; canonical codes (mincode / maxcode / valptr); a
 *            size-0 AC symbol is ZRL for run 15 and EOB for every other run, as libjpeg reads it.  The interval ENDS with a status
 *            kind at: a code that needs more bits than the interval has (SWF_JPEG_STREAM_TRUNCATED); a ZRL or a run that puts the next
 *            coefficient past 63 (SWF_JPEG_STREAM_RUN); 16 bits that start no code, a DC category above 11 or a DC value outside int16
 *            (SWF_JPEG_STREAM_CODE).  Blocks the interval did not reach are zero, the block it ended in keeps what was decoded.
 *            status[file] = the largest kind over the file's intervals (0: none), so it does not depend on timing.
 *   IDCT     dequantised in int32, libjpeg's "islow" 8 x 8 inverse DCT (13-bit constants 2446 3196 4433 6270 7373 9633 12299 15137
 *            16069 16819 20995 25172, columns rounded at 11 bits, rows at 18), + 128, CLAMPED to 0..255 (libjpeg wraps out-of-range
 *            results of crafted coefficients instead; a stream an encoder wrote never reaches that).
 *   finish   libjpeg's "fancy" chroma upsampling: h2v1 (3 this + previous + 1) >> 2 for the even output sample, (3 this + next + 2) >>
 *            2 for the odd one; h2v2 column sums 3 near + far over the two nearest rows, then (3 this + previous + 8) >> 4 and (3 this +
 *            next + 7) >> 4; at the edges the outermost real row / column of the down-sampled component (ceil(H / 2), ceil(W / 2))
 *            repeats.  R = Y + ((91881 (Cr - 128) + 32768) >> 16), B = Y + ((116130 (Cb - 128) + 32768) >> 16), G = Y + ((-22554
 *            (Cb - 128) - 46802 (Cr - 128) + 32768) >> 16), clamped.  Gray from three components is Pillow's convert("L") of that RGB,
 *            (19595 R + 38470 G + 7471 B + 32768) >> 16; colour from one component is R = G = B = Y.
 *   split    swf_jpeg_decode_split: the same result by another entropy pass, for files whose restart intervals are long (no restart
 *            markers: one interval, one lane above).  The self-synchronising decode of Klein & Wiseman and Weissenberger & Schmidt:
 *            each interval's bytes are unstuffed (0xFF00 -> 0xFF, ending as above) into words of the workspace and cut into SEGMENTS of
 *            segment_bytes unstuffed bytes, max(1, ceil(raw length / segment_bytes)) of them, the raw length being what the host knows
 *            (trailing segments may be empty).  A decode state is (bit position, block slot in the MCU, zig-zag index).  Every segment is
 *            decoded speculatively from (its first bit, slot 0, a DC symbol due), one lane per segment, storing nothing; a decode that
 *            meets what the interval path ends at notes the first such failure and goes on by a fixed rule, since from a wrong state
 *            failures are the rule and stopping would keep it from ever falling into step.  Then one workgroup per interval hands end
 *            states from left to right: in round r every segment whose predecessor's end state is not the state it was decoded from
 *            decodes again; after round r segments 0 .. r are final, so at most segments - 1 rounds, fewer when a round changes
 *            nothing.  A prefix sum of completed blocks gives each segment its first block; the first noted failure of the final chain,
 *            if it lies below the interval's block count, is the interval path's.  One more decode per segment stores the coefficients
 *            (DC differences) into the zero-filled area, up to the failure; a last pass per interval sums the differences per
 *            component, finds the first predictor outside int16 (the interval path ends there before writing that block), zeroes from
 *            there on and settles status[file].  IDCT and finish are the launches above.  Coefficients, status and pixels are those of
 *            swf_jpeg_decode whatever the file bytes are.
 * swf_jpeg_parse and the two workspace queries are host-only and touch no GPU. */
enum { SWF_JPEG_OUT_BGR = 0, SWF_JPEG_OUT_RGB = 1, SWF_JPEG_OUT_GRAY = 2 };   /* [H][W][3], [H][W][3], [H][W] */
enum { SWF_JPEG_STREAM_OK = 0, SWF_JPEG_STREAM_TRUNCATED = 1, SWF_JPEG_STREAM_RUN = 2, SWF_JPEG_STREAM_CODE = 3 };
typedef struct swf_jpeg_huff {     /* one Huffman table, Annex F.2.2.3: a code c of length l is a symbol iff c <= maxcode[l] */
    int32_t mincode[17];           /* [l], l = 1..16: the first code of length l */
    int32_t maxcode[17];           /* the last one, -1 when the table has none of that length */
    int32_t valptr[17];            /* index in vals of the symbol of mincode[l] */
    uint8_t vals[256];
    uint16_t look[256];            /* by the next 8 bits: (l << 8) | symbol of the code of length l <= 8 they start with, 0 when they start none */
    int32_t defined;               /* a DHT segment defined it */
} swf_jpeg_huff;
typedef struct swf_jpeg_file {
    uint64_t data_off;             /* SET BY THE CALLER: where the file's bytes start in swf_jpeg_decode's data buffer */
    uint64_t out_off;              /* SET BY THE CALLER: where its pixels go in swf_jpeg_decode's output buffer */
    uint32_t data_bytes;           /* the file's size */
    uint32_t scan_off, scan_end;   /* the entropy-coded data: bytes [scan_off, scan_end) of the file */
    int32_t H, W, components;      /* components 1 or 3 */
    int32_t hs, vs;                /* luma sampling: 1 x 1, 2 x 1 or 2 x 2 (hs x vs); 1 x 1 with one component */
    int32_t mcus_x, mcus_y;        /* ceil(W / (8 hs)), ceil(H / (8 vs)) */
    int32_t blocks;                /* mcus_x mcus_y (hs vs + components - 1): 8 x 8 blocks of all components */
    int32_t restart_interval;      /* DRI's Ri in MCUs; 0: the scan is one interval */
    int32_t intervals;             /* ceil(mcus_x mcus_y / Ri), 1 for Ri = 0 */
    int32_t comp_quant[3], comp_dc[3], comp_ac[3];   /* table index of each component */
    uint16_t quant[4][64];         /* natural (row-major) order; tables no segment defined are zero */
    swf_jpeg_huff dc[4], ac[4];
} swf_jpeg_file;
/* Host only.  data[0 .. n): one file.  *file <- its descriptor (data_off = out_off = 0), *intervals_needed <- file->intervals.
 * intervals: NULL (a size query), or room for intervals_cap pairs of uint32: pair i <- (begin, end) of restart interval i, byte
 * offsets in the file, the marker behind it excluded; SWF_ERR_WORKSPACE when intervals_cap < file->intervals.  The refusals are
 * listed above; SWF_ERR_NULL for a NULL data, file or intervals_needed. */
int swf_jpeg_parse(const uint8_t* data, size_t n, swf_jpeg_file* file, uint32_t* intervals, size_t intervals_cap, size_t* intervals_needed);
/* Bytes of workspace swf_jpeg_decode needs for these files (the carve of kernels_jpegdec.hip run without memory): two uint32 per file
 * and one (first interval, first block; a prefix sum the first launch computes), per 8 x 8 block 64 int16 quantised coefficients and 64
 * uint8 samples.  0 for what the call would refuse.  Host only. */
size_t swf_jpeg_decode_workspace_bytes(const swf_jpeg_file* files_host, int32_t n_files);
/* data: device buffer of data_bytes bytes holding every file at its data_off.  files_host / files_dev: the n_files descriptors in host
 * memory, where they are checked, and the same bytes in device memory, where the kernels read them.  intervals_dev: device, the pairs
 * swf_jpeg_parse wrote, all files' one after another in file order.  out: device buffer of out_bytes bytes; file i's pixels <- out +
 * out_off in `layout`, H W 3 or H W bytes.  status: device int32 [n_files] <- the stream status of each file.  The workspace holds,
 * after the call, per file and component the quantised coefficients, [block row][block column][64] int16 in natural order over the
 * component's grid of whole MCUs (tests read them).  Four launches (prefix sums and status reset; entropy decode, one lane per
 * interval of any file; dequantise + IDCT, one thread per block; upsample + colour, one thread per pixel); no allocation, no copy to
 * the host and no synchronisation, so the call can be captured into a hipGraph on one stream.  A file's pixels depend on that file
 * alone: not on the other files, their order, an earlier use of the workspace, or timing.  Whatever the FILE BYTES are, nothing
 * outside the file's own coefficients, samples, pixels and status word is written, and nothing outside its bytes is read; the
 * descriptors and intervals are trusted to be what swf_jpeg_parse wrote (the host copy is checked).
 * SWF_ERR_NULL for a NULL pointer; SWF_ERR_BAD_SHAPE for n_files < 1, an unknown layout, a descriptor swf_jpeg_parse could not have
 * written, a file that leaves the data buffer, or pixels that leave the output buffer or overlap another file's; SWF_ERR_UNSUPPORTED
 * for more than 65535 files or 2^31 - 1 blocks or intervals in one call; SWF_ERR_WORKSPACE for a workspace below the query; all before
 * anything is launched. */
int swf_jpeg_decode(const uint8_t* data, size_t data_bytes, const swf_jpeg_file* files_host, const swf_jpeg_file* files_dev, int32_t n_files,
                    const uint32_t* intervals_dev, uint8_t* out, size_t out_bytes, int32_t* status, int32_t layout, void* workspace,
                    size_t workspace_bytes, swf_stream_t stream);
/* The split path (see "split" above).  intervals_host: the pairs of intervals_dev in host memory; segment counts, grid sizes and the
 * carve depend on the interval lengths.  segment_bytes: a multiple of 4 in 32 .. 4096.  The workspace starts with the areas of
 * swf_jpeg_decode at their offsets there (tests read the coefficients the same way); at offset swf_jpeg_decode_workspace_bytes(files_host,
 * n_files) follows one swf_jpeg_split_diag per interval of the call, in file order; behind them the split pass's own tables (first
 * segment and first word per interval, unstuffed lengths and words, four records per segment, one per interval).  Ten launches
 * on the stream (two prefix sums, zero fill, unstuff, speculate, synchronise, write, DC, IDCT, finish); no lane waits
 * for another workgroup of its launch; otherwise every guarantee and every refusal of swf_jpeg_decode, plus SWF_ERR_NULL for a NULL
 * intervals_host, SWF_ERR_BAD_SHAPE for another segment_bytes and SWF_ERR_UNSUPPORTED for more than 2^31 - 1 segments or unstuffed
 * words in one call; all before anything is launched.  The query returns 0 for what the call would refuse.  With SWF_DEBUG_SWITCHES=1,
 * SWF_JPEG_DECODE_STAGES selects this call's launches by its own bits: 1 prefix sums and zero fill, 2 unstuff, 4 speculate,
 * 8 synchronise, 16 write, 32 DC, 64 IDCT, 128 finish. */
typedef struct swf_jpeg_split_diag {
    uint32_t segments;             /* of the interval */
    uint32_t rounds;               /* synchronisation rounds run, the one that changed nothing included; 0 for one segment */
    uint32_t wrong;                /* segments whose speculative end state was not their final one */
    uint32_t pad_;
} swf_jpeg_split_diag;
size_t swf_jpeg_decode_split_workspace_bytes(const swf_jpeg_file* files_host, int32_t n_files, const uint32_t* intervals_host,
                                             int32_t segment_bytes);
int swf_jpeg_decode_split(const uint8_t* data, size_t data_bytes, const swf_jpeg_file* files_host, const swf_jpeg_file* files_dev,
                          int32_t n_files, const uint32_t* intervals_dev, const uint32_t* intervals_host, int32_t segment_bytes, uint8_t* out,
                          size_t out_bytes, int32_t* status, int32_t layout, void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- PNG decoder: the files swf_png_encode, libpng and Pillow write, many files per call -------------------------------------------------
 * Pixels equal to Pillow's (Image.open(...).convert("L" | "RGB")), bit for bit.
 *   scope    non-interlaced PNG of bit depth 8, colour types 0 (gray), 2 (RGB), 3 (palette), 4 (gray + alpha) and 6 (RGBA); any number
 *            of IDAT chunks of any length, zero included; any ancillary chunks.
 *   parse    host only.  SWF_ERR_UNSUPPORTED (a caller falls back to another decoder): bit depths 1, 2, 4 and 16, Adam7 interlacing, an
 *            acTL chunk (animated PNG), a critical chunk other than IHDR PLTE IDAT IEND, a file of 2^32 - 1 bytes or more, H (1 + W bpp)
 *            or the IDAT payload above 2^31 - 1.  SWF_ERR_BAD_SHAPE (broken): a bad signature, a chunk running past the file, no IHDR
 *            in front, a second IHDR or PLTE, W or H of 0, an unknown colour type, depth, compression, filter or interlace method, a
 *            CRC-32 mismatch in IHDR or PLTE, no IDAT, IDATs that are not consecutive, type 3 without a PLTE in front of the IDATs, no
 *            IEND, a bad zlib header (CM = 8, CINFO <= 7, FCHECK, FDICT clear; its two bytes may lie in different IDATs).  The CRC-32 of
 *            IDAT chunks is NOT checked: the integrity of the pixel data rests on the stream's Adler-32, which the device verifies.
 *            (Pillow does not appear to check IDAT CRCs either; this was inferred from its behaviour, not verified in its sources.)
 *   gather   each file's IDAT ranges are copied into one contiguous, 16-byte aligned, zero-padded zlib stream in the workspace.
 *   inflate  one wavefront per file; stored, fixed and dynamic blocks, distances up to 32 768 into the file's own earlier output.  The
 *            symbol chain is serial; the lanes share the table construction and the byte copies.  It stops when the final block ends or
 *            at the first error.  Bytes beyond H (1 + W bpp) are counted, never written.
 *   Adler-32 over the inflated bytes, in parallel, against the four bytes behind the final block.
 *   unfilter None, Sub, Up, Average floor((a + b) / 2), Paeth (ties a, b, c), 64 rows in flight, a row a pixel behind the row above.
 *   finish   to gray: the sample of types 0 and 4 (alpha dropped), (19595 R + 38470 G + 7471 B + 32768) >> 16 of types 2, 6 and of the
 *            palette colour of type 3.  To RGB / BGR: the samples of types 2 and 6 (alpha dropped), the palette colour, the gray sample
 *            three times.  A palette index at or beyond the PLTE's length is black.  tRNS is ignored for every type.
 *   status   per file, in this order: the stream's own end (SWF_PNG_STREAM_TRUNCATED: the bits run out before the final block ends;
 *            _CODE: BTYPE 3, stored LEN != ~NLEN, HLIT > 286 or HDIST > 30, an over-subscribed or incomplete set of code lengths other
 *            than an empty distance set or the single one-bit distance code zlib allows, no code for end-of-block, a repeat code with
 *            nothing to repeat or running past HLIT + HDIST, bits that start no code, literal/length symbols 286 and 287, distance
 *            symbols 30 and 31; _DISTANCE: a distance reaching before the first output byte); _TRUNCATED for fewer than H (1 + W bpp)
 *            bytes or fewer than four bytes behind the final block; _LONG for more bytes than expected (the image is complete; the
 *            Adler-32 covers bytes that were dropped and is not compared); _ADLER; _FILTER for a filter byte above 4 in a file whose
 *            stream was sound.  Whole rows the stream delivered are unfiltered and converted up to the first bad filter byte; the rows
 *            behind are zero.
 * Every kernel terminates on every input: the loops are bounded by the bits and the output space remaining, no workgroup waits for
 * another, and the waits inside a workgroup are barriers every lane reaches.
 * swf_png_parse and the workspace query are host-only and touch no GPU. */
enum { SWF_PNG_OUT_BGR = 0, SWF_PNG_OUT_RGB = 1, SWF_PNG_OUT_GRAY = 2 };   /* the values of SWF_JPEG_OUT_*: [H][W][3], [H][W][3], [H][W] */
enum { SWF_PNG_STREAM_OK = 0, SWF_PNG_STREAM_TRUNCATED = 1, SWF_PNG_STREAM_CODE = 2, SWF_PNG_STREAM_DISTANCE = 3, SWF_PNG_STREAM_LONG = 4,
       SWF_PNG_STREAM_ADLER = 5, SWF_PNG_STREAM_FILTER = 6 };
typedef struct swf_png_file {
    uint64_t data_off;             /* SET BY THE CALLER: where the file's bytes start in swf_png_decode's data buffer */
    uint64_t out_off;              /* SET BY THE CALLER: where its pixels go in swf_png_decode's output buffer */
    uint32_t data_bytes;           /* the file's size */
    int32_t H, W;
    int32_t color_type;            /* 0, 2, 3, 4 or 6 */
    int32_t bpp;                   /* bytes per pixel: 1, 3, 1, 2, 4 */
    int32_t palette_entries;       /* PLTE's length for type 3 (1 .. 256), else 0 */
    uint32_t idat_ranges;          /* IDAT chunks, empty ones included */
    uint32_t idat_bytes;           /* their payload in all: the zlib stream's length */
    uint8_t palette[768];          /* RGB triples; zero from palette_entries on */
} swf_png_file;
/* Host only.  data[0 .. n): one file.  *file <- its descriptor (data_off = out_off = 0), *ranges_needed <- file->idat_ranges.  ranges: NULL
 * (a size query), or room for ranges_cap pairs of uint32: pair i <- (offset in the file, length) of the payload of IDAT chunk i;
 * SWF_ERR_WORKSPACE when ranges_cap < file->idat_ranges.  The refusals are listed above; SWF_ERR_NULL for a NULL data, file or
 * ranges_needed. */
int swf_png_parse(const uint8_t* data, size_t n, swf_png_file* file, uint32_t* ranges, size_t ranges_cap, size_t* ranges_needed);
/* Bytes of workspace swf_png_decode needs for these files (the carve of kernels_pngdec.hip run without memory): three uint32 per file
 * and one (prefix sums), a 48-byte record per file, per file its zlib stream + 16 and its H (1 + W bpp) inflated bytes, each rounded up
 * to 16.  0 for what the call would refuse.  Host only. */
size_t swf_png_decode_workspace_bytes(const swf_png_file* files_host, int32_t n_files);
/* data: device buffer of data_bytes bytes holding every file at its data_off.  files_host / files_dev: the n_files descriptors in host
 * memory, where they are checked, and the same bytes in device memory, where the kernels read them.  ranges_dev: device, the pairs
 * swf_png_parse wrote, all files' one after another in file order.  out: device buffer of out_bytes bytes; file i's pixels <- out +
 * out_off in `layout`, H W 3 or H W bytes.  status: device int32 [n_files] <- SWF_PNG_STREAM_* of each file.  Six launches (prefix sums;
 * gather and zero fill; inflate; Adler-32; unfilter; finish); no allocation, no copy to the host and no synchronisation, so the call can
 * be captured into a hipGraph on one stream.  A file's pixels and status depend on that file alone: not on the other files, their order,
 * an earlier use of the workspace, or timing.  Whatever the FILE BYTES are, nothing outside the file's own workspace areas, pixels and
 * status word is written, and nothing outside its bytes is read; the descriptors are trusted to be what swf_png_parse wrote (the host
 * copy is checked), and a range that leaves the file or the stream's area ends the gather of that file.
 * SWF_ERR_NULL for a NULL pointer; SWF_ERR_BAD_SHAPE for n_files < 1, an unknown layout, a descriptor swf_png_parse could not have
 * written, a file that leaves the data buffer, or pixels that leave the output buffer or overlap another file's; SWF_ERR_UNSUPPORTED
 * for more than 65535 files, or inflated bytes, stream bytes or ranges above 2^31 - 1 in one call; SWF_ERR_WORKSPACE for a workspace
 * below the query; all before anything is launched.  With SWF_DEBUG_SWITCHES=1, SWF_PNG_DECODE_STAGES selects the launches by its bits:
 * 1 prefix sums, 2 gather, 4 inflate, 8 Adler-32, 16 unfilter, 32 finish. */
int swf_png_decode(const uint8_t* data, size_t data_bytes, const swf_png_file* files_host, const swf_png_file* files_dev, int32_t n_files,
                   const uint32_t* ranges_dev, uint8_t* out, size_t out_bytes, int32_t* status, int32_t layout, void* workspace,
                   size_t workspace_bytes, swf_stream_t stream);

/* ---- resident paired dataset: the reference's training-time input transform (a015_dataset.py:57-66, :89-103) in one launch --------
 * The decoded uint8 images of a training set lie in two device arenas (gray [H][W], BGR [H][W][3], cv2.imread layouts).  A batch is
 * described by B rows; the launch writes ir = u8/255 and vis_y = cv2's uint8 luma/255 (the BGR->YCrCb restatement above) of the crop
 * box, resized to out_h x out_w as torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False) resizes the
 * cropped float image (which is what torchvision's resized_crop does), then mirrored if flip.  Per axis, with in = crop length,
 * out = output length, scale = in/out, support = max(scale, 1), inv = min(1/scale, 1), output index o: c = scale (o + 0.5),
 * xmin = max(int(c - support + 0.5), 0), xsize = min(int(c + support + 0.5), in) - xmin, weights max(0, 1 - |(j + xmin - c + 0.5) inv|)
 * over their sum, j < xsize.  The geometry is evaluated in fp64 and each normalised weight rounded to fp32 once; horizontal pass, then
 * vertical pass, fp32 fmaf chains in ascending tap order.  Taps never leave the box (crop, then resize); no clamp; no atomics: the
 * result is bit-reproducible, and a sample's result does not depend on the other rows of its launch.  Both images of a row share
 * the geometry, which is what the reference's re-seeding before each image of a pair achieves (a015:100-103). */
typedef struct swf_crop_row {      /* one output sample */
    uint64_t ir_off;               /* byte offset of the gray image [H][W]    in ir_base  */
    uint64_t vis_off;              /* byte offset of the BGR  image [H][W][3] in vis_base */
    int32_t H, W;                  /* source size (both images of a pair have the same) */
    int32_t top, left, h, w;       /* crop box, inside the source, h, w >= 1 */
    int32_t flip;                  /* != 0: mirror the OUTPUT columns */
    int32_t pad_;
} swf_crop_row;
/* Bytes of a table of B rows (host and device buffers alike); 0 for B <= 0. */
size_t swf_paired_crop_rows_bytes(int32_t B);
/* Host only: the rows live in device memory when the kernel reads them and cannot be checked there, so the caller checks its host copy
 * before every upload.  SWF_ERR_BAD_SHAPE for a box that leaves its image or an image that passes its arena of ir_bytes / vis_bytes. */
int swf_paired_crop_rows_check(const swf_crop_row* rows_host, int32_t B, uint64_t ir_bytes, uint64_t vis_bytes);
/* ir_out, vis_y_out: [B][1][out_h][out_w] fp32.  rows_device: B rows in DEVICE memory that passed swf_paired_crop_rows_check; rows are
 * per sample, so images of different sizes share one launch.  One launch, no workspace. */
int swf_paired_crop_resize_fwd(const uint8_t* ir_base, const uint8_t* vis_base, const swf_crop_row* rows_device, int32_t B,
                               int32_t out_h, int32_t out_w, float* ir_out, float* vis_y_out, swf_stream_t stream);

/* ---- the reference's fusion loss (a008_loss.py MyLoss), value and d total / d fusion in one call -----------------
 * total = ssim_ratio*ssim_scale*S + texture_ratio*texture_scale*T + intensity_ratio*intensity_scale*I + psnr_ratio*psnr_scale*P on
 * single-channel fp32 images: S = MS-SSIM + L1 (five Gaussian scales, 33 taps, zero border) or single-scale SSIM (11 taps, sigma
 * 1.5, reflect border) of (fusion, ir) and (fusion, vis); T = mean |Sobel(fusion) - max(Sobel(ir), Sobel(vis))|; I = mean
 * |fusion - max(ir, vis)|; P = 10 log10(mse).  The operators are restated from the published definitions of the kornia classes the
 * reference calls (kornia is not available to this build): PARITY WITH KORNIA ITSELF IS UNPINNED.  Canny is not provided. */
typedef struct swf_loss_desc {
    int32_t ssim_mode;          /* 0 = MS-SSIM + L1 (CHOOSE_MS_SSIM), 1 = single-scale SSIM, window 11 */
    int32_t use_psnr;
    float ir_ssim_weight, ir_psnr_weight;
    float ssim_scale, texture_scale, intensity_scale, psnr_scale;
    float ssim_ratio, texture_ratio, intensity_ratio, psnr_ratio;
} swf_loss_desc;
/* 0 for arguments swf_fusion_loss would refuse */
size_t swf_fusion_loss_workspace_bytes(const swf_loss_desc* desc, int32_t B, int32_t H, int32_t W, int32_t with_grad);
/* fusion, ir, vis: [B][H][W].  terms: device float[5] = S, T, I, P (unscaled, as the four calcu_*_loss methods return them; P = 0
 * when use_psnr = 0) and total.  grad_fusion: NULL, or [B][H][W] <- d total / d fusion, computed in the same call (a term whose
 * ratio*scale is 0 contributes nothing).  Fixed-order reductions, no atomics: results are bit-reproducible; nothing is allocated
 * and the host is not synchronised, so the call can be captured into a hipGraph.  ssim_mode 1 needs H, W >= 6 (SWF_ERR_PAD). */
int swf_fusion_loss(const swf_loss_desc* desc, const float* fusion, const float* ir, const float* vis, float* terms, float* grad_fusion,
                    int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- fusion-quality metrics of fused images against their two sources, ten values per image in one call ------------
 * The numbers the field reports for a fusion method (the reference's README claims them; neither it nor a016 / a017 computes one).
 * Restated from the published definitions and the common open evaluators; no MATLAB or VIFB toolkit is available to this build:
 * PARITY WITH ANY OF THEM IS UNPINNED.  VIF and Nabf are swf_fusion_fidelity's, SSIM, MS-SSIM and the Piella / Cvejic / Yang indices
 * swf_fusion_structure's (both below); the SSIM of swf_fusion_loss is the training loss's, on unit-range floats, not a metric on levels.
 * Levels.  Every metric is a function of 8-bit levels, quantised as torchvision save_image does, in fp32 with two roundings:
 * q = (int) min(max(fadd(fmul(x, 255), 0.5), 0), 255) (never one fused multiply-add; NaN -> 0), so a stored uint8 image passed as
 * u8 / 255.0f evaluates exactly.  F, A, B = the level images of fusion, ir, vis as reals 0..255, N = H W.
 *   EN    -sum p_k log2 p_k over F's 256-bin histogram, empty bins skipped (+0 for one bin)
 *   MI    MI(F, A) + MI(F, B), MI(X, Y) = sum p_xy log2(p_xy / (p_x p_y)) over the 256x256 joint histogram, empty cells skipped
 *   SD    sqrt(mean (F - mean F)^2)
 *   SF    sqrt(RF^2 + CF^2), RF^2 = mean of (F[h][w] - F[h][w-1])^2 over the H (W - 1) differences, CF^2 the same down the columns;
 *         an axis of length 1 contributes 0
 *   AG    mean over the (H - 1)(W - 1) positions of sqrt((gx^2 + gy^2) / 2), gx = F[h][w+1] - F[h][w], gy = F[h+1][w] - F[h][w];
 *         0 when H or W is 1
 *   CC    (r(A, F) + r(B, F)) / 2, r = Pearson's coefficient, defined as 0 when either variance is 0
 *   SCD   r(F - B, A) + r(F - A, B), same convention
 *   MSE   (mean (F - A)^2 + mean (F - B)^2) / 2 on levels;   PSNR = 10 log10(255^2 / MSE), +inf at MSE = 0
 *   QABF  Xydeas & Petrovic: Sobel responses with a zero border, sx with [-1 0 1; -2 0 2; -1 0 1], sy with [1 2 1; 0 0 0; -1 -2 -1];
 *         g = sqrt(sx^2 + sy^2), alpha = atan(sy / sx), pi/2 where sx = 0; sx, sy are exact integers and every comparison is made on
 *         them and on the integer sx^2 + sy^2.  For X in {A, B}: G = g_F / g_X where g_X > g_F, g_F where they are equal (the
 *         published code's convention: 0 on flat pixels), else g_X / g_F; A = 1 - |alpha_X - alpha_F| / (pi/2);
 *         Q_X = Tg / (1 + e^(kg (G - Dg))) Ta / (1 + e^(ka (A - Da))); QABF = sum(Q_A g_A + Q_B g_B) / sum(g_A + g_B), 0 when the
 *         denominator is 0.  Usual constants: Tg 0.9994, kg -15, Dg 0.5, Ta 0.9879, ka -22, Da 0.8.
 * Arithmetic.  Counts and sums of integer products are exact (u32 counters, u64 sums, integer atomics); everything the histograms
 * determine is derived from them (centred fp64 sums over bins and cells); AG and Qabf per pixel in fp64 (IEEE sqrt and division,
 * ocml atan and exp), summed through per-tile partials in a fixed order.  No float atomics: results are bit-identical from call to
 * call, and an image's row does not depend on the rest of its batch. */
typedef struct swf_metrics_desc { double Tg, kg, Dg, Ta, ka, Da; } swf_metrics_desc;   /* Qabf constants */
enum { SWF_METRIC_EN, SWF_METRIC_MI, SWF_METRIC_SD, SWF_METRIC_SF, SWF_METRIC_AG, SWF_METRIC_CC,
       SWF_METRIC_SCD, SWF_METRIC_MSE, SWF_METRIC_PSNR, SWF_METRIC_QABF, SWF_METRIC_COUNT };
/* 0 for a shape swf_fusion_metrics would refuse */
size_t swf_fusion_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* fusion, ir, vis: [B][H][W] fp32.  out: device double [B][SWF_METRIC_COUNT], one row per image.  The call zeroes the part of the
 * workspace it accumulates into, allocates nothing and does not synchronise the host, so it can be captured into a hipGraph.
 * SWF_ERR_BAD_SHAPE for H W > 2^30 (the pixel indices and u32 counters of the kernels) or B > 65535 (split the batch). */
int swf_fusion_metrics(const swf_metrics_desc* desc, const float* fusion, const float* ir, const float* vis,
                       double* out /* device [B][SWF_METRIC_COUNT] */, int32_t B, int32_t H, int32_t W,
                       void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- VIF and Nabf: the two remaining numbers of the field's table, five values per image in one call -----------------------------
 * Restated from the published definitions and the common open evaluators (vifp_mscale; Kumar's objective fusion performance
 * scheme); no MATLAB, VIFB or sewar copy is available to this build: PARITY WITH ANY OF THEM IS UNPINNED.
 * Levels.  F, A, B = the level images of fusion, ir, vis of the metrics above (the same quantiser: fp32, two roundings, never one
 * fused multiply-add, NaN -> 0), taken as reals 0..255.
 *   VIF   VIF_IR + VIF_VIS, VIF_IR = vifp(A, F), VIF_VIS = vifp(B, F): the multi-scale pixel-domain visual information fidelity of
 *         Sheikh and Bovik.  vifp(R, D), with sigma_nsq = 2 and eps = 1e-10, keeps running sums num and den over scales s = 1..4:
 *         N = 2^(5-s) + 1 taps (17, 9, 5, 3); window g[i][j] = exp(-((i-c)^2 + (j-c)^2) / (2 (N/5)^2)), c = (N-1)/2, normalised to
 *         sum 1 (separable: the 1-D factor is normalised).  For s > 1, R and D are first replaced by their "valid" filtering with
 *         this scale's window sampled at even rows and even columns (ceil((n - N + 1) / 2) per axis).  Once a scale's input is
 *         smaller than N in either axis (before or after that step), that scale and all later ones contribute nothing.  With * the
 *         "valid" filtering: mu1 = g*R, mu2 = g*D, s1 = g*(R R) - mu1^2, s2 = g*(D D) - mu2^2, s12 = g*(R D) - mu1 mu2; s1 and s2
 *         are clamped below at 0; gg = s12 / (s1 + eps), sv = s2 - gg s12; then in this order (i) where s1 < eps: gg = 0, sv = s2,
 *         s1 = 0; (ii) where s2 < eps: gg = 0, sv = 0; (iii) where gg < 0: sv = s2, gg = 0; (iv) where sv <= eps: sv = eps;
 *         (v) num += sum log10(1 + gg^2 s1 / (sv + sigma_nsq)), den += sum log10(1 + s1 / sigma_nsq).  vifp = num / den, and 0 when
 *         den = 0 (an image under 17 pixels in an axis, a flat source).
 *   NABF  Kumar's modified fusion-artifact measure, given with its loss term LABF.  Sobel responses with a REPLICATED border, gv with
 *         [-1 0 1; -2 0 2; -1 0 1] / 8, gh with [-1 -2 -1; 0 0 0; 1 2 1] / 8; g = sqrt(gv^2 + gh^2); alpha = atan(gv / gh),
 *         sign(gv) pi/2 where gh = 0 (0 where both are 0).  For X in {A, B}: G_XF = 0 where g_X = 0 or g_F = 0, g_F / g_X where
 *         g_X > g_F, else g_X / g_F; A_XF = | |alpha_X - alpha_F| - pi/2 | 2/pi;
 *         Q_XF = sqrt(Nrg / (1 + e^(-kg (G_XF - sg))) Nra / (1 + e^(-ka (A_XF - sa)))); w_X = g_X sqrt(g_X) where g_X >= Td, else
 *         wt_min.  With loss = (1 - Q_AF) w_A + (1 - Q_BF) w_B, na = (g_F > g_A and g_F > g_B), W = sum (w_A + w_B):
 *         NABF = sum(na loss) / W, LABF = sum((1 - na) loss) / W, so 1 - NABF - LABF = sum(Q_AF w_A + Q_BF w_B) / W.  Every comparison
 *         between magnitudes, and g >= Td, is made on the exact integers 64 g^2 (the unnormalised Sobel sums squared; Td as
 *         64 Td^2).  W > 0 always.  Usual constants: Td 2, wt_min 0.001, Nrg 0.9999, kg 19, sg 0.5, Nra 0.9995, ka 22, sa 0.5.
 * Arithmetic.  fp64 throughout after the quantiser: the variances are differences of sums of products up to 65 025 (an fp32
 * evaluation is 1e-8 to 3e-6 off, every fp64 order within 3e-13).  Window weights are computed on the host in fp64.  Sums go through
 * per-tile partials added in a fixed order; no atomics: results are bit-identical from call to call, and an image's row does not
 * depend on the rest of its batch. */
typedef struct swf_fidelity_desc { double sigma_nsq, eps, Td, wt_min, Nrg, kg, sg, Nra, ka, sa; } swf_fidelity_desc;
enum { SWF_FIDELITY_VIF, SWF_FIDELITY_VIF_IR, SWF_FIDELITY_VIF_VIS, SWF_FIDELITY_NABF, SWF_FIDELITY_LABF, SWF_FIDELITY_COUNT };
/* 0 for a shape swf_fusion_fidelity would refuse */
size_t swf_fusion_fidelity_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* fusion, ir, vis: [B][H][W] fp32.  out: device double [B][SWF_FIDELITY_COUNT], one row per image.  The call writes every workspace
 * element it reads, allocates nothing and does not synchronise the host, so it can be captured into a hipGraph.
 * SWF_ERR_BAD_SHAPE for H W > 2^30 or B > 65535 (the limits of swf_fusion_metrics). */
int swf_fusion_fidelity(const swf_fidelity_desc* desc, const float* fusion, const float* ir, const float* vis,
                        double* out /* device [B][SWF_FIDELITY_COUNT] */, int32_t B, int32_t H, int32_t W,
                        void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- the structural-similarity group: SSIM, MS-SSIM and the Piella / Cvejic / Yang indices, nine values per image in one call ------
 * Restated from the published definitions (Wang et al.'s SSIM and MS-SSIM; Piella and Heijmans' Q_S, Q_W, Q_E; Cvejic et al.'s Q_C;
 * Yang et al.'s Q_Y, as Liu et al.'s assessment of fusion metrics gives them); no MATLAB or toolbox copy is available to this build:
 * PARITY WITH ANY OF THEM IS UNPINNED.
 * Levels.  F, A, B = the level images of fusion, ir, vis of the metrics above (the same quantiser: fp32, two roundings, never one
 * fused multiply-add, NaN -> 0).  C1 = (255 K1)^2, C2 = (255 K2)^2; K1, K2 > 0 is required, so no denominator below is 0.
 * Gaussian group.  Window of 11 taps, sigma 1.5, g[i] = exp(-(i - 5)^2 / (2 1.5^2)) normalised to sum 1 (the 1-D factor; the window is
 * separable); * is the "valid" filtering.  Biased moments, not clamped: mu_X = g*X, var_X = g*(X X) - mu_X^2, cov_XY = g*(X Y) - mu_X mu_Y;
 * l = (2 mu_X mu_Y + C1) / (mu_X^2 + mu_Y^2 + C1), cs = (2 cov_XY + C2) / (var_X + var_Y + C2), ssim(X, Y) = mean(l cs).
 *   SSIM      SSIM_IR + SSIM_VIS, SSIM_IR = ssim(A, F), SSIM_VIS = ssim(B, F) (the sum follows the VIF convention above).  All three
 *             are exactly 0 when min(H, W) < 11.
 *   MS_SSIM   msssim(A, F) + msssim(B, F) over five scales with weights w = 0.0448, 0.2856, 0.3001, 0.2363, 0.1333.  Plane j + 1 is the
 *             mean of the non-overlapping 2x2 blocks of plane j, floor(h / 2) x floor(w / 2) (an odd last row or column is dropped),
 *             kept in fp64 and not re-quantised.  msssim = prod_{j <= 4} max(mean cs_j, 0)^w_j  max(mean (l cs)_5, 0)^w_5.  Exactly 0
 *             when the scale-5 plane is under 11 in an axis, that is when min(H, W) < 176.
 * Box group.  w x w windows at valid positions only, n = w^2; a group's values are exactly 0 when the image is smaller than its
 * window.  Per window the INTEGER sums S_X, S_XX, S_XY; V_X = n S_XX - S_X^2, C_XY = n S_XY - S_X S_Y; mu_X = S_X / n, var_X = V_X / n^2,
 * cov_XY = C_XY / n^2; s(X, Y) = (2 mu_X mu_Y + C1)(2 cov_XY + C2) / ((mu_X^2 + mu_Y^2 + C1)(var_X + var_Y + C2)).
 *   QS        Piella, w = 8: mean t, t = lambda s(A, F) + (1 - lambda) s(B, F), lambda = V_A / (V_A + V_B), 1/2 when V_A + V_B = 0
 *   QW        sum(m t) / sum(m), m = max(V_A, V_B); QS when sum(m) = 0
 *   QE        QW max(QW', 0)^alpha, QW' the same formula on the edge images E_X = |sx| + |sy|, sx and sy the Sobel responses of the
 *             QABF section (its masks, its zero border).  The L1 magnitude is chosen on purpose: an integer of at most 2040, so the
 *             moments of the edge images stay exact.
 *   QC        Cvejic, w = 8: mean [sim s(A, F) + (1 - sim) s(B, F)], sim = clip(C_AF / (C_AF + C_BF), 0, 1), 1/2 when C_AF + C_BF = 0
 *   QY        Yang, w = 7: mean over the windows of lambda s(A, F) + (1 - lambda) s(B, F) where s(A, B) >= Ty, of
 *             max(s(A, F), s(B, F)) elsewhere
 * Usual constants: K1 0.01, K2 0.03, alpha 1, Ty 0.75.
 * Arithmetic.  Box group: the window sums are exact (int32 sums, int64 V and C), EVERY ZERO TEST IS MADE ON THE INTEGERS (V_A + V_B,
 * C_AF + C_BF, sum(m)), and the per-window value is then one fp64 expression.  Gaussian group: fp64 throughout after the quantiser;
 * window weights are computed on the host in fp64.  Sums over windows go through per-tile partials added in a fixed order; no float
 * atomics; one finishing workgroup per image: results are bit-identical from call to call, and an image's row does not depend on the
 * rest of its batch. */
typedef struct swf_structure_desc { double K1, K2, alpha, Ty; } swf_structure_desc;   /* defaults 0.01, 0.03, 1.0, 0.75 */
enum { SWF_STRUCTURE_SSIM, SWF_STRUCTURE_SSIM_IR, SWF_STRUCTURE_SSIM_VIS, SWF_STRUCTURE_MS_SSIM, SWF_STRUCTURE_QS,
       SWF_STRUCTURE_QW, SWF_STRUCTURE_QE, SWF_STRUCTURE_QC, SWF_STRUCTURE_QY, SWF_STRUCTURE_COUNT };
/* 0 for a shape swf_fusion_structure would refuse, and for an image under 7 pixels in an axis, which has no window of any kind and
 * needs no workspace (the call then takes a NULL one and writes nine zeros) */
size_t swf_fusion_structure_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* fusion, ir, vis: [B][H][W] fp32.  out: device double [B][SWF_STRUCTURE_COUNT], one row per image.  The call writes every workspace
 * element it reads, allocates nothing and does not synchronise the host, so it can be captured into a hipGraph on one stream.
 * SWF_ERR_BAD_SHAPE for H W > 2^30 or B > 65535 (the limits of swf_fusion_metrics), and for a non-finite constant, K1 <= 0, K2 <= 0
 * or alpha < 0, before anything is launched. */
int swf_fusion_structure(const swf_structure_desc* desc, const float* fusion, const float* ir, const float* vis,
                         double* out /* device [B][SWF_STRUCTURE_COUNT] */, int32_t B, int32_t H, int32_t W,
                         void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- the human-perception group: Q_CB, Q_CV, and CE, EI, RMSE, five values per image in one call ----------------------------------
 * With the calls above this covers VIFB's thirteen as well (AG, CE, EI, EN, MI, PSNR, Qabf, Q_CB, Q_CV, RMSE, SF, SSIM, SD).  Restated
 * from the published definitions (Chen and Blum 2009; Chen and Varshney 2007; Liu et al.'s assessment of fusion metrics) and the open
 * MATLAB evaluators; none of them is available to this build: PARITY WITH ANY OF THEM IS UNPINNED.  These definitions are this project's.
 * Levels.  F, A, B = the level images of fusion, ir, vis of the metrics above (the same quantiser: fp32, two roundings, never one
 * fused multiply-add, NaN -> 0), N = H W.
 *   stretch(X)   rint((255 (X - min X)) / (max X - min X)); a flat image becomes all zeros
 *   s(j, n)      j if j < ceil(n / 2), else j - n: freqspace with fftshift, written without the shift
 *   spec(X, G)   Re(IDFT2(DFT2(X) o G)), G evaluated at bin (u, v) from rho = sqrt(s(u, H)^2 + s(v, W)^2)
 *   QCB    Chen and Blum.  r = rho / 15, S = exp(-(r / f0)^2) - a exp(-(r / f1)^2).  For each X of A, B, F: X' = spec(stretch(X), S);
 *          b1, b2 = X' filtered with zero padding and 'same' size by the 31x31 kernels exp(-(x^2 + y^2) / (2 sd^2)) / (2 pi sd^2),
 *          x, y = -15 .. 15, sd = 2 for b1 and 4 for b2 (separable; not normalised to sum 1); C = |b1 / b2 - 1|, 0 where b2 = 0;
 *          C' = C^p / (C^q + Z).  Q_XF = min(C'_X, C'_F) / max(C'_X, C'_F), 1 where both are 0; lambda_A = C'_A^2 / (C'_A^2 + C'_B^2),
 *          1/2 where the denominator is 0; QCB = mean(lambda_A Q_AF + (1 - lambda_A) Q_BF).
 *   QCV    Chen and Varshney; LOWER IS BETTER.  On sA, sB, sF = stretch(A), stretch(B), stretch(F): G_X = sqrt(sx^2 + sy^2), the Sobel
 *          responses of the QABF section (its masks, its zero border) of sA and sB; 16x16 blocks tiling from the top-left, partial
 *          blocks kept; lambda_X(block) = sum of G_X^alpha over the block's pixels inside the image;
 *          theta = 2.6 (0.0192 + 0.144 r) exp(-(0.144 r)^1.1), r = rho / 4 (Mannos and Sakrison); D_X(block) = the sum of
 *          spec(sX - sF, theta)^2 over those pixels, divided by 256 always (a partial block is zero-padded);
 *          QCV = sum(lambda_A D_A + lambda_B D_B) / sum(lambda_A + lambda_B) over the blocks, 0 when that denominator is 0.
 *   CE     (ce(A, F) + ce(B, F)) / 2, ce(X, F) = sum_k p_X(k) log2(p_X(k) / p_F(k)) over the bins of the 256-bin histograms where both
 *          are non-zero
 *   EI     mean over the N pixels of sqrt(gv^2 + gh^2), the unnormalised Sobel sums of F of the NABF section (its replicated border)
 *   RMSE   (sqrt(sum (A - F)^2 / N) + sqrt(sum (B - F)^2 / N)) / (2 255): on levels / 255
 * Usual constants: f0 15.3870, f1 1.3456, a 0.7622, p 3, q 2, Z 1e-4, alpha 1.
 * Arithmetic.  fp64 throughout after the quantiser.  spec runs as dense fp64 products on the matrix cores against twiddle matrices
 * exp(-+2 pi i ((j k) mod n) / n) that the call itself builds in its workspace (arguments reduced in integers), over the half
 * spectrum a real image and a real, even filter need.  Histograms are counted without atomics; sums go through per-tile partials added
 * in a fixed order; one finishing workgroup per image: results are bit-identical from call to call, and an image's row does not
 * depend on the rest of its batch.  f0, f1, a, p, q, Z reach QCB only and alpha QCV only. */
typedef struct swf_perception_desc { double f0, f1, a, p, q, Z, alpha; } swf_perception_desc;   /* defaults 15.3870, 1.3456, 0.7622, 3, 2, 1e-4, 1 */
enum { SWF_PERCEPTION_QCB, SWF_PERCEPTION_QCV, SWF_PERCEPTION_CE, SWF_PERCEPTION_EI, SWF_PERCEPTION_RMSE, SWF_PERCEPTION_COUNT };
/* 0 for a shape swf_fusion_perception would refuse */
size_t swf_fusion_perception_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* fusion, ir, vis: [B][H][W] fp32.  out: device double [B][SWF_PERCEPTION_COUNT], one row per image.  The call writes every workspace
 * element it reads, allocates nothing and does not synchronise the host, so it can be captured into a hipGraph on one stream.
 * SWF_ERR_BAD_SHAPE for B, H or W <= 0, and for a non-finite constant, f0 <= 0, f1 <= 0, Z <= 0, p < 0, q < 0 or alpha < 0;
 * SWF_ERR_UNSUPPORTED for H or W > 16384 or B > 13107 (the int32 indices of the dense transforms; the work grows as H W (H + W));
 * all before anything is launched. */
int swf_fusion_perception(const swf_perception_desc* desc, const float* fusion, const float* ir, const float* vis,
                          double* out /* device [B][SWF_PERCEPTION_COUNT] */, int32_t B, int32_t H, int32_t W,
                          void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- the comparative-study group: Q_MI, Q_TE, Q_NCIE, Q_M, Q_SF, Q_P, six values per image in one call ---------------------------
 * The six of the twelve measures of Liu et al.'s comparative study (TPAMI 2012) that the calls above lack (they have Q_G = QABF, Q_S,
 * Q_C, Q_Y, Q_CV, Q_CB).  Restated from memory of the published definitions (Hossny et al.; Cvejic et al. / Nava et al.; Wang et al.;
 * Wang and Liu; Zheng et al.; Zhao et al. with Kovesi's phase congruency); no copy of a paper or of an evaluator is available to this
 * build: PARITY WITH ANY OF THEM IS UNPINNED.  These definitions are this project's, and where a paper differs the text here holds.
 * Known differences from the papers as recalled: Wang and Liu's Q_M uses a wavelet with more scales and a normalised edge-preservation
 * map, here it is two scales of the Haar transform with exp(-|difference|); Kovesi's noise estimate may use the Rayleigh mean or the
 * median and compensates frequency spread, here it is the median and no more; Zhao's Q_P is restated with plain correlation
 * coefficients of whole maps, where the paper may take them over blocks.
 * Levels.  A, B, F = the level images of ir, vis, fusion of the metrics above (the same quantiser), N = H W.  p_X, p_XY = the 256-bin
 * and 256 x 256-bin relative frequencies; H(X) = the entropy with log2, H_b = the entropy with base-256 logarithms (log2 / 8); sums
 * over non-zero bins only; MI(X, Y) = sum p_XY log2(p_XY / (p_X p_Y)).
 *   QMI    2 [MI(A, F) / (H(A) + H(F)) + MI(B, F) / (H(B) + H(F))]; a term whose denominator is 0 contributes 0
 *   QTE    I(X, Y) = (1 - sum p_XY^q / (p_X p_Y)^(q - 1)) / (1 - q), Hq(X) = (1 - sum p_X^q) / (q - 1);
 *          QTE = (I(A, F) + I(B, F)) / (Hq(A) + Hq(B) - I(A, B)), 0 where that denominator is 0
 *   QNCIE  NCC(X, Y) = H_b(X) + H_b(Y) - H_b(X, Y); R = the symmetric 3 x 3 matrix with unit diagonal and the three NCCs in the order
 *          (A, B, F); lambda_i = its eigenvalues by cyclic Jacobi sweeps (pairs (0,1), (0,2), (1,2); t = sign(theta) / (|theta| +
 *          sqrt(theta^2 + 1)), theta = (r_qq - r_pp) / (2 r_pq); until the off-diagonal squares sum to <= 1e-60, 64 sweeps at most);
 *          QNCIE = 1 + sum_i (lambda_i / 3) log_256(lambda_i / 3), a term with lambda_i <= 0 being 0
 *   QSF    D_h = I(i, j) - I(i, j-1), D_v = I(i, j) - I(i-1, j), D_md = I(i, j) - I(i-1, j-1), D_sd = I(i, j) - I(i-1, j+1), each
 *          where both pixels exist; SF = sqrt((sum D_h^2 + sum D_v^2 + w_d sum D_md^2 + w_d sum D_sd^2) / N), w_d = 1 / sqrt 2.  SF_F
 *          from F's differences, SF_R from max(|D(A)|, |D(B)|) per pixel and direction; QSF = (SF_F - SF_R) / SF_R, 0 where SF_R = 0.
 *          The sums are exact integers; the weight is applied once to each exact sum.
 *   QM     on levels / 255: two scales of the decimated orthonormal Haar transform, per 2 x 2 block [a b; c d] of the previous
 *          approximation LL = (a + b + c + d) / 2, LH = (a + b - c - d) / 2, HL = (a - b + c - d) / 2, HH = (a - b - c + d) / 2, an odd
 *          trailing row or column dropped.  At scale s, for X of A, B: EP_X = (exp(-|LH_X - LH_F|) + exp(-|HL_X - HL_F|) +
 *          exp(-|HH_X - HH_F|)) / 3, w_X = LH_X^2 + HL_X^2 + HH_X^2, Q_s = sum(EP_A w_A + EP_B w_B) / sum(w_A + w_B); Q_s = 1 for a
 *          scale without coefficients (an axis under 2, under 4 for the second), 0 when its weights sum to 0;
 *          QM = Q_1^alpha1 Q_2^alpha2
 *   QP     phase congruency of the levels (as doubles), 4 scales s = 1..4 and 6 orientations o = 1..6.  fx = s(v, W) / W,
 *          fy = s(u, H) / H at bin (u, v), s(j, n) of the perception group; rho = sqrt(fx^2 + fy^2), rho(0, 0) = 1;
 *          theta = atan2(-fy, fx); lp = 1 / (1 + (rho / 0.45)^30); G_s = exp(-ln(rho / f_s)^2 / (2 ln(sigma_onf)^2)) lp,
 *          f_s = 1 / (min_wavelength mult^(s-1)), G_s(0, 0) = 0; a = (o - 1) pi / 6, dtheta = min(3 |atan2(sin theta cos a -
 *          cos theta sin a, cos theta cos a + sin theta sin a)|, pi), spread = (cos dtheta + 1) / 2;
 *          EO_so = IDFT2(DFT2(X) G_s spread), E = Re, O = Im, An = |EO|.
 *          Per orientation: sumE, sumO, sumAn = sums over s, maxAn the maximum; XE = sqrt(sumE^2 + sumO^2) + eps, mE = sumE / XE,
 *          mO = sumO / XE; Energy = sum_s (E mE + O mO - |E mO - O mE|); tau = the median over the N pixels of An at s = 1 (the mean
 *          of the two middle values for even N) / sqrt(ln 4); tt = tau (1 - (1 / mult)^4) / (1 - 1 / mult);
 *          T = tt sqrt(pi / 2) + k tt sqrt((4 - pi) / 2); Energy <- max(Energy - T, 0); width = (sumAn / (maxAn + eps) - 1) / 3;
 *          weight = 1 / (1 + exp((cutoff - width) g)); PC_o = weight Energy / (sumAn + eps).
 *          Over orientations: cx2 = sum (PC_o cos a)^2 / 3, cy2 = sum (PC_o sin a)^2 / 3, cxy = sum PC_o^2 cos a sin a / 3;
 *          den = sqrt(cxy^2 + (cx2 - cy2)^2) + eps; M = (cy2 + cx2 + den) / 2, m = (cy2 + cx2 - den) / 2, p = sum_o PC_o.
 *          For each map kind X of p, M, m: S_X = max(X_A, X_B) per pixel; c(U, V) = (cov(U, V) + C) / (sd(U) sd(V) + C), population
 *          moments over the whole image; P_X = max(c(X_A, X_F), c(X_B, X_F), c(S_X, X_F), 0); QP = P_p^ep P_M^eM P_m^em.
 * So F = A = B gives QMI = 2 (not flat), QSF = 0, QM = 1 (not flat), QP = 1; three flat images give QMI = 0, QTE = 0,
 * QNCIE = 1 - log_256 3, QSF = 0, QM = 0 (1 under 2 pixels in an axis), QP = 1.  An axis of one pixel leaves only the differences
 * along the other in QSF.
 * Usual constants: q 1.85, alpha1 1, alpha2 1, min_wavelength 3, mult 2.1, sigma_onf 0.55, k 2, cutoff 0.5, g 10, eps 1e-4, C 1e-4,
 * ep 1, eM 1, em 1.
 * Arithmetic.  fp64 throughout after the quantiser.  The three joint histograms are u32 counts (integer atomics: exact, so their
 * order is immaterial), the marginals their column sums.  QP's transforms are the dense fp64 products of the perception group on the
 * half spectrum: one forward transform per image plane; a filter G_s spread_o splits into its even and odd parts under (u, v) ->
 * (-u, -v), whose filtered spectra invert to E and to i O, so each of the 24 takes two real inverse transforms, the filter applied
 * as the spectrum is loaded.  The median is a radix select over the bit patterns of the non-negative doubles.  Floating-point sums
 * go through per-tile partials added in a fixed order; no floating-point atomics: results are bit-identical from call to call, and
 * an image's row does not depend on the rest of its batch.
 * Workspace (every carve rounded up to 256 bytes), Wh = floor(W / 2) + 1, P = 2 H Wh, t1 = ceil(H / 32) ceil(W / 32),
 * t2 = ceil(N / 1024): doubles 8 H^2 + 4 W Wh (twiddles) + 48 H Wh (filters) + B (3 N + 3 P + 24 P + 24 N + 12 N + 3 + 288 + 12 t1 +
 * 12 t2 + 21 t2), and B 3 65536 u32 counters. */
typedef struct swf_comparative_desc {
    double q, alpha1, alpha2, min_wavelength, mult, sigma_onf, k, cutoff, g, eps, C, ep, eM, em;
} swf_comparative_desc;   /* defaults 1.85, 1, 1, 3, 2.1, 0.55, 2, 0.5, 10, 1e-4, 1e-4, 1, 1, 1 */
enum { SWF_COMPARATIVE_QMI, SWF_COMPARATIVE_QTE, SWF_COMPARATIVE_QNCIE, SWF_COMPARATIVE_QM, SWF_COMPARATIVE_QSF, SWF_COMPARATIVE_QP,
       SWF_COMPARATIVE_COUNT };
/* 0 for a shape swf_fusion_comparative would refuse */
size_t swf_fusion_comparative_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* fusion, ir, vis: [B][H][W] fp32.  out: device double [B][SWF_COMPARATIVE_COUNT], one row per image.  The call zeroes what it
 * accumulates into and writes every other workspace element it reads, allocates nothing and does not synchronise the host, so it
 * can be captured into a hipGraph on one stream.
 * SWF_ERR_BAD_SHAPE for B, H or W <= 0, and for a non-finite constant, q <= 0, q = 1, mult <= 1, sigma_onf outside (0, 1),
 * min_wavelength < 2, eps <= 0, C <= 0 or a negative exponent (alpha1, alpha2, ep, eM, em);
 * SWF_ERR_UNSUPPORTED for H or W > 16384 or B > 2730 (the int32 indices of the dense transforms, 24 transform planes per image);
 * all before anything is launched. */
int swf_fusion_comparative(const swf_comparative_desc* desc, const float* fusion, const float* ir, const float* vis,
                           double* out /* device [B][SWF_COMPARATIVE_COUNT] */, int32_t B, int32_t H, int32_t W,
                           void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- feature mutual information: FMI_pixel, FMI_dct, FMI_w, FMI_edge, four values per image in one call ---------------------------
 * Haghighat and Razian's feature mutual information, the row of the infrared / visible fusion tables the calls above lack.  Restated
 * from memory of the method and of the common open evaluators; no copy of the paper or of an evaluator is available to this build:
 * PARITY WITH ANY OF THEM IS UNPINNED.  These definitions are this project's, and where a paper or an evaluator differs the text here
 * holds.
 * Feature planes.  For X of A = ir, B = vis, F = fusion, L_X = the H x W plane of levels of the metrics above (the same quantiser,
 * NaN -> 0).  T(X) is
 *   pixel  L_X, H x W
 *   edge   |sx| + |sy| of the 3 x 3 Sobel pair (sx = [-1 0 1; -2 0 2; -1 0 1], sy = [1 2 1; 0 0 0; -1 -2 -1]) on L_X with replicated
 *          borders, H x W; exact integers
 *   w      one level of the decimated orthonormal Haar transform with QM's formulas: per 2 x 2 block [a b; c d] LL = (a + b + c + d) / 2,
 *          LH = (a + b - c - d) / 2, HL = (a - b + c - d) / 2, HH = (a - b - c + d) / 2, an odd trailing row or column dropped; the four
 *          sub-bands laid out as the mosaic [LL LH; HL HH], 2 floor(H / 2) x 2 floor(W / 2); multiples of 1/2, exact
 *   dct    the orthonormal 2-D DCT-II D_H L_X D_W^T, D_n[k][i] = s_k sqrt(2 / n) cos(pi (2 i + 1) k / (2 n)), s_0 = 1 / sqrt 2, s_k = 1
 *          otherwise, the cosine argument reduced in integers first (m = ((2 i + 1) k) mod 4 n, then cospi(m / (2 n))); every
 *          coefficient then snapped to rint(T / dct_step) dct_step, ties to even.  The snap makes the value well defined: without it
 *          the windows of a flat or symmetric image would normalise rounding noise of 1e-13 up to full range.
 * FMI of one feature.  The plane is h x w', the window is window x window, every window wholly inside the plane:
 * (h - window + 1)(w' - window + 1) windows; the value is 0 when that count is <= 0.  The l = window^2 samples of a window are read
 * column-major, k = (column offset) window + (row offset), as MATLAB's (:) does.  For a pair (X, F) with window samples x_k, f_k:
 *   1  if x_k = f_k for every k, I(X, F) = 1.
 *   2  otherwise the window pdf: x'_k = 1 for all k when max x = min x, else x'_k = (x_k - min x) / (max x - min x);
 *      p_k = x'_k / sum x'; q_k from f the same way; P_k = sum_{i <= k} p_i, Q_k likewise.
 *   3  c = sum (p_k - 1 / l)(q_k - 1 / l) / sqrt(sum (p_k - 1 / l)^2 sum (q_k - 1 / l)^2), 0 when the denominator is 0.
 *   4  with k counted from 1: mu_p = sum k p_k, sigma_p = sqrt(max(sum k^2 p_k - mu_p^2, 0)); mu_q, sigma_q likewise.
 *   5  the Frechet bound G_ij = min(P_i, Q_j) if c >= 0, max(P_i + Q_j - 1, 0) if c < 0.
 *   6  rho = sum_ij (G_ij - P_i Q_j) / (sigma_p sigma_q), 0 when sigma_p sigma_q = 0.
 *   7  phi = clamp(c / rho, 0, 1), 0 when rho = 0.
 *   8  the joint cdf J_ij = phi G_ij + (1 - phi) P_i Q_j.
 *   9  the joint pdf j_ij = (J_ij - J_(i-1)j) - (J_i(j-1) - J_(i-1)(j-1)), J = 0 at index -1, the parentheses as written.
 *   10 with H(t) = -sum_{t > 0} t log2 t: I(X, F) = 2 (H(p) + H(q) - H(j)) / (H(p) + H(q)), 0 when H(p) + H(q) = 0.
 * The window's value is (I(A, F) + I(B, F)) / 2; FMI is the mean over all windows.
 * So F = A = B gives 1 for every feature that has a window; a 3 x 3 image has one pixel window and no 'w' window at window 3 (its Haar
 * plane is 2 x 2); an axis shorter than the window gives 0.
 * Known differences from the evaluators as recalled: they estimate the joint distribution with further special cases and offer a
 * 'gradient' feature and other wavelets, which are left out here; FMI_EDGE is this project's name for the Sobel plane.
 * Usual constants: window 3, dct_step 2^-16.
 * Arithmetic.  fp64 throughout after the quantiser.  The DCT is two dense fp64 products per plane on the matrix cores against
 * matrices the call builds.  One thread evaluates one window; sums over a window run in the order of k (rows i outer, columns j inner
 * for the cells); the windows' values go through per-tile partials added in a fixed order; no atomics: results are bit-identical from
 * call to call, and an image's row does not depend on the rest of its batch.
 * Workspace (every carve rounded up to 256 bytes), N = H W, hh = floor(H / 2), wh = floor(W / 2), t(h, w) = ceil(max(h - 2, 0) / 16)
 * ceil(max(w - 2, 0) / 16): doubles H^2, W^2 (the DCT matrices), 3 B N, 3 B N (operand and product of the transforms), 12 B hh wh (the
 * Haar mosaics), B (3 t(H, W) + t(2 hh, 2 wh)) (per-tile sums). */
typedef struct swf_feature_desc {
    double window, dct_step;
} swf_feature_desc;   /* defaults 3, 2^-16 */
enum { SWF_FEATURE_FMI_PIXEL, SWF_FEATURE_FMI_DCT, SWF_FEATURE_FMI_W, SWF_FEATURE_FMI_EDGE, SWF_FEATURE_COUNT };
/* 0 for a shape swf_fusion_feature would refuse */
size_t swf_fusion_feature_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* fusion, ir, vis: [B][H][W] fp32.  out: device double [B][SWF_FEATURE_COUNT], one row per image.  The call writes every workspace
 * element it reads, allocates nothing and does not synchronise the host, so it can be captured into a hipGraph on one stream; it
 * writes nothing outside out and its workspace.
 * SWF_ERR_BAD_SHAPE for B, H or W <= 0, for a window that is not 3 or 5 and for a dct_step that is not finite and > 0;
 * SWF_ERR_UNSUPPORTED for H or W > 16384 (the DCT matrices are dense; the work grows as H W (H + W)), H W > 2^30 or B > 21845 (three
 * transform planes per image); all before anything is launched. */
int swf_fusion_feature(const swf_feature_desc* desc, const float* fusion, const float* ir, const float* vis,
                       double* out /* device [B][SWF_FEATURE_COUNT] */, int32_t B, int32_t H, int32_t W,
                       void* workspace, size_t workspace_bytes, swf_stream_t stream);

/* ---- optimiser: torch.optim.Adam's step over a whole parameter group in one launch (a016:67, :165) --------------------------------
 * Per element, in torch's non-capturable order:  g' = clip * g (+ weight_decay * p);  m += (g' - m)(1 - beta1);
 * v = beta2 v + (1 - beta2) g'^2;  p -= step_size * m / (sqrt(v) / bc2_sqrt + eps), IEEE sqrt and division, no atomics.
 * The tensors are described by a TABLE the caller builds in pinned host memory with swf_adam_table_fill: n_tensors rows, then a chunk
 * map (chunk -> row; a chunk is 4096 consecutive elements of one tensor), then room the device side uses for the norm's per-chunk
 * partial sums.  swf_adam_step copies rows and map to table_device with ONE asynchronous copy on `stream` and launches; the host
 * table must stay untouched until that copy has run (the caller double-buffers it or guards it with an event).  No synchronisation,
 * no read-back.  Launches: 1, plus 2 when the call computes the gradient norm. */
typedef struct swf_adam_desc {
    double beta1, beta2, eps, weight_decay;   /* doubles: 1 - beta is formed in double and rounded once, as torch forms it from Python floats */
    double max_grad_norm;                     /* > 0: clip the gradients' global L2 norm (torch.nn.utils.clip_grad_norm_); <= 0: off */
    int32_t norm_ready;                       /* != 0 (with max_grad_norm > 0): norm_out_device already holds this step's norm and coefficient
                                                 (swf_adam_grad_norm over a table that spans several groups); the norm launches are skipped */
} swf_adam_desc;
typedef struct swf_adam_tensor {              /* one table row; device pointers, fp32, contiguous, numel > 0 */
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    int64_t numel;
    float step_size;                          /* lr / (1 - beta1^t), t = this tensor's own step count, computed in double */
    float bc2_sqrt;                           /* sqrt(1 - beta2^t) */
    int32_t first_chunk;                      /* index of the tensor's first chunk (written by swf_adam_table_fill) */
    int32_t reserved;
} swf_adam_tensor;
/* Bytes of a table (host and device buffers alike) for n_tensors tensors of total_elems elements in all; 0 for arguments
 * swf_adam_table_fill would refuse. */
size_t swf_adam_table_bytes(int32_t n_tensors, int64_t total_elems);
/* Host only: write the rows and the chunk map from plain arrays of n_tensors entries (param .. exp_avg_sq: device addresses). */
int swf_adam_table_fill(void* table_host, size_t table_bytes, int32_t n_tensors, const void* const* param, const void* const* grad,
                        const void* const* exp_avg, const void* const* exp_avg_sq, const int64_t* numel, const float* step_size,
                        const float* bc2_sqrt);
/* norm_out_device[0] <- the L2 norm of every gradient of the table (two-level fixed-order fp64 reduction: bit-reproducible, and independent of
 * the gradients' alignment),
 * norm_out_device[1] <- min(1, max_grad_norm / (norm + 1e-6)).  Uploads the table as swf_adam_step does. */
int swf_adam_grad_norm(double max_grad_norm, const void* table_pinned_host, void* table_device, size_t table_bytes, int32_t n_tensors,
                       float* norm_out_device, swf_stream_t stream);
/* One Adam step of every row.  norm_out_device: 2 floats (norm, clip coefficient), written first unless desc->norm_ready, then read
 * by the update; may be NULL when clipping is off.  The gradients themselves are never written. */
int swf_adam_step(const swf_adam_desc* desc, const void* table_pinned_host, void* table_device, size_t table_bytes, int32_t n_tensors,
                  float* norm_out_device, swf_stream_t stream);

/* ---- gather / scatter of a tensor list in one launch (the gradient all-reduce of data-parallel training) ---------------------------
 * n_tensors contiguous fp32 tensors <-> consecutive, UNPADDED segments of one flat fp32 buffer, in the table's order.  The table is the
 * optimiser's (swf_adam_table_bytes / swf_adam_table_fill, uploaded the same way): a row's `grad` is the SOURCE of its elements and its
 * `param` their DESTINATION; exp_avg / exp_avg_sq are not read.  One workgroup per 4096-element chunk, 16-byte stores between the
 * destination's 16-byte boundaries (segment offsets are not aligned), no atomics, no synchronisation, no read-back: capturable.
 * swf_tensors_gather: row i has param = flat + (numel of the rows before it); flat segment <- grad[i] * scale, each product rounded once,
 * so flat is bit for bit scale * cat(tensors).  A row whose grad is NULL (set it after swf_adam_table_fill) fills its segment with zeros.
 * swf_tensors_scatter: row i has grad = flat + (numel of the rows before it); param[i] <- that segment, unscaled.
 * Both check, before the upload, that the rows address exactly those segments and that they end within flat_elems. */
int swf_tensors_gather(const void* table_pinned_host, void* table_device, size_t table_bytes, int32_t n_tensors, float* flat,
                       int64_t flat_elems, float scale, swf_stream_t stream);
int swf_tensors_scatter(const void* table_pinned_host, void* table_device, size_t table_bytes, int32_t n_tensors, const float* flat,
                        int64_t flat_elems, swf_stream_t stream);

/* ---- misc ------------------------------------------------------------------------------------ */
int swf_version(void);                     /* major*1000 + minor */
const char* swf_last_error_string(void);   /* thread-local, never NULL */
const char* swf_status_string(int status);

#ifdef __cplusplus
}
#endif
#endif /* SWINFUSE_H */
