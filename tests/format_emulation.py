"""Tests only: the fast tier's declared arithmetic restated on the float64 oracle.

window_attention / basic_block below are oracle/swin_fusion_oracle.py's, evaluated in float64, with a rounding inserted at every place
where the kernel source shows one and nowhere else.  What stays float64: LayerNorm, the softmax's exp2, the residual stream, the
relative-position bias (the kernels keep it in fp32 times log2 e), every accumulation.  The result is what the FORMAT costs against the float64 oracle; a
kernel that serves the same shape may differ from it by an independent sample of fp32 rounding noise and by the order of its sums, not by
more (tests/test_gpu_regimes.py holds every kernel to 2x its rel-L2 and 4x its max-rel, plus the exact tier's gate).

Roundings per route family, each with the source line that performs it (paths under swin_unet_image_fusion_amd/csrc/):

  every family, the four projections and the two MLP linears: split-bf16 x3, a.w = a_hi.w_hi + a_hi.w_lo + a_lo.w_hi with hi = bf16(v),
  lo = bf16(v - hi), the lo.lo term left out
      win_frag.h:35-40 (mma3), :42-52 (split8), :54-61 (split4); weights split when they are packed: kernels_win24.hip:666-667,
      kernels_win48.hip:706-707, kernels_win96.hip:1103-1104, kernels_qkvattn.hip:344-345; activations: kernels_win24.hip:95-96 (LayerNorm
      rows), :221-222 (normalised O), :417 (hidden tile), kernels_mlp.hip:213, :290, kernels_deep.hip:196-199, :259-261

  "win"      levels 0 - 2 (kernels_win24 / 48 / 96.hip), 8x8 and 7x7 windows, block and attention half
      Q (weights and bias pre-scaled by d^-0.5 log2 e: kernels_win24.hip:627, :643), K, V -> f16   kernels_win24.hip:337-338, :349-350, :359-360
                                                                                                    kernels_win48.hip:282-298, kernels_win96.hip:300-314
      row maximum -> f16 before it is subtracted                                                    kernels_win24.hip:151, kernels_win48.hip:135, kernels_win96.hip:135
      P = exp2(s - max) -> f16                                                                      kernels_win24.hip:171, kernels_win48.hip:154, kernels_win96.hip:147
      denominator = the sum of the ROUNDED P (V's constant-one channel)                             kernels_win24.hip:644-647 with :216, kernels_win48.hip:339-340,
                                                                                                    kernels_win96.hip:357-358
  "win16"    levels 0 - 2, 16x16 windows: as "win", online softmax over chunks of 64 keys; the running maximum is kept as the f16 value
             that was subtracted, o = o 2^(m_old - m_new) + t in fp32
                                                                                                    kernels_win24.hip:152-158, :180, :553-570, kernels_win48.hip:137-143,
                                                                                                    kernels_win96.hip:950-952
  "qkvattn"  C = 192, 8x8 / 7x7 (kernels_qkvattn.hip): as "win"
      Q (pre-scaled in the pack: :334, :342), K, V -> f16                                           kernels_qkvattn.hip:168-169, :176-177, :182-183
      maximum -> f16; P -> f16; denominator from the rounded P (row 24 of V is 1)                   kernels_qkvattn.hip:228, :249, :253-255
  "core8"    the stand-alone 8x8 / 7x7 core (attn_core_mfma_kernel) and the C = 384 attention + projection kernel
      Q scaled AFTER its linear layer, Q, K, V -> f16                                               kernels_window.hip:148-150; as GEMM epilogue kernels_deep.hip:183-193
                                                                                                    (f16 for all three, copied as they are into the f16 images:
                                                                                                    kernels_window.hip:57-58, :101-103)
      maximum in fp32; denominator = the sum of the UNROUNDED P; P -> f16                           kernels_window.hip:190-206, :218, :227; kernels_attnproj.hip:154-163,
                                                                                                    :173, :179
  "core16"   the stand-alone 16x16 core (attn_core_mfma16_kernel): every deep 16x16 block, and WindowAttention alone on 16x16 windows
      Q scaled after its linear layer, Q, K, V -> f16                                               kernels_window.hip:382-384
      online softmax over tiles of 32 keys, running maximum in fp32; P -> f16                       kernels_window.hip:412, :427-440, :445
      denominator from the rounded P (row D of V^T is 1)                                            kernels_window.hip:315, :449, :454-458

  every family, the MLP's ELU: exp(v) - 1 as an fp32 exp2 and an fp32 subtraction.  2^u is an fp32 number next to 1 (spacing 6e-8 below
  1, 1.2e-7 above), so ELU(v) for v <= 0 carries an ABSOLUTE error of up to 3e-8 .. 6e-8 whatever |v| is: harmless while the hidden
  activations are of order 1, the whole error once fc1's outputs are small and fc2 large (regime mlpsmallK of tests/regime_cases.py)
      "exp2m1"   the deep levels' MLP (families "qkvattn", "core8", "core16"): fl32(fl32(exp2(fl32(v log2 e))) - 1) for v <= 0
                                                                                                    win_frag.h:113 (elu_fast), called at kernels_mlp.hip:286-287
                                                                                                    (the fused MLP) and kernels_deep.hip:195 (the fc1 GEMM's epilogue)
      "folded"   levels 0 - 2 (families "win", "win16"): fc1's weights and bias times fl32(log2 e) and fc2's weights times fl32(ln 2),
                 each rounded to fp32 BEFORE the split; u = fc1'(z); h' = med3(u, L, 0) with L = fl32(fma(fl32(exp2(u)), log2 e, -log2 e))
                                                                                                    win_frag.h:162-165 (elu_exp2), :166-178 (elu_tile); level 2's copy
                                                                                                    kernels_win96.hip:721; the packs: kernels_win24.hip:675, :681,
                                                                                                    kernels_win48.hip:716, :721, :743, kernels_win96.hip:1097, :1101, :1123

Not modelled, because it is below every figure here: the bias of a linear layer riding on a split k slot (kernels_win24.hip:642),
v_exp_f32 / v_rcp_f32 / v_rsq_f32 against libm (1 ulp of fp32; in the ELU that ulp of 2^u is of the size of the rounding modelled above:
at mlpsmall16 the deep levels' kernels measure 8 - 9 % above the emulation in rel-L2, levels 0 - 2 1.00: profiles/r26_range_parity.json).  With every rounding off (Format()) the functions run the oracle's own operations and return its bits; EXP2_ONLY runs the
kernels' formulation (exp2 units, normalisation after P.V, -inf masks, chunks) with no rounding, which agrees with the oracle to 1e-12."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import swin_fusion_oracle as O

Tensor = torch.Tensor
LOG2E = 1.4426950408889634


@dataclass(frozen=True)
class Format:
    split_linear: bool = False     # split-bf16 x3 products in the projections and the MLP
    qkv_f16: bool = False          # Q (pre-scaled), K, V rounded to f16
    scale_in_weights: bool = True  # d^-0.5 log2 e folded into Wq / bq before the split; False: applied to Q after its linear layer
    max_f16: bool = False          # the subtracted maximum rounded to f16
    p_f16: bool = False            # P rounded to f16 for P.V
    den_rounded: bool = False      # the denominator sums the rounded P
    chunk: int = 0                 # keys per step of the online softmax; 0: the whole window at once
    elu: str = ""                  # the MLP's ELU: "" float64 expm1 (the oracle's), "exp2m1" fp32 exp2(v log2 e) - 1, "folded" levels 0 - 2's form
    exp2_path: bool = False        # run the kernels' formulation even with every rounding off
    qk_bf16: bool = False          # NO kernel's arithmetic: Q and K in bf16, as a comment of kernels_window.hip once had it (the host test
                                   # shows that the recorded kernel errors and the GPU test's bounds both rule it out)

    @property
    def kernel_path(self) -> bool:
        return self.exp2_path or self.qkv_f16 or self.max_f16 or self.p_f16 or self.chunk > 0


OFF = Format()
EXP2_ONLY = Format(exp2_path=True)
_WIN = Format(split_linear=True, qkv_f16=True, max_f16=True, p_f16=True, den_rounded=True, elu="folded")
FORMATS = {
    "win": _WIN,
    "win16": replace(_WIN, chunk=64),
    "qkvattn": replace(_WIN, elu="exp2m1"),
    "core8": Format(split_linear=True, qkv_f16=True, scale_in_weights=False, p_f16=True, elu="exp2m1"),
    "core16": Format(split_linear=True, qkv_f16=True, scale_in_weights=False, p_f16=True, den_rounded=True, chunk=32, elu="exp2m1"),
}


def block_family(C: int, heads: int, head_dim: int, win: int) -> str:
    """Which attention arithmetic swf_basic_block_fwd's fast tier applies to a two-stream block (tests/block_cases.route names the
    kernels)"""
    if C < 128:
        return "win16" if win == 16 else "win"
    if win == 16:
        return "core16"
    return "qkvattn" if (C, heads, head_dim) == (192, 8, 24) else "core8"


def attention_family(C: int, heads: int, head_dim: int, win: int) -> str:
    """... and swf_window_attention_fwd_prec's to WindowAttention alone (swf_api.hip:1169-1188: the attention half of the level 0 - 2
    kernels on 8x8 / 7x7 windows, else bf16x3 GEMMs around a stand-alone core)"""
    if C in (24, 48, 96) and heads == 8 and head_dim * 8 == C and win in (7, 8):
        return "win"
    return "core16" if win == 16 else "core8"


# ---- roundings ------------------------------------------------------------------------------------------------------------------------
def bf16(t: Tensor) -> Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def f16(t: Tensor) -> Tensor:
    return t.to(torch.float32).to(torch.float16).to(t.dtype)


def fl32(t: Tensor) -> Tensor:
    return t.to(torch.float32).to(t.dtype)


LOG2E_F32 = float(torch.tensor(LOG2E, dtype=torch.float32))        # kLog2e, kLn2 of win_frag.h:22
LN2_F32 = float(torch.tensor(math.log(2.0), dtype=torch.float32))


def split(t: Tensor) -> Tuple[Tensor, Tensor]:
    hi = bf16(t)
    return hi, bf16(t - hi)


def linear(z: Tensor, w: Tensor, b: Optional[Tensor], fmt: Format) -> Tensor:
    if not fmt.split_linear:
        return F.linear(z, w, b)
    zh, zl = split(z)
    wh, wl = split(w)
    out = zl @ wh.t() + zh @ wl.t() + zh @ wh.t()
    return out if b is None else out + b


def conv1x1(z: Tensor, w: Tensor, b: Tensor, fmt: Format) -> Tensor:
    if not fmt.split_linear:
        return F.conv2d(z, w, b)
    return linear(z.permute(0, 2, 3, 1), w[:, :, 0, 0], b, fmt).permute(0, 3, 1, 2)


# ---- the attention core in the kernels' formulation -------------------------------------------------------------------------------------
def _core(s: Tensor, vh: Tensor, fmt: Format) -> Tensor:
    """s: (windows, heads, t, t) scores in exp2 units, -inf where masked; vh: (windows, heads, t, d).  Online softmax over chunks of
    fmt.chunk keys (one chunk: the two-pass form), normalised after P.V."""
    t = s.shape[-1]
    step = fmt.chunk or t
    m = torch.full_like(s[..., :1], -math.inf)
    o = torch.zeros_like(vh)
    den = torch.zeros_like(m)
    for c0 in range(0, t, step):
        sc = s[..., c0:c0 + step]
        m_new = torch.maximum(m, sc.amax(-1, keepdim=True))
        if fmt.max_f16:
            m_new = f16(m_new)
        dead = torch.isinf(m_new)                        # every key so far masked (the kernels skip such a chunk)
        shift = torch.where(dead, torch.zeros_like(m_new), m_new)
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - shift))
        p = torch.exp2(sc - shift)
        p = torch.where(dead, torch.zeros_like(p), p)
        pr = f16(p) if fmt.p_f16 else p
        o = o * alpha + pr @ vh[..., c0:c0 + step, :]
        den = den * alpha + (pr if fmt.den_rounded else p).sum(-1, keepdim=True)
        m = m_new
    return o / den


def window_attention(sd, prefix: str, q: Tensor, k: Tensor, v: Tensor, *, num_heads: int, dims_per_head: int,
                     window_size: Tuple[int, int], use_cyclic_shift: bool, fmt: Format = OFF) -> Tensor:
    """oracle.window_attention with the roundings of `fmt`"""
    b, c, h, w = q.shape
    wh, ww = window_size
    if h % wh or w % ww:
        raise ValueError(f"map {h}x{w} is not a multiple of the window {wh}x{ww}")
    sh, sw = wh // 2, ww // 2
    if use_cyclic_shift:
        q, k, v = (torch.roll(t, shifts=(-sh, -sw), dims=(2, 3)) for t in (q, k, v))
    t = wh * ww
    qw, kw, vw = (O.window_partition(z, window_size) for z in (q, k, v))
    wgt = lambda name: (sd[prefix + name + ".weight"], sd.get(prefix + name + ".bias"))
    split_heads = lambda z: z.reshape(z.shape[0], t, num_heads, dims_per_head).permute(0, 2, 1, 3)
    table = O.relative_position_bias(sd[prefix + "relative_position_bias_table"], window_size)
    mask = None
    if use_cyclic_shift:
        ids = O.shift_region_ids(h, w, window_size)[None, None].float()
        ids = O.window_partition(ids, window_size)[..., 0]
        mask = ids[:, :, None] != ids[:, None, :]                      # (nW, t, t)
    n_win = (h // wh) * (w // ww)
    if not fmt.kernel_path:                                           # the oracle's own operations
        qh, kh, vh = (split_heads(linear(z, *wgt(n), fmt)) for z, n in ((qw, "q_for_heads"), (kw, "k_for_heads"), (vw, "v_for_heads")))
        scores = torch.matmul(qh, kh.transpose(-1, -2)) * (dims_per_head ** -0.5)
        scores = scores + table
        if mask is not None:
            scores = scores.reshape(b, n_win, num_heads, t, t).masked_fill(mask[None, :, None], -1e10).reshape(b * n_win, num_heads, t, t)
        out = torch.matmul(torch.softmax(scores, dim=-1), vh)
    else:
        scale = dims_per_head ** -0.5 * LOG2E
        wq, bq = wgt("q_for_heads")
        if fmt.scale_in_weights:
            qh = linear(qw, wq * scale, None if bq is None else bq * scale, fmt)
        else:
            qh = linear(qw, wq, bq, fmt) * scale
        kh, vh = linear(kw, *wgt("k_for_heads"), fmt), linear(vw, *wgt("v_for_heads"), fmt)
        if fmt.qkv_f16:
            qh, kh, vh = (bf16(qh), bf16(kh), f16(vh)) if fmt.qk_bf16 else (f16(qh), f16(kh), f16(vh))
        qh, kh, vh = split_heads(qh), split_heads(kh), split_heads(vh)
        scores = torch.matmul(qh, kh.transpose(-1, -2)) + table * LOG2E
        if mask is not None:
            scores = scores.reshape(b, n_win, num_heads, t, t).masked_fill(mask[None, :, None], -math.inf).reshape(b * n_win, num_heads, t, t)
        out = _core(scores, vh, fmt)
    out = out.permute(0, 2, 1, 3).reshape(-1, t, num_heads * dims_per_head)
    out = linear(out, sd[prefix + "linear_projection.weight"], sd[prefix + "linear_projection.bias"], fmt)
    out = O.window_reverse(out, window_size, b, h, w)
    if use_cyclic_shift:
        out = torch.roll(out, shifts=(sh, sw), dims=(2, 3))
    return out


def basic_block(sd, prefix: str, x: Tensor, y: Tensor, *, cross: bool, shift: bool, num_heads: int, dims_per_head: int,
                window_size: Tuple[int, int], fmt: Format = OFF) -> Tuple[Tensor, Tensor]:
    """oracle.basic_block with the roundings of `fmt`"""
    if cross and bool((x == y).all()):
        raise ValueError("cross attention received identical x and y")
    ln = lambda z, name: O.layer_norm_channels(z, sd[prefix + name + ".weight"], sd[prefix + name + ".bias"])
    nx, ny = ln(x, "stage_1.norm_layer_1"), ln(y, "stage_1.norm_layer_2")
    kw = dict(num_heads=num_heads, dims_per_head=dims_per_head, window_size=window_size, use_cyclic_shift=shift, fmt=fmt)
    px, py = prefix + "auto_path_win_att.window_attention_x.", prefix + "auto_path_win_att.window_attention_y."
    if cross:
        ax, ay = window_attention(sd, px, nx, ny, ny, **kw), window_attention(sd, py, ny, nx, nx, **kw)
    else:
        ax, ay = window_attention(sd, px, nx, nx, nx, **kw), window_attention(sd, py, ny, ny, ny, **kw)
    x, y = x + ax, y + ay
    nx, ny = ln(x, "stage_2.norm_layer_1"), ln(y, "stage_2.norm_layer_2")

    def mlp(z, s):
        p = f"{prefix}auto_path_mlp.mlp_{s}_"
        w1, b1, w2, b2 = sd[p + "1.weight"], sd[p + "1.bias"], sd[p + "2.weight"], sd[p + "2.bias"]
        if fmt.elu == "folded":      # h' = ELU(v) log2 e out of u = v log2 e; fc2 carries ln 2
            u = fl32(conv1x1(z, fl32(w1 * LOG2E_F32), fl32(b1 * LOG2E_F32), fmt))
            low = fl32(fl32(torch.exp2(u)) * LOG2E_F32 - LOG2E_F32)      # the fma: the product of two fp32 numbers is exact in float64
            h = torch.maximum(torch.minimum(u, low), torch.minimum(torch.maximum(u, low), torch.zeros_like(u)))     # v_med3_f32(u, L, 0)
            return conv1x1(h, fl32(w2 * LN2_F32), b2, fmt)
        v = conv1x1(z, w1, b1, fmt)
        if fmt.elu == "exp2m1":
            v = fl32(v)
            h = torch.where(v > 0, v, fl32(fl32(torch.exp2(fl32(v * LOG2E_F32))) - 1.0))
        else:
            assert fmt.elu == "", fmt.elu
            h = F.elu(v)
        return conv1x1(h, w2, b2, fmt)
    return x + mlp(nx, "x"), y + mlp(ny, "y")
