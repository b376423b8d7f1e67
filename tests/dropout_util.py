"""Test-side restatements of the training-mode dropout (include/swinfuse.h, swf_dropout): Philox4x32-10 and the keep rule in numpy,
and BasicBlock / WindowAttention / AutoPathMLP / MyModel with the reference's four dropout points (a001:351-354, a001:412-414,
a003:25-31) on top of the CPU oracle's pieces.  Masks enter the restatements as tensors: from `mask_np` on the CPU, or from the
library's swf_dropout_mask with a module's last_dropout_seed on the GPU."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import swin_fusion_oracle as O

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Random123's philox4x32_R(10): ctr = four uint32 arrays (or scalars), key = two uint32; returns four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) for v in ctr]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
            k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
    return [v.astype(np.uint32) for v in c]


def mask_np(seed: int, stream: int, site: int, count: int, p: float) -> np.ndarray:
    """The factor (0 or 1 / (1 - p) in fp32) of elements 0 .. count-1, as swf_dropout_mask writes it."""
    g = np.arange((count + 3) // 4, dtype=np.uint64)
    n = g.shape[0]
    words = philox4x32_10([g & _M32, g >> np.uint64(32), np.full(n, site, np.uint64), np.full(n, stream, np.uint64)],
                          (seed & 0xFFFFFFFF, seed >> 32))
    r = np.stack(words, axis=1).reshape(-1)[:count]
    p32 = np.float32(p)
    keep = (r >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 >= float(p32)
    with np.errstate(divide="ignore"):
        scale = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(keep, scale, np.float32(0.0)).astype(np.float32)


def nchw_mask(factors, b: int, h: int, w: int, width: int) -> torch.Tensor:
    """[tokens][width] factors in image order -> a (b, width, h, w) tensor to multiply an NCHW map with."""
    t = torch.as_tensor(np.asarray(factors, dtype=np.float32)).reshape(b, h, w, width)
    return t.permute(0, 3, 1, 2).contiguous()


def window_attention_drop(sd, prefix, q, k, v, m_attn, m_proj, *, num_heads, dims_per_head, window_size, use_cyclic_shift):
    """oracle.window_attention with site 0 on the attention values (in image order, after undoing the window partition and the shift)
    and site 1 on the projection output.  m_attn: (b, heads*d, h, w), m_proj: (b, C, h, w); None = no mask."""
    b, c, h, w = q.shape
    wh, ww = window_size
    sh, sw = wh // 2, ww // 2
    if use_cyclic_shift:
        q, k, v = (torch.roll(t, shifts=(-sh, -sw), dims=(2, 3)) for t in (q, k, v))
    t = wh * ww
    hd = num_heads * dims_per_head
    qw, kw, vw = (O.window_partition(z, window_size) for z in (q, k, v))
    lin = lambda z, name: F.linear(z, sd[prefix + name + ".weight"], sd.get(prefix + name + ".bias"))
    split = lambda z: z.reshape(z.shape[0], t, num_heads, dims_per_head).permute(0, 2, 1, 3)
    qh, kh, vh = split(lin(qw, "q_for_heads")), split(lin(kw, "k_for_heads")), split(lin(vw, "v_for_heads"))
    scores = torch.matmul(qh, kh.transpose(-1, -2)) * (dims_per_head ** -0.5)
    scores = scores + O.relative_position_bias(sd[prefix + "relative_position_bias_table"], window_size)
    if use_cyclic_shift:
        ids = O.shift_region_ids(h, w, window_size)[None, None].float()
        ids = O.window_partition(ids, window_size)[..., 0]
        mask = ids[:, :, None] != ids[:, None, :]
        n_win = mask.shape[0]
        scores = scores.reshape(b, n_win, num_heads, t, t).masked_fill(mask[None, :, None], -1e10).reshape(b * n_win, num_heads, t, t)
    vals = torch.matmul(torch.softmax(scores, dim=-1), vh).permute(0, 2, 1, 3).reshape(-1, t, hd)
    vals = O.window_reverse(vals, window_size, b, h, w)
    if use_cyclic_shift:
        vals = torch.roll(vals, shifts=(sh, sw), dims=(2, 3))
    if m_attn is not None:
        vals = vals * m_attn
    out = F.linear(vals.permute(0, 2, 3, 1), sd[prefix + "linear_projection.weight"], sd[prefix + "linear_projection.bias"])
    out = out.permute(0, 3, 1, 2)
    return out * m_proj if m_proj is not None else out


def mlp_drop(sd, prefix, z, s, m_hidden, m_out):
    """one stream of oracle.auto_path_mlp with sites 2 and 3"""
    z = F.elu(F.conv2d(z, sd[f"{prefix}mlp_{s}_1.weight"], sd[f"{prefix}mlp_{s}_1.bias"]))
    if m_hidden is not None:
        z = z * m_hidden
    z = F.conv2d(z, sd[f"{prefix}mlp_{s}_2.weight"], sd[f"{prefix}mlp_{s}_2.bias"])
    return z * m_out if m_out is not None else z


def block_drop(sd, prefix, x, y, masks, *, cross, shift, num_heads, dims_per_head, window_size):
    """BasicBlock.forward (a005:127-145) with dropout.  masks(stream, site, width) -> (b, width, h, w) tensor or None.  y None = a
    single-path block (stream x only)."""
    streams = [("x", "1", x)] + ([("y", "2", y)] if y is not None else [])
    kw = dict(num_heads=num_heads, dims_per_head=dims_per_head, window_size=window_size, use_cyclic_shift=shift)
    hd = num_heads * dims_per_head
    c = x.shape[1]
    n1 = {s: O.layer_norm_channels(z, sd[f"{prefix}stage_1.norm_layer_{i}.weight"], sd[f"{prefix}stage_1.norm_layer_{i}.bias"])
          for s, i, z in streams}
    outs = []
    for sid, (s, i, z) in enumerate(streams):
        kv = n1["y" if s == "x" else "x"] if (cross and y is not None) else n1[s]
        a = window_attention_drop(sd, f"{prefix}auto_path_win_att.window_attention_{s}.", n1[s], kv, kv, masks(sid, 0, hd), masks(sid, 1, c), **kw)
        z1 = z + a
        n2 = O.layer_norm_channels(z1, sd[f"{prefix}stage_2.norm_layer_{i}.weight"], sd[f"{prefix}stage_2.norm_layer_{i}.bias"])
        hid = sd[f"{prefix}auto_path_mlp.mlp_{s}_1.weight"].shape[0]
        outs.append(z1 + mlp_drop(sd, f"{prefix}auto_path_mlp.", n2, s, masks(sid, 2, hid), masks(sid, 3, c)))
    return tuple(outs) if y is not None else outs[0]


def model_forward_drop(sd, cfg, in_x, in_y, block_masks, training=True):
    """oracle.model_forward with every BasicBlock replaced by block_drop; block_masks(prefix, b, h, w) -> the masks function of the block
    whose state_dict prefix is `prefix` (e.g. 'encoder_list.0.3.self_att_block.normal_window_block.') on its b x h x w map."""
    win, msz = tuple(cfg.window_size), tuple(cfg.merging_size)
    n = len(cfg.in_dims_list)

    def pair(prefix, x, y, lvl):
        kw = dict(num_heads=cfg.att_num_heads, dims_per_head=math.floor(cfg.out_dims_list[lvl] * cfg.att_dims_per_head_ratio),
                  window_size=win)
        for group, cross in (("self_att_block.", False), ("cross_att_block.", True)):
            for blk, shift in (("normal_window_block.", False), ("shifted_window_block.", True)):
                p = prefix + group + blk
                x, y = block_drop(sd, p, x, y, block_masks(p, x.shape[0], x.shape[2], x.shape[3]), cross=cross, shift=shift, **kw)
        return x, y

    x, y = in_x, in_y
    pads, skips = [], []
    for s in range(n):
        x, p = O.pad_to_multiple(x, msz); y, _ = O.pad_to_multiple(y, msz); pads.append(p)
        x, y = O.patch_layer(sd, f"encoder_list.{s}.1.", x, y, encoder=True, merging_size=msz)
        x, p = O.pad_to_multiple(x, win); y, _ = O.pad_to_multiple(y, win); pads.append(p)
        x, y = pair(f"encoder_list.{s}.3.", x, y, s)
        if s < n - 1:
            skips.append((x, y))
    for j in range(n):
        if j > 0:
            hx, hy = skips.pop()
            x, y = x + hx, y + hy
        x, y = pair(f"decoder_list.{j}.0.", x, y, n - 1 - j)
        p = pads.pop(); x, y = O.crop_padding(x, p), O.crop_padding(y, p)
        x, y = O.patch_layer(sd, f"decoder_list.{j}.2.", x, y, encoder=False, merging_size=msz)
        p = pads.pop(); x, y = O.crop_padding(x, p), O.crop_padding(y, p)
    return O.final_head(sd, x, y, cfg.final_conv_layer_kernel_size, training=training)
