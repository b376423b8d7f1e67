"""Time of the two attention-backward families (swf_bwd_attn: thread / phased) where both run, and of what only the phased family
runs, all in one process on one GPU.  Shapes: the deep levels of `win16` at B = 2, 512 x 512 — level 2 (C = 96, d = 12, a
64 x 64 map), level 3 (C = 192, d = 24, 32 x 32) and level 4 (C = 384, d = 48, 16 x 16: one window per image, the tile the thread family
refuses).  Per shape: WindowAttention's differentiable forward + backward with each family (the same Q / K / V recompute and gradient
GEMMs around either core, so the difference of two rows is the difference of the cores), and one whole training step of `win16`
(forward, MyLoss, backward, FusedAdam) with the phased family.  Median of --iters timed calls after --warmup, HIP events.  One JSON
document on stdout, and in --out when given.

    python tools/backward_phased_bench.py [--iters 10] [--warmup 3] [--out FILE] [--commit ID]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch import nn

import __graft_entry__ as entry

LEVELS = [("level2", 96, 12, 64), ("level3", 192, 24, 32), ("level4", 384, 48, 16)]   # name, C, head_dim, map side at B = 2, 512 x 512
BATCH, SIDE, HEADS, WIN = 2, 512, 8, (16, 16)


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(statistics.median(times), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import CONFIGS, FusedAdam, MyLoss, MyModel, WindowAttention, load_recipe_into, synthetic_pair, train_step
    from swin_unet_image_fusion_amd import _lib as L

    dev = "cuda:0"
    rows = []
    for name, c, d, side in LEVELS:
        m = WindowAttention(c, HEADS, d, WIN, True, True, True, 0.0, 0.0).eval()
        load_recipe_into(m, seed=3, flavor="default")
        m.to(dev)
        m.precision = "fp32"
        g = torch.Generator().manual_seed(5)
        q, kv, up = (torch.randn(BATCH, c, side, side, generator=g).to(dev) for _ in range(3))
        row = {"shape": name, "channels": c, "head_dim": d, "map": [BATCH, side, side], "window": list(WIN), "heads": HEADS,
               "workgroups": BATCH * (side // WIN[0]) * (side // WIN[1]) * HEADS}
        for family in ("thread", "phased"):
            m.backward_attention = family
            row[f"{family}_lds_bytes"] = int(L.lib().swf_attention_bwd_lds_bytes(m._bwd_options().attention, *WIN, d))

            def step():
                ql, kl = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
                m.zero_grad(set_to_none=True)
                (m(ql, kl, kl) * up).sum().backward()

            if row[f"{family}_lds_bytes"] == 0:
                row[f"{family}_fwd_bwd_ms"] = None      # the family refuses the tile
                continue
            row[f"{family}_fwd_bwd_ms"] = median_ms(step, args.iters, args.warmup)
            row[f"{family}_route"] = int(m.last_backward_route.attention)
        if row["thread_fwd_bwd_ms"] is not None:
            row["phased_minus_thread_ms"] = round(row["phased_fwd_bwd_ms"] - row["thread_fwd_bwd_ms"], 4)
        rows.append(row)

    cfg = CONFIGS["win16"]
    model = MyModel(**cfg.model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="default")
    model.to(dev).train()
    model.backward_attention = "phased"
    ir, vis = (torch.from_numpy(a).to(dev) for a in synthetic_pair(BATCH, SIDE, SIDE))
    loss_fn, opt = MyLoss(), FusedAdam(model.parameters(), lr=1e-4)
    step_ms = median_ms(lambda: train_step(model, loss_fn, opt, ir, vis), max(3, args.iters // 2), 2)
    routes = sorted({int(r.attention) for r in model.backward_routes().values()})
    doc = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "what": "median ms, HIP events; *_fwd_bwd_ms: WindowAttention forward (exact fp32) + backward through swf_window_attention_bwd_opt "
                   "(recompute of Q / K / V and the core, 4 dX and 4 dW GEMMs, the attention core of the family); untuned",
           "attention": rows,
           "train_step": {"config": "win16", "batch": BATCH, "side": SIDE, "backward_attention": "phased", "ms": step_ms,
                          "attention_routes": routes}}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
