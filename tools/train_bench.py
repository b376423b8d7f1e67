"""Time of one training step of the module-by-module autograd path: forward under autograd + backward of every
parameter (exact fp32, atomics-free) + the optimiser's update, model.train() as the reference trains (a016:137).  Prints one JSON line.
--opt sgd (default) is plain SGD at lr 1e-3, adam is torch.optim.Adam() with its defaults, fused-adam is this package's FusedAdam (the
reference's optimiser, a016:67, as one HIP launch).
--loss standin (default) is a smooth stand-in, the mean squared distance to max(ir, vis); --loss fusion is the reference's step
(a016:150-165): clamp_(0, 1), then MyLoss().calcu_total_loss on the fused HIP loss.

--backward-tier fma (default) | mfma selects the kernel family of the gradient GEMMs (MyModel.backward_tier: the same bits either way);
both times the two tiers in one process, each on a fresh model from the same weights, and reports them side by side.

    python tools/train_bench.py [--batch 4] [--size 128] [--config win8] [--iters 5] [--drop P] [--loss standin|fusion]
                                [--opt sgd|adam|fused-adam] [--backward-tier fma|mfma|both]

--drop P sets the three dropout ratios (attention, projection, MLP) to P: every block then runs the exact-fp32 *_drop entries.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch import nn

import __graft_entry__ as entry


def time_steps(args, tier):
    """args.iters timed steps (after one untimed) of a fresh model in backward tier `tier`: ({phase: ms per step}, losses)"""
    from swin_unet_image_fusion_amd import CONFIGS, FusedAdam, MyLoss, MyModel, load_recipe_into, synthetic_pair
    dev = torch.device("cuda:0")
    cfg = CONFIGS[args.config]
    kw = cfg.model_kwargs(nn.ELU(inplace=True))
    kw.update(attention_drop_ratio=args.drop, linear_after_att_drop_ratio=args.drop, mlp_drop_ratio=args.drop)
    model = MyModel(**kw)
    load_recipe_into(model, seed=0, flavor="kaiming")
    model.to(dev).train()
    model.backward_tier = tier
    if args.opt == "sgd":
        opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    else:
        opt = torch.optim.Adam(model.parameters()) if args.opt == "adam" else FusedAdam(model.parameters())
    bumps_versions = args.opt == "fused-adam"   # FusedAdam.step() bumps the version counters itself: no refresh_weights() needed
    ir, vis = (torch.from_numpy(a).to(dev) for a in synthetic_pair(args.batch, args.size, args.size, seed_ir=1, seed_vis=2))
    tgt = torch.maximum(ir, vis)
    fusion_loss = MyLoss() if args.loss == "fusion" else None
    times = {"forward": 0.0, "backward": 0.0, "update": 0.0}
    losses = []
    torch.manual_seed(0)   # the dropout seeds of --drop: the same for every tier
    for it in range(args.iters + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = model(ir, vis)
        if fusion_loss is None:
            loss = (out - tgt).square().mean()
        else:
            loss, _ = fusion_loss.calcu_total_loss(out.clamp_(0, 1), ir, vis)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.cuda.synchronize(); t2 = time.perf_counter()
        opt.step()
        if not bumps_versions:
            model.refresh_weights()
        torch.cuda.synchronize(); t3 = time.perf_counter()
        losses.append(float(loss))
        if it:
            times["forward"] += t1 - t0; times["backward"] += t2 - t1; times["update"] += t3 - t2
    return {k: round(v / args.iters * 1e3, 2) for k, v in times.items()}, losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--config", default="win8")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--drop", type=float, default=0.0, help="attention_drop_ratio = linear_after_att_drop_ratio = mlp_drop_ratio")
    ap.add_argument("--loss", choices=["standin", "fusion"], default="standin")
    ap.add_argument("--opt", choices=["sgd", "adam", "fused-adam"], default="sgd")
    ap.add_argument("--backward-tier", choices=["fma", "mfma", "both"], default="fma", help="kernel family of the gradient GEMMs (MyModel.backward_tier)")
    args = ap.parse_args()
    entry.build()
    label = "SGD" if args.opt == "sgd" else args.opt
    what = f"training step B={args.batch} {args.size}x{args.size} {args.config}, model.train(), autograd path, {label}, dropout {args.drop}, loss {args.loss}"
    tiers = ["fma", "mfma"] if args.backward_tier == "both" else [args.backward_tier]
    res = {}
    for tier in tiers:
        ms, losses = time_steps(args, tier)
        total = sum(ms.values())
        res[tier] = {"ms": ms, "ms_per_step": round(total, 2), "pairs_per_s": round(args.batch / total * 1e3, 1), "loss_first_last": [losses[0], losses[-1]],
                     "losses": losses}
    if len(tiers) == 1:
        r = res[tiers[0]]
        del r["losses"]
        print(json.dumps({"what": what, "backward_tier": tiers[0], **r}))
        return
    # the two families return the same bits, so the two runs must have walked the same losses
    same = res["fma"].pop("losses") == res["mfma"].pop("losses")
    b0, b1 = res["fma"]["ms"]["backward"], res["mfma"]["ms"]["backward"]
    print(json.dumps({"what": what, "tiers": res, "same_losses": same, "backward_ms_fma_over_mfma": round(b0 / b1, 3),
                      "backward_gain_percent": round(100.0 * (b0 - b1) / b0, 1)}))


if __name__ == "__main__":
    main()
