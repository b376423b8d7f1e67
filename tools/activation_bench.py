"""What an activation other than ELU(alpha=1) costs: the forward in both tiers and one training step, per activation.

    python tools/activation_bench.py [--batch 16] [--size 256] [--config win8] [--out FILE.json]

nn.ELU() runs the fused fast-tier kernels, every other activation the generic family at the requested precision, so the
fast-tier ratio is the price of leaving the fused kernels; the exact tier and the training step (exact fp32 backward) run the same
kernels for every activation but their epilogues.  Device events around eager calls on one stream, warmed; median with min - max.
Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swin_unet_image_fusion_amd import CONFIGS, FusedAdam, MyLoss, MyModel, load_recipe_into, synthetic_pair, train_step  # noqa: E402

ACTIVATIONS = {"elu": nn.ELU, "gelu": lambda: nn.GELU(approximate="none"), "relu": nn.ReLU}
DEV = "cuda:0"


def timed(fn, warmup, iters):
    """[ms] of `iters` calls of fn, each between two device events, after `warmup` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--config", default="win8")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--train-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("activation_bench needs a GPU")
    ir, vis = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(args.batch, args.size, args.size))
    result = {"workload": f"{args.config}, B={args.batch}, {args.size}x{args.size}, eager, one stream", "activations": {}}
    for name, make in ACTIVATIONS.items():
        model = MyModel(**CONFIGS[args.config].model_kwargs(make()))
        load_recipe_into(model, seed=0, flavor="default")
        model.to(DEV).eval()
        rec = {}
        with torch.no_grad():
            for prec in ("fast", "fp32"):
                model.precision = prec
                model(ir, vis)                      # the first forward runs the input check and builds the arena
                rec[f"forward_{prec}"] = stats(timed(lambda: model(ir, vis), args.warmup, args.iters))
        model.precision = "fast"
        model.train()
        opt, loss = FusedAdam(model.parameters(), lr=1e-4), MyLoss()
        rec["train_step"] = stats(timed(lambda: train_step(model, loss, opt, ir, vis), 1, args.train_iters))
        result["activations"][name] = rec
        print(name, json.dumps(rec), flush=True)
    base = result["activations"]["elu"]
    result["ratio_to_elu"] = {n: {k: round(r[k]["median_ms"] / base[k]["median_ms"], 3) for k in r} for n, r in result["activations"].items()}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
