"""Time of the optimiser step alone: FusedAdam, FusedAdam(max_grad_norm=1.0), torch.optim.Adam() and torch.optim.Adam(fused=True) on the
parameters of the win8 model (33.15 M elements in 1 446 tensors) and of `tiny`, in one process on one GPU.  Gradients are pre-filled;
each figure is the median of --calls step() calls after --warmup, timed with HIP events around the call (host work of the step that the
GPU waits for is inside the interval; host_ms is the wall time of the step() call itself, which does not synchronise).  Prints one JSON
line: per optimiser ms, host_ms, GB/s (7 x 4 B per element: p, g, m, v read, p, m, v
written; plus 4 B per element for the norm pass) and that rate as a fraction of the 6.29 TB/s float4-copy rate of the MI355X.

    python tools/optim_bench.py [--calls 20] [--warmup 5] [--configs win8,tiny]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch import nn

import __graft_entry__ as entry

COPY_RATE_GBS = 6290.0


def time_steps(opt, calls, warmup):
    for _ in range(warmup):
        opt.step()
    torch.cuda.synchronize()
    ms, host = [], []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        opt.step()
        host.append((time.perf_counter() - t0) * 1e3)   # step() does not synchronise: this is the host's share of the interval
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), statistics.median(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="win8,tiny")
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import CONFIGS, FusedAdam, MyModel, load_recipe_into
    dev = torch.device("cuda:0")
    makers = {
        "fused_adam": (lambda ps: FusedAdam(ps), 28),
        "fused_adam_clip": (lambda ps: FusedAdam(ps, max_grad_norm=1.0), 32),
        "fused_adam_clip_two_groups": (lambda ps: FusedAdam([{"params": ps[0::2]}, {"params": ps[1::2]}], max_grad_norm=1.0), 32),
        "torch_adam": (lambda ps: torch.optim.Adam(ps), 28),
        "torch_adam_fused": (lambda ps: torch.optim.Adam(ps, fused=True), 28),
    }
    out = {"what": f"optimiser step alone, median of {args.calls} calls after {args.warmup}, HIP events around step()", "configs": {}}
    for name in args.configs.split(","):
        model = MyModel(**CONFIGS[name].model_kwargs(nn.ELU(inplace=True)))
        load_recipe_into(model, seed=0, flavor="kaiming")
        model.to(dev)
        params = list(model.parameters())
        elems = sum(p.numel() for p in params)
        gen = torch.Generator(device=dev).manual_seed(0)
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
        res = {"tensors": len(params), "elements": elems}
        for label, (make, bytes_per_elem) in makers.items():
            ms, host_ms = time_steps(make(params), args.calls, args.warmup)
            gbs = bytes_per_elem * elems / (ms * 1e-3) / 1e9
            res[label] = {"ms": round(ms, 4), "host_ms": round(host_ms, 4), "GB_per_s": round(gbs, 1), "fraction_of_copy_rate": round(gbs / COPY_RATE_GBS, 4)}
        out["configs"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
