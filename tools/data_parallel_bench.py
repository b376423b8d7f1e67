"""What the data-parallel step adds on ONE GPU: DataParallelStep(force_collective=True) over a one-rank RCCL group on the full `win8`
model.  Three figures, each the median of --calls calls after --warmup, timed with HIP events around the call:

    reduce_ms          reduce_gradients() alone: the gather of all gradients (33.15 M elements in 1 446 tensors, scale 1), the
                       one-rank all-reduce, and the re-pointing of every p.grad (host_ms: the wall time of the call)
    step_ms            DataParallelStep.step: train_step's order with reduce_gradients() before optimizer.step()
    step_plain_ms      training.train_step on the same model, loss and optimiser

The scaling over real peers cannot be measured on a box with one GPU: a one-rank all-reduce moves nothing between devices.  Writes
profiles/r15_data_parallel.json (with the commit) and prints it as one JSON line.

    python tools/data_parallel_bench.py [--batch 2] [--size 256] [--calls 10] [--warmup 3] [--collective rccl|inprocess]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
from torch import nn

import __graft_entry__ as entry


class OneRank:
    """--collective inprocess: no process group at all (the sum over one rank is the tensor itself)."""
    world_size, rank = 1, 0

    def all_reduce_(self, t):
        return t

    def broadcast_(self, t, src=0):
        return t


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms, host = [], []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4), round(statistics.median(host), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--collective", choices=("rccl", "inprocess"), default="rccl")
    ap.add_argument("--commit", default=None, help="recorded in the file; default: git rev-parse HEAD")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r15_data_parallel.json"))
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import CONFIGS, DataParallelStep, FusedAdam, MyLoss, MyModel, TorchCollective, load_recipe_into, synthetic_pair, train_step
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if args.collective == "rccl":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 200))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        coll = TorchCollective()
    else:
        coll = OneRank()
    model = MyModel(**CONFIGS["win8"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(model, seed=0, flavor="kaiming")
    model.to(dev).train()
    params = list(model.parameters())
    loss_fn, opt = MyLoss(), FusedAdam(params, lr=1e-4, max_grad_norm=1.0)
    dp = DataParallelStep(model, loss_fn, opt, group=coll, force_collective=True)
    ir, vis = (torch.from_numpy(a).to(dev) for a in synthetic_pair(args.batch, args.size, args.size, 1, 2))

    step_ms, step_host = timed(lambda: dp.step(ir, vis), args.calls, args.warmup)
    plain_ms, plain_host = timed(lambda: train_step(model, loss_fn, opt, ir, vis), args.calls, args.warmup)
    gen = torch.Generator(device=dev).manual_seed(0)
    fresh = [torch.randn(p.shape, device=dev, generator=gen) * 1e-3 for p in params]

    def reduce_only():
        for p, g in zip(params, fresh):   # separately allocated gradients, as the backward leaves them
            p.grad = g
        dp.reduce_gradients()
    reduce_ms, reduce_host = timed(reduce_only, args.calls, args.warmup)
    elems = sum(p.numel() for p in params)
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True, check=True).stdout.strip()
        except (OSError, subprocess.CalledProcessError):
            commit = "unknown"
    out = {
        "what": f"data-parallel step on one GPU, force_collective=True, win8, B={args.batch} {args.size}x{args.size}, median of {args.calls} "
                f"calls after {args.warmup}, HIP events around the call",
        "commit": commit, "collective": "one-rank RCCL group" if args.collective == "rccl" else "in-process one-rank stand-in",
        "tensors": len(params), "elements": elems,
        "reduce_gradients": {"ms": reduce_ms, "host_ms": reduce_host, "gather_GB_per_s_if_all_of_it": round(8 * elems / (reduce_ms * 1e-3) / 1e9, 1)},
        "step": {"ms": step_ms, "host_ms": step_host},
        "step_plain": {"ms": plain_ms, "host_ms": plain_host},
        "note": "no threshold; scaling over real peers is not measurable on a one-GPU box (a one-rank all-reduce moves nothing between devices)",
    }
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    if args.collective == "rccl":
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
