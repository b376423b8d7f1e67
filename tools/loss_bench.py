"""Time per call of the fusion loss: (a) swf_fusion_loss value only, (b) value + gradient, (c) the torch restatement
(tests/loss_restatement.py: dense 2-D masks through F.conv2d, what a user without this kernel runs, and what kornia runs in the
reference) forward + backward() in fp32 on the same GPU.  Median of --iters timed calls after warm-up, HIP events.  One JSON line.

    python tools/loss_bench.py [--batch 16] [--size 256] [--iters 20] [--single-scale] [--no-baseline]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__ as entry


def median_ms(fn, iters, warmup=3):
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--single-scale", action="store_true", help="CHOOSE_MS_SSIM = False")
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import MyLoss, _lib as L, synthetic_pair
    from swin_unet_image_fusion_amd.modules import _stream
    from tests import loss_restatement as R
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    b, h, w = args.batch, args.size, args.size
    ir, vis = (torch.from_numpy(a).to(dev) for a in synthetic_pair(b, h, w, seed_ir=1, seed_vis=2))
    fus = (0.5 * torch.maximum(ir, vis) + 0.5 * torch.from_numpy(synthetic_pair(b, h, w, seed_ir=3)[0]).to(dev)).clamp(0, 1)
    loss = MyLoss(choose_ms_ssim=not args.single_scale)
    desc, lib = loss._desc(), L.lib()
    terms, grad = torch.empty(5, device=dev), torch.empty_like(fus)
    need = lib.swf_fusion_loss_workspace_bytes(C.byref(desc), b, h, w, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = _stream(dev)

    def call(g):
        L.check(lib.swf_fusion_loss(C.byref(desc), fus.data_ptr(), ir.data_ptr(), vis.data_ptr(), terms.data_ptr(), g, b, h, w,
                                    ws.data_ptr(), need, stream))

    res = {"what": f"fusion loss B={b} {h}x{w} {'single-scale SSIM' if args.single_scale else 'MS-SSIM + L1'}, ms per call, median of {args.iters}",
           "hip_value_ms": median_ms(lambda: call(None), args.iters),
           "hip_value_and_grad_ms": median_ms(lambda: call(grad.data_ptr()), args.iters),
           "workspace_mb": round(need / 2 ** 20, 1)}

    def module_step():
        f = fus.detach().requires_grad_(True)
        loss.calcu_total_loss(f, ir, vis)[0].backward()

    res["hip_myloss_backward_ms"] = median_ms(module_step, args.iters)   # through autograd, with the 5-float read-back
    if not args.no_baseline:
        def restatement_step():
            f = fus.detach().requires_grad_(True)
            R.fusion_loss(f, ir, vis, choose_ms_ssim=not args.single_scale)[4].backward()
        res["torch_restatement_fwd_bwd_ms"] = median_ms(restatement_step, args.iters)
        res["speedup_vs_restatement"] = round(res["torch_restatement_fwd_bwd_ms"] / res["hip_value_and_grad_ms"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
