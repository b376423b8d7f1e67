"""Time per call of the fusion-quality metrics (Evaluation), all in one process on one GPU: (a) swf_fusion_metrics, (b) each
of its kernels alone, with the joint-histogram kernel in both forms (LDS-private packed counters / atomics straight to global memory),
(c) the same ten values composed from torch ops (torch.bincount on F * 256 + A for the joint histograms, F.conv2d for Sobel, fp64),
what a user without the kernel runs, and (d) the model forward of the same batch.  Median of --iters timed calls after --warmup, HIP
events.  One JSON line per shape.  The kernels timed alone run without the zeroing stage: each starts from a full call's workspace, so
the finish kernel sees that call's set of non-zero cells (the histogram kernel alone adds to them; the set of cells does not change).

    python tools/metrics_bench.py [--iters 20] [--warmup 5] [--kind noise|smooth] [--no-forward]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

os.environ["SWF_DEBUG_SWITCHES"] = "1"   # before the library loads: the per-kernel timings use its stage switch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torch import nn

import __graft_entry__ as entry

SHAPES = [(16, 256, "win8"), (20, 224, "win7")]


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


def torch_metrics(fus, ir, vis, c):
    """The ten values of include/swinfuse.h from torch ops, batched, fp64 after the fp32 quantiser.  -> (B, 10)"""
    q = lambda x: torch.nan_to_num(x * 255.0 + 0.5, nan=0.0).clamp(0, 255).to(torch.int64)   # torch rounds the product, then the sum
    Fq, A, B_ = q(fus)[:, 0], q(ir)[:, 0], q(vis)[:, 0]
    nb, h, w = Fq.shape
    n = h * w
    base = (torch.arange(nb, device=fus.device) * 65536).view(nb, 1, 1)
    joint = lambda X: torch.bincount((base + Fq * 256 + X).flatten(), minlength=nb * 65536).view(nb, 256, 256).double() / n

    def mi(p):
        px, py = p.sum(2, keepdim=True), p.sum(1, keepdim=True)
        return torch.where(p > 0, p * torch.log2(p / (px * py).clamp_min(1e-300)), torch.zeros_like(p)).sum((1, 2))

    pa, pb = joint(A), joint(B_)
    pf = pa.sum(2)
    en = 0.0 - torch.where(pf > 0, pf * torch.log2(pf.clamp_min(1e-300)), torch.zeros_like(pf)).sum(1)
    Fd, Ad, Bd = Fq.double(), A.double(), B_.double()
    cen = lambda X: X - X.mean((1, 2), keepdim=True)

    def r(X, Y):
        dx, dy = cen(X), cen(Y)
        vx, vy = (dx * dx).mean((1, 2)), (dy * dy).mean((1, 2))
        return torch.where((vx == 0) | (vy == 0), torch.zeros_like(vx), (dx * dy).mean((1, 2)) / (vx * vy).sqrt().clamp_min(1e-300))

    sd = (cen(Fd) ** 2).mean((1, 2)).sqrt()
    rf2 = ((Fd[:, :, 1:] - Fd[:, :, :-1]) ** 2).mean((1, 2)) if w > 1 else torch.zeros_like(sd)
    cf2 = ((Fd[:, 1:] - Fd[:, :-1]) ** 2).mean((1, 2)) if h > 1 else torch.zeros_like(sd)
    gx, gy = Fd[:, :-1, 1:] - Fd[:, :-1, :-1], Fd[:, 1:, :-1] - Fd[:, :-1, :-1]
    ag = ((gx * gx + gy * gy) / 2).sqrt().mean((1, 2)) if h > 1 and w > 1 else torch.zeros_like(sd)
    mse = (((Fd - Ad) ** 2).mean((1, 2)) + ((Fd - Bd) ** 2).mean((1, 2))) / 2
    psnr = 10 * torch.log10(255.0 ** 2 / mse)
    kx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float64, device=fus.device)
    ky = torch.tensor([[1., 2., 1.], [0., 0., 0.], [-1., -2., -1.]], dtype=torch.float64, device=fus.device)
    k = torch.stack([kx, ky]).unsqueeze(1)

    def edge(X):
        s = F.conv2d(X.unsqueeze(1), k, padding=1)
        sx, sy = s[:, 0], s[:, 1]
        alpha = torch.where(sx == 0, torch.full_like(sx, math.pi / 2), torch.atan(sy / torch.where(sx == 0, torch.ones_like(sx), sx)))
        return sx * sx + sy * sy, alpha

    nF, aF = edge(Fd)
    gF = nF.sqrt()
    num = den = 0
    for X in (Ad, Bd):
        nX, aX = edge(X)
        gX = nX.sqrt()
        G = torch.where(nX > nF, gF / gX.clamp_min(1e-300), torch.where(nX == nF, gF, gX / gF.clamp_min(1e-300)))
        Aa = 1 - (aX - aF).abs() / (math.pi / 2)
        Q = c["Tg"] / (1 + torch.exp(c["kg"] * (G - c["Dg"]))) * c["Ta"] / (1 + torch.exp(c["ka"] * (Aa - c["Da"])))
        num, den = num + (Q * gX).sum((1, 2)), den + gX.sum((1, 2))
    qabf = torch.where(den == 0, torch.zeros_like(den), num / den.clamp_min(1e-300))
    return torch.stack([en, mi(pa) + mi(pb), sd, (rf2 + cf2).sqrt(), ag, (r(Ad, Fd) + r(Bd, Fd)) / 2, r(Fd - Bd, Ad) + r(Fd - Ad, Bd), mse,
                        psnr, qabf], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kind", default="noise", choices=["noise", "smooth"], help="smooth: 7x7 box blur (counts crowd the diagonal)")
    ap.add_argument("--no-forward", action="store_true")
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import CONFIGS, MyModel, _lib as L, fusion_metrics, load_recipe_into, synthetic_pair
    from swin_unet_image_fusion_amd.metrics import QABF_DEFAULTS
    from swin_unet_image_fusion_amd.modules import _stream
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    lib, desc = L.lib(), L.MetricsDesc(*QABF_DEFAULTS.values())
    torch.set_grad_enabled(False)
    for b, size, cfg in SHAPES:
        h = w = size
        ir, vis = (torch.from_numpy(a).to(dev) for a in synthetic_pair(b, h, w, seed_ir=1, seed_vis=2))
        noise = torch.from_numpy(synthetic_pair(b, h, w, seed_ir=3)[0]).to(dev)
        if args.kind == "smooth":
            blur = lambda x: F.avg_pool2d(F.pad(x, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
            ir, vis, noise = blur(ir), blur(vis), blur(noise)
        fus = (0.5 * torch.maximum(ir, vis) + 0.5 * noise).clamp(0, 1)
        need = lib.swf_fusion_metrics_workspace_bytes(b, h, w)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((b, L.METRIC_COUNT), dtype=torch.float64, device=dev)
        stream = _stream(dev)

        def call():
            L.check(lib.swf_fusion_metrics(C.byref(desc), fus.data_ptr(), ir.data_ptr(), vis.data_ptr(), out.data_ptr(), b, h, w,
                                           ws.data_ptr(), need, stream))

        def timed(stages=None, hist=None):
            for key, val in (("SWF_METRICS_STAGES", stages), ("SWF_METRICS_HIST", hist)):
                os.environ.pop(key, None)
                if val is not None:
                    os.environ[key] = str(val)
            ms = median_ms(call, args.iters, args.warmup)
            os.environ.pop("SWF_METRICS_STAGES", None)
            os.environ.pop("SWF_METRICS_HIST", None)
            return ms

        res = {"what": f"fusion metrics B={b} {h}x{w} ({args.kind} images), ms per call, median of {args.iters} after {args.warmup}",
               "hip_call_ms": timed(),
               "hip_call_hist_global_atomics_ms": timed(hist="global"),
               "zeroing_ms": timed(stages=1),
               "hist_kernel_lds_private_ms": timed(stages=2),
               "hist_kernel_global_atomics_ms": timed(stages=2, hist="global"),
               "grad_kernel_ms": timed(stages=4),
               "finish_kernel_ms": (call(), timed(stages=8))[1],   # a full call first: the finish kernel reads counts that sum to N
               "workspace_mb": round(need / 2 ** 20, 1)}
        call()
        fused = out.clone()
        res["torch_composition_ms"] = median_ms(lambda: torch_metrics(fus, ir, vis, QABF_DEFAULTS), args.iters, args.warmup)
        res["speedup_vs_torch_composition"] = round(res["torch_composition_ms"] / res["hip_call_ms"], 1)
        res["max_distance_to_torch_composition"] = float(((torch_metrics(fus, ir, vis, QABF_DEFAULTS) - fused).abs()
                                                          / fused.abs().clamp_min(1.0)).max())
        res["python_fusion_metrics_ms"] = median_ms(lambda: fusion_metrics(fus, ir, vis), args.iters, args.warmup)
        if not args.no_forward:
            model = MyModel(**CONFIGS[cfg].model_kwargs(nn.ELU(inplace=True))).eval()
            load_recipe_into(model, seed=0, flavor="default")
            model.to(dev)
            model.precision = "fast"
            res["model_forward_eager_ms"] = median_ms(lambda: model(ir, vis), args.iters, args.warmup)
            res["forward_config"] = cfg
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
