"""Time per call of the perception group (Evaluation), all in one process on one GPU: (a) swf_fusion_perception, (b) its
kernel groups alone (tables, min / max and planes; the four DFT products; the Q_CB, Q_CV and level kernels; the finish), (c) the same
five values composed from torch fp64 ops (torch.fft.fft2 / ifft2, F.conv2d with the separable 31-tap kernels, F.conv2d for Sobel,
F.avg_pool2d for the block sums, torch.bincount for the histograms), what a user without the kernels runs, and (d) the model forward of
the same batch.  Median of --iters timed calls after --warmup, HIP events.  One JSON line per shape; --out also writes the list to a
file.  The kernel groups timed alone start from a full call's workspace.

    python tools/perception_bench.py [--iters 20] [--warmup 5] [--kind noise|smooth] [--no-forward] [--out profiles/r14_perception.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

os.environ["SWF_DEBUG_SWITCHES"] = "1"   # before the library loads: the per-group timings use its stage switch
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


def _rho(h, w, dev):
    s = lambda n: torch.where(torch.arange(n, device=dev) < (n + 1) // 2, torch.arange(n, device=dev), torch.arange(n, device=dev) - n).double()
    return torch.sqrt(s(h)[:, None] ** 2 + s(w)[None, :] ** 2)


def torch_perception(fus, ir, vis, c):
    """The five values of include/swinfuse.h from torch ops, batched, fp64 after the fp32 quantiser.  -> (B, 5)"""
    q = lambda x: torch.nan_to_num(x * 255.0 + 0.5, nan=0.0).clamp(0, 255).to(torch.int64).double()
    Fd, Ad, Bd = q(fus), q(ir), q(vis)   # (B, 1, H, W)
    nb, _, h, w = Fd.shape
    dev = fus.device

    def stretch(X):
        lo, hi = X.amin((2, 3), keepdim=True), X.amax((2, 3), keepdim=True)
        flat = hi == lo
        return torch.where(flat, torch.zeros_like(X), torch.round((255.0 * (X - lo)) / torch.where(flat, torch.ones_like(hi), hi - lo)))

    spec = lambda X, G: torch.fft.ifft2(torch.fft.fft2(X) * G).real
    sA, sB, sF = stretch(Ad), stretch(Bd), stretch(Fd)
    rho = _rho(h, w, dev)
    r = rho / 15.0
    S = torch.exp(-(r / c["f0"]) ** 2) - c["a"] * torch.exp(-(r / c["f1"]) ** 2)
    x = torch.arange(-15, 16, dtype=torch.float64, device=dev)
    taps = [torch.exp(-(x * x) / (2.0 * sd * sd)) / math.sqrt(2.0 * math.pi * sd * sd) for sd in (2.0, 4.0)]

    def same(X, g):   # zero padding, separable, planes as channels
        ch = X.shape[1]
        X = F.conv2d(X, g.view(1, 1, 1, -1).expand(ch, 1, 1, -1), padding=(0, 15), groups=ch)
        return F.conv2d(X, g.view(1, 1, -1, 1).expand(ch, 1, -1, 1), padding=(15, 0), groups=ch)

    Xf = spec(torch.cat([sA, sB, sF], dim=1), S)
    b1, b2 = same(Xf, taps[0]), same(Xf, taps[1])
    zero = b2 == 0
    Cc = torch.where(zero, torch.zeros_like(b1), (b1 / torch.where(zero, torch.ones_like(b2), b2) - 1.0).abs())
    Cp = Cc ** c["p"] / (Cc ** c["q"] + c["Z"])
    cA, cB, cF = Cp[:, 0], Cp[:, 1], Cp[:, 2]

    def ratio(cX):
        both = (cX == 0) & (cF == 0)
        return torch.where(both, torch.ones_like(cX), torch.minimum(cX, cF) / torch.where(both, torch.ones_like(cX), torch.maximum(cX, cF)))

    den = cA * cA + cB * cB
    lam = torch.where(den == 0, torch.full_like(den, 0.5), cA * cA / torch.where(den == 0, torch.ones_like(den), den))
    qcb = (lam * ratio(cA) + (1 - lam) * ratio(cB)).mean((1, 2))

    kx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float64, device=dev)
    ky = torch.tensor([[1., 2., 1.], [0., 0., 0.], [-1., -2., -1.]], dtype=torch.float64, device=dev)
    k2 = torch.stack([kx, ky]).unsqueeze(1)
    mag = lambda X: (F.conv2d(X, k2) ** 2).sum(1, keepdim=True).sqrt()
    rv = rho / 4.0
    theta = 2.6 * (0.0192 + 0.144 * rv) * torch.exp(-((0.144 * rv) ** 1.1))
    ph, pw = -h % 16, -w % 16
    blocks = lambda X: F.avg_pool2d(F.pad(X, (0, pw, 0, ph)), 16, divisor_override=1)
    num = den = 0.0
    for sX in (sA, sB):
        lam_b = blocks(mag(F.pad(sX, (1, 1, 1, 1))) ** c["alpha"])
        D = blocks(spec(sX - sF, theta) ** 2) / 256.0
        num, den = num + (lam_b * D).sum((1, 2, 3)), den + lam_b.sum((1, 2, 3))
    qcv = torch.where(den == 0, torch.zeros_like(den), num / torch.where(den == 0, torch.ones_like(den), den))

    off = torch.arange(nb, device=dev).view(nb, 1) * 256
    hist = lambda X: torch.bincount((X.view(nb, -1).long() + off).view(-1), minlength=nb * 256).view(nb, 256).double() / (h * w)
    pF, ce = hist(Fd), 0.0
    for X in (Ad, Bd):
        pX = hist(X)
        m = (pX > 0) & (pF > 0)
        one = torch.ones_like(pX)
        ce = ce + torch.where(m, pX * torch.log2(torch.where(m, pX, one) / torch.where(m, pF, one)), torch.zeros_like(pX)).sum(1)
    ei = mag(F.pad(Fd, (1, 1, 1, 1), mode="replicate")).mean((1, 2, 3))
    rm = lambda X: ((X - Fd) ** 2).mean((1, 2, 3)).sqrt() / 255.0
    return torch.stack([qcb, qcv, ce / 2.0, ei, (rm(Ad) + rm(Bd)) / 2.0], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kind", default="noise", choices=["noise", "smooth"], help="smooth: 7x7 box blur")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=None, help="also write the list of results to this JSON file")
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import CONFIGS, PERCEPTION_DEFAULTS, MyModel, _lib as L, fusion_perception, load_recipe_into, synthetic_pair
    from swin_unet_image_fusion_amd.modules import _stream
    if not torch.cuda.is_available():
        raise SystemExit("perception_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    lib, desc = L.lib(), L.PerceptionDesc(*PERCEPTION_DEFAULTS.values())
    torch.set_grad_enabled(False)
    results = []
    for b, size, cfg in SHAPES:
        h = w = size
        ir, vis = (torch.from_numpy(a).to(dev) for a in synthetic_pair(b, h, w, seed_ir=1, seed_vis=2))
        noise = torch.from_numpy(synthetic_pair(b, h, w, seed_ir=3)[0]).to(dev)
        if args.kind == "smooth":
            blur = lambda x: F.avg_pool2d(F.pad(x, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
            ir, vis, noise = blur(ir), blur(vis), blur(noise)
        fus = (0.5 * torch.maximum(ir, vis) + 0.5 * noise).clamp(0, 1)
        need = lib.swf_fusion_perception_workspace_bytes(b, h, w)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((b, L.PERCEPTION_COUNT), dtype=torch.float64, device=dev)
        stream = _stream(dev)

        def call():
            L.check(lib.swf_fusion_perception(C.byref(desc), fus.data_ptr(), ir.data_ptr(), vis.data_ptr(), out.data_ptr(), b, h, w,
                                              ws.data_ptr(), need, stream))

        def timed(stages=None):
            os.environ.pop("SWF_PERCEPTION_STAGES", None)
            if stages is not None:
                os.environ["SWF_PERCEPTION_STAGES"] = str(stages)
            ms = median_ms(call, args.iters, args.warmup)
            os.environ.pop("SWF_PERCEPTION_STAGES", None)
            return ms

        wh = w // 2 + 1
        flop = 5 * b * 2.0 * (h * w * 2 * wh + 2 * (2 * h) * (2 * h) * wh + h * 2 * wh * w)   # the four products over 5 B planes
        res = {"what": f"Q_CB / Q_CV / CE / EI / RMSE B={b} {h}x{w} ({args.kind} images), ms per call, median of {args.iters} after {args.warmup}",
               "hip_call_ms": timed(),
               "tables_minmax_planes_kernels_ms": timed(stages=1),
               "dft_product_kernels_ms": timed(stages=2),
               "qcb_qcv_levels_kernels_ms": timed(stages=4),
               "finish_kernel_ms": timed(stages=8),
               "dft_products_gflop": round(flop / 1e9, 2),
               "workspace_mb": round(need / 2 ** 20, 2)}
        res["dft_products_fp64_tflops"] = round(flop / (res["dft_product_kernels_ms"] * 1e-3) / 1e12, 2)
        call()
        fused = out.clone()
        res["torch_composition_ms"] = median_ms(lambda: torch_perception(fus, ir, vis, PERCEPTION_DEFAULTS), args.iters, args.warmup)
        res["speedup_vs_torch_composition"] = round(res["torch_composition_ms"] / res["hip_call_ms"], 2)
        res["max_distance_to_torch_composition"] = float(((torch_perception(fus, ir, vis, PERCEPTION_DEFAULTS) - fused).abs()
                                                          / fused.abs().clamp_min(1.0)).max())
        res["python_fusion_perception_ms"] = median_ms(lambda: fusion_perception(fus, ir, vis), args.iters, args.warmup)
        if not args.no_forward:
            model = MyModel(**CONFIGS[cfg].model_kwargs(nn.ELU(inplace=True))).eval()
            load_recipe_into(model, seed=0, flavor="default")
            model.to(dev)
            model.precision = "fast"
            res["model_forward_eager_ms"] = median_ms(lambda: model(ir, vis), args.iters, args.warmup)
            res["share_of_forward"] = round(res["hip_call_ms"] / res["model_forward_eager_ms"], 3)
            res["forward_config"] = cfg
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "python tools/perception_bench.py (one MI355X, one process, HIP events)", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
