"""Time per call of the structural-similarity group (Evaluation), all in one process on one GPU: (a) swf_fusion_structure,
(b) its kernel groups alone (the Gaussian moment kernels, the 2x2 means, the three box-moment launches, the finish), (c) the same nine
values composed from torch fp64 ops (F.conv2d with the same separable window, F.avg_pool2d for the pyramid and the box sums, F.conv2d
for Sobel), what a user without the kernels runs, and (d) the model forward of the same batch.  Median of --iters timed calls after
--warmup, HIP events.  One JSON line per shape; --out also writes the list to a file.  The kernel groups timed alone start from a full
call's workspace.

    python tools/structure_bench.py [--iters 20] [--warmup 5] [--kind noise|smooth] [--no-forward] [--out profiles/r13_structure.json]
"""
import argparse
import ctypes as C
import json
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
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


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


def _window(dev):
    i = torch.arange(11, dtype=torch.float64, device=dev)
    g = torch.exp(-((i - 5) ** 2) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def torch_structure(fus, ir, vis, c, g):
    """The nine values of include/swinfuse.h from torch ops, batched, fp64 after the fp32 quantiser (the box sums are sums of integers
    below 2^53, so fp64 holds them exactly).  -> (B, 9)"""
    q = lambda x: torch.nan_to_num(x * 255.0 + 0.5, nan=0.0).clamp(0, 255).to(torch.int64).double()
    Fd, Ad, Bd = q(fus), q(ir), q(vis)   # (B, 1, H, W)
    nb, dev = Fd.shape[0], fus.device
    C1, C2 = (255.0 * c["K1"]) ** 2, (255.0 * c["K2"]) ** 2
    zeros = torch.zeros(nb, dtype=torch.float64, device=dev)

    def filt(x):   # 'valid', separable, any number of planes as channels
        ch = x.shape[1]
        x = F.conv2d(x, g.view(1, 1, 1, -1).expand(ch, 1, 1, -1), groups=ch)
        return F.conv2d(x, g.view(1, 1, -1, 1).expand(ch, 1, -1, 1), groups=ch)

    def gauss(x):   # x: (B, 3, h, w) = A, B, F -> mean l cs and mean cs of (A, F) and (B, F), each (B, 2)
        a, b, f = x[:, 0:1], x[:, 1:2], x[:, 2:3]
        m = filt(torch.cat([x, a * a, b * b, f * f, a * f, b * f], dim=1))
        lcs, cs = [], []
        for k in range(2):
            mx, my = m[:, k], m[:, 2]
            vx, vy, cxy = m[:, 3 + k] - mx * mx, m[:, 5] - my * my, m[:, 6 + k] - mx * my
            l = (2 * mx * my + C1) / (mx * mx + my * my + C1)
            s = (2 * cxy + C2) / (vx + vy + C2)
            lcs.append((l * s).mean((1, 2)))
            cs.append(s.mean((1, 2)))
        return torch.stack(lcs, 1), torch.stack(cs, 1)

    x = torch.cat([Ad, Bd, Fd], dim=1)
    small = min(x.shape[2], x.shape[3])
    ssim = gauss(x)[0] if small >= 11 else torch.zeros(nb, 2, dtype=torch.float64, device=dev)
    if small >= 176:
        ms = torch.ones(nb, 2, dtype=torch.float64, device=dev)
        for j, wj in enumerate(MS_WEIGHTS):
            if j > 0:
                x = F.avg_pool2d(x, 2)
            lcs, cs = gauss(x)
            ms = ms * (lcs if j == 4 else cs).clamp_min(0) ** wj
    else:
        ms = torch.zeros(nb, 2, dtype=torch.float64, device=dev)

    def box(Fi, Ai, Bi, w):   # per window: s(A,F), s(B,F), s(A,B), V_A, V_B, C_AF, C_BF
        n = float(w * w)
        planes = torch.cat([Ai, Bi, Fi, Ai * Ai, Bi * Bi, Fi * Fi, Ai * Fi, Bi * Fi, Ai * Bi], dim=1)
        S = F.avg_pool2d(planes, w, stride=1, divisor_override=1)
        SA, SB, SF = S[:, 0], S[:, 1], S[:, 2]
        VA, VB, VF = n * S[:, 3] - SA * SA, n * S[:, 4] - SB * SB, n * S[:, 5] - SF * SF
        CAF, CBF, CAB = n * S[:, 6] - SA * SF, n * S[:, 7] - SB * SF, n * S[:, 8] - SA * SB

        def s(SX, SY, VX, VY, CXY):
            mx, my = SX / n, SY / n
            return ((2 * mx * my + C1) * (2 * CXY / (n * n) + C2)) / ((mx * mx + my * my + C1) * (VX / (n * n) + VY / (n * n) + C2))

        return s(SA, SF, VA, VF, CAF), s(SB, SF, VB, VF, CBF), s(SA, SB, VA, VB, CAB), VA, VB, CAF, CBF

    def ratio(num, den):
        z = den == 0
        return torch.where(z, torch.full_like(num, 0.5), num / torch.where(z, torch.ones_like(den), den))

    def piella(Fi, Ai, Bi):
        sAF, sBF, _, VA, VB, CAF, CBF = box(Fi, Ai, Bi, 8)
        lam = ratio(VA, VA + VB)
        t = lam * sAF + (1 - lam) * sBF
        m = torch.maximum(VA, VB)
        qs, sm = t.mean((1, 2)), m.sum((1, 2))
        qw = torch.where(sm == 0, qs, (m * t).sum((1, 2)) / torch.where(sm == 0, torch.ones_like(sm), sm))
        sim = ratio(CAF, CAF + CBF).clamp(0, 1)
        return qs, qw, (sim * sAF + (1 - sim) * sBF).mean((1, 2))

    kx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float64, device=dev)
    ky = torch.tensor([[1., 2., 1.], [0., 0., 0.], [-1., -2., -1.]], dtype=torch.float64, device=dev)
    k2 = torch.stack([kx, ky]).unsqueeze(1)
    edge = lambda X: F.conv2d(X, k2, padding=1).abs().sum(1, keepdim=True)   # zero border

    if small >= 8:
        qs, qw, qc = piella(Fd, Ad, Bd)
        qe = qw * piella(edge(Fd), edge(Ad), edge(Bd))[1].clamp_min(0) ** c["alpha"]
    else:
        qs = qw = qc = qe = zeros
    if small >= 7:
        sAF, sBF, sAB, VA, VB, _, _ = box(Fd, Ad, Bd, 7)
        lam = ratio(VA, VA + VB)
        qy = torch.where(sAB >= c["Ty"], lam * sAF + (1 - lam) * sBF, torch.maximum(sAF, sBF)).mean((1, 2))
    else:
        qy = zeros
    return torch.stack([ssim[:, 0] + ssim[:, 1], ssim[:, 0], ssim[:, 1], ms[:, 0] + ms[:, 1], qs, qw, qe, qc, qy], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kind", default="noise", choices=["noise", "smooth"], help="smooth: 7x7 box blur")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=None, help="also write the list of results to this JSON file")
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import CONFIGS, STRUCTURE_DEFAULTS, MyModel, _lib as L, fusion_structure, load_recipe_into, synthetic_pair
    from swin_unet_image_fusion_amd.modules import _stream
    if not torch.cuda.is_available():
        raise SystemExit("structure_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    lib, desc = L.lib(), L.StructureDesc(*STRUCTURE_DEFAULTS.values())
    g = _window(dev)
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
        need = lib.swf_fusion_structure_workspace_bytes(b, h, w)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((b, L.STRUCTURE_COUNT), dtype=torch.float64, device=dev)
        stream = _stream(dev)

        def call():
            L.check(lib.swf_fusion_structure(C.byref(desc), fus.data_ptr(), ir.data_ptr(), vis.data_ptr(), out.data_ptr(), b, h, w,
                                             ws.data_ptr(), need, stream))

        def timed(stages=None):
            os.environ.pop("SWF_STRUCTURE_STAGES", None)
            if stages is not None:
                os.environ["SWF_STRUCTURE_STAGES"] = str(stages)
            ms = median_ms(call, args.iters, args.warmup)
            os.environ.pop("SWF_STRUCTURE_STAGES", None)
            return ms

        res = {"what": f"SSIM / MS-SSIM / Piella / Cvejic / Yang B={b} {h}x{w} ({args.kind} images), ms per call, median of {args.iters} "
                       f"after {args.warmup}",
               "hip_call_ms": timed(),
               "gaussian_moment_kernels_ms": timed(stages=1),
               "mean2x2_kernels_ms": timed(stages=2),
               "box_moment_kernels_ms": timed(stages=4),
               "finish_kernel_ms": timed(stages=8),
               "workspace_mb": round(need / 2 ** 20, 2)}
        call()
        fused = out.clone()
        res["torch_composition_ms"] = median_ms(lambda: torch_structure(fus, ir, vis, STRUCTURE_DEFAULTS, g), args.iters, args.warmup)
        res["speedup_vs_torch_composition"] = round(res["torch_composition_ms"] / res["hip_call_ms"], 1)
        res["beats_torch_composition_by_more_than_5_percent"] = bool(res["torch_composition_ms"] > 1.05 * res["hip_call_ms"])
        res["max_distance_to_torch_composition"] = float(((torch_structure(fus, ir, vis, STRUCTURE_DEFAULTS, g) - fused).abs()
                                                          / fused.abs().clamp_min(1.0)).max())
        res["python_fusion_structure_ms"] = median_ms(lambda: fusion_structure(fus, ir, vis), args.iters, args.warmup)
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
            json.dump({"tool": "python tools/structure_bench.py (one MI355X, one process, HIP events)", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
