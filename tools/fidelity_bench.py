"""Time per call of VIF / Nabf (Evaluation), all in one process on one GPU: (a) swf_fusion_fidelity, (b) its kernel groups
alone (the four moment kernels, the three decimating kernels, the Sobel kernel, the finish), (c) the same five values composed from
torch fp64 ops (F.conv2d with the same separable windows for VIF, F.conv2d for Sobel), what a user without the kernels runs, and
(d) the model forward of the same batch.  Median of --iters timed calls after --warmup, HIP events.  One JSON line per shape.  The
kernel groups timed alone start from a full call's workspace.

    python tools/fidelity_bench.py [--iters 20] [--warmup 5] [--kind noise|smooth] [--no-forward]
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
TAPS = (17, 9, 5, 3)


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


def _windows(dev):
    out = []
    for n in TAPS:
        i = torch.arange(n, dtype=torch.float64, device=dev)
        g = torch.exp(-((i - (n - 1) / 2) ** 2) / (2.0 * (n / 5.0) ** 2))
        out.append(g / g.sum())
    return out


def torch_fidelity(fus, ir, vis, c, wins):
    """The five values of include/swinfuse.h from torch ops, batched, fp64 after the fp32 quantiser.  -> (B, 5)"""
    q = lambda x: torch.nan_to_num(x * 255.0 + 0.5, nan=0.0).clamp(0, 255).to(torch.int64).double()
    Fd, Ad, Bd = q(fus), q(ir), q(vis)   # (B, 1, H, W)
    nb = Fd.shape[0]

    def filt(x, g):   # 'valid', separable, any number of planes as channels of one batch entry each
        ch = x.shape[1]
        x = F.conv2d(x, g.view(1, 1, 1, -1).expand(ch, 1, 1, -1), groups=ch)
        return F.conv2d(x, g.view(1, 1, -1, 1).expand(ch, 1, -1, 1), groups=ch)

    num = torch.zeros(nb, 2, dtype=torch.float64, device=fus.device)
    den = torch.zeros_like(num)
    x = torch.cat([Ad, Bd, Fd], dim=1)
    eps, sig = c["eps"], c["sigma_nsq"]
    for s, g in enumerate(wins):
        n = len(g)
        if x.shape[2] < n or x.shape[3] < n:
            break
        if s > 0:
            x = filt(x, g)[:, :, ::2, ::2]
            if x.shape[2] < n or x.shape[3] < n:
                break
        a, b, f = x[:, 0:1], x[:, 1:2], x[:, 2:3]
        m = filt(torch.cat([x, a * a, b * b, f * f, a * f, b * f], dim=1), g)
        mu2, d2 = m[:, 2], m[:, 5] - m[:, 2] * m[:, 2]
        for k in range(2):
            mu1 = m[:, k]
            s1, s2, s12 = (m[:, 3 + k] - mu1 * mu1).clamp_min(0), d2.clamp_min(0), m[:, 6 + k] - mu1 * mu2
            gg = s12 / (s1 + eps)
            sv = s2 - gg * s12
            z = s1 < eps
            gg, sv, s1 = torch.where(z, 0.0, gg), torch.where(z, s2, sv), torch.where(z, 0.0, s1)
            z = s2 < eps
            gg, sv = torch.where(z, 0.0, gg), torch.where(z, 0.0, sv)
            z = gg < 0
            sv, gg = torch.where(z, s2, sv), torch.where(z, 0.0, gg)
            sv = torch.where(sv <= eps, eps, sv)
            num[:, k] += torch.log10(1 + gg * gg * s1 / (sv + sig)).sum((1, 2))
            den[:, k] += torch.log10(1 + s1 / sig).sum((1, 2))
    vif = torch.where(den == 0, torch.zeros_like(den), num / den.clamp_min(1e-300))

    kv = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float64, device=fus.device)
    kh = torch.tensor([[-1., -2., -1.], [0., 0., 0.], [1., 2., 1.]], dtype=torch.float64, device=fus.device)
    k2 = torch.stack([kv, kh]).unsqueeze(1)

    def edge(X):
        s = F.conv2d(F.pad(X, (1, 1, 1, 1), mode="replicate"), k2)
        gv, gh = s[:, 0], s[:, 1]
        alpha = torch.where(gh == 0, torch.sign(gv) * (math.pi / 2), torch.atan(gv / torch.where(gh == 0, torch.ones_like(gh), gh)))
        n = gv * gv + gh * gh
        return n, n.sqrt() / 8.0, alpha

    nF, gF, aF = edge(Fd)
    loss, wsum, na = 0, 0, torch.ones_like(nF, dtype=torch.bool)
    for X in (Ad, Bd):
        nX, gX, aX = edge(X)
        G = torch.where((nX == 0) | (nF == 0), torch.zeros_like(gX),
                        torch.where(nX > nF, gF / gX.clamp_min(1e-300), gX / gF.clamp_min(1e-300)))
        Aa = ((aX - aF).abs() - math.pi / 2).abs() * (2 / math.pi)
        Q = (c["Nrg"] / (1 + torch.exp(-c["kg"] * (G - c["sg"]))) * (c["Nra"] / (1 + torch.exp(-c["ka"] * (Aa - c["sa"]))))).sqrt()
        w = torch.where(nX >= 64.0 * c["Td"] * c["Td"], gX * gX.sqrt(), torch.full_like(gX, c["wt_min"]))
        loss, wsum, na = loss + (1 - Q) * w, wsum + w, na & (nF > nX)
    W = wsum.sum((1, 2))
    nabf, labf = torch.where(na, loss, 0.0).sum((1, 2)) / W, torch.where(na, 0.0, loss).sum((1, 2)) / W
    return torch.stack([vif[:, 0] + vif[:, 1], vif[:, 0], vif[:, 1], nabf, labf], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kind", default="noise", choices=["noise", "smooth"], help="smooth: 7x7 box blur")
    ap.add_argument("--no-forward", action="store_true")
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import CONFIGS, FIDELITY_DEFAULTS, MyModel, _lib as L, fusion_fidelity, load_recipe_into, synthetic_pair
    from swin_unet_image_fusion_amd.modules import _stream
    if not torch.cuda.is_available():
        raise SystemExit("fidelity_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    lib, desc = L.lib(), L.FidelityDesc(*FIDELITY_DEFAULTS.values())
    wins = _windows(dev)
    torch.set_grad_enabled(False)
    for b, size, cfg in SHAPES:
        h = w = size
        ir, vis = (torch.from_numpy(a).to(dev) for a in synthetic_pair(b, h, w, seed_ir=1, seed_vis=2))
        noise = torch.from_numpy(synthetic_pair(b, h, w, seed_ir=3)[0]).to(dev)
        if args.kind == "smooth":
            blur = lambda x: F.avg_pool2d(F.pad(x, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
            ir, vis, noise = blur(ir), blur(vis), blur(noise)
        fus = (0.5 * torch.maximum(ir, vis) + 0.5 * noise).clamp(0, 1)
        need = lib.swf_fusion_fidelity_workspace_bytes(b, h, w)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((b, L.FIDELITY_COUNT), dtype=torch.float64, device=dev)
        stream = _stream(dev)

        def call():
            L.check(lib.swf_fusion_fidelity(C.byref(desc), fus.data_ptr(), ir.data_ptr(), vis.data_ptr(), out.data_ptr(), b, h, w,
                                            ws.data_ptr(), need, stream))

        def timed(stages=None):
            os.environ.pop("SWF_FIDELITY_STAGES", None)
            if stages is not None:
                os.environ["SWF_FIDELITY_STAGES"] = str(stages)
            ms = median_ms(call, args.iters, args.warmup)
            os.environ.pop("SWF_FIDELITY_STAGES", None)
            return ms

        res = {"what": f"VIF / Nabf B={b} {h}x{w} ({args.kind} images), ms per call, median of {args.iters} after {args.warmup}",
               "hip_call_ms": timed(),
               "vif_moment_kernels_ms": timed(stages=1),
               "vif_decimating_kernels_ms": timed(stages=2),
               "nabf_kernel_ms": timed(stages=4),
               "finish_kernel_ms": timed(stages=8),
               "workspace_mb": round(need / 2 ** 20, 2)}
        call()
        fused = out.clone()
        res["torch_composition_ms"] = median_ms(lambda: torch_fidelity(fus, ir, vis, FIDELITY_DEFAULTS, wins), args.iters, args.warmup)
        res["speedup_vs_torch_composition"] = round(res["torch_composition_ms"] / res["hip_call_ms"], 1)
        res["max_distance_to_torch_composition"] = float(((torch_fidelity(fus, ir, vis, FIDELITY_DEFAULTS, wins) - fused).abs()
                                                          / fused.abs().clamp_min(1.0)).max())
        res["python_fusion_fidelity_ms"] = median_ms(lambda: fusion_fidelity(fus, ir, vis), args.iters, args.warmup)
        if not args.no_forward:
            model = MyModel(**CONFIGS[cfg].model_kwargs(nn.ELU(inplace=True))).eval()
            load_recipe_into(model, seed=0, flavor="default")
            model.to(dev)
            model.precision = "fast"
            res["model_forward_eager_ms"] = median_ms(lambda: model(ir, vis), args.iters, args.warmup)
            res["share_of_forward"] = round(res["hip_call_ms"] / res["model_forward_eager_ms"], 3)
            res["forward_config"] = cfg
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
