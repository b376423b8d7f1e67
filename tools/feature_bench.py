"""Time per call of feature mutual information (Evaluation), all in one process on one GPU: (a) swf_fusion_feature, (b) its
launches alone (tables, levels and Haar mosaics; the two DCT products; the window kernel of each feature; the finish), (c) the same four
values composed from torch fp64 ops (F.unfold for the windows, cosine matrices through matmul for the DCT), what a user without the
kernels runs, and (d) the model forward of the same batch.  Median, minimum and maximum of --iters timed calls after --warmup, HIP
events.  One JSON line per shape; --out also writes the list to a file.  The launches timed alone start from a full call's workspace.

    python tools/feature_bench.py [--iters 200] [--warmup 10] [--window 3|5] [--no-forward] [--out profiles/r27_feature.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

os.environ["SWF_DEBUG_SWITCHES"] = "1"   # before the library loads: the per-launch timings use its stage switches
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torch import nn

import __graft_entry__ as entry
from tools.perception_bench import SHAPES


def times_ms(fn, iters, warmup):
    """-> {median, min, max} in ms over `iters` calls, each between two HIP events."""
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
    return {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}


def dct_matrix(n, dev):
    k, i = torch.arange(n, device=dev)[:, None], torch.arange(n, device=dev)[None, :]
    m = ((2 * i + 1) * k) % (4 * n)
    s = torch.ones(n, 1, dtype=torch.float64, device=dev)
    s[0, 0] = 1.0 / math.sqrt(2.0)
    return s * math.sqrt(2.0 / n) * torch.cos(math.pi * (m.double() / (2 * n)))


def torch_pair(x, f):
    """x, f: (N, l) window samples -> I(X, F) per window, the steps of include/swinfuse.h."""
    l = x.shape[1]
    one = lambda t: torch.ones_like(t)
    zero = lambda t: torch.zeros_like(t)

    def pdf(v):
        mn, mx = v.amin(1, keepdim=True), v.amax(1, keepdim=True)
        flat = mx == mn
        vn = torch.where(flat, one(v), (v - mn) / torch.where(flat, one(mx), mx - mn))
        return vn / vn.sum(1, keepdim=True)

    def ent(t):
        pos = t > 0
        return -torch.where(pos, t * torch.log2(torch.where(pos, t, one(t))), zero(t)).flatten(1).sum(1)

    ratio = lambda num, den: torch.where(den == 0, zero(den), num / torch.where(den == 0, one(den), den))
    p, q = pdf(x), pdf(f)
    P, Q = p.cumsum(1), q.cumsum(1)
    pc, qc = p - 1.0 / l, q - 1.0 / l
    c = ratio((pc * qc).sum(1), torch.sqrt((pc * pc).sum(1) * (qc * qc).sum(1)))
    k = torch.arange(1, l + 1, device=x.device, dtype=torch.float64)
    sigma = lambda t: torch.sqrt(((k * k * t).sum(1) - (k * t).sum(1) ** 2).clamp_min(0.0))
    Pi, Qj = P[:, :, None], Q[:, None, :]
    G = torch.where((c >= 0)[:, None, None], torch.minimum(Pi, Qj), (Pi + Qj - 1.0).clamp_min(0.0))
    PQ = Pi * Qj
    rho = ratio((G - PQ).sum((1, 2)), sigma(p) * sigma(q))
    phi = torch.where(rho == 0, zero(rho), ratio(c, rho).clamp(0.0, 1.0))
    J = F.pad(phi[:, None, None] * G + (1.0 - phi)[:, None, None] * PQ, (1, 0, 1, 0))
    j = (J[:, 1:, 1:] - J[:, :-1, 1:]) - (J[:, 1:, :-1] - J[:, :-1, :-1])
    hs = ent(p) + ent(q)
    info = ratio(2.0 * (hs - ent(j)), hs)
    return torch.where((x == f).all(1), one(info), info)


def torch_feature(fus, ir, vis, c):
    """The four values of include/swinfuse.h from torch ops, batched, fp64 after the fp32 quantiser.  -> (B, 4)"""
    win, step = int(c["window"]), c["dct_step"]
    q = lambda x: torch.nan_to_num(x * 255.0 + 0.5, nan=0.0).clamp(0, 255).to(torch.int64).double()
    X = torch.stack([q(t)[:, 0] for t in (ir, vis, fus)], dim=1)          # (B, 3, H, W): A, B, F
    nb, _, h, w = X.shape

    def edge(T):
        p = F.pad(T, (1, 1, 1, 1), mode="replicate")
        a, b, cc, d, e = p[..., :-2, :-2], p[..., :-2, 1:-1], p[..., :-2, 2:], p[..., 1:-1, :-2], p[..., 1:-1, 2:]
        f, g, hh = p[..., 2:, :-2], p[..., 2:, 1:-1], p[..., 2:, 2:]
        return ((cc - a) + 2 * (e - d) + (hh - f)).abs() + ((a + 2 * b + cc) - (f + 2 * g + hh)).abs()

    def haar(T):
        hh, ww = h // 2 * 2, w // 2 * 2
        a, b, cc, d = T[..., 0:hh:2, 0:ww:2], T[..., 0:hh:2, 1:ww:2], T[..., 1:hh:2, 0:ww:2], T[..., 1:hh:2, 1:ww:2]
        top = torch.cat([(a + b + cc + d) / 2.0, (a + b - cc - d) / 2.0], dim=-1)
        return torch.cat([top, torch.cat([(a - b + cc - d) / 2.0, (a - b - cc + d) / 2.0], dim=-1)], dim=-2)

    def dct(T):
        return torch.round(dct_matrix(h, T.device) @ T @ dct_matrix(w, T.device).T / step) * step

    out = []
    for plane in (X, dct(X), haar(X), edge(X)):                            # the order of the names
        ph, pw = plane.shape[-2:]
        if ph < win or pw < win:
            out.append(torch.zeros(nb, dtype=torch.float64, device=X.device))
            continue
        # the transposed plane unfolds column-major: k = (column offset) window + (row offset)
        u = F.unfold(plane.transpose(-1, -2).reshape(nb * 3, 1, pw, ph), win)   # (3 B, l, N)
        u = u.view(nb, 3, win * win, -1).permute(1, 0, 3, 2)                       # (3, B, N, l)
        n = u.shape[2]
        a, b, f = (u[k].reshape(nb * n, win * win) for k in range(3))
        out.append(((torch_pair(a, f) + torch_pair(b, f)) / 2.0).view(nb, n).sum(1) / n)
    return torch.stack(out, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=20, help="timed calls of the torch composition")
    ap.add_argument("--window", type=int, default=3, choices=[3, 5])
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=None, help="also write the list of results to this JSON file")
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import CONFIGS, FEATURE_DEFAULTS, FEATURE_NAMES, MyModel, _lib as L, fusion_feature, load_recipe_into, synthetic_pair
    from swin_unet_image_fusion_amd.modules import _stream
    if not torch.cuda.is_available():
        raise SystemExit("feature_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    constants = {**FEATURE_DEFAULTS, "window": float(args.window)}
    lib, desc = L.lib(), L.FeatureDesc(*constants.values())
    torch.set_grad_enabled(False)
    results = []
    for b, size, cfg in SHAPES:
        h = w = size
        ir, vis = (torch.from_numpy(a).to(dev) for a in synthetic_pair(b, h, w, seed_ir=1, seed_vis=2))
        noise = torch.from_numpy(synthetic_pair(b, h, w, seed_ir=3)[0]).to(dev)
        fus = (0.5 * torch.maximum(ir, vis) + 0.5 * noise).clamp(0, 1)
        need = lib.swf_fusion_feature_workspace_bytes(b, h, w)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((b, L.FEATURE_COUNT), dtype=torch.float64, device=dev)
        stream = _stream(dev)

        def call():
            L.check(lib.swf_fusion_feature(C.byref(desc), fus.data_ptr(), ir.data_ptr(), vis.data_ptr(), out.data_ptr(), b, h, w, ws.data_ptr(),
                                           need, stream))

        def timed(stages=None, windows=None):
            for name, value in (("SWF_FEATURE_STAGES", stages), ("SWF_FEATURE_WINDOWS", windows)):
                os.environ.pop(name, None)
                if value is not None:
                    os.environ[name] = str(value)
            t = times_ms(call, args.iters, args.warmup)
            os.environ.pop("SWF_FEATURE_STAGES", None)
            os.environ.pop("SWF_FEATURE_WINDOWS", None)
            return t

        flop = 3 * b * 2.0 * (h * w * w + h * h * w)
        res = {"what": f"FMI_pixel / FMI_dct / FMI_w / FMI_edge B={b} {h}x{w} window {args.window} (noise images), ms per call, median, min and "
                       f"max of {args.iters} after {args.warmup}",
               "hip_call_ms": timed(),
               "tables_levels_haar_kernels_ms": timed(stages=1),
               "dct_product_kernels_ms": timed(stages=2)}
        for k, name in enumerate(FEATURE_NAMES):
            res[f"window_kernel_{name}_ms"] = timed(stages=4, windows=1 << k)
        res["finish_kernel_ms"] = timed(stages=8)
        res["dct_products_gflop"] = round(flop / 1e9, 3)
        res["dct_products_fp64_tflops"] = round(flop / (res["dct_product_kernels_ms"]["median"] * 1e-3) / 1e12, 2)
        res["workspace_mb"] = round(need / 2 ** 20, 2)
        call()
        fused = out.clone()
        res["torch_composition_ms"] = times_ms(lambda: torch_feature(fus, ir, vis, constants), args.torch_iters, 3)
        res["torch_composition_iters"] = args.torch_iters
        res["speedup_vs_torch_composition"] = round(res["torch_composition_ms"]["median"] / res["hip_call_ms"]["median"], 2)
        res["max_distance_to_torch_composition"] = float(((torch_feature(fus, ir, vis, constants) - fused).abs() / fused.abs().clamp_min(1.0)).max())
        res["python_fusion_feature_ms"] = times_ms(lambda: fusion_feature(fus, ir, vis, **constants), args.iters, args.warmup)
        if not args.no_forward:
            model = MyModel(**CONFIGS[cfg].model_kwargs(nn.ELU(inplace=True))).eval()
            load_recipe_into(model, seed=0, flavor="default")
            model.to(dev)
            model.precision = "fast"
            res["model_forward_eager_ms"] = times_ms(lambda: model(ir, vis), args.iters, args.warmup)
            res["share_of_forward"] = round(res["hip_call_ms"]["median"] / res["model_forward_eager_ms"]["median"], 3)
            res["forward_config"] = cfg
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "python tools/feature_bench.py (one MI355X, one process, HIP events)", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
