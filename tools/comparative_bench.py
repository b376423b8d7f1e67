"""Time per call of the comparative-study group (Evaluation), all in one process on one GPU: (a) swf_fusion_comparative,
(b) its kernel groups alone (tables, levels, histograms with their measures and the Q_SF / Q_M pass; the transforms; the medians and
phase congruency; the moments and the finish), (c) the same six values composed from torch fp64 ops (torch.fft.fft2 / ifft2,
torch.bincount for the joint histograms, torch.linalg.eigvalsh, torch.median), what a user without the kernels runs, and (d) the model
forward of the same batch.  Median of --iters timed calls after --warmup, HIP events.  One JSON line per shape; --out also writes the
list to a file.  The kernel groups timed alone start from a full call's workspace.

    python tools/comparative_bench.py [--iters 20] [--warmup 5] [--kind noise|smooth] [--no-forward] [--out profiles/r16_comparative.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

os.environ["SWF_DEBUG_SWITCHES"] = "1"   # before the library loads: the per-group timings use its stage switch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torch import nn

import __graft_entry__ as entry
from tools.perception_bench import SHAPES, median_ms


def torch_comparative(fus, ir, vis, c):
    """The six values of include/swinfuse.h from torch ops, batched, fp64 after the fp32 quantiser.  -> (B, 6)"""
    q = lambda x: torch.nan_to_num(x * 255.0 + 0.5, nan=0.0).clamp(0, 255).to(torch.int64)
    Fi, Ai, Bi = (q(x)[:, 0] for x in (fus, ir, vis))   # (B, H, W) int64
    nb, h, w = Fi.shape
    n, dev = h * w, fus.device
    one = lambda x: torch.ones_like(x)

    # ---- information measures
    off = torch.arange(nb, device=dev).view(nb, 1)
    marg = lambda X: torch.bincount((X.view(nb, -1) + off * 256).view(-1), minlength=nb * 256).view(nb, 256).double() / n
    joint = lambda X, Y: torch.bincount((X.view(nb, -1) * 256 + Y.view(nb, -1) + off * 65536).view(-1),
                                        minlength=nb * 65536).view(nb, 256, 256).double() / n
    plogp = lambda p: torch.where(p > 0, p * torch.log2(torch.where(p > 0, p, one(p))), torch.zeros_like(p))
    ent = lambda p: -plogp(p).flatten(1).sum(1)
    pA, pB, pF = marg(Ai), marg(Bi), marg(Fi)
    pairs = {"AF": (joint(Ai, Fi), pA, pF), "BF": (joint(Bi, Fi), pB, pF), "AB": (joint(Ai, Bi), pA, pB)}

    def mi(key):
        pxy, px, py = pairs[key]
        pp, nz = px[:, :, None] * py[:, None, :], pxy > 0
        return torch.where(nz, pxy * torch.log2(torch.where(nz, pxy, one(pxy)) / torch.where(nz, pp, one(pp))), torch.zeros_like(pxy)).sum((1, 2))

    def ratio(num, den):
        return torch.where(den == 0, torch.zeros_like(den), num / torch.where(den == 0, one(den), den))

    qmi = 2.0 * (ratio(mi("AF"), ent(pA) + ent(pF)) + ratio(mi("BF"), ent(pB) + ent(pF)))
    qq = c["q"]

    def tsallis(key):
        pxy, px, py = pairs[key]
        pp, nz = px[:, :, None] * py[:, None, :], pxy > 0
        s = torch.where(nz, torch.where(nz, pxy, one(pxy)) ** qq / torch.where(nz, pp, one(pp)) ** (qq - 1.0), torch.zeros_like(pxy)).sum((1, 2))
        return (1.0 - s) / (1.0 - qq)

    hq = lambda p: (1.0 - torch.where(p > 0, p, torch.zeros_like(p)).pow(qq).sum(1)) / (qq - 1.0)
    qte = ratio(tsallis("AF") + tsallis("BF"), hq(pA) + hq(pB) - tsallis("AB"))
    ncc = lambda key: ent(pairs[key][1]) / 8.0 + ent(pairs[key][2]) / 8.0 - ent(pairs[key][0]) / 8.0
    R = torch.eye(3, dtype=torch.float64, device=dev).repeat(nb, 1, 1)
    R[:, 0, 1] = R[:, 1, 0] = ncc("AB")
    R[:, 0, 2] = R[:, 2, 0] = ncc("AF")
    R[:, 1, 2] = R[:, 2, 1] = ncc("BF")
    lam = torch.linalg.eigvalsh(R) / 3.0
    pos = lam > 0
    qncie = 1.0 + torch.where(pos, lam * torch.log2(torch.where(pos, lam, one(lam))) / 8.0, torch.zeros_like(lam)).sum(1)

    # ---- Qsf
    Ad, Bd, Fd = Ai.double(), Bi.double(), Fi.double()
    diffs = lambda X: (X[:, :, 1:] - X[:, :, :-1], X[:, 1:, :] - X[:, :-1, :], X[:, 1:, 1:] - X[:, :-1, :-1], X[:, 1:, :-1] - X[:, :-1, 1:])
    wd = 1.0 / math.sqrt(2.0)
    sf = lambda ds: torch.sqrt(sum(wk * (d * d).sum((1, 2)) for wk, d in zip((1.0, 1.0, wd, wd), ds)) / n)
    sf_f = sf(diffs(Fd))
    sf_r = sf([torch.maximum(da.abs(), db.abs()) for da, db in zip(diffs(Ad), diffs(Bd))])
    qsf = ratio(sf_f - sf_r, sf_r)

    # ---- Qm
    def haar(X):
        hh, ww = X.shape[1] // 2 * 2, X.shape[2] // 2 * 2
        a, b, cc, d = X[:, 0:hh:2, 0:ww:2], X[:, 0:hh:2, 1:ww:2], X[:, 1:hh:2, 0:ww:2], X[:, 1:hh:2, 1:ww:2]
        return (a + b + cc + d) / 2.0, (a + b - cc - d) / 2.0, (a - b + cc - d) / 2.0, (a - b - cc + d) / 2.0

    x = {"A": Ad / 255.0, "B": Bd / 255.0, "F": Fd / 255.0}
    qm = torch.ones(nb, dtype=torch.float64, device=dev)
    for alpha in (c["alpha1"], c["alpha2"]):
        t = {k: haar(v) for k, v in x.items()}
        if t["F"][0].numel() > 0:
            num = den = 0.0
            for k in ("A", "B"):
                ep = sum(torch.exp(-(t[k][j] - t["F"][j]).abs()) for j in (1, 2, 3)) / 3.0
                wgt = t[k][1] ** 2 + t[k][2] ** 2 + t[k][3] ** 2
                num, den = num + (ep * wgt).sum((1, 2)), den + wgt.sum((1, 2))
            qm = qm * ratio(num, den) ** alpha
        x = {k: v[0] for k, v in t.items()}

    # ---- Qp
    s = lambda m: torch.where(torch.arange(m, device=dev) < (m + 1) // 2, torch.arange(m, device=dev), torch.arange(m, device=dev) - m).double()
    fy, fx = (s(h) / h)[:, None].expand(h, w), (s(w) / w)[None, :].expand(h, w)
    rho = torch.sqrt(fx * fx + fy * fy)
    rho[0, 0] = 1.0
    theta = torch.atan2(-fy, fx)
    lp = 1.0 / (1.0 + (rho / 0.45) ** 30)
    sint, cost = torch.sin(theta), torch.cos(theta)
    G = []
    for sc in range(4):
        fs = 1.0 / (c["min_wavelength"] * c["mult"] ** sc)
        g = torch.exp(-torch.log(rho / fs) ** 2 / (2.0 * math.log(c["sigma_onf"]) ** 2)) * lp
        g[0, 0] = 0.0
        G.append(g)
    G = torch.stack(G)                                                   # (4, H, W)
    spectrum = torch.fft.fft2(torch.stack([Ad, Bd, Fd], dim=1))          # (B, 3, H, W)
    eps = c["eps"]
    p = sxx = syy = sxy = 0.0
    for o in range(6):
        a = o * math.pi / 6.0
        ds, dc = sint * math.cos(a) - cost * math.sin(a), cost * math.cos(a) + sint * math.sin(a)
        spread = (torch.cos(torch.minimum(torch.atan2(ds, dc).abs() * 3.0, torch.full_like(ds, math.pi))) + 1.0) / 2.0
        EO = torch.fft.ifft2(spectrum[:, :, None] * (G * spread)[None, None])   # (B, 3, 4, H, W)
        E, O, An = EO.real, EO.imag, EO.abs()
        sumE, sumO, sumAn, maxAn = E.sum(2), O.sum(2), An.sum(2), An.amax(2)
        XE = torch.sqrt(sumE ** 2 + sumO ** 2) + eps
        mE, mO = (sumE / XE)[:, :, None], (sumO / XE)[:, :, None]
        energy = (E * mE + O * mO - (E * mO - O * mE).abs()).sum(2)
        flat = An[:, :, 0].flatten(2)
        med = (torch.median(flat, dim=2).values - torch.median(-flat, dim=2).values) / 2.0   # lower and upper middle values
        tau = med / math.sqrt(math.log(4.0))
        tt = tau * (1.0 - (1.0 / c["mult"]) ** 4) / (1.0 - 1.0 / c["mult"])
        T = tt * math.sqrt(math.pi / 2.0) + c["k"] * tt * math.sqrt((4.0 - math.pi) / 2.0)
        energy = (energy - T[:, :, None, None]).clamp_min(0.0)
        width = (sumAn / (maxAn + eps) - 1.0) / 3.0
        pc = 1.0 / (1.0 + torch.exp((c["cutoff"] - width) * c["g"])) * energy / (sumAn + eps)
        p, sxx, syy = p + pc, sxx + (pc * math.cos(a)) ** 2, syy + (pc * math.sin(a)) ** 2
        sxy = sxy + pc * pc * math.cos(a) * math.sin(a)
    cx2, cy2, cxy = sxx / 3.0, syy / 3.0, sxy / 3.0
    den = torch.sqrt(cxy ** 2 + (cx2 - cy2) ** 2) + eps
    maps = (p, (cy2 + cx2 + den) / 2.0, (cy2 + cx2 - den) / 2.0)          # each (B, 3, H, W): A, B, F

    def corr(U, V):
        du, dv = U - U.mean((1, 2), keepdim=True), V - V.mean((1, 2), keepdim=True)
        return ((du * dv).mean((1, 2)) + c["C"]) / ((du * du).mean((1, 2)).sqrt() * (dv * dv).mean((1, 2)).sqrt() + c["C"])

    qp = torch.ones(nb, dtype=torch.float64, device=dev)
    for m, e in zip(maps, (c["ep"], c["eM"], c["em"])):
        xa, xb, xf = m[:, 0], m[:, 1], m[:, 2]
        best = torch.stack([corr(xa, xf), corr(xb, xf), corr(torch.maximum(xa, xb), xf)]).amax(0).clamp_min(0.0)
        qp = qp * best ** e
    return torch.stack([qmi, qte, qncie, qm, qsf, qp], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kind", default="noise", choices=["noise", "smooth"], help="smooth: 7x7 box blur")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=None, help="also write the list of results to this JSON file")
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import CONFIGS, COMPARATIVE_DEFAULTS, MyModel, _lib as L, fusion_comparative, load_recipe_into, synthetic_pair
    from swin_unet_image_fusion_amd.modules import _stream
    if not torch.cuda.is_available():
        raise SystemExit("comparative_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    lib, desc = L.lib(), L.ComparativeDesc(*COMPARATIVE_DEFAULTS.values())
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
        need = lib.swf_fusion_comparative_workspace_bytes(b, h, w)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((b, L.COMPARATIVE_COUNT), dtype=torch.float64, device=dev)
        stream = _stream(dev)

        def call():
            L.check(lib.swf_fusion_comparative(C.byref(desc), fus.data_ptr(), ir.data_ptr(), vis.data_ptr(), out.data_ptr(), b, h, w,
                                               ws.data_ptr(), need, stream))

        def timed(stages=None):
            os.environ.pop("SWF_COMPARATIVE_STAGES", None)
            if stages is not None:
                os.environ["SWF_COMPARATIVE_STAGES"] = str(stages)
            ms = median_ms(call, args.iters, args.warmup)
            os.environ.pop("SWF_COMPARATIVE_STAGES", None)
            return ms

        wh = w // 2 + 1
        fwd = 3 * b * 2.0 * (h * w * 2 * wh + (2 * h) * (2 * h) * wh)                    # steps 1 and 2 over 3 B planes
        inv = 6 * 24 * b * 2.0 * ((2 * h) * (2 * h) * wh + h * 2 * wh * w)               # steps 3 and 4 over 24 B planes, six times
        res = {"what": f"Q_MI / Q_TE / Q_NCIE / Q_M / Q_SF / Q_P B={b} {h}x{w} ({args.kind} images), ms per call, median of {args.iters} "
                       f"after {args.warmup}",
               "hip_call_ms": timed(),
               "tables_levels_histograms_sfm_kernels_ms": timed(stages=1),
               "dft_product_kernels_ms": timed(stages=2),
               "median_and_phase_congruency_kernels_ms": timed(stages=4),
               "moment_and_finish_kernels_ms": timed(stages=8),
               "dft_products_gflop": round((fwd + inv) / 1e9, 2),
               "workspace_mb": round(need / 2 ** 20, 2)}
        res["dft_products_fp64_tflops"] = round((fwd + inv) / (res["dft_product_kernels_ms"] * 1e-3) / 1e12, 2)
        call()
        fused = out.clone()
        res["torch_composition_ms"] = median_ms(lambda: torch_comparative(fus, ir, vis, COMPARATIVE_DEFAULTS), args.iters, args.warmup)
        res["speedup_vs_torch_composition"] = round(res["torch_composition_ms"] / res["hip_call_ms"], 2)
        res["max_distance_to_torch_composition"] = float(((torch_comparative(fus, ir, vis, COMPARATIVE_DEFAULTS) - fused).abs()
                                                          / fused.abs().clamp_min(1.0)).max())
        res["python_fusion_comparative_ms"] = median_ms(lambda: fusion_comparative(fus, ir, vis), args.iters, args.warmup)
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
            json.dump({"tool": "python tools/comparative_bench.py (one MI355X, one process, HIP events)", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
