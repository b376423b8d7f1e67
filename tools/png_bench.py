"""Time per call of the PNG encoder (Test loop), all in one process on one GPU: (a) swf_png_encode on buffers allocated once,
(b) its six launches alone (each on the workspace a whole call left), (c) encode_png as Python calls it (allocations included) and
fuse_images + encode_png, (d) the copy of the files to the host, and (e) Pillow's save(..., "PNG") of the same arrays on the same
machine, on one host thread and with 16 images in flight.  The images are the fused outputs of synthetic_pair through the win8 model:
RGB, and gray (the green channel of the fused image of gray sources).  Median of --iters timed calls after --warmup, HIP events for the
device side, the host clock for Pillow; the spread (min, max) is stated beside every median.  One JSON line per shape and mode; --out
also writes the list to a file.

    python tools/png_bench.py [--iters 200] [--warmup 10] [--out profiles/r21_png.json]
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

os.environ["SWF_DEBUG_SWITCHES"] = "1"   # before the library loads: the per-launch timings use its stage switch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from torch import nn

import __graft_entry__ as entry

SHAPES = [(16, 256, 256), (1, 512, 640)]   # (B, H, W)
HOST_THREADS = 16
LAUNCHES = [("filter", 1), ("tokens_and_codes", 2), ("framing", 4), ("emit", 8), ("crc_segments", 16), ("crc", 32)]


def spread(times):
    return {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}


def device_ms(fn, iters, warmup):
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
    return spread(times)


def host_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return spread(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=10, help="timed calls of the Pillow side, which takes tens of ms per image")
    ap.add_argument("--out", default=None, help="also write the list of results to this JSON file")
    args = ap.parse_args()
    entry.build()
    from PIL import Image
    from swin_unet_image_fusion_amd import CONFIGS, MyModel, _lib as L, encode_png, load_recipe_into, synthetic_pair
    from swin_unet_image_fusion_amd.imaging import fuse_images
    from swin_unet_image_fusion_amd.modules import _stream
    if not torch.cuda.is_available():
        raise SystemExit("png_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    lib = L.lib()
    torch.set_grad_enabled(False)
    model = MyModel(**CONFIGS["win8"].model_kwargs(nn.ELU(inplace=True))).eval()
    load_recipe_into(model, seed=0, flavor="default")
    model.to(dev)
    model.precision = "fast"
    results = []
    for b, h, w in SHAPES:
        u8 = lambda a: torch.from_numpy(np.clip(np.rint(a * 255.0), 0, 255).astype(np.uint8))
        ir = u8(synthetic_pair(b, h, w, seed_ir=1, seed_vis=2)[0])[:, 0].contiguous().to(dev)
        vis = torch.stack([u8(synthetic_pair(b, h, w, seed_ir=3 + k, seed_vis=2)[0])[:, 0] for k in range(3)], dim=-1).contiguous().to(dev)
        vis_gray = vis[..., :1].repeat(1, 1, 1, 3).contiguous()
        for mode in ("gray", "rgb"):
            src = vis if mode == "rgb" else vis_gray
            fuse = (lambda: fuse_images(model, ir, src, as_uint8=True)) if mode == "rgb" else \
                (lambda: fuse_images(model, ir, src, as_uint8=True)[..., 1].contiguous())
            pixels = fuse()
            desc = L.PngDesc(3 if mode == "rgb" else 1, 0, 0)
            cap, need = lib.swf_png_capacity_bytes(C.byref(desc), h, w), lib.swf_png_workspace_bytes(C.byref(desc), b, h, w)
            out = torch.empty((b, cap), dtype=torch.uint8, device=dev)
            lengths = torch.empty((b,), dtype=torch.int32, device=dev)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            stream = _stream(dev)

            def call():
                L.check(lib.swf_png_encode(C.byref(desc), pixels.data_ptr(), out.data_ptr(), cap, lengths.data_ptr(), b, h, w, ws.data_ptr(), need, stream))

            def timed(stages=None):
                os.environ.pop("SWF_PNG_STAGES", None)
                if stages is not None:
                    os.environ["SWF_PNG_STAGES"] = str(stages)
                ms = device_ms(call, args.iters, args.warmup)
                os.environ.pop("SWF_PNG_STAGES", None)
                return ms

            res = {"what": f"PNG, {mode}, 16 rows per block, B={b} {h}x{w} (win8 fused outputs of synthetic_pair), ms per batch: median, min and "
                           f"max of {args.iters} after {args.warmup}",
                   "hip_call_ms": timed()}
            res["launch_ms"] = {name: timed(bit) for name, bit in LAUNCHES}
            call()
            files = encode_png(pixels).to_bytes()
            torch.cuda.synchronize()
            assert [bytes(out[k, :n].cpu().numpy()) for k, n in enumerate(lengths.cpu().tolist())] == files
            host_px = pixels.cpu().numpy()
            for k, f in enumerate(files):   # Pillow decodes every file to its source
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), host_px[k])
            res["bytes_per_image"] = round(sum(len(f) for f in files) / b, 1)
            res["capacity_bytes_per_image"], res["workspace_mb"] = cap, round(need / 2 ** 20, 2)
            res["python_encode_png_ms"] = device_ms(lambda: encode_png(pixels), args.iters, args.warmup)
            res["fuse_images_ms"] = device_ms(fuse, args.iters, args.warmup)
            res["fuse_images_plus_encode_png_ms"] = device_ms(lambda: encode_png(fuse()), args.iters, args.warmup)
            res["encode_png_and_copy_to_host_ms"] = host_ms(lambda: encode_png(pixels).to_bytes(), args.host_iters, 2)

            def pillow(img):
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, "PNG")
                return buf.tell()

            images = [host_px[k] for k in range(b)]
            res["pillow_bytes_per_image"] = round(sum(pillow(i) for i in images) / b, 1)
            res["pillow_1_thread_ms"] = host_ms(lambda: [pillow(i) for i in images], args.host_iters, 1)
            many = images if b >= HOST_THREADS else images * (HOST_THREADS // b)     # every thread an image
            with ThreadPoolExecutor(HOST_THREADS) as pool:
                t = host_ms(lambda: list(pool.map(pillow, many)), args.host_iters, 1)
            res[f"pillow_{HOST_THREADS}_in_flight_ms"] = {k: round(v * b / len(many), 4) for k, v in t.items()}
            res[f"pillow_{HOST_THREADS}_in_flight_images"] = len(many)
            res["speedup_vs_pillow_1_thread"] = round(res["pillow_1_thread_ms"]["median"] / res["hip_call_ms"]["median"], 2)
            res[f"speedup_vs_pillow_{HOST_THREADS}_in_flight"] = round(res[f"pillow_{HOST_THREADS}_in_flight_ms"]["median"] / res["hip_call_ms"]["median"], 2)
            print(json.dumps(res), flush=True)
            results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "python tools/png_bench.py (one MI355X, one process, HIP events; Pillow on the host clock of the same machine, "
                               f"{HOST_THREADS} threads used, {args.host_iters} timed calls)", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
