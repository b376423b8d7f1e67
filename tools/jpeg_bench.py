"""Time per call of the JPEG encoder (Test loop), all in one process on one GPU: (a) swf_jpeg_encode on buffers allocated
once, (b) its three passes alone (coefficients, entropy coding, packing; each on the workspace a whole call left), (c) encode_jpeg
as Python calls it (allocations included) and fuse_images + encode_jpeg, (d) the copy of the files to the host, and (e) Pillow's
encoder on the same RGB at the same quality and subsampling, on one host thread and on 16 (the reference's save_image is one thread
per image).  The images are the fused outputs of synthetic_pair through the win8 model.  Median of --iters timed calls after --warmup,
HIP events for the device side, the host clock for Pillow; the spread (min, max) is stated beside every median.  One JSON line per
shape; --out also writes the list to a file.

    python tools/jpeg_bench.py [--iters 30] [--warmup 5] [--quality 75] [--out profiles/r17_jpeg.json]
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

os.environ["SWF_DEBUG_SWITCHES"] = "1"   # before the library loads: the per-pass timings use its stage switch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from torch import nn

import __graft_entry__ as entry

SHAPES = [(16, 256, 256), (1, 512, 640)]   # (B, H, W)
HOST_THREADS = 16


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--out", default=None, help="also write the list of results to this JSON file")
    args = ap.parse_args()
    entry.build()
    from PIL import Image
    from swin_unet_image_fusion_amd import CONFIGS, MyModel, _lib as L, encode_jpeg, load_recipe_into, synthetic_pair
    from swin_unet_image_fusion_amd.imaging import _jpeg_header, fuse_images
    from swin_unet_image_fusion_amd.modules import _stream
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
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
        rgb = fuse_images(model, ir, vis, as_uint8=True)
        desc = L.JpegDesc(3, L.JPEG_420, args.quality)
        cap, need = lib.swf_jpeg_capacity_bytes(C.byref(desc), h, w), lib.swf_jpeg_workspace_bytes(C.byref(desc), b, h, w)
        out = torch.empty((b, cap), dtype=torch.uint8, device=dev)
        lengths = torch.empty((b,), dtype=torch.int32, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        header, stream = _jpeg_header(desc, dev, h, w), _stream(dev)

        def call():
            L.check(lib.swf_jpeg_encode(C.byref(desc), rgb.data_ptr(), header.data_ptr(), out.data_ptr(), cap, lengths.data_ptr(), b, h, w,
                                        ws.data_ptr(), need, stream))

        def timed(stages=None):
            os.environ.pop("SWF_JPEG_STAGES", None)
            if stages is not None:
                os.environ["SWF_JPEG_STAGES"] = str(stages)
            ms = device_ms(call, args.iters, args.warmup)
            os.environ.pop("SWF_JPEG_STAGES", None)
            return ms

        res = {"what": f"baseline JPEG, 4:2:0, quality {args.quality}, B={b} {h}x{w} RGB (win8 fused outputs of synthetic_pair), ms per batch: "
                       f"median, min and max of {args.iters} after {args.warmup}",
               "hip_call_ms": timed(), "coefficient_pass_ms": timed(1), "entropy_pass_ms": timed(2), "pack_pass_ms": timed(4)}
        call()
        files = encode_jpeg(rgb, quality=args.quality).to_bytes()
        torch.cuda.synchronize()
        assert [bytes(out[k, :n].cpu().numpy()) for k, n in enumerate(lengths.cpu().tolist())] == files
        host_rgb = rgb.cpu().numpy()
        for k, f in enumerate(files):   # Pillow decodes every file close to its source
            dec = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"), dtype=np.float64)
            assert dec.shape == host_rgb[k].shape
        res["bytes_per_image"] = round(sum(len(f) for f in files) / b, 1)
        res["capacity_bytes_per_image"], res["workspace_mb"] = cap, round(need / 2 ** 20, 2)
        res["python_encode_jpeg_ms"] = device_ms(lambda: encode_jpeg(rgb, quality=args.quality), args.iters, args.warmup)
        res["fuse_images_ms"] = device_ms(lambda: fuse_images(model, ir, vis, as_uint8=True), args.iters, args.warmup)
        res["fuse_images_plus_encode_jpeg_ms"] = device_ms(lambda: encode_jpeg(fuse_images(model, ir, vis, as_uint8=True), quality=args.quality),
                                                           args.iters, args.warmup)
        res["encode_jpeg_and_copy_to_host_ms"] = host_ms(lambda: encode_jpeg(rgb, quality=args.quality).to_bytes(), args.iters, args.warmup)
        res["uncompressed_rgb_copy_to_host_ms"] = host_ms(lambda: rgb.cpu(), args.iters, args.warmup)

        def pillow(img):
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "JPEG", quality=args.quality)
            return buf.tell()

        images = [host_rgb[k] for k in range(b)]
        res["pillow_bytes_per_image"] = round(sum(pillow(i) for i in images) / b, 1)
        res["pillow_1_thread_ms"] = host_ms(lambda: [pillow(i) for i in images], args.iters, args.warmup)
        many = images if b >= HOST_THREADS else images * (HOST_THREADS // b)     # every thread an image
        with ThreadPoolExecutor(HOST_THREADS) as pool:
            t = host_ms(lambda: list(pool.map(pillow, many)), args.iters, args.warmup)
        res[f"pillow_{HOST_THREADS}_threads_ms"] = {k: round(v * b / len(many), 4) for k, v in t.items()}
        res[f"pillow_{HOST_THREADS}_threads_images_in_flight"] = len(many)
        res["speedup_vs_pillow_1_thread"] = round(res["pillow_1_thread_ms"]["median"] / res["hip_call_ms"]["median"], 2)
        res[f"speedup_vs_pillow_{HOST_THREADS}_threads"] = round(res[f"pillow_{HOST_THREADS}_threads_ms"]["median"] / res["hip_call_ms"]["median"], 2)
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "python tools/jpeg_bench.py (one MI355X, one process, HIP events; Pillow on the host clock of the same machine, "
                               f"{os.cpu_count()} CPUs visible, {HOST_THREADS} threads used)", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
