"""Time per call of the PNG decoder (Data), all in one process on one GPU: (a) swf_png_decode on buffers allocated and tables
uploaded once, (b) its six launches alone (prefix sums, gather, inflate, Adler-32, unfilter, finish; each on the workspace a whole call
left), (c) the host parse of the same files, (d) Pillow decoding the same bytes on one host thread and on 16, and (e)
ResidentPairs.from_folder with decode="pil" against decode="device" on a folder of PNG pairs, wall time.  The files are 640x512, gray and
RGB, of test_fusion-like content (synthetic_pair noise at 1/8 resolution enlarged bicubically plus +-4 of noise), in Pillow's default
encoding and in this project's own (imaging.encode_png); `--distinct` different images, repeated to the count.  Median of --iters timed
calls after --warmup, HIP events for the device side, the host clock for Pillow and the folder; the spread (min, max) is stated beside
every median.  One JSON line per workload; --out also writes the list to a file.

    python tools/png_decode_bench.py [--iters 20] [--warmup 3] [--counts 1 64 256 1024] [--out profiles/r23_png_decode.json]
    python tools/png_decode_bench.py --rehearse      # no GPU: builds small workloads, parses them and times Pillow only
"""
import argparse
import ctypes as C
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

os.environ["SWF_DEBUG_SWITCHES"] = "1"   # before the library loads: the per-launch timings use its stage switch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import __graft_entry__ as entry

H, W = 512, 640
HOST_THREADS = 16
STAGES = (("place_launch_ms", 1), ("gather_launch_ms", 2), ("inflate_launch_ms", 4), ("adler_launch_ms", 8), ("unfilter_launch_ms", 16),
          ("finish_launch_ms", 32))


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


def make_images(distinct):
    """`distinct` RGB (H, W, 3) uint8 images."""
    from PIL import Image
    from swin_unet_image_fusion_amd import synthetic_pair
    out = []
    for k in range(distinct):
        planes = [synthetic_pair(1, H // 8, W // 8, seed_ir=10 + 3 * k + c)[0][0, 0] for c in range(3)]
        small = Image.fromarray(np.clip(np.rint(np.stack(planes, axis=-1) * 255.0), 0, 255).astype(np.uint8))
        img = np.asarray(small.resize((W, H), Image.BICUBIC), dtype=np.float64)
        img = img + np.random.default_rng(k).integers(-4, 5, img.shape)
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


def encode(img, gray, own, dev):
    """Pillow's default encoding, or (own, needs the GPU) imaging.encode_png's."""
    img = img[..., 1].copy() if gray else img
    if own:
        from swin_unet_image_fusion_amd import encode_png
        return encode_png(torch.from_numpy(img)[None].to(dev)).to_bytes()[0]
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "PNG")
    return buf.getvalue()


def pillow_decode(data, mode):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert(mode))


def pillow_times(files, mode, iters, warmup):
    one = host_ms(lambda: [pillow_decode(f, mode) for f in files], iters, warmup)
    many = files if len(files) >= HOST_THREADS else files * (HOST_THREADS // len(files))   # every thread a file
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        t = host_ms(lambda: list(pool.map(lambda f: pillow_decode(f, mode), many)), iters, warmup)
    return one, {k: round(v * len(files) / len(many), 4) for k, v in t.items()}, len(many)


class DeviceCall:
    """swf_png_decode over `files` with everything allocated and uploaded once."""

    def __init__(self, files, layout, dev):
        from swin_unet_image_fusion_amd import _lib as L, imaging
        from swin_unet_image_fusion_amd.modules import _stream
        self.L, self.lib, n = L, L.lib(), len(files)
        t = time.perf_counter()
        parsed = [imaging.parse_png(f, i) for i, f in enumerate(files)]
        self.parse_ms = (time.perf_counter() - t) * 1e3
        code, px = imaging._LAYOUTS[layout]
        self.descs = (L.PngFile * n)()
        pos = end = 0
        self.ranges = []
        for i, ((d, _), f) in enumerate(zip(parsed, files)):
            start = -(-end // 16) * 16
            end = start + d.H * d.W * px
            d.data_off, d.out_off = pos, start
            self.descs[i] = d
            self.ranges.append((start, end))
            pos += len(f)
        tables = np.concatenate([np.frombuffer(self.descs, dtype=np.uint8)] + [r.reshape(-1).view(np.uint8) for _, r in parsed])
        self.tables = torch.from_numpy(tables.copy()).to(dev)
        self.data = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).to(dev)
        self.need = self.lib.swf_png_decode_workspace_bytes(self.descs, n)
        self.out = torch.empty(end, dtype=torch.uint8, device=dev)
        self.status = torch.empty(n, dtype=torch.int32, device=dev)
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=dev)
        self.n, self.code, self.stream = n, code, _stream(dev)
        self.idat_chunks = sum(len(r) for _, r in parsed)

    def __call__(self):
        self.L.check(self.lib.swf_png_decode(self.data.data_ptr(), self.data.numel(), self.descs, self.tables.data_ptr(), self.n,
                                             self.tables.data_ptr() + self.n * C.sizeof(self.L.PngFile), self.out.data_ptr(), self.out.numel(),
                                             self.status.data_ptr(), self.code, self.ws.data_ptr(), self.need, self.stream))

    def timed(self, iters, warmup, stages=None):
        os.environ.pop("SWF_PNG_DECODE_STAGES", None)
        if stages is not None:
            os.environ["SWF_PNG_DECODE_STAGES"] = str(stages)
        ms = device_ms(self, iters, warmup)
        os.environ.pop("SWF_PNG_DECODE_STAGES", None)
        return ms


def workload(images, n, gray, own, args, dev):
    files = [encode(images[k % len(images)], gray, own, dev) for k in range(min(n, len(images)))]
    files = [files[k % len(files)] for k in range(n)]
    layout, mode = ("gray", "L") if gray else ("bgr", "RGB")
    res = {"what": f"{n} files of {W}x{H}, {'gray' if gray else 'RGB'}, {'encode_png' if own else 'Pillow default'} encoding, decoded as {layout}; "
                   f"ms per call: median, min and max of {args.iters} after {args.warmup}",
           "files": n, "gray": gray, "encoder": "encode_png" if own else "pillow", "bytes_per_file": round(sum(len(f) for f in files) / n, 1)}
    if dev is not None:
        call = DeviceCall(files, layout, dev)
        iters = args.iters if n <= 64 else max(5, args.iters // 2)
        res.update(idat_chunks=call.idat_chunks, workspace_mb=round(call.need / 2 ** 20, 2), host_parse_ms=round(call.parse_ms, 3),
                   device_iters=iters)
        res["hip_call_ms"] = call.timed(iters, args.warmup)
        for name, bit in STAGES:
            res[name] = call.timed(iters, min(args.warmup, 1), bit)
        call()
        torch.cuda.synchronize()
        assert call.status.cpu().tolist() == [0] * n
        for k in sorted({0, n // 2, n - 1}):   # the timed call decodes what Pillow decodes
            want = pillow_decode(files[k], mode)
            want = want[..., ::-1] if not gray else want
            assert np.array_equal(call.out[call.ranges[k][0]:call.ranges[k][1]].cpu().numpy().reshape(want.shape), want)
        res["files_per_second"] = round(n / res["hip_call_ms"]["median"] * 1e3, 1)
        res["slowest_launch"] = max(STAGES, key=lambda s: res[s[0]]["median"])[0]
        del call
    piters = args.iters if n <= 16 else 3                  # Pillow: whole seconds per pass at the larger counts
    one, many, in_flight = pillow_times(files, mode, piters, 1)
    res["pillow_1_thread_ms"], res[f"pillow_{HOST_THREADS}_threads_ms"], res[f"pillow_{HOST_THREADS}_threads_files_in_flight"] = one, many, in_flight
    if "hip_call_ms" in res:
        res["speedup_vs_pillow_1_thread"] = round(one["median"] / res["hip_call_ms"]["median"], 3)
        res[f"speedup_vs_pillow_{HOST_THREADS}_threads"] = round(many["median"] / res["hip_call_ms"]["median"], 3)
    print(json.dumps(res), flush=True)
    return res


def folder(images, pairs, args, dev):
    """from_folder on `pairs` gray ir and RGB vis files in Pillow's encoding: wall time of each decode path, the arenas compared."""
    from swin_unet_image_fusion_amd import ResidentPairs
    root = tempfile.mkdtemp(prefix="png_decode_bench_")
    try:
        for sub in ("ir", "vis"):
            os.makedirs(os.path.join(root, sub))
        ir = [encode(i, True, False, dev) for i in images]
        vis = [encode(i, False, False, dev) for i in images]
        for k in range(pairs):
            for sub, files in (("ir", ir), ("vis", vis)):
                with open(os.path.join(root, sub, f"{k:05d}.png"), "wb") as f:
                    f.write(files[k % len(files)])
        stores = {}

        def load(decode):
            stores[decode] = ResidentPairs.from_folder(root, device=dev, decode=decode)
            torch.cuda.synchronize()

        res = {"what": f"ResidentPairs.from_folder on {pairs} pairs of {W}x{H} PNG (ir gray, vis RGB, Pillow's default encoding), files in the "
                       "page cache, wall ms until the arenas are complete: reading, parsing, uploading and decoding included", "pairs": pairs}
        res["decode_pil_ms"] = host_ms(lambda: load("pil"), 2, 1)
        res["decode_device_ms"] = host_ms(lambda: load("device"), 2, 1)
        assert torch.equal(stores["pil"].ir_arena, stores["device"].ir_arena) and torch.equal(stores["pil"].vis_arena, stores["device"].vis_arena)
        res["speedup"] = round(res["decode_pil_ms"]["median"] / res["decode_device_ms"]["median"], 3)
        print(json.dumps(res), flush=True)
        return res
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 64, 256, 1024])
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--rehearse", action="store_true", help="no GPU: small workloads, the host parse and Pillow only")
    ap.add_argument("--out", default=None, help="also write the list of results to this JSON file")
    args = ap.parse_args()
    entry.build()
    dev = None
    if args.rehearse:
        args.counts, args.distinct, args.iters, args.warmup = [1, 4], 2, 2, 1
    elif not torch.cuda.is_available():
        raise SystemExit("png_decode_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    else:
        dev = torch.device("cuda:0")
    images = make_images(args.distinct)
    results = []
    for gray in (False, True):
        for own in ((False, True) if dev is not None else (False,)):
            for n in args.counts:
                results.append(workload(images, n, gray, own, args, dev))
    if dev is not None:
        results.append(folder(images, args.pairs, args, dev))
        cross = {}
        for key in ("pillow_1_thread_ms", f"pillow_{HOST_THREADS}_threads_ms"):
            wins = [r["files"] for r in results if not r.get("gray", True) and r.get("encoder") == "pillow" and r["hip_call_ms"]["median"] < r[key]["median"]]
            cross[key] = min(wins) if wins else None
        results.append({"what": "the smallest measured count of RGB files in Pillow's encoding at which one swf_png_decode call takes less time than "
                                "Pillow (null: at none of the counts measured); the counts between two measured ones were not measured",
                        "counts_measured": args.counts, "device_call_faster_from": cross})
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "python tools/png_decode_bench.py (one MI355X, one process, HIP events; Pillow on the host clock of the same machine, "
                               f"{os.cpu_count()} CPUs visible, {HOST_THREADS} threads used)", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
