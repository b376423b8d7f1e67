"""Time per call of the JPEG decoder (Data), all in one process on one GPU: (a) swf_jpeg_decode on buffers allocated and tables
uploaded once, (b) its four launches alone (prefix sums, entropy decode, IDCT, finish; each on the workspace a whole call left), (c) the
host parse of the same files, (d) Pillow decoding the same bytes on one host thread and on 16, and (e) ResidentPairs.from_folder with
decode="pil" against decode="device" on a folder of pairs, wall time.  The files are 640x480, quality 75, written by Pillow: colour
4:2:0 and gray, without restart markers and with one interval per MCU row; `--distinct` different images, repeated to the count.  Content
"smooth" is synthetic_pair noise at 1/8 resolution enlarged bicubically plus +-4 of noise (photograph-like statistics); "noise" is
synthetic_pair itself, the longest streams a file of this size can have.  Median of --iters timed calls after --warmup, HIP events for
the device side, the host clock for Pillow and the folder; the spread (min, max) is stated beside every median.  One JSON line per
workload; --out also writes the list to a file.  --entropy split (or both: the two paths in one process on the same files) times
swf_jpeg_decode_split at every --segment-bytes, its eight stages (SPLIT_STAGES says how the synchronise and DC launches are timed), and
reads the rounds it took from its diagnostics records.

    python tools/jpeg_decode_bench.py [--iters 20] [--warmup 3] [--counts 1 16 64 256 1024] [--out profiles/r18_jpeg_decode.json]
    python tools/jpeg_decode_bench.py --entropy both --segment-bytes 64 128 256 512 --counts 1 64 256 1024 --out profiles/r19_jpeg_split.json
    python tools/jpeg_decode_bench.py --rehearse      # no GPU: builds small workloads, parses them and times Pillow only
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

H, W, QUALITY = 480, 640, 75
HOST_THREADS = 16
STAGES = (("place_launch_ms", 1), ("entropy_launch_ms", 2), ("idct_launch_ms", 4), ("finish_launch_ms", 8))
# (name, stage bits timed, stage bits whose median is taken off).  A stage alone runs on the workspace a whole call left.  That is the
# stage's own work for all but two: the synchronise launch alone would find every segment already decoded from its true state and run
# one round that changes nothing, and the DC launch alone would sum predictors as if they were differences.  So synchronise is timed
# behind the speculation that resets the records, DC behind the write decode that stores the differences, and the median of the first
# launch alone is subtracted.
SPLIT_STAGES = (("place_and_zero_launches_ms", 1, 0), ("unstuff_launch_ms", 2, 0), ("speculate_launch_ms", 4, 0),
                ("synchronise_launch_ms", 4 | 8, 4), ("write_launch_ms", 16, 0), ("dc_launch_ms", 16 | 32, 16), ("idct_launch_ms", 64, 0),
                ("finish_launch_ms", 128, 0))


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


def make_images(distinct, content):
    """`distinct` RGB (H, W, 3) uint8 images."""
    from PIL import Image
    from swin_unet_image_fusion_amd import synthetic_pair
    out = []
    for k in range(distinct):
        if content == "noise":
            planes = [synthetic_pair(1, H, W, seed_ir=10 + 3 * k + c)[0][0, 0] for c in range(3)]
            img = np.stack(planes, axis=-1) * 255.0
        else:
            planes = [synthetic_pair(1, H // 8, W // 8, seed_ir=10 + 3 * k + c)[0][0, 0] for c in range(3)]
            small = Image.fromarray(np.clip(np.rint(np.stack(planes, axis=-1) * 255.0), 0, 255).astype(np.uint8))
            img = np.asarray(small.resize((W, H), Image.BICUBIC), dtype=np.float64)
            img = img + np.random.default_rng(k).integers(-4, 5, img.shape)
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


def encode(img, gray, rows):
    from PIL import Image
    buf = io.BytesIO()
    kw = {"restart_marker_rows": 1} if rows else {}
    Image.fromarray(img[..., 1].copy() if gray else img).save(buf, "JPEG", quality=QUALITY, **({} if gray else {"subsampling": 2}), **kw)
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
    """swf_jpeg_decode, or swf_jpeg_decode_split at `segment_bytes`, over `files` with everything allocated and uploaded once."""

    def __init__(self, files, layout, dev, segment_bytes=None):
        from swin_unet_image_fusion_amd import _lib as L, imaging
        from swin_unet_image_fusion_amd.modules import _stream
        self.L, self.lib, n = L, L.lib(), len(files)
        t = time.perf_counter()
        parsed = [imaging.parse_jpeg(f, i) for i, f in enumerate(files)]
        self.parse_ms = (time.perf_counter() - t) * 1e3
        code, px = imaging._LAYOUTS[layout]
        self.descs = (L.JpegFile * n)()
        pos = end = 0
        self.ranges = []
        for i, ((d, _), f) in enumerate(zip(parsed, files)):
            start = -(-end // 16) * 16
            end = start + d.H * d.W * px
            d.data_off, d.out_off = pos, start
            self.descs[i] = d
            self.ranges.append((start, end))
            pos += len(f)
        tables = np.concatenate([np.frombuffer(self.descs, dtype=np.uint8)] + [iv.reshape(-1).view(np.uint8) for _, iv in parsed])
        self.tables = torch.from_numpy(tables.copy()).to(dev)
        self.data = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).to(dev)
        self.base = self.need = self.lib.swf_jpeg_decode_workspace_bytes(self.descs, n)
        self.segment_bytes = segment_bytes
        self.iv_host = np.ascontiguousarray(np.concatenate([iv.reshape(-1) for _, iv in parsed]), dtype=np.uint32)
        if segment_bytes:
            self.need = self.lib.swf_jpeg_decode_split_workspace_bytes(self.descs, n, self.iv_host.ctypes.data, segment_bytes)
        self.out = torch.empty(end, dtype=torch.uint8, device=dev)
        self.status = torch.empty(n, dtype=torch.int32, device=dev)
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=dev)
        self.n, self.code, self.stream = n, code, _stream(dev)
        self.intervals = sum(d.intervals for d, _ in parsed)
        self.blocks = sum(d.blocks for d, _ in parsed)

    def __call__(self):
        if self.segment_bytes:
            return self.L.check(self.lib.swf_jpeg_decode_split(
                self.data.data_ptr(), self.data.numel(), self.descs, self.tables.data_ptr(), self.n,
                self.tables.data_ptr() + self.n * C.sizeof(self.L.JpegFile), self.iv_host.ctypes.data, self.segment_bytes, self.out.data_ptr(),
                self.out.numel(), self.status.data_ptr(), self.code, self.ws.data_ptr(), self.need, self.stream))
        self.L.check(self.lib.swf_jpeg_decode(self.data.data_ptr(), self.data.numel(), self.descs, self.tables.data_ptr(), self.n,
                                              self.tables.data_ptr() + self.n * C.sizeof(self.L.JpegFile), self.out.data_ptr(), self.out.numel(),
                                              self.status.data_ptr(), self.code, self.ws.data_ptr(), self.need, self.stream))

    def diag(self):
        """The split call's record per interval, summed up: segments, and the rounds and wrong speculations the intervals took."""
        d = self.ws[self.base:self.base + 16 * self.intervals].cpu().numpy().view(np.uint32).reshape(-1, 4).astype(np.int64)
        return {"segments": int(d[:, 0].sum()), "segments_per_interval_max": int(d[:, 0].max()), "rounds_median": float(np.median(d[:, 1])),
                "rounds_max": int(d[:, 1].max()), "wrong_speculations": int(d[:, 2].sum())}

    def timed(self, iters, warmup, stages=None):
        os.environ.pop("SWF_JPEG_DECODE_STAGES", None)
        if stages is not None:
            os.environ["SWF_JPEG_DECODE_STAGES"] = str(stages)
        ms = device_ms(self, iters, warmup)
        os.environ.pop("SWF_JPEG_DECODE_STAGES", None)
        return ms


def workload(images, n, gray, rows, content, args, dev):
    files = [encode(images[k % len(images)], gray, rows) for k in range(min(n, len(images)))]
    files = [files[k % len(files)] for k in range(n)]
    layout, mode = ("gray", "L") if gray else ("bgr", "RGB")
    res = {"what": f"{n} files of {W}x{H}, quality {QUALITY}, {'gray' if gray else 'colour 4:2:0'}, {content} content, "
                   f"{'one restart interval per MCU row' if rows else 'no restart markers'}, decoded as {layout}; ms per call: median, min and "
                   f"max of {args.iters} after {args.warmup}",
           "files": n, "gray": gray, "interval_per_mcu_row": rows, "content": content, "bytes_per_file": round(sum(len(f) for f in files) / n, 1)}
    iters = args.iters if n <= 16 else max(3, args.iters // 4)   # Pillow: whole seconds per pass at the larger counts
    def check(call):
        call()
        torch.cuda.synchronize()
        assert call.status.cpu().tolist() == [0] * n
        flat = call.out.cpu().numpy()
        for k in sorted({0, n // 2, n - 1}):   # the timed call decodes what Pillow decodes
            want = pillow_decode(files[k], mode)
            want = want[..., ::-1] if not gray else want
            assert np.array_equal(flat[call.ranges[k][0]:call.ranges[k][1]].reshape(want.shape), want)

    if dev is not None and args.entropy != "split":
        call = DeviceCall(files, layout, dev)
        res.update(intervals=call.intervals, blocks=call.blocks, workspace_mb=round(call.need / 2 ** 20, 2), host_parse_ms=round(call.parse_ms, 3))
        res["hip_call_ms"] = call.timed(args.iters, args.warmup)
        for name, bit in STAGES:
            res[name] = call.timed(args.iters, args.warmup, bit)
        check(call)
        res["files_per_second"] = round(n / res["hip_call_ms"]["median"] * 1e3, 1)
    if dev is not None and args.entropy != "interval":
        res["split"] = {}
        for seg in args.segment_bytes:
            call = DeviceCall(files, layout, dev, seg)
            r = {"workspace_mb": round(call.need / 2 ** 20, 2), "hip_call_ms": call.timed(args.iters, args.warmup)}
            alone = {}
            for name, bits, minus in SPLIT_STAGES:
                t = call.timed(args.iters, args.warmup, bits)
                if minus:   # timed behind the launch that prepares its input: that launch's median comes off
                    r[name] = {"median": round(t["median"] - alone[minus]["median"], 4), "with_stages": bits, "with_stages_ms": t,
                               "minus_stages": minus}
                else:
                    r[name] = alone[bits] = t
            r["stages_sum_ms"] = round(sum(r[name]["median"] for name, _, _ in SPLIT_STAGES), 4)
            check(call)
            r.update(call.diag())
            if "hip_call_ms" in res:
                r["speedup_vs_interval"] = round(res["hip_call_ms"]["median"] / r["hip_call_ms"]["median"], 3)
                r["faster_beyond_the_spread"] = r["hip_call_ms"]["max"] < res["hip_call_ms"]["min"]
            res["split"][str(seg)] = r
        res.setdefault("intervals", call.intervals)
    one, many, in_flight = pillow_times(files, mode, iters, min(args.warmup, 1))
    res["pillow_1_thread_ms"], res[f"pillow_{HOST_THREADS}_threads_ms"], res[f"pillow_{HOST_THREADS}_threads_files_in_flight"] = one, many, in_flight
    if dev is not None and "hip_call_ms" in res:
        res["speedup_vs_pillow_1_thread"] = round(one["median"] / res["hip_call_ms"]["median"], 3)
        res[f"speedup_vs_pillow_{HOST_THREADS}_threads"] = round(many["median"] / res["hip_call_ms"]["median"], 3)
    for r in res.get("split", {}).values():
        r["speedup_vs_pillow_1_thread"] = round(one["median"] / r["hip_call_ms"]["median"], 3)
        r[f"speedup_vs_pillow_{HOST_THREADS}_threads"] = round(many["median"] / r["hip_call_ms"]["median"], 3)
    print(json.dumps(res), flush=True)
    return res


def folder(images, pairs, args, dev):
    """from_folder on `pairs` gray ir and colour 4:2:0 vis files: wall time of each decode path, the arenas compared."""
    from swin_unet_image_fusion_amd import ResidentPairs
    root = tempfile.mkdtemp(prefix="jpeg_decode_bench_")
    try:
        for sub in ("ir", "vis"):
            os.makedirs(os.path.join(root, sub))
        ir = [encode(i, True, False) for i in images]
        vis = [encode(i, False, False) for i in images]
        for k in range(pairs):
            for sub, files in (("ir", ir), ("vis", vis)):
                with open(os.path.join(root, sub, f"{k:05d}.jpg"), "wb") as f:
                    f.write(files[k % len(files)])
        stores = {}

        def load(decode, entropy="interval"):
            stores[decode] = ResidentPairs.from_folder(root, device=dev, decode=decode, entropy=entropy)
            torch.cuda.synchronize()

        res = {"what": f"ResidentPairs.from_folder on {pairs} pairs of {W}x{H} (ir gray, vis colour 4:2:0, quality {QUALITY}, smooth content, no "
                       "restart markers), files in the page cache, wall ms until the arenas are complete: reading, parsing, uploading and "
                       "decoding included", "pairs": pairs}
        iters = max(2, args.iters // 8)
        res["decode_pil_ms"] = host_ms(lambda: load("pil"), iters, 1)
        res["decode_device_ms"] = host_ms(lambda: load("device"), iters, 1)
        if args.entropy != "interval":
            assert torch.equal(stores["pil"].ir_arena, stores["device"].ir_arena) and torch.equal(stores["pil"].vis_arena, stores["device"].vis_arena)
            res["decode_device_split_ms"] = host_ms(lambda: load("device", "split"), iters, 1)
            res["speedup_split"] = round(res["decode_pil_ms"]["median"] / res["decode_device_split_ms"]["median"], 3)
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
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 16, 64, 256, 1024])
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--entropy", choices=("interval", "split", "both"), default="interval", help="the entropy pass of the timed calls")
    ap.add_argument("--segment-bytes", type=int, nargs="+", default=[128], help="segment sizes of the split calls")
    ap.add_argument("--rehearse", action="store_true", help="no GPU: small workloads, the host parse and Pillow only")
    ap.add_argument("--out", default=None, help="also write the list of results to this JSON file")
    args = ap.parse_args()
    entry.build()
    dev = None
    if args.rehearse:
        args.counts, args.distinct, args.iters, args.warmup = [1, 4], 2, 2, 1
    elif not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    else:
        dev = torch.device("cuda:0")
    smooth = make_images(args.distinct, "smooth")
    results = []
    for n in args.counts:          # colour, no restart markers, every count: where the device call and Pillow cross
        results.append(workload(smooth, n, False, False, "smooth", args, dev))
    for n in [c for c in args.counts if c >= 256] or args.counts[-1:]:
        for gray, rows in ((True, False), (False, True), (True, True)):
            results.append(workload(smooth, n, gray, rows, "smooth", args, dev))
    results.append(workload(smooth, 1, False, True, "smooth", args, dev))
    big = max(c for c in args.counts if c <= 256)
    noise = make_images(min(args.distinct, 8), "noise")
    results.append(workload(noise, big, False, False, "noise", args, dev))
    results.append(workload(noise, big, False, True, "noise", args, dev))
    if dev is not None:
        results.append(folder(smooth, args.pairs, args, dev))
        cross = {}
        for key in ("pillow_1_thread_ms", f"pillow_{HOST_THREADS}_threads_ms"):
            wins = [r["files"] for r in results[:len(args.counts)] if "hip_call_ms" in r and r["hip_call_ms"]["median"] < r[key]["median"]]
            cross[key] = min(wins) if wins else None
        results.append({"what": "the smallest measured count of colour files without restart markers at which one swf_jpeg_decode call takes less "
                                "time than Pillow (null: at none of the counts measured); the counts between two measured ones were not measured",
                        "counts_measured": args.counts, "device_call_faster_from": cross})
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "python tools/jpeg_decode_bench.py (one MI355X, one process, HIP events; Pillow on the host clock of the same machine, "
                               f"{os.cpu_count()} CPUs visible, {HOST_THREADS} threads used)", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
