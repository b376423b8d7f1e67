"""Time of one training batch from the resident paired dataset (DESIGN 6c "Data"): --batch pairs cut from resident --height x --width
uint8 pairs to --size x --size by swf_paired_crop_resize_fwd, against the same pairs and boxes through the CPU restatement of the
reference's per-item transform (cv2-formula luma on uint8, /255, torch CPU F.interpolate(antialias=True) on the crop, flip; the
reference's own cv2 / torchvision are not available here).  NEITHER side includes file decoding: the reference decodes two files per
item in every step on top of what is timed here, the resident store decodes once.  Gates nothing; one JSON line.

    kernel_ms           HIP events around the launch alone, rows already on the device, median of --iters
    batch_event_ms      HIP events around PairLoader's whole batch (draws, row fill, check, upload, allocation, launch)
    batch_host_ms       host clock around next(it) without a synchronise: what the training loop waits before it can enqueue the step
    copy_same_bytes_ms  a device-to-device copy of as many bytes as the kernel reads + writes (the floor of its traffic)
    cpu_restatement_ms  host clock around the CPU restatement of the same batch, median of --cpu-iters

    python tools/data_bench.py [--batch 20] [--size 224] [--height 512] [--width 640] [--pairs 100] [--iters 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__ as entry


def event_ms(fn, iters, warmup=5):
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


def cpu_item(ir_u8, vis_u8, box, size):
    """The reference's per-item work after decoding, restated: BGR->Y on uint8 (OpenCV's published fixed point), scale, resized crop, flip."""
    top, left, h, w, flip = box
    v = vis_u8.to(torch.int32)
    y8 = ((v[..., 0] * 1868 + v[..., 1] * 9617 + v[..., 2] * 4899 + (1 << 13)) >> 14).clamp_(0, 255).to(torch.uint8)
    outs = []
    for img in (ir_u8, y8):
        x = (img.to(torch.float32) / 255)[None, None, top:top + h, left:left + w]
        x = F.interpolate(x, size=size, mode="bilinear", antialias=True, align_corners=False)
        outs.append(x.flip(-1) if flip else x)
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--pairs", type=int, default=100)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cpu-iters", type=int, default=5)
    args = ap.parse_args()
    entry.build()
    from swin_unet_image_fusion_amd import PairLoader, ResidentPairs, data as D, sample_crop_params
    if not torch.cuda.is_available():
        raise SystemExit("data_bench needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    B, size, H, W = args.batch, (args.size, args.size), args.height, args.width
    rng = np.random.default_rng(0)
    pairs = [(rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)) for _ in range(args.pairs)]
    store = ResidentPairs.from_arrays(pairs, device=dev)
    g = torch.Generator().manual_seed(0)
    picks = torch.randperm(len(store), generator=g).tolist()[:B]
    boxes = [sample_crop_params(H, W, size, generator=g) for _ in picks]
    loader = PairLoader(store, None, batch_size=B, size=size, generator=g)

    # the launch alone
    bt = loader.batch(picks, boxes)
    rows_dev = loader._dev[loader._turn ^ 1]
    ir, vis = bt["ir"], bt["vis"]
    kernel_ms = event_ms(lambda: D._crop_resize(store, rows_dev, B, size[0], size[1], ir, vis), args.iters)
    batch_event_ms = event_ms(lambda: loader.batch(picks, boxes), args.iters)

    it, host = iter(loader), []
    for _ in range(len(loader)):                       # one epoch of drawn batches, no synchronise inside the clock
        t0 = time.perf_counter()
        next(it)
        host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    it, epoch_ev = iter(loader), []
    for _ in range(len(loader)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        next(it)
        b.record()
        b.synchronize()
        epoch_ev.append(a.elapsed_time(b))

    read_bytes = sum(4 * h * w for _, _, h, w, _ in boxes)                # 1 gray + 3 BGR bytes per pixel of the box
    write_bytes = 2 * B * size[0] * size[1] * 4
    n = (read_bytes + write_bytes) // 4 * 4
    src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    copy_ms = event_ms(lambda: dst.copy_(src), args.iters)

    # CPU restatement of the same batch
    host_pairs = [(torch.from_numpy(pairs[p][0]), torch.from_numpy(pairs[p][1])) for p in picks]
    cpu = []
    for _ in range(args.cpu_iters + 1):
        t0 = time.perf_counter()
        outs = [cpu_item(i8, v8, box, size) for (i8, v8), box in zip(host_pairs, boxes)]
        ir_c, vis_c = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        cpu.append((time.perf_counter() - t0) * 1e3)
    cpu = cpu[1:]
    bt = loader.batch(picks, boxes)
    torch.cuda.synchronize()
    diff = max(float((bt["ir"].cpu() - ir_c).abs().max()), float((bt["vis"].cpu() - vis_c).abs().max()))

    res = {"what": f"one batch of {B} at {size[0]}x{size[1]} from {len(store)} resident {H}x{W} pairs; ms; decode time in neither side",
           "kernel_ms": kernel_ms, "batch_event_ms": batch_event_ms,
           "batch_host_ms": round(statistics.median(host[1:] or host), 4), "batch_drawn_event_ms": round(statistics.median(epoch_ev), 4),
           "kernel_read_mb": round(read_bytes / 1e6, 2), "kernel_write_mb": round(write_bytes / 1e6, 2),
           "kernel_gb_per_s": round((read_bytes + write_bytes) / 1e6 / kernel_ms, 1), "copy_same_bytes_ms": copy_ms,
           "cpu_restatement_ms": round(statistics.median(cpu), 2), "cpu_threads": torch.get_num_threads(),
           "max_abs_diff_gpu_vs_cpu_restatement": diff,
           "store_mb": round((store.ir_arena.numel() + store.vis_arena.numel()) / 1e6, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
