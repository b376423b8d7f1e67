// Dataset kernel (kernels_data.hip): the reference's training-time input transform (a015_dataset.py:57-66, :89-103) for image pairs
// that already lie in device memory as uint8 — BGR->Y on uint8, /255, antialiased bilinear resized-crop and horizontal flip, both
// images of a pair with one geometry, one launch per batch.  The per-axis tap geometry below is the one of
// torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False) on the crop (which is what torchvision's
// resized_crop does to a float tensor); it is evaluated in fp64 and the normalised weight is rounded to fp32 once, so the kernel's
// error is that of its fp32 sums alone.
#pragma once
#include "swf_common.h"

namespace swf {

constexpr int kCropTileW = 64;      // output columns of a workgroup's tile (one wave-wide row)
constexpr int kCropTileH = 16;      // output rows of the tile
constexpr int kCropStripRows = 48;  // source rows whose horizontal pass LDS holds at a time (2 images x 48 x 64 fp32 = 24 KB)
constexpr int kCropThreads = 256;

// Taps of one output index along one axis: source indices [lo, lo + n) of the crop, tap j weighing crop_raw(j) * inv_sum.
struct CropAxis {
    double c, inv_sum;
    int lo, n;
};

__host__ __device__ inline double crop_raw(double c, double inv, int lo, int j) {
#pragma clang fp contract(off)
    const double t = 1.0 - fabs(((double)(j + lo) - c + 0.5) * inv);
    return t > 0.0 ? t : 0.0;
}

// in = crop length, out = output length, o = output index; inv = (in/out >= 1 ? out/in : 1) is the same for every o.
__host__ __device__ inline double crop_inv(int in, int out) {
    const double scale = (double)in / (double)out;
    return scale >= 1.0 ? 1.0 / scale : 1.0;
}

__host__ __device__ inline CropAxis crop_axis(int in, int out, int o) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double support = scale >= 1.0 ? scale : 1.0;
    const double inv = crop_inv(in, out);
    CropAxis a;
    a.c = scale * ((double)o + 0.5);
    const int lo = (int)(a.c - support + 0.5), hi = (int)(a.c + support + 0.5);
    a.lo = lo > 0 ? lo : 0;
    a.n = (hi < in ? hi : in) - a.lo;
    double sum = 0.0;
    for (int j = 0; j < a.n; ++j) sum += crop_raw(a.c, inv, a.lo, j);
    a.inv_sum = 1.0 / sum;   // the tap nearest c lies within 0.5 of it and support >= 1: sum >= 0.5
    return a;
}

}  // namespace swf
