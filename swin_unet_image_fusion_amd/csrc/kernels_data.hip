// The reference's training-time input transform for a resident dataset (a015_dataset.py): per output sample one swf_crop_row names a
// gray and a BGR uint8 image in two device arenas, a crop box and a flip; one launch writes ir and vis_y, [B][1][out_h][out_w] fp32:
//   tap value  : ir u8 / 255.0f;  vis cv2's uint8 luma (color_fixed.h) / 255.0f
//   resize     : crop, then separable antialiased bilinear (kernels_data.h), horizontal pass then vertical pass, fp32 fmaf chains in
//                ascending tap order; taps never leave the crop box;  flip mirrors the output columns;  no clamp.
// One workgroup owns a 16 x 64 output tile of one sample and both of its images.  It computes the tile's column and row taps once
// (fp64, into LDS), runs the horizontal pass from global uint8 into an LDS strip of fp32 (source rows x 64 tile columns, both images),
// the vertical pass from that strip into registers, and stores 256-byte output rows.  The tile's source rows are walked in strips of
// kCropStripRows, so LDS does not grow with the scale (a large image cropped whole); the tap order, and so every bit of the result,
// does not depend on where the strips fall.  No atomics; plain loads and stores.
#include "color_fixed.h"
#include "kernels_data.h"

namespace swf {

__global__ __launch_bounds__(kCropThreads) void paired_crop_resize_kernel(const uint8_t* __restrict__ ir_base,
                                                                          const uint8_t* __restrict__ vis_base,
                                                                          const swf_crop_row* __restrict__ rows, int out_h, int out_w,
                                                                          float* __restrict__ ir_out, float* __restrict__ vis_out) {
    __shared__ float unit[256];   // u8 / 255.0f
    __shared__ double xc[kCropTileW], xis[kCropTileW], yc[kCropTileH], yis[kCropTileH];
    __shared__ int xlo[kCropTileW], xn[kCropTileW], ylo[kCropTileH], yn[kCropTileH];
    __shared__ float strip[2][kCropStripRows][kCropTileW];

    const int tid = threadIdx.x, b = blockIdx.z;
    const swf_crop_row r = rows[b];
    const int ox0 = blockIdx.x * kCropTileW, oy0 = blockIdx.y * kCropTileH;

    unit[tid] = (float)tid / 255.0f;
    if (tid < kCropTileW) {
        CropAxis a = {0.0, 0.0, 0, 0};
        if (ox0 + tid < out_w) a = crop_axis(r.w, out_w, ox0 + tid);
        xc[tid] = a.c, xis[tid] = a.inv_sum, xlo[tid] = a.lo, xn[tid] = a.n;
    } else if (tid < kCropTileW + kCropTileH) {
        const int i = tid - kCropTileW;
        CropAxis a = {0.0, 0.0, 0, 0};
        if (oy0 + i < out_h) a = crop_axis(r.h, out_h, oy0 + i);
        yc[i] = a.c, yis[i] = a.inv_sum, ylo[i] = a.lo, yn[i] = a.n;
    }
    __syncthreads();

    const int tcol = tid % kCropTileW, trow = tid / kCropTileW;   // trow: 0..3, the wave
    constexpr int kRowsPerThread = kCropTileH / (kCropThreads / kCropTileW);
    constexpr int kRowStep = kCropThreads / kCropTileW;
    const double inv_x = crop_inv(r.w, out_w), inv_y = crop_inv(r.h, out_h);
    const int ny = min(kCropTileH, out_h - oy0);                  // >= 1 by the grid
    const int y_begin = ylo[0], y_end = ylo[ny - 1] + yn[ny - 1];  // lo and lo + n do not decrease with the output index
    const int lo = xlo[tcol], n = xn[tcol];
    const double c = xc[tcol], is = xis[tcol];
    const uint8_t* ir_img = ir_base + r.ir_off;
    const uint8_t* vis_img = vis_base + r.vis_off;

    float acc_i[kRowsPerThread], acc_v[kRowsPerThread];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) acc_i[k] = 0.f, acc_v[k] = 0.f;

    for (int s = y_begin; s < y_end; s += kCropStripRows) {
        const int rows_here = min(kCropStripRows, y_end - s);
        // horizontal pass: crop rows [s, s + rows_here) -> strip
        for (int rr = trow; rr < rows_here; rr += kRowStep) {
            const int64_t px = (int64_t)(r.top + s + rr) * r.W + r.left + lo;
            const uint8_t* pi = ir_img + px;
            const uint8_t* pv = vis_img + px * 3;
            float ai = 0.f, av = 0.f;
            for (int j = 0; j < n; ++j) {
                const float wgt = (float)(crop_raw(c, inv_x, lo, j) * is);
                ai = fmaf(wgt, unit[pi[j]], ai);
                av = fmaf(wgt, unit[sat8(bgr_to_y8(pv[3 * j], pv[3 * j + 1], pv[3 * j + 2]))], av);
            }
            strip[0][rr][tcol] = ai;
            strip[1][rr][tcol] = av;
        }
        __syncthreads();
        // vertical pass: the taps of this thread's output rows that fall into the strip
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            const int i = trow + k * kRowStep;
            if (i < ny) {
                const int lo_y = ylo[i];
                const double c_y = yc[i], is_y = yis[i];
                const int j0 = max(0, s - lo_y), j1 = min(yn[i], s + rows_here - lo_y);
                for (int j = j0; j < j1; ++j) {
                    const float wgt = (float)(crop_raw(c_y, inv_y, lo_y, j) * is_y);
                    acc_i[k] = fmaf(wgt, strip[0][lo_y + j - s][tcol], acc_i[k]);
                    acc_v[k] = fmaf(wgt, strip[1][lo_y + j - s][tcol], acc_v[k]);
                }
            }
        }
        __syncthreads();
    }

    const int ox = ox0 + tcol;
    if (ox < out_w) {
        const int xo = r.flip ? out_w - 1 - ox : ox;
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            const int oy = oy0 + trow + k * kRowStep;
            if (oy < out_h) {
                const int64_t e = ((int64_t)b * out_h + oy) * out_w + xo;
                ir_out[e] = acc_i[k];
                vis_out[e] = acc_v[k];
            }
        }
    }
}

}  // namespace swf

using namespace swf;

extern "C" {

size_t swf_paired_crop_rows_bytes(int32_t B) { return B > 0 ? (size_t)B * sizeof(swf_crop_row) : 0; }

int swf_paired_crop_rows_check(const swf_crop_row* rows_host, int32_t B, uint64_t ir_bytes, uint64_t vis_bytes) {
    if (!rows_host) return fail(SWF_ERR_NULL, "paired_crop_rows_check: NULL rows");
    if (B <= 0) return fail(SWF_ERR_BAD_SHAPE, "paired_crop_rows_check: B = %d", B);
    for (int32_t i = 0; i < B; ++i) {
        const swf_crop_row& r = rows_host[i];
        if (r.H < 1 || r.W < 1) return fail(SWF_ERR_BAD_SHAPE, "paired_crop_rows_check: row %d: image %d x %d", i, r.H, r.W);
        if (r.h < 1 || r.w < 1 || r.top < 0 || r.left < 0 || (int64_t)r.top + r.h > r.H || (int64_t)r.left + r.w > r.W)
            return fail(SWF_ERR_BAD_SHAPE, "paired_crop_rows_check: row %d: box top %d left %d h %d w %d leaves its %d x %d image", i, r.top,
                        r.left, r.h, r.w, r.H, r.W);
        const uint64_t px = (uint64_t)r.H * (uint64_t)r.W;   // < 2^62
        if (r.ir_off > ir_bytes || px > ir_bytes - r.ir_off)
            return fail(SWF_ERR_BAD_SHAPE, "paired_crop_rows_check: row %d: gray image at %llu (+%llu) passes its arena of %llu bytes", i,
                        (unsigned long long)r.ir_off, (unsigned long long)px, (unsigned long long)ir_bytes);
        if (r.vis_off > vis_bytes || 3 * px > vis_bytes - r.vis_off)
            return fail(SWF_ERR_BAD_SHAPE, "paired_crop_rows_check: row %d: BGR image at %llu (+%llu) passes its arena of %llu bytes", i,
                        (unsigned long long)r.vis_off, (unsigned long long)(3 * px), (unsigned long long)vis_bytes);
    }
    return SWF_OK;
}

int swf_paired_crop_resize_fwd(const uint8_t* ir_base, const uint8_t* vis_base, const swf_crop_row* rows_device, int32_t B, int32_t out_h,
                               int32_t out_w, float* ir_out, float* vis_y_out, swf_stream_t stream) {
    if (!ir_base || !vis_base || !rows_device || !ir_out || !vis_y_out) return fail(SWF_ERR_NULL, "paired_crop_resize: NULL pointer");
    if (B <= 0 || out_h <= 0 || out_w <= 0) return fail(SWF_ERR_BAD_SHAPE, "paired_crop_resize: B %d, output %d x %d", B, out_h, out_w);
    const int gx = cdiv(out_w, kCropTileW), gy = cdiv(out_h, kCropTileH);
    if (B > 65535 || gy > 65535) return fail(SWF_ERR_BAD_SHAPE, "paired_crop_resize: B %d or out_h %d beyond one launch's grid", B, out_h);
    hipLaunchKernelGGL(paired_crop_resize_kernel, dim3(gx, gy, B), dim3(kCropThreads), 0, as_stream(stream), ir_base, vis_base,
                       rows_device, out_h, out_w, ir_out, vis_y_out);
    return check_launch("paired_crop_resize");
}

}  // extern "C"
