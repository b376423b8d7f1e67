// C-ABI entry points of the four codecs (JPEG and PNG, encoder and decoder): argument checks and workspace sizes.  The kernels differ per
// format; what stands between the ABI and them is written once here: the encoders' ladder, the decoders' file table and call checks.
// Every argument check comes before the first HIP call.
#include <algorithm>
#include <utility>
#include <vector>

#include "kernels_jpeg.h"
#include "kernels_jpegdec.h"
#include "kernels_png.h"
#include "kernels_pngdec.h"

using namespace swf;

static_assert(SWF_PNG_OUT_BGR == SWF_JPEG_OUT_BGR && SWF_PNG_OUT_RGB == SWF_JPEG_OUT_RGB && SWF_PNG_OUT_GRAY == SWF_JPEG_OUT_GRAY,
              "one layout check serves both decoders");

// What a decoder is to the shared checks.  `who` prefixes every sentence; `tables` is the NULL sentence's word for the offset table.
template <class File>
struct FileChecks {
    const char *who, *tables, *overflow;
    int max_files;
    int (*file_ok)(const File&, int);
    size_t (*workspace_bytes)(const File*, int);
};
static const FileChecks<swf_jpeg_file> kJpegFiles = {"jpeg_decode", "intervals", "more than 2^31 - 1 blocks or intervals in one call",
                                                     kJpegDecMaxFiles, jpegdec_file_ok, jpegdec_workspace_bytes};
static const FileChecks<swf_png_file> kPngFiles = {"png_decode", "ranges", "more than 2^31 - 1 inflated bytes, stream bytes or IDAT ranges in one call",
                                                   kPngDecMaxFiles, pngdec_file_ok, pngdec_workspace_bytes};

// The host copy of the descriptors: the count, every file's own check, and sums that stay within int32.
template <class File>
static int check_file_table(const FileChecks<File>& c, const File* files, int32_t n_files) {
    if (!files) return fail(SWF_ERR_NULL, "%s: NULL descriptors", c.who);
    if (n_files < 1) return fail(SWF_ERR_BAD_SHAPE, "%s: %d files", c.who, n_files);
    if (n_files > c.max_files) return fail(SWF_ERR_UNSUPPORTED, "%s: %d files in one call (%d at most)", c.who, n_files, c.max_files);
    for (int32_t i = 0; i < n_files; ++i) SWF_TRY(c.file_ok(files[i], i));
    if (c.workspace_bytes(files, n_files) == 0) return fail(SWF_ERR_UNSUPPORTED, "%s: %s", c.who, c.overflow);
    return SWF_OK;
}

// What the decode entries check alike: pointers, layout, descriptors, every file's place in both buffers, pixels that do not overlap.
template <class File>
static int check_decode_call(const FileChecks<File>& c, const uint8_t* data, size_t data_bytes, const File* files_host, const File* files_dev,
                             int32_t n_files, const uint32_t* tables_dev, const uint8_t* out, size_t out_bytes, const int32_t* status,
                             int32_t layout) {
    if (!data || !files_host || !files_dev || !tables_dev || !out || !status)
        return fail(SWF_ERR_NULL, "%s: NULL data, descriptors, %s, output or status", c.who, c.tables);
    if (layout != SWF_JPEG_OUT_BGR && layout != SWF_JPEG_OUT_RGB && layout != SWF_JPEG_OUT_GRAY)
        return fail(SWF_ERR_BAD_SHAPE, "%s: layout %d (0 BGR, 1 RGB, 2 gray)", c.who, layout);
    SWF_TRY(check_file_table(c, files_host, n_files));
    const uint64_t px = layout == SWF_JPEG_OUT_GRAY ? 1 : 3;
    std::vector<std::pair<uint64_t, uint64_t>> spans((size_t)n_files);
    for (int32_t i = 0; i < n_files; ++i) {
        const File& f = files_host[i];
        if (f.data_off > data_bytes || f.data_bytes > data_bytes - f.data_off)
            return fail(SWF_ERR_BAD_SHAPE, "%s: file %d: bytes [%llu, + %u) leave the data buffer of %zu bytes", c.who, i,
                        (unsigned long long)f.data_off, f.data_bytes, data_bytes);
        const uint64_t n = (uint64_t)f.H * f.W * px;
        if (f.out_off > out_bytes || n > out_bytes - f.out_off)
            return fail(SWF_ERR_BAD_SHAPE, "%s: file %d: pixels [%llu, + %llu) leave the output buffer of %zu bytes", c.who, i,
                        (unsigned long long)f.out_off, (unsigned long long)n, out_bytes);
        spans[(size_t)i] = {f.out_off, f.out_off + n};
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); ++i)
        if (spans[i].first < spans[i - 1].second)
            return fail(SWF_ERR_BAD_SHAPE, "%s: the pixels of two files overlap at byte %llu of the output", c.who, (unsigned long long)spans[i].first);
    return SWF_OK;
}

// The encoders' ladder: descriptor -> NULL check -> shape -> capacity -> workspace.
template <class DESC>
static int check_encode_call(const char* who, int (*check_desc)(const DESC*), int (*check_shape)(const DESC&, int32_t, int32_t, int32_t),
                             size_t (*capacity_bytes)(const DESC&, int, int), size_t (*workspace_need)(const DESC&, int, int, int),
                             const DESC* desc, const uint8_t* pixels, const uint8_t* out, size_t capacity, const int32_t* lengths, int32_t B,
                             int32_t H, int32_t W, const void* workspace, size_t workspace_bytes) {
    SWF_TRY(check_desc(desc));
    if (!pixels || !out || !lengths) return fail(SWF_ERR_NULL, "%s: NULL pixels, output or lengths", who);
    SWF_TRY(check_shape(*desc, B, H, W));
    const size_t cap = capacity_bytes(*desc, H, W);
    if (capacity < cap) return fail(SWF_ERR_WORKSPACE, "%s: capacity of %zu bytes per image, %zu needed", who, capacity, cap);
    return need_workspace(who, workspace, workspace_bytes, workspace_need(*desc, B, H, W));
}

// Baseline JPEG encoder.  One check of the descriptor and one of the shape serve the four queries and the call.
static int check_jpeg_desc(const swf_jpeg_desc* d) {
    if (!d) return fail(SWF_ERR_NULL, "jpeg: NULL descriptor");
    if (!jpeg_desc_ok(*d))
        return fail(SWF_ERR_BAD_SHAPE, "jpeg: channels=%d subsampling=%d quality=%d (channels 1 or 3, subsampling 0 (4:4:4) or, with three "
                    "channels, 1 (4:2:0), quality 1..100)", d->channels, d->subsampling, d->quality);
    return SWF_OK;
}

static int check_jpeg_shape(const swf_jpeg_desc& d, int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "jpeg: empty tensor (B=%d H=%d W=%d)", B, H, W);
    if (!jpeg_shape_ok(d, B, H, W))
        return fail(SWF_ERR_UNSUPPORTED, "jpeg: B=%d H=%d W=%d: H, W <= 65535 (the frame header's 16 bits), B H W and one image's capacity "
                    "within int32", B, H, W);
    return SWF_OK;
}

// PNG encoder.  One check of the descriptor and one of the shape serve the two queries and the call.
static int check_png_desc(const swf_png_desc* d) {
    if (!d) return fail(SWF_ERR_NULL, "png: NULL descriptor");
    if (!png_desc_ok(*d))
        return fail(SWF_ERR_BAD_SHAPE, "png: channels=%d rows_per_block=%d reserved=%d (channels 1 or 3, rows_per_block >= 0, reserved 0)",
                    d->channels, d->rows_per_block, d->reserved);
    return SWF_OK;
}

static int check_png_shape(const swf_png_desc& d, int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "png: empty tensor (B=%d H=%d W=%d)", B, H, W);
    if (!png_shape_ok(d, B, H, W))
        return fail(SWF_ERR_UNSUPPORTED, "png: B=%d H=%d W=%d rows_per_block=%d: B H W channels, the streams of the batch and one image's "
                    "capacity must fit int32, and a block %lld stream bytes", B, H, W, d.rows_per_block, (long long)kPngMaxBlockBytes);
    return SWF_OK;
}

extern "C" {

size_t swf_jpeg_header_bytes(const swf_jpeg_desc* desc) { return check_jpeg_desc(desc) == SWF_OK ? jpeg_header_bytes(*desc) : 0; }

int swf_jpeg_header(const swf_jpeg_desc* desc, int32_t H, int32_t W, uint8_t* host_out, size_t n) {
    SWF_TRY(check_jpeg_desc(desc));
    if (!host_out) return fail(SWF_ERR_NULL, "jpeg_header: NULL output");
    if (H <= 0 || W <= 0) return fail(SWF_ERR_BAD_SHAPE, "jpeg_header: empty image (H=%d W=%d)", H, W);
    if (H > 65535 || W > 65535) return fail(SWF_ERR_UNSUPPORTED, "jpeg_header: H=%d W=%d beyond the frame header's 16 bits", H, W);
    if (n < jpeg_header_bytes(*desc)) return fail(SWF_ERR_WORKSPACE, "jpeg_header: room for %zu bytes, %zu needed", n, jpeg_header_bytes(*desc));
    jpeg_header(*desc, H, W, host_out);
    return SWF_OK;
}

size_t swf_jpeg_capacity_bytes(const swf_jpeg_desc* desc, int32_t H, int32_t W) {
    return check_jpeg_desc(desc) == SWF_OK && check_jpeg_shape(*desc, 1, H, W) == SWF_OK ? jpeg_capacity_bytes(*desc, H, W) : 0;
}

size_t swf_jpeg_workspace_bytes(const swf_jpeg_desc* desc, int32_t B, int32_t H, int32_t W) {
    return check_jpeg_desc(desc) == SWF_OK && check_jpeg_shape(*desc, B, H, W) == SWF_OK ? jpeg_workspace_bytes(*desc, B, H, W) : 0;
}

int swf_jpeg_encode(const swf_jpeg_desc* desc, const uint8_t* pixels, const uint8_t* header_dev, uint8_t* out, size_t capacity,
                    int32_t* lengths, int32_t B, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_encode_call<swf_jpeg_desc>("jpeg_encode", check_jpeg_desc, check_jpeg_shape, jpeg_capacity_bytes, jpeg_workspace_bytes, desc,
                                             pixels, out, capacity, lengths, B, H, W, workspace, workspace_bytes));
    return jpeg_encode(*desc, pixels, header_dev, out, capacity, lengths, B, H, W, workspace, workspace_bytes, as_stream(stream));
}

size_t swf_png_capacity_bytes(const swf_png_desc* desc, int32_t H, int32_t W) {
    return check_png_desc(desc) == SWF_OK && check_png_shape(*desc, 1, H, W) == SWF_OK ? png_capacity_bytes(*desc, H, W) : 0;
}

size_t swf_png_workspace_bytes(const swf_png_desc* desc, int32_t B, int32_t H, int32_t W) {
    return check_png_desc(desc) == SWF_OK && check_png_shape(*desc, B, H, W) == SWF_OK ? png_workspace_bytes(*desc, B, H, W) : 0;
}

int swf_png_encode(const swf_png_desc* desc, const uint8_t* pixels, uint8_t* out, size_t capacity, int32_t* lengths, int32_t B, int32_t H,
                   int32_t W, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_encode_call<swf_png_desc>("png_encode", check_png_desc, check_png_shape, png_capacity_bytes, png_workspace_bytes, desc, pixels,
                                            out, capacity, lengths, B, H, W, workspace, workspace_bytes));
    return png_encode(*desc, pixels, out, capacity, lengths, B, H, W, workspace, workspace_bytes, as_stream(stream));
}

// The decoders.  The parses and the workspace queries are host-only; a call checks the host copy of the descriptors, every file's place
// in the data buffer and every file's pixels in the output buffer before the first launch.
int swf_jpeg_parse(const uint8_t* data, size_t n, swf_jpeg_file* file, uint32_t* intervals, size_t intervals_cap, size_t* intervals_needed) {
    if (!data || !file || !intervals_needed) return fail(SWF_ERR_NULL, "jpeg_parse: NULL data, descriptor or count");
    return jpegdec_parse(data, n, file, intervals, intervals ? intervals_cap : 0, intervals_needed);
}

size_t swf_jpeg_decode_workspace_bytes(const swf_jpeg_file* files_host, int32_t n_files) {
    return check_file_table(kJpegFiles, files_host, n_files) == SWF_OK ? jpegdec_workspace_bytes(files_host, n_files) : 0;
}

int swf_jpeg_decode(const uint8_t* data, size_t data_bytes, const swf_jpeg_file* files_host, const swf_jpeg_file* files_dev, int32_t n_files,
                    const uint32_t* intervals_dev, uint8_t* out, size_t out_bytes, int32_t* status, int32_t layout, void* workspace,
                    size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_decode_call(kJpegFiles, data, data_bytes, files_host, files_dev, n_files, intervals_dev, out, out_bytes, status, layout));
    SWF_TRY(need_workspace("jpeg_decode", workspace, workspace_bytes, jpegdec_workspace_bytes(files_host, n_files)));
    return jpegdec_decode(data, files_host, files_dev, n_files, intervals_dev, out, status, layout, workspace, workspace_bytes, as_stream(stream));
}

size_t swf_jpeg_decode_split_workspace_bytes(const swf_jpeg_file* files_host, int32_t n_files, const uint32_t* intervals_host, int32_t segment_bytes) {
    if (check_file_table(kJpegFiles, files_host, n_files) != SWF_OK || jpegdec_split_check(files_host, n_files, intervals_host, segment_bytes) != SWF_OK)
        return 0;
    return jpegdec_split_workspace_bytes(files_host, n_files, intervals_host, segment_bytes);
}

// The shared checks speak as jpeg_decode: the split entry refuses what that one refuses, in its words.
int swf_jpeg_decode_split(const uint8_t* data, size_t data_bytes, const swf_jpeg_file* files_host, const swf_jpeg_file* files_dev, int32_t n_files,
                          const uint32_t* intervals_dev, const uint32_t* intervals_host, int32_t segment_bytes, uint8_t* out, size_t out_bytes,
                          int32_t* status, int32_t layout, void* workspace, size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_decode_call(kJpegFiles, data, data_bytes, files_host, files_dev, n_files, intervals_dev, out, out_bytes, status, layout));
    SWF_TRY(jpegdec_split_check(files_host, n_files, intervals_host, segment_bytes));
    SWF_TRY(need_workspace("jpeg_decode_split", workspace, workspace_bytes,
                           jpegdec_split_workspace_bytes(files_host, n_files, intervals_host, segment_bytes)));
    return jpegdec_split_decode(data, files_host, files_dev, n_files, intervals_dev, intervals_host, segment_bytes, out, status, layout, workspace,
                                workspace_bytes, as_stream(stream));
}

int swf_png_parse(const uint8_t* data, size_t n, swf_png_file* file, uint32_t* ranges, size_t ranges_cap, size_t* ranges_needed) {
    if (!data || !file || !ranges_needed) return fail(SWF_ERR_NULL, "png_parse: NULL data, descriptor or count");
    return pngdec_parse(data, n, file, ranges, ranges ? ranges_cap : 0, ranges_needed);
}

size_t swf_png_decode_workspace_bytes(const swf_png_file* files_host, int32_t n_files) {
    return check_file_table(kPngFiles, files_host, n_files) == SWF_OK ? pngdec_workspace_bytes(files_host, n_files) : 0;
}

int swf_png_decode(const uint8_t* data, size_t data_bytes, const swf_png_file* files_host, const swf_png_file* files_dev, int32_t n_files,
                   const uint32_t* ranges_dev, uint8_t* out, size_t out_bytes, int32_t* status, int32_t layout, void* workspace,
                   size_t workspace_bytes, swf_stream_t stream) {
    SWF_TRY(check_decode_call(kPngFiles, data, data_bytes, files_host, files_dev, n_files, ranges_dev, out, out_bytes, status, layout));
    SWF_TRY(need_workspace("png_decode", workspace, workspace_bytes, pngdec_workspace_bytes(files_host, n_files)));
    return pngdec_decode(data, files_host, files_dev, n_files, ranges_dev, out, status, layout, workspace, workspace_bytes, as_stream(stream));
}

}  // extern "C"
