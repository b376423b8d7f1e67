// Baseline JPEG encoder (kernels_jpeg.hip): the format include/swinfuse.h states at swf_jpeg_encode, in three launches.  A coefficient
// pass (colour transform, 2 x 2 chroma mean, edge replication, integer DCT, quantiser, zig-zag), an entropy pass per MCU row (one
// restart interval each, so rows are independent) and a pack pass that lines the rows up behind the header.
#pragma once
#include "swf_common.h"

namespace swf {

constexpr int kJpegThreads = 256;
constexpr int kJpegStripPixels = 128;            // pixels across one workgroup of the coefficient pass
constexpr int kJpegChunkBlocks = 128;            // blocks one pass of the entropy workgroup codes; a longer MCU row takes several passes
constexpr int kJpegWorstBlockBits = 20 + 63 * 26;   // a DC symbol of 9 + 11 bits and 63 AC symbols of 16 + 10 bits

// channels 1 | 3, subsampling SWF_JPEG_444 | SWF_JPEG_420 (three channels only), quality 1..100
bool jpeg_desc_ok(const swf_jpeg_desc& d);
// H, W <= 65535, B H W and one image's capacity within int32 (lengths[] is int32)
bool jpeg_shape_ok(const swf_jpeg_desc& d, int B, int H, int W);

size_t jpeg_header_bytes(const swf_jpeg_desc& d);
// out[0 .. jpeg_header_bytes) <- the header (host memory)
void jpeg_header(const swf_jpeg_desc& d, int H, int W, uint8_t* out);
size_t jpeg_capacity_bytes(const swf_jpeg_desc& d, int H, int W);
size_t jpeg_workspace_bytes(const swf_jpeg_desc& d, int B, int H, int W);

// Arguments are already validated (swf_api.hip).
int jpeg_encode(const swf_jpeg_desc& d, const uint8_t* pixels, const uint8_t* header_dev, uint8_t* out, size_t capacity, int32_t* lengths,
                int B, int H, int W, void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
