// PNG encoder (kernels_png.hip): the format include/swinfuse.h states at swf_png_encode, in six launches.  A filter pass per row, a token
// and code pass per deflate block, a framing pass per image (bit offsets, Adler-32, the constant chunks), an emit pass per block and two
// passes for the IDAT chunk's CRC-32.  The code construction and the checksum combination are png_core.h.
#pragma once
#include "png_core.h"
#include "swf_common.h"

namespace swf {

constexpr int kPngThreads = 256;
constexpr int kPngTile = kPngThreads * 8;          // stream bytes one pass of a block's workgroup takes, 8 per thread
constexpr int kPngDefaultRows = 16;                // rows_per_block = 0
constexpr int64_t kPngMaxBlockBytes = 1 << 22;     // a block's histogram counts stay below kPngMaxCount
constexpr int kPngCrcSegment = 1024;               // bytes one lane of the CRC pass walks
constexpr int kPngFrameBytes = 8 + 25 + 12 + 2 + 4 + 12;   // signature, IHDR, IDAT's length, type and CRC, zlib's header and Adler-32, IEND
constexpr int kPngDataOffset = 8 + 25 + 8 + 2;     // where the deflate blocks start in the file
// A block of n stream bytes in bits, at most: the longest dynamic header, 15 bits per byte (a literal's longest code; a match covers
// three bytes or more in at most 15 + 5 + 1 bits) and the end-of-block symbol.  The fixed code is taken only where it is smaller.
constexpr int kPngBlockOverheadBits = kPngHeaderBitsMax + kPngMaxBits;

// channels 1 | 3, rows_per_block >= 0, reserved 0
bool png_desc_ok(const swf_png_desc& d);
// B H W channels and one image's capacity within int32 (lengths[] is int32), a block within kPngMaxBlockBytes
bool png_shape_ok(const swf_png_desc& d, int B, int H, int W);

size_t png_capacity_bytes(const swf_png_desc& d, int H, int W);
size_t png_workspace_bytes(const swf_png_desc& d, int B, int H, int W);

// Arguments are already validated (swf_api.hip).
int png_encode(const swf_png_desc& d, const uint8_t* pixels, uint8_t* out, size_t capacity, int32_t* lengths, int B, int H, int W,
               void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
