// Baseline JPEG decoder (kernels_jpegdec.hip): the format include/swinfuse.h states at swf_jpeg_decode.  A host parser (segments,
// canonical Huffman descriptions, quantisation tables, restart-interval offsets) and four launches over all files of a call: prefix
// sums, entropy decode (jpegdec_core.h, one lane per restart interval), dequantise + islow IDCT, fancy upsampling + colour.  A second
// entropy path decodes in parallel INSIDE an interval (jpegdec_split_core.h), for files without restart markers.
#pragma once
#include "swf_common.h"

namespace swf {

constexpr int kJpegDecMaxFiles = 65535;     // the finish launch has one grid row per file
constexpr int kJpegDecEntropyThreads = 64;  // one wave per workgroup: the intervals of a call spread over as many CUs as they can
constexpr int kJpegDecThreads = 256;

// Host only; the statuses and their reasons are those of swf_jpeg_parse.
int jpegdec_parse(const uint8_t* data, size_t n, swf_jpeg_file* file, uint32_t* intervals, size_t intervals_cap, size_t* intervals_needed);
// SWF_OK for a descriptor the parser could have written (geometry, table indices, offsets inside the file).  Host only.
int jpegdec_file_ok(const swf_jpeg_file& f, int index);
// 0 when the totals leave int32.
size_t jpegdec_workspace_bytes(const swf_jpeg_file* files_host, int n_files);
// Arguments are already validated (swf_api.hip).
int jpegdec_decode(const uint8_t* data, const swf_jpeg_file* files_host, const swf_jpeg_file* files_dev, int n_files,
                   const uint32_t* intervals_dev, uint8_t* out, int32_t* status, int layout, void* workspace, size_t workspace_bytes,
                   hipStream_t stream);

// The split path (swf_jpeg_decode_split; jpegdec_split_core.h): the files as above, plus the host copy of the intervals and the segment
// size.  check: the split call's own refusals (NULL host intervals, the segment size, more than 2^31 - 1 segments), on files
// jpegdec_file_ok has passed.
int jpegdec_split_check(const swf_jpeg_file* files_host, int n_files, const uint32_t* intervals_host, int segment_bytes);
size_t jpegdec_split_workspace_bytes(const swf_jpeg_file* files_host, int n_files, const uint32_t* intervals_host, int segment_bytes);
int jpegdec_split_decode(const uint8_t* data, const swf_jpeg_file* files_host, const swf_jpeg_file* files_dev, int n_files,
                         const uint32_t* intervals_dev, const uint32_t* intervals_host, int segment_bytes, uint8_t* out, int32_t* status,
                         int layout, void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
