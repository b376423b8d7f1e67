// PNG decoder (kernels_pngdec.hip): the format include/swinfuse.h states at swf_png_decode.  A host parser (chunks, IHDR, PLTE, the IDAT
// ranges, the zlib header) and six launches over all files of a call: prefix sums, gather + zero fill, inflate (one wavefront per file),
// Adler-32, unfilter (one wavefront per file, a skewed band of rows), finish.  The serial parts are pngdec_core.h.
#pragma once
#include "swf_common.h"

namespace swf {

constexpr int kPngDecMaxFiles = 65535;      // the gather, Adler and finish launches have one grid row per file
constexpr int kPngDecWave = 64;             // inflate and unfilter: one wavefront per workgroup, one workgroup per file
constexpr int kPngDecThreads = 256;
constexpr int kPngDecBandRows = 64;         // rows the unfilter keeps in flight: one per lane
constexpr int kPngDecAdlerSegment = 16384;  // inflated bytes per workgroup of the Adler launch

// Host only; the statuses and their reasons are those of swf_png_parse.
int pngdec_parse(const uint8_t* data, size_t n, swf_png_file* file, uint32_t* ranges, size_t ranges_cap, size_t* ranges_needed);
// SWF_OK for a descriptor the parser could have written.  Host only.
int pngdec_file_ok(const swf_png_file& f, int index);
// 0 when the inflated bytes, the streams or the ranges of the call leave int32.
size_t pngdec_workspace_bytes(const swf_png_file* files_host, int n_files);
// Arguments are already validated (swf_api.hip).
int pngdec_decode(const uint8_t* data, const swf_png_file* files_host, const swf_png_file* files_dev, int n_files, const uint32_t* ranges_dev,
                  uint8_t* out, int32_t* status, int layout, void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace swf
