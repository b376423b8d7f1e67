// Gather / scatter of a list of tensors in one launch (kernels_flat.hip): n contiguous fp32 tensors <-> consecutive, unpadded segments
// of one flat fp32 buffer.  The tensors are described by the optimiser's table (kernels_optim.h): a row's `grad` is the source of its
// elements and its `param` their destination, so a gather's rows point their `param` into the flat buffer and a scatter's their `grad`.
#pragma once
#include "kernels_optim.h"

namespace swf {

// dst[i] = src[i] * scale (scaled != 0) or src[i] for every element of every row; a row whose source is NULL is filled with zeros.
// One workgroup per chunk of the table.
int launch_tensors_copy(const swf_adam_tensor* rows, const int32_t* chunk_row, int n_chunks, float scale, int scaled, hipStream_t stream);

}  // namespace swf
