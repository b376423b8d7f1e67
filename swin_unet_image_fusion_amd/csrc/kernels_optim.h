// Multi-tensor optimiser kernels (kernels_optim.hip): one Adam launch over every tensor of a parameter group, and the global L2 norm
// of their gradients as a two-level fixed-order reduction.  The tensors are described by a device-resident table of swf_adam_tensor
// rows followed by a chunk map (chunk -> row index); a chunk is kAdamChunk consecutive elements of ONE tensor.
#pragma once
#include "swf_common.h"

namespace swf {

constexpr int kAdamChunk = 4096;   // elements: 256 threads x 4 float4 per array

// Byte offsets inside the table buffer: rows at 0, the chunk map behind them, the fp64 per-chunk partials of the norm (device side
// only, never copied) behind the map.
struct AdamLayout {
    size_t map_off, copy_bytes, partial_off, total_bytes;
};
inline AdamLayout adam_layout(int64_t n_tensors, int64_t n_chunks) {
    AdamLayout l;
    l.map_off = (size_t)n_tensors * sizeof(swf_adam_tensor);
    l.copy_bytes = l.map_off + (size_t)n_chunks * sizeof(int32_t);
    l.partial_off = align_up(l.copy_bytes, 256);
    l.total_bytes = l.partial_off + (size_t)n_chunks * sizeof(double);
    return l;
}

// The device image of a table after its upload.
struct AdamTable {
    const swf_adam_tensor* rows;
    const int32_t* map;
    double* partials;
    int n_chunks;
};
// ONE asynchronous copy of rows and chunk map to table_device on `stream`; shared by every entry that takes a table (the optimiser's
// and kernels_flat's).  The host table must stay untouched until the copy has run.
int upload_adam_table(const char* who, const void* table_host, void* table_device, int32_t n_tensors, int64_t n_chunks, hipStream_t stream,
                      AdamTable* t);

// norm_out[0] <- || all gradients ||_2, norm_out[1] <- min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_).
int launch_gradnorm(const swf_adam_tensor* rows, const int32_t* chunk_row, int n_chunks, double* partials, float max_norm,
                    float* norm_out, hipStream_t stream);

// torch.optim.Adam's non-capturable update of every row; clip (device, may be NULL = 1) is the factor on the gradients.
int launch_adam_multi(const swf_adam_tensor* rows, const int32_t* chunk_row, int n_chunks, const swf_adam_desc& d, const float* clip,
                      hipStream_t stream);

}  // namespace swf
