// Gather / scatter of a tensor list for gfx950: the copy that puts every gradient of a model behind one collective.
//
// tensors_copy_kernel   one workgroup per 4096-element chunk of one tensor.  A segment of the flat buffer starts wherever the running sum
//                       of the sizes puts it (the model's bias tables have 225 or 169 elements), so the two addresses of a chunk are
//                       4-byte aligned and no more: the chunk is split at the DESTINATION's 16-byte boundaries into a scalar head, a body
//                       of 16-byte stores and a scalar tail.  The body's loads are 16-byte too where the source has the destination's phase,
//                       four 4-byte loads otherwise.  Each value is multiplied by `scale` and rounded once (torch's t * scale), or
//                       copied as it is.  No atomics, no synchronisation, nothing read back: capturable.
#include "kernels_flat.h"

#include <algorithm>

namespace swf {
namespace {

constexpr int kThreads = 256;

// The addresses come out of the table, so the compiler cannot tell their address space: say "global" for them.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

template <bool SCALED>
__global__ __launch_bounds__(kThreads) void tensors_copy_kernel(const swf_adam_tensor* __restrict__ rows, const int32_t* __restrict__ chunk_row,
                                                                int n_chunks, float scale) {
    const int c = blockIdx.x, tid = threadIdx.x;
    if (c >= n_chunks) return;
    const swf_adam_tensor row = rows[chunk_row[c]];
    const int64_t off = (int64_t)(c - row.first_chunk) * kAdamChunk;
    const int n = (int)std::min<int64_t>(kAdamChunk, row.numel - off);
    gf32* dst = (gf32*)(row.param + off);
    const gf32* src = row.grad ? (const gf32*)(row.grad + off) : nullptr;   // NULL: a zero segment
    auto one = [&](int i) -> float {
        if (!src) return 0.f;
        return SCALED ? src[i] * scale : src[i];
    };
    // [0, head) up to the destination's first 16-byte boundary, then nv groups of four, then the rest
    const int head = std::min(n, (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2));
    const int nv = (n - head) >> 2;
    const bool src_vec = src && (((uintptr_t)(src + head)) & 15) == 0;
    if (tid < head) dst[tid] = one(tid);
    for (int i = tid; i < nv; i += kThreads) {
        const int e = head + 4 * i;
        f32x4 v;
        if (src_vec) {
            v = *(const gf32x4*)(src + e);
            if (SCALED) v *= scale;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = one(e + k);
        }
        *(gf32x4*)(dst + e) = v;
    }
    for (int i = head + 4 * nv + tid; i < n; i += kThreads) dst[i] = one(i);
}

}  // namespace

int launch_tensors_copy(const swf_adam_tensor* rows, const int32_t* chunk_row, int n_chunks, float scale, int scaled, hipStream_t stream) {
    if (scaled)
        tensors_copy_kernel<true><<<n_chunks, kThreads, 0, stream>>>(rows, chunk_row, n_chunks, scale);
    else
        tensors_copy_kernel<false><<<n_chunks, kThreads, 0, stream>>>(rows, chunk_row, n_chunks, 1.f);
    return check_launch("tensors_copy_kernel");
}

}  // namespace swf
