// Multi-tensor Adam step and global gradient norm for gfx950.
//
// adam_multi_kernel     one persistent grid over the chunks of every tensor of a parameter group: reads p, g, m, v and writes p, m, v
//                       once (28 bytes per element), 16-byte accesses where p, m and v of a tensor allow them (the gradient may be a
//                       4-byte-aligned view: only its loads differ, the update's bits do not).
// gradnorm_partials_kernel / gradnorm_finish_kernel
//                       sum of squares per chunk in fp64 (fixed chunking, fixed tree), then one block adds the partials in a fixed
//                       order: the norm does not depend on the grid size and is bit-reproducible.  No atomics anywhere.
//
// The arithmetic of the update is torch.optim.Adam's non-capturable single-tensor path, in its order:
//   g' = clip * g (+ weight_decay * p);  m += (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g'^2;
//   p -= step_size * m / (sqrt(v) / bc2_sqrt + eps)
// with IEEE sqrtf and division (no approximate reciprocal), step_size and bc2_sqrt per tensor from the host.
#include "kernels_optim.h"

#include <algorithm>

namespace swf {
namespace {

constexpr int kThreads = 256;
constexpr int kVecPerThread = kAdamChunk / 4 / kThreads;   // float4 per thread per array in a full chunk
static_assert(kVecPerThread * 4 * kThreads == kAdamChunk, "chunk = threads x whole float4s");

struct AdamScalars {
    float w1;        // 1 - beta1
    float beta2, w2; // beta2, 1 - beta2
    float eps, weight_decay;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamScalars& k, float clip, float step_size,
                                         float bc2_sqrt) {
    g *= clip;
    if (k.weight_decay != 0.f) g += k.weight_decay * p;
    m += (g - m) * k.w1;
    v = k.beta2 * v + k.w2 * (g * g);
    const float denom = sqrtf(v) / bc2_sqrt + k.eps;
    p -= step_size * (m / denom);
}

// The tensors' addresses come out of the table, so the compiler cannot tell their address space: say "global" for them.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
__device__ __forceinline__ f32x4 ld4(const float* p, int i) { return ((const gf32x4*)p)[i]; }
__device__ __forceinline__ void st4(float* p, int i, f32x4 x) { ((gf32x4*)p)[i] = x; }
__device__ __forceinline__ float ld1(const float* p, int i) { return ((const gf32*)p)[i]; }
__device__ __forceinline__ void st1(float* p, int i, float x) { ((gf32*)p)[i] = x; }

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

__global__ __launch_bounds__(kThreads) void adam_multi_kernel(const swf_adam_tensor* __restrict__ rows, const int32_t* __restrict__ chunk_row,
                                                              int n_chunks, AdamScalars k, const float* __restrict__ clip_ptr) {
    const int tid = threadIdx.x;
    const float clip = clip_ptr ? clip_ptr[1] : 1.f;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const swf_adam_tensor row = rows[chunk_row[c]];
        const int64_t off = (int64_t)(c - row.first_chunk) * kAdamChunk;
        const int n = (int)std::min<int64_t>(kAdamChunk, row.numel - off);
        float* __restrict__ p = row.param + off;
        const float* __restrict__ g = row.grad + off;
        float* __restrict__ m = row.exp_avg + off;
        float* __restrict__ v = row.exp_avg_sq + off;
        int done = 0;   // elements handled by the 16-byte path (chunk offsets are multiples of 16 bytes: alignment is the tensor's)
        // The gradient alone may sit at any 4-byte address (a view into a flat buffer of reduced gradients): its group of four is then
        // four 4-byte loads, and everything after the loads is the same code, so the update does not depend on the gradient's alignment.
        if (aligned16(p, p, m, v)) {
            const int nv = n >> 2;
            const bool gvec = ((uintptr_t)g & 15) == 0;
            f32x4 P[kVecPerThread], G[kVecPerThread], M[kVecPerThread], V[kVecPerThread];
#pragma unroll
            for (int j = 0; j < kVecPerThread; ++j) {
                const int i = tid + j * kThreads;
                if (i < nv) {
                    P[j] = ld4(p, i);
                    if (gvec) {
                        G[j] = ld4(g, i);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) G[j][e] = ld1(g, 4 * i + e);
                    }
                    M[j] = ld4(m, i);
                    V[j] = ld4(v, i);
                }
            }
#pragma unroll
            for (int j = 0; j < kVecPerThread; ++j) {
                const int i = tid + j * kThreads;
                if (i < nv) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float pp = P[j][e], mm = M[j][e], vv = V[j][e];
                        adam_one(pp, G[j][e], mm, vv, k, clip, row.step_size, row.bc2_sqrt);
                        P[j][e] = pp;
                        M[j][e] = mm;
                        V[j][e] = vv;
                    }
                    st4(p, i, P[j]);
                    st4(m, i, M[j]);
                    st4(v, i, V[j]);
                }
            }
            done = nv << 2;
        }
        for (int i = done + tid; i < n; i += kThreads) {   // the tail of an aligned tensor, or the whole of an unaligned one
            float pp = ld1(p, i), mm = ld1(m, i), vv = ld1(v, i);
            adam_one(pp, ld1(g, i), mm, vv, k, clip, row.step_size, row.bc2_sqrt);
            st1(p, i, pp);
            st1(m, i, mm);
            st1(v, i, vv);
        }
    }
}

// fixed tree over the block's 256 values; the result is in red[0]
__device__ __forceinline__ void block_tree_sum(double* red, int tid) {
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
}

// partials[c] = sum of g^2 over chunk c, in fp64: thread t adds its groups of four elements, then a tree
__global__ __launch_bounds__(kThreads) void gradnorm_partials_kernel(const swf_adam_tensor* __restrict__ rows,
                                                                     const int32_t* __restrict__ chunk_row, int n_chunks,
                                                                     double* __restrict__ partials) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const swf_adam_tensor row = rows[chunk_row[c]];
        const int64_t off = (int64_t)(c - row.first_chunk) * kAdamChunk;
        const int n = (int)std::min<int64_t>(kAdamChunk, row.numel - off);
        const float* __restrict__ g = row.grad + off;
        // ONE order for every alignment: thread t owns the groups of four elements t, t + 256, ...; an aligned full group comes as one
        // 16-byte load, any other element by a guarded 4-byte load (0 beyond the end), and the sums are formed the same way.
        const bool vec = ((uintptr_t)g & 15) == 0;
        const int nv = n >> 2;
        f32x4 G[kVecPerThread];
#pragma unroll
        for (int j = 0; j < kVecPerThread; ++j) {
            const int i = tid + j * kThreads;
            if (vec && i < nv) {
                G[j] = ld4(g, i);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) G[j][e] = 4 * i + e < n ? ld1(g, 4 * i + e) : 0.f;
            }
        }
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kVecPerThread; ++j)
            acc += (double)G[j].x * G[j].x + (double)G[j].y * G[j].y + (double)G[j].z * G[j].z + (double)G[j].w * G[j].w;
        red[tid] = acc;
        block_tree_sum(red, tid);
        if (tid == 0) partials[c] = red[0];
        __syncthreads();   // red is reused by the next chunk
    }
}

// out[0] = sqrt(sum of the partials), out[1] = min(1, max_norm / (out[0] + 1e-6)); one block, every thread its strided share in order
__global__ __launch_bounds__(kThreads) void gradnorm_finish_kernel(const double* __restrict__ partials, int n_chunks, float max_norm,
                                                                   float* __restrict__ out) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n_chunks; i += kThreads) acc += partials[i];
    red[tid] = acc;
    block_tree_sum(red, tid);
    if (tid == 0) {
        const float total = (float)sqrt(red[0]);
        out[0] = total;
        out[1] = fminf(1.f, max_norm / (total + 1e-6f));
    }
}

// memory-bound grid: at most 8 blocks of 256 threads per CU, grid-stride over the rest
int stream_grid(int n_chunks) { return std::max(1, std::min(n_chunks, num_cus() * 8)); }

}  // namespace

int upload_adam_table(const char* who, const void* table_host, void* table_device, int32_t n_tensors, int64_t n_chunks, hipStream_t stream,
                      AdamTable* t) {
    const AdamLayout lay = adam_layout(n_tensors, n_chunks);
    hipError_t e = hipMemcpyAsync(table_device, table_host, lay.copy_bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return fail(SWF_ERR_HIP, "%s: table copy: %s", who, hipGetErrorString(e));
    char* base = static_cast<char*>(table_device);
    t->rows = reinterpret_cast<const swf_adam_tensor*>(base);
    t->map = reinterpret_cast<const int32_t*>(base + lay.map_off);
    t->partials = reinterpret_cast<double*>(base + lay.partial_off);
    t->n_chunks = (int)n_chunks;
    return SWF_OK;
}

int launch_gradnorm(const swf_adam_tensor* rows, const int32_t* chunk_row, int n_chunks, double* partials, float max_norm,
                    float* norm_out, hipStream_t stream) {
    gradnorm_partials_kernel<<<stream_grid(n_chunks), kThreads, 0, stream>>>(rows, chunk_row, n_chunks, partials);
    SWF_TRY(check_launch("gradnorm_partials_kernel"));
    gradnorm_finish_kernel<<<1, kThreads, 0, stream>>>(partials, n_chunks, max_norm, norm_out);
    return check_launch("gradnorm_finish_kernel");
}

int launch_adam_multi(const swf_adam_tensor* rows, const int32_t* chunk_row, int n_chunks, const swf_adam_desc& d, const float* clip,
                      hipStream_t stream) {
    AdamScalars k;
    k.w1 = (float)(1.0 - d.beta1);   // the complements in double, rounded once, as torch forms them from Python floats
    k.beta2 = (float)d.beta2;
    k.w2 = (float)(1.0 - d.beta2);
    k.eps = (float)d.eps;
    k.weight_decay = (float)d.weight_decay;
    adam_multi_kernel<<<stream_grid(n_chunks), kThreads, 0, stream>>>(rows, chunk_row, n_chunks, k, clip);
    return check_launch("adam_multi_kernel");
}

}  // namespace swf
