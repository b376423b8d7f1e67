// Device helpers of the fast-tier kernels, defined here and nowhere else: vector types, 32x32x16 MFMA wrappers on 16-byte
// operand fragments, split-bf16 / f16 packing of accumulator registers, the lane-half exchange, wave-uniform pointers, the fast
// ELU and the V^T key order.  See kernels_win24.hip for the layout conventions (rho order, lane (column, half)).
#pragma once
#include <hip/hip_runtime.h>

namespace swf {
namespace wf {

using bf16 = __bf16;
using f16 = _Float16;
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef f16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

// row of accumulator register i in lane half hf (C/D map of the 32x32 MFMAs) == k index of element i & 7 of k-step i >> 3
__host__ __device__ constexpr int rho(int i, int hf) { return (i & 3) + 8 * (i >> 2) + 4 * hf; }

__device__ __forceinline__ f32x16 mfma_bf16(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_f16(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// P.V of ONE head on the 16x16x32 shape (levels 0 / 1: a head's V rows are 4 / 8 of the 32 virtual channels of a V^T image, so
// the 32-row product of the 32x32x16 shape is 7/8 resp. 3/4 another head's V times this head's P).  16 cycles against 32.
//   B = the P fragment exactly as pack8_f16 leaves it: lane l is column n = l & 15 and k-group kg = l >> 4 = 2 hf + qh, where
//       qh is bit 4 of the lane's QUERY — lanes with qh = 1 hold queries 16..31, not a second k-group of queries 0..15.
//   A = a per-lane read of the V^T image: row m = l & 15 = 4 g + c takes, for k-group kg, the image slot of lane half kg >> 1
//       when (kg & 1) == (g & 1) and 16 bytes of zeros otherwise (pv_match), so row group g sums the keys of both lane halves
//       against the queries of half g & 1 only.
//   D: register j of lane l = row 4 (l >> 4) + j, column l & 15, i.e. row group g = l >> 4 = 2 hf + qh: the lane receives rows
//       4 (g >> 1) .. +3 of ITS OWN query (16 qh + n = l & 31) — at level 0 both lane halves get the head's four rows.
//       (kernels_win24.hip: pv_src24), at level 1 lane half hf the rows 4 hf .. +3 of the head's eight (kernels_win48.hip: pv_src48).
__device__ __forceinline__ f32x4 mfma16_f16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ bool pv_match(int lane) { return ((lane >> 4) & 1) == ((lane >> 2) & 1); }
// The lanes that do not match read zeros: a 4 KB LDS region filled once per launch.  Their base sits 128 bytes into it, so that the
// one address they share never falls into the banks of the 64-byte run (level 1: the two adjacent runs) that the matching lanes of
// the same 16-lane group read; image and zero region are 256-byte aligned.  The head / pv-step offsets are instruction immediates
// added to either base (at most 3 * 1024 + 7 * 64 at level 0, 3 * 1024 + 3 * 128 at level 1).
constexpr int kPvZeroBytes = 4096, kPvZeroBase = 128;
static_assert(kPvZeroBase + 3 * 1024 + 7 * 64 + 16 <= kPvZeroBytes, "zero region covers every immediate");
template <int NTHREADS>
__device__ __forceinline__ void pv_fill_zeros(char* zreg, int tid) {
    for (int i = tid; i < kPvZeroBytes / 16; i += NTHREADS) reinterpret_cast<u32x4*>(zreg)[i] = u32x4{0u, 0u, 0u, 0u};
}

// acc += a . b over one 16-deep k-step with split-bf16 operands (a = a_hi + a_lo, b = b_hi + b_lo): three MFMAs, small cross
// terms first so they are not absorbed by the large hi.hi partial sums
__device__ __forceinline__ f32x16 mma3(u32x4 ahi, u32x4 alo, u32x4 bhi, u32x4 blo, f32x16 acc) {
    acc = mfma_bf16(alo, bhi, acc);
    acc = mfma_bf16(ahi, blo, acc);
    acc = mfma_bf16(ahi, bhi, acc);
    return acc;
}
// 8 fp32 values -> one k-step fragment in split-bf16 (hi = bf16(v), lo = bf16(v - hi))
__device__ __forceinline__ void split8(const float* v, u32x4& hi, u32x4& lo) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const bf16x2 h = {(bf16)v[2 * p], (bf16)v[2 * p + 1]};
        const unsigned hu = __builtin_bit_cast(unsigned, h);
        const float h0 = __builtin_bit_cast(float, hu << 16), h1 = __builtin_bit_cast(float, hu & 0xffff0000u);
        const bf16x2 l = {(bf16)(v[2 * p] - h0), (bf16)(v[2 * p + 1] - h1)};
        hi[p] = hu;
        lo[p] = __builtin_bit_cast(unsigned, l);
    }
}
// 4 fp32 values -> split-bf16 hi / lo vectors (the plane formats of the deep-level GEMMs)
__device__ __forceinline__ void split4(const float4 v, bf16x4& hi, bf16x4& lo) {
    const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        hi[i] = (bf16)f[i];
        lo[i] = (bf16)(f[i] - (float)hi[i]);
    }
}
__device__ __forceinline__ u32x4 pack8_f16(const float* v) {
    u32x4 o;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const f16x2 h = {(f16)v[2 * p], (f16)v[2 * p + 1]};   // v_cvt_pk_f16_f32, round to nearest even
        o[p] = __builtin_bit_cast(unsigned, h);
    }
    return o;
}
// a = the value of lanes 0..31 (in every lane), b = the value of lanes 32..63.  v_permlane32_swap exchanges the upper half of
// its first operand with the lower half of its second (inline asm: hipcc 7.2 folds the builtin's second result into the
// first; the s_nop covers the VALU-write -> permlane hazard)
__device__ __forceinline__ void halves(float v, float& a, float& b) {
    a = v;
    b = v;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float sum_halves(float v) { float a, b; halves(v, a, b); return a + b; }
__device__ __forceinline__ float max_halves(float v) { float a, b; halves(v, a, b); return __builtin_fmaxf(a, b); }
// max of three; with -fno-honor-nans hipcc folds this into one v_max3_f32 (and drops the canonicalising v_max it would otherwise
// put in front of fmaxf on MFMA outputs).  NOT inline asm: an asm statement that reads an MFMA result gets none of the
// MFMA->VALU wait states and reads stale registers.
__device__ __forceinline__ float max3f(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

// ELU(alpha = 1) for the fast tier: exp(v) - 1 through v_exp_f32.  Near 0 the subtraction cancels, leaving an ABSOLUTE error of
// ~1e-7 whatever |v| is.  That is four orders below the tier's error budget ONLY while fc1's outputs and fc2's weights are of
// order 1: fc2 multiplies it.  Measured (DESIGN "Operand magnitude", tests/test_gpu_range.py; elu_exp2 below behaves the same):
// with fc1 x 2^-12 and fc2 x 2^12 the ELU adds 2 .. 15 % to a block's rel-L2, with 2^-16 / 2^16 it is the whole error, 3.5 .. 11x
// the tier's formats (5e-4 .. 8e-4 rel-L2, max-rel at the 1e-3 gate); the crossing lies between the two.  The exact tier keeps
// expm1f.
__device__ __forceinline__ float elu_fast(float v) { return v > 0.f ? v : __builtin_amdgcn_exp2f(v * kLog2e) - 1.0f; }

// Position of key `tok` (0..63) inside a V^T row, the order in which the S^T accumulators hold the keys (a layout the writer of a
// V^T image and the P.V MFMAs must agree on): the 8 halves a lane needs for k-step s of key tile T sit contiguously.  Register
// 8s+e of lane half h is key row 32T + 16s + 8(e>>2) + 4h + (e&3) (C/D map of the 32x32 MFMA), so pos = 32T + 16s + 8h + e.
// For tok = 4a .. 4a+3 the positions are consecutive (only e&3 changes): one 8-byte store.
__device__ __forceinline__ int vt_pos(int tok) {
    const int k16 = tok & 15;
    const int e = ((k16 >> 3) << 2) | (k16 & 3);
    const int h = (k16 >> 2) & 1;
    return (tok & 48) | (h << 3) | e;
}

// A pointer that is the same in every lane of the wave but derived from the wave index: made provably uniform so that hipcc
// keeps it in SGPRs and addresses fragments as (scalar base + lane offset + immediate) instead of holding a 64-bit per-lane
// address per fragment group in VGPRs across the window loop.
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}


// Copy the fp32 vector sections of the two streams' packed images (n4 16-byte groups each) into LDS with every load of a thread
// issued before its first store (the obvious strided loop "lvec[i] = src[i]" runs one dependent global round trip per iteration;
// worth 0.7 us of a 48-us level-1 launch).
template <int N4, int NTHREADS>
__device__ __forceinline__ void fill_vectors(float* lvec, const char* vec0, const char* vec1, int tid) {
    constexpr int PER = (2 * N4 + NTHREADS - 1) / NTHREADS;
    f32x4 tmp[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int idx = tid + NTHREADS * k;
        if (idx < 2 * N4) tmp[k] = reinterpret_cast<const f32x4*>(idx < N4 ? vec0 : vec1)[idx < N4 ? idx : idx - N4];
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int idx = tid + NTHREADS * k;
        if (idx < 2 * N4) reinterpret_cast<f32x4*>(lvec)[idx] = tmp[k];
    }
}

// ---- block stages that are the same at every level of the register-resident block kernels (kernels_win24 / 48 / 96.hip) ----

// One hidden tile of the MLP: ELU(alpha = 1) in exp2 units.  The packed fc1 weights carry log2(e) (acc = u = v log2 e) and the
// packed fc2 weights ln 2, so the kernel needs h' = ELU(v) log2(e) = u for u > 0, L = log2(e) (2^u - 1) otherwise.  u <= L
// everywhere (convexity) and L <= 0 exactly when u <= 0, so h' is the median of (u, L, 0): 3 instructions per hidden
// activation (exp, fma, med3) instead of multiply, exp, add, compare, select.
__device__ __forceinline__ float elu_exp2(float u) {
    const float L = __builtin_fmaf(__builtin_amdgcn_exp2f(u), kLog2e, -kLog2e);
    return __builtin_amdgcn_fmed3f(u, L, 0.f);
}
__device__ __forceinline__ void elu_tile(const f32x16& acc, float (&e)[16]) {   // level 0: the fc1 bias rides on a k slot
#pragma unroll
    for (int i = 0; i < 16; ++i) e[i] = elu_exp2(acc[i]);
}
__device__ __forceinline__ void elu_tile(const f32x16& acc, const float* b1, float (&e)[16]) {   // b1: the tile's 16 fc1 biases of this lane half
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 b = *reinterpret_cast<const float4*>(b1 + 4 * g);
        const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) e[4 * g + j] = elu_exp2(acc[4 * g + j] + bb[j]);
    }
}

// Column seam of a shifted 16x16 window (last window column), on the two bias tiles of a 64-key chunk: key column (register
// bit 2) and query column (bit 3 of r = lane & 31) on different sides of column 8 -> -inf
__device__ __forceinline__ void col_seam16(f32x16 (&bias)[2], int r) {
    const bool qhi = (r & 8) != 0;
    const float pen_lo = qhi ? -INFINITY : 0.f, pen_hi = qhi ? 0.f : -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float pen = ((i >> 2) & 1) ? pen_hi : pen_lo;
        bias[0][i] += pen; bias[1][i] += pen;
    }
}

// Two consecutive S^T bias tiles of the [tile][reg/4 4][lane 64][4] fp32 section (levels 1 and 2) that starts at byte p_bias
// of the packed image behind wrs; tile0 is wave-uniform, loff = lane * 16
__device__ __forceinline__ void load_bias_tiles(const __amdgpu_buffer_rsrc_t& wrs, unsigned loff, int p_bias, int tile0, f32x16 (&bias)[2]) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, loff, p_bias + ((tile0 + kt) * 4 + a) * 1024, 0));
            bias[kt][4 * a] = v.x; bias[kt][4 * a + 1] = v.y; bias[kt][4 * a + 2] = v.z; bias[kt][4 * a + 3] = v.w;
        }
}

// Tail of a block kernel: L2 warm-up of the next block's packed weights (cold since the previous forward; see
// kernels_window.hip), called when args.warm[0] is set.  Args = WinArgs (warm, warm_bytes; B and out only keep the loads alive).
template <int NTHREADS, class Args>
__device__ __forceinline__ void warm_next_block(const Args& args, int tid) {
    const int nsl = max(1, (int)gridDim.x / 8), sl = ((int)blockIdx.x / 8) % nsl;
    const int lines = (args.warm_bytes + 127) / 128;
    const int per = (lines + nsl - 1) / nsl, l0 = sl * per, l1 = min(lines, l0 + per);
    unsigned acc = 0;
    for (int s2 = 0; s2 < 2; ++s2)
        for (int l = l0 + tid; l < l1; l += NTHREADS) acc ^= *reinterpret_cast<const unsigned*>(args.warm[s2] + (size_t)l * 128);
    if (acc == 0x9e3779b9u && args.B < 0) args.out[0][0] = 0.f;   // never true: keeps the loads alive
}

}  // namespace wf
}  // namespace swf

// Compiler-only barrier, no instruction: the loop-invariant weight fragment loads must not be hoisted out of the window loop (or
// to the top of an iteration), where they would spill.
#define SWF_WF_FENCE() asm volatile("" ::: "memory")
