// Shared host-side helpers of libswinfuse (gfx950 only), and the reflect-pad index maps both kernel tiers use.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/swinfuse.h"

namespace swf {

// thread-local error text behind swf_last_error_string()
char* err_buf();
int fail(int status, const char* fmt, ...);

// The workspace refusal of every entry that takes one: SWF_OK, or SWF_ERR_WORKSPACE with `who`, what was given and what is needed.
inline int need_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
    if (workspace && workspace_bytes >= need) return SWF_OK;
    return fail(SWF_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace ? workspace_bytes : (size_t)0, need);
}

inline hipStream_t as_stream(swf_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Check the launch that was just enqueued (no sync: only launch-configuration errors show up here).
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SWF_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return SWF_OK;
}

// A/B switches of the dispatch (every one selects between HIP kernels of this library; there is no CPU path).  They are
// read ONLY when SWF_DEBUG_SWITCHES=1 is set as well, so that a stray variable in a production environment — or on one rank of a
// sharded job, where it would break the bit-identity of batch shards — cannot change the kernel path.  tests/test_gpu_switches.py
// runs the main fallbacks in child processes with the opt-in set.
inline const char* debug_env(const char* name) {
    static const bool on = [] { const char* e = std::getenv("SWF_DEBUG_SWITCHES"); return e && e[0] == '1'; }();
    return on ? std::getenv(name) : nullptr;
}

// Compute units of the current device (256 if the query fails), queried once.  Inline: the tools/ probes compile kernel files
// into programs that also link the library.
inline int num_cus() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        return v;
    }();
    return n;
}

// Raise kernel K's dynamic-LDS limit to `bytes` (a launch with more than 64 KB needs it).  The attribute is set by the first
// call only (thread-safe static initialisation); every call returns the status of that attempt.
template <auto K>
int raise_lds_limit(int bytes, const char* what) {
    static const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return e == hipSuccess ? SWF_OK : fail(SWF_ERR_HIP, "hipFuncSetAttribute(%s): %s", what, hipGetErrorString(e));
}

// Index maps of 'reflect' padding (F.pad mode="reflect": the edge element is not repeated): reflect_br for a pad on the bottom /
// right edge only, reflect2 for both edges.
__device__ __forceinline__ int reflect_br(int i, int n) { return i < n ? i : 2 * n - 2 - i; }
__device__ __forceinline__ int reflect2(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// Route report of a block (swf_block_route): the branch that launches ORs its flag into the caller's code, when there is one.
inline void trace_block(int* route, int flags) { if (route) *route |= flags; }

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Bump allocator over the caller's workspace; every carve is 256-byte aligned.  A unit carves its buffers in ONE function that takes a
// Carver&; its implementation runs that function on the real workspace, its size query runs the same function on Carver::measure()
// and returns bytes(), so one byte less than the query is refused.  While measuring, floats() returns nullptr and no pointer is formed.
struct Carver {
    char* base;
    size_t cap, used;
    bool measuring;
    Carver(void* p, size_t bytes, bool measure_only = false) : base(static_cast<char*>(p)), cap(bytes), used(0), measuring(measure_only) {}
    static Carver measure() { return Carver(nullptr, 0, true); }
    float* floats(int64_t n) {
        const size_t off = align_up(used, 256);
        used = off + static_cast<size_t>(n) * sizeof(float);
        return (measuring || !base) ? nullptr : reinterpret_cast<float*>(base + off);
    }
    size_t bytes() const { return align_up(used, 256); }   // what a size query returns, and what ok() asks of a real workspace
    bool ok() const { return base != nullptr ? bytes() <= cap : used == 0; }   // no workspace is fine when nothing was carved
};

}  // namespace swf

#define SWF_TRY(expr)                      \
    do {                                   \
        int _st = (expr);                  \
        if (_st != SWF_OK) return _st;     \
    } while (0)
