// What the two rocPRIM units (lookup.hip, tablegen.hip) share and nobody else includes: work space that goes back to the
// context's pool when a call ends, and the radix sort and scans with their temporary storage taken from it.  Internal linkage,
// like the rest of those units' helpers.
#pragma once
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "device_ctx.h"
#include "gl.cuh"

namespace ola {

namespace {

struct Scratch {
    DeviceCtx* ctx;
    std::vector<void*> ptrs;
    explicit Scratch(DeviceCtx* c) : ctx(c) {}
    template <typename T>
    T* alloc(size_t elems) {
        void* p = ctx->alloc(elems * sizeof(T));
        ptrs.push_back(p);
        return (T*)p;
    }
    ~Scratch() {
        (void)hipStreamSynchronize(ctx->stream);
        for (void* p : ptrs) ctx->free(p);
    }
};

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

// radix sorts of one length share their temporary storage (everything runs on one stream)
struct SortU64 {
    size_t n, bytes = 0;
    void* tmp = nullptr;
    SortU64(Scratch& mem, hipStream_t stream, size_t n_) : n(n_) {
        HIP_CHECK(rocprim::radix_sort_keys(nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, n, 0, 64, stream));
        tmp = mem.alloc<unsigned char>(bytes);
    }
    void run(hipStream_t stream, const u64* in, u64* out) { HIP_CHECK(rocprim::radix_sort_keys(tmp, bytes, in, out, n, 0, 64, stream)); }
};

template <typename T, typename Op>
void scan_exclusive(Scratch& mem, hipStream_t stream, const T* in, T* out, T init, size_t n, Op op) {
    size_t bytes = 0;
    HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, out, init, n, op, stream));
    void* tmp = mem.alloc<unsigned char>(bytes);
    HIP_CHECK(rocprim::exclusive_scan(tmp, bytes, in, out, init, n, op, stream));
}
// inclusive scan that starts again wherever the key changes
template <typename T, typename Op>
void scan_inclusive_by_key(Scratch& mem, hipStream_t stream, const u32* keys, const T* in, T* out, size_t n, Op op) {
    size_t bytes = 0;
    HIP_CHECK(rocprim::inclusive_scan_by_key(nullptr, bytes, keys, in, out, n, op, rocprim::equal_to<u32>(), stream));
    void* tmp = mem.alloc<unsigned char>(bytes);
    HIP_CHECK(rocprim::inclusive_scan_by_key(tmp, bytes, keys, in, out, n, op, rocprim::equal_to<u32>(), stream));
}

inline u32 bit_length(u64 v) { u32 b = 0; while (v) { b++; v >>= 1; } return b; }

}  // namespace

}  // namespace ola
