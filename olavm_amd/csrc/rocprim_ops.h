// What the two rocPRIM units (lookup.hip, tablegen.hip) share and nobody else includes: the radix sorts and scans, each an object
// that is sized once for a length, takes its temporary storage from the caller's DevBuf and then runs any number of times on the
// stream (everything of a call runs on one stream, so its runs share that storage).  Internal linkage, like the rest of those units'
// helpers; the two that check.hip needs are declared in lookup.h and defined in lookup.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "dev_buf.h"
#include "gl.cuh"

namespace ola {

namespace {

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }
inline u32 bit_length(u64 v) { u32 b = 0; while (v) { b++; v >>= 1; } return b; }

// n 64-bit keys, all bits
struct SortU64 {
    size_t n, bytes = 0;
    void* tmp = nullptr;
    SortU64(DevBuf& mem, size_t n_) : n(n_) {
        HIP_CHECK(rocprim::radix_sort_keys(nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, n, 0, 64, mem.ctx->stream));
        tmp = mem.alloc<unsigned char>(bytes);
    }
    void run(hipStream_t stream, const u64* in, u64* out) { HIP_CHECK(rocprim::radix_sort_keys(tmp, bytes, in, out, n, 0, 64, stream)); }
};

// n (key, 32-bit payload) pairs by the low `bits` <= max_bits of the key; stable: equal keys keep the order of their payloads.  The
// length is 32 bits wide on purpose: rocPRIM instantiates its sort on the type of the size, and every length here is below 2^32.
template <typename K>
struct SortPairs {
    u32 n;
    size_t bytes = 0;
    void* tmp = nullptr;
    SortPairs(DevBuf& mem, u32 n_, u32 max_bits) : n(n_) {
        HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, (K*)nullptr, (K*)nullptr, (u32*)nullptr, (u32*)nullptr, n, 0, max_bits, mem.ctx->stream));
        tmp = mem.alloc<unsigned char>(bytes);
    }
    void run(hipStream_t stream, K* keys_in, K* keys_out, u32* payload_in, u32* payload_out, u32 bits) {
        HIP_CHECK(rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, payload_in, payload_out, n, 0, bits, stream));
    }
};

// exclusive sums of at most max_n values of T
template <typename T>
struct ExclusiveSum {
    size_t bytes = 0;
    void* tmp = nullptr;
    ExclusiveSum(DevBuf& mem, size_t max_n) {
        HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, (const T*)nullptr, (T*)nullptr, T(0), max_n, rocprim::plus<T>(), mem.ctx->stream));
        tmp = mem.alloc<unsigned char>(bytes);
    }
    void run(hipStream_t stream, const T* in, T* out, size_t n) { HIP_CHECK(rocprim::exclusive_scan(tmp, bytes, in, out, T(0), n, rocprim::plus<T>(), stream)); }
};

// inclusive scan of n values of T that starts again wherever the 32-bit key changes
// (sized with null pointers: rocPRIM then assumes that keys and output overlap and asks for its larger amount)
template <typename T>
struct ScanInclusiveByKey {
    size_t n, bytes = 0;
    void* tmp = nullptr;
    ScanInclusiveByKey(DevBuf& mem, size_t n_) : n(n_) {
        HIP_CHECK(rocprim::inclusive_scan_by_key(nullptr, bytes, (const u32*)nullptr, (const T*)nullptr, (T*)nullptr, n, rocprim::plus<T>(),
                                                 rocprim::equal_to<u32>(), mem.ctx->stream));
        tmp = mem.alloc<unsigned char>(bytes);
    }
    template <typename Op>
    void run(hipStream_t stream, const u32* keys, const T* in, T* out, Op op) {
        HIP_CHECK(rocprim::inclusive_scan_by_key(tmp, bytes, keys, in, out, n, op, rocprim::equal_to<u32>(), stream));
    }
};

}  // namespace

}  // namespace ola
