// Device-side generation of lookup-argument columns, and the radix sort and prefix sum that check.hip borrows (lookup.hip, its own
// translation unit).  The table generators that end in a batch of permuted_cols are tablegen.h / tablegen.hip.
#pragma once
#include <cstddef>
#include <cstdint>

#include "dev_buf.h"
#include "device_ctx.h"
#include "gl.cuh"

namespace ola {

// permuted_cols (circuits/src/stark/lookup.rs:68-132): all four pointers are device memory of n words; inputs / table may
// hold non-canonical words.  permuted_inputs = the inputs sorted (canonical), permuted_table as the reference builds it.
void permuted_cols_dev(DeviceCtx* ctx, const u64* inputs, const u64* table, size_t n, u64* permuted_inputs, u64* permuted_table);

// The same for a batch of pairs of one height n: tables[0 .. n_tables) are the table columns, pair p looks into
// tables[pairs[p].table].  A table column that several pairs share (the same pointer) is canonicalised and sorted once; the
// classification, scans, bracket matching and fill run over all pairs together, one launch each.  permuted_cols_dev is the
// batch of one.
struct PermutedPair {
    const u64* inputs;
    u32 table;
    u64* permuted_inputs;
    u64* permuted_table;
};
void permuted_cols_batch_dev(DeviceCtx* ctx, size_t n, const u64* const* tables, size_t n_tables, const PermutedPair* pairs, size_t n_pairs);

// The radix sort and the prefix sum of this unit for a caller outside it (ola_check_lookup, check.hip), in the shape of
// rocprim_ops.h: sized once, temporary storage from the caller's DevBuf, any number of runs, everything enqueued on `stream` and
// nothing synchronises.  SortPairsU64: one stable pass over n (64-bit key, 32-bit payload) pairs over all 64 key bits.
// ExclusiveSumU32: the exclusive sum of n <= max_n 32-bit words.  n >= 1.
struct SortPairsU64 {
    size_t n, bytes = 0;
    void* tmp = nullptr;
    SortPairsU64(DevBuf& mem, size_t n);
    void run(hipStream_t stream, const u64* keys_in, u64* keys_out, const u32* payload_in, u32* payload_out);
};
struct ExclusiveSumU32 {
    size_t bytes = 0;
    void* tmp = nullptr;
    ExclusiveSumU32(DevBuf& mem, size_t max_n);
    void run(hipStream_t stream, const u32* in, u32* out, size_t n);
};

}  // namespace ola
