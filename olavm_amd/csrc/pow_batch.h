// How many nonces one launch of the proof-of-work search tries (fri/prover.rs:126-148 -> pow_kernel, one nonce per thread, 256 threads
// per workgroup).  Host only, no HIP: tests/host_pow_batch_check.cpp includes it with g++.
#pragma once
#include <cstdint>

namespace ola {

enum : uint64_t {
    POW_BLOCK = 256,                              // pow_kernel's workgroup
    POW_MIN_BATCH = (uint64_t)1 << 14,
    // The largest batch: 2^23 workgroups, 2^31 threads -- below every limit a launch has (a grid's x dimension holds 2^31 - 1
    // workgroups, and a launch of 2^32 threads or more is refused by some HIP runtimes), and below the issue's bound of 2^30
    // workgroups.  It is 4 << 29, so every size up to 29 bits is what it always was, and from 30 bits on the batch stays there.
    POW_MAX_BATCH = (uint64_t)1 << 31,
};

// The expected witness is about 2^bits: a batch of 4 * 2^bits nonces holds it 98 % of the time, so the search is one launch; at
// least 2^14 nonces, and at most POW_MAX_BATCH, beyond which the search goes on batch by batch (run_pow's loop).
// Without the upper bound the workgroup count of 37 bits and more, (4 << bits) / 256 >= 2^31, did not fit the launch's 32-bit
// grid (2^31 is refused, 2^32 .. 2^34 truncate to 0): nothing ran and the loop never ended.
inline uint64_t pow_batch(uint32_t bits) {
    const uint64_t want = bits >= 29 ? (uint64_t)POW_MAX_BATCH : (uint64_t)4 << bits;
    return want < POW_MIN_BATCH ? (uint64_t)POW_MIN_BATCH : want > POW_MAX_BATCH ? (uint64_t)POW_MAX_BATCH : want;
}
// workgroups of one batch: what launch_pow_batch hands to the launch, as the 32-bit number a grid dimension is
inline uint32_t pow_batch_blocks(uint64_t count) { return (uint32_t)(count / POW_BLOCK); }

}  // namespace ola
