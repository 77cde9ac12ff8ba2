// The hashers of the GenericConfigs the library proves under (include/ola_gpu.h OLA_HASH_*), host side: one row per hasher with
// everything the host code asks about it -- the digest on the wire, the transcript's permutation, how a cap is observed, which cap
// words a verifier accepts, the InnerHasher of the proof of work, the work a leaf costs.  Host only (no HIP), like challenger_host.h
// and verify_host.h, which read it.  (The device side -- leaf and node hashing -- is the policies of hasher.cuh.)
//
// Reference (plonky2/plonky2/src): plonk/config.rs:117-161 (the configurations), iop/challenger.rs:75-84,134-153,
// hash/hash_types.rs:133-153 (BytesHash::to_vec), util/serialization.rs:89-97 (BytesHash::to_bytes).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/ola_gpu.h"
#include "blake3.cuh"
#include "gl.cuh"
#include "keccak.cuh"
#include "ola_error.h"
#include "poseidon2_host.h"
#include "poseidon_host.h"

namespace ola {

struct HasherInfo {
    bool bytes;                  // the family: true = byte hash (the digest is bytes, never reduced), false = sponge (a HashOut of four field words)
    int wire_bytes;              // bytes of a digest on the wire (BytesHash<N>::to_bytes, written as they are); 0: four canonical field words
    uint32_t inner;              // C::InnerHasher, as the OLA_HASH_* value of its permutation: Poseidon2 in Poseidon2GoldilocksConfig only
    void (*permute)(u64[12]);    // H::Permutation of Challenger<F, H>
    int cap_elements;            // GenericHashOut::to_vec: the elements a cap digest is observed as, made by cap_to_elements (at most 5)
    void (*cap_to_elements)(const u64 digest[4], u64* out);
    bool cap_canonical;          // a verifier refuses a cap word >= p
    u64 cap_word3_max;           // ... and a word 3 above this: a Keccak digest is 25 bytes, word 3 holds byte 24 only
    double (*leaf_calls)(size_t words);   // hash invocations per leaf of `words` field elements
};

namespace hasher_detail {
static inline void hashout_elements(const u64 h[4], u64* out) { for (int i = 0; i < 4; i++) out[i] = h[i]; }
static inline void b3_elements(const u64 h[4], u64* out) { u64 e[5]; b3_digest_elements(h, e); for (int i = 0; i < 5; i++) out[i] = e[i]; }
static inline void keccak_elements(const u64 h[4], u64* out) { u64 e[4]; keccak_digest_elements(h, e); for (int i = 0; i < 4; i++) out[i] = e[i]; }
// sponge permutations (rate 8)
static inline double sponge_calls(size_t words) { return (double)((words + 7) / 8); }
// Blake3 compressions: 64-byte blocks, plus the parent compressions of a multi-chunk leaf
static inline double b3_calls(size_t words) { return (double)((words * 8 + 63) / 64 + (words * 8 + 1023) / 1024 - 1); }
// Keccak-f permutations: rate 17 words, the padding always in the count
static inline double keccak_calls(size_t words) { return (double)(words / KECCAK_RATE_WORDS + 1); }
}  // namespace hasher_detail

// the row of `hasher`, or nullptr for a value that names no configuration (4 is unassigned)
inline const HasherInfo* hasher_info(uint32_t hasher) {
    using namespace hasher_detail;
    static const u64 any = ~0ull;
    //                                          bytes  wire                 inner               permute                  cap observed as       canonical  word 3  leaf calls
    static const HasherInfo poseidon        = {false, 0,                   OLA_HASH_POSEIDON,  poseidon_permute_host,   4, hashout_elements,  true,      any,    sponge_calls};
    static const HasherInfo blake3          = {true,  32,                  OLA_HASH_POSEIDON,  b3_permutation_host,     5, b3_elements,       false,     any,    b3_calls};
    static const HasherInfo poseidon2       = {false, 0,                   OLA_HASH_POSEIDON2, poseidon2_permute_host,  4, hashout_elements,  true,      any,    sponge_calls};
    static const HasherInfo poseidon2_pow_p = {false, 0,                   OLA_HASH_POSEIDON,  poseidon2_permute_host,  4, hashout_elements,  true,      any,    sponge_calls};
    static const HasherInfo keccak          = {true,  KECCAK_DIGEST_BYTES, OLA_HASH_POSEIDON,  keccak_permutation_host, 4, keccak_elements,   false,     0xFF,   keccak_calls};
    switch (hasher) {
        case OLA_HASH_POSEIDON: return &poseidon;
        case OLA_HASH_BLAKE3: return &blake3;
        case OLA_HASH_POSEIDON2: return &poseidon2;
        case OLA_HASH_POSEIDON2_POW_POSEIDON: return &poseidon2_pow_p;
        case OLA_HASH_KECCAK: return &keccak;
        default: return nullptr;
    }
}
// the row of a hasher that has been validated (a context's configuration, a transcript's)
inline const HasherInfo& hasher_row(uint32_t hasher) {
    const HasherInfo* h = hasher_info(hasher);
    if (!h) throw OlaError(OLA_E_INTERNAL, "challenger of an unknown hasher");
    return *h;
}

}  // namespace ola
