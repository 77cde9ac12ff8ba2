// The hashers of the GenericConfigs the library proves under, device side: one policy type per hash, and the one dispatch from an
// OLA_HASH_* value to its policy.  (The host side -- wire format, transcript, InnerHasher -- is the table in hasher_host.h.)
//
// A policy H has
//   H::leaf(word, nwords, out4)   Hasher::hash_no_pad of the words word(0) .. word(nwords - 1)  (hashing.rs:84-107, blake3.rs:203-213, keccak.rs)
//   H::node(children8, out4)      Hasher::two_to_one of two adjacent digests                    (hashing.rs:66-74, blake3.rs:215-233, keccak.rs)
//   H::BYTES                      the digest is bytes (never reduced) and the leaf's words must be canonical
//   H::Small                      the policy for nodes and for leaves of at most 128 words: H itself but for Blake3's multi-chunk form
// out4 and children8 are 16-byte aligned (digests in the heap, or alignas(16) locals).  The kernels of merkle.hip and verify.hip are
// templates over H; whether `word` canonicalises is the kernel's business and stays where each kernel had it.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/ola_gpu.h"
#include "blake3.cuh"
#include "gl.cuh"
#include "keccak.cuh"
#include "ola_error.h"
#include "poseidon.cuh"
#include "poseidon2.cuh"

namespace ola {

// the algebraic permutation of a sponge kernel
enum : int { PERM_POSEIDON = 0, PERM_POSEIDON2 = 1 };
template <int PERM>
__device__ __forceinline__ void permute12(u64 (&s)[12]) {
    if constexpr (PERM == PERM_POSEIDON2) poseidon2_permute(s);
    else poseidon_permute(s);
}
// quad-cooperative form (4 threads per state, poseidon.cuh): lane q of a quad owns sponge lanes 3q..3q+2
template <int PERM>
__device__ __forceinline__ void permute_quad(u64 (&x)[3], int q) {
    if constexpr (PERM == PERM_POSEIDON2) poseidon2_permute_quad(x, q);
    else poseidon_permute_quad(x, q);
}

__device__ __forceinline__ void store_digest(u64* __restrict__ out4, u64 d0, u64 d1, u64 d2, u64 d3) {
    ulonglong2* o = reinterpret_cast<ulonglong2*>(out4);
    o[0] = make_ulonglong2(d0, d1);
    o[1] = make_ulonglong2(d2, d3);
}

// Poseidon / Poseidon2: overwrite-mode sponge, rate 8, 4-element digest; compress = permute(l || r || 0)[0..4]
template <int PERM>
struct SpongeHash {
    static constexpr bool BYTES = false;
    static constexpr int perm = PERM;
    using Small = SpongeHash;
    template <class WordFn>
    static __device__ __forceinline__ void leaf(WordFn word, u32 nwords, u64* __restrict__ out4) {
        u64 s[12];
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = 0;
        const int n = (int)nwords;
        for (int c0 = 0; c0 < n; c0 += 8) {
            const int len = min(8, n - c0);
#pragma unroll
            for (int i = 0; i < 8; i++)
                if (i < len) s[i] = word((u32)(c0 + i));
            permute12<PERM>(s);
        }
        store_digest(out4, s[0], s[1], s[2], s[3]);
    }
    static __device__ __forceinline__ void node(const u64* __restrict__ children8, u64* __restrict__ out4) {
        const ulonglong2* ch = reinterpret_cast<const ulonglong2*>(children8);
        const ulonglong2 c0 = ch[0], c1 = ch[1], c2 = ch[2], c3 = ch[3];
        u64 s[12] = {c0.x, c0.y, c1.x, c1.y, c2.x, c2.y, c3.x, c3.y, 0, 0, 0, 0};
        permute12<PERM>(s);
        store_digest(out4, s[0], s[1], s[2], s[3]);
    }
};
// the same sponge over the lanes of a quad: x holds lane q's three sponge lanes, the digest is lanes 0..3 (x of q = 0, x[0] of q = 1)
template <int PERM, class WordFn>
__device__ __forceinline__ void sponge_quad_leaf(WordFn word, u32 nwords, u64 (&x)[3], int q) {
    x[0] = x[1] = x[2] = 0;
    for (u32 c0 = 0; c0 < nwords; c0 += 8) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const u32 e = 3 * q + k;   // sponge lane
            if (e < 8 && c0 + e < nwords) x[k] = word(c0 + e);
        }
        permute_quad<PERM>(x, q);
    }
}

// Blake3_256 of the words as little-endian bytes.  MULTI = leaves of more than one 1024-byte chunk (more than 128 elements: the
// 134-column Poseidon table); the single-chunk form needs no stack of chaining values and therefore no scratch memory.
template <bool MULTI>
struct Blake3Hash {
    static constexpr bool BYTES = true;
    using Small = Blake3Hash<false>;
    template <class WordFn>
    static __device__ __forceinline__ void leaf(WordFn word, u32 nwords, u64* __restrict__ out4) {
        u32 d[8];
        if (MULTI) b3_hash_words(word, nwords, d);
        else b3_chunk_cv(word, 0, nwords, 0, true, d);
        b3_store_digest(out4, d);
    }
    static __device__ __forceinline__ void node(const u64* __restrict__ children8, u64* __restrict__ out4) { b3_node(children8, out4); }
};

// KeccakHash<25>: the first 25 bytes of Keccak-256
struct KeccakHash {
    static constexpr bool BYTES = true;
    using Small = KeccakHash;
    template <class WordFn>
    static __device__ __forceinline__ void leaf(WordFn word, u32 nwords, u64* __restrict__ out4) {
        u64 d[4];
        keccak_hash_words(word, nwords, d);
        store_digest(out4, d[0], d[1], d[2], d[3]);
    }
    static __device__ __forceinline__ void node(const u64* __restrict__ children8, u64* __restrict__ out4) { keccak_node(children8, out4); }
};

template <class T>
struct PolicyTag { using type = T; };

// f(PolicyTag<H>) with the policy of `hasher` (the context's Hasher) for leaves of at most `leaf_words` words.  Every hasher the
// context accepts is named here: a new one is an error until it is, never a silent Poseidon.
template <class F>
static void with_hash(uint32_t hasher, size_t leaf_words, F&& f) {
    switch (hasher) {
        case OLA_HASH_POSEIDON: f(PolicyTag<SpongeHash<PERM_POSEIDON>>()); return;
        case OLA_HASH_POSEIDON2:
        case OLA_HASH_POSEIDON2_POW_POSEIDON: f(PolicyTag<SpongeHash<PERM_POSEIDON2>>()); return;
        case OLA_HASH_BLAKE3:
            if (leaf_words > (size_t)B3_CHUNK_WORDS) f(PolicyTag<Blake3Hash<true>>());
            else f(PolicyTag<Blake3Hash<false>>());
            return;
        case OLA_HASH_KECCAK: f(PolicyTag<KeccakHash>()); return;
        default: throw OlaError(OLA_E_INTERNAL, "no hash kernels for this hasher");
    }
}
// f(std::integral_constant<int, PERM>) with the permutation `hasher` names (OLA_HASH_POSEIDON or a Poseidon2 value): for the callers
// that want a permutation and no tree -- whole states, and the proof of work with the configuration's InnerHasher
template <class F>
static void with_perm(uint32_t hasher, F&& f) {
    switch (hasher) {
        case OLA_HASH_POSEIDON: f(std::integral_constant<int, PERM_POSEIDON>()); return;
        case OLA_HASH_POSEIDON2:
        case OLA_HASH_POSEIDON2_POW_POSEIDON: f(std::integral_constant<int, PERM_POSEIDON2>()); return;
        default: throw OlaError(OLA_E_INTERNAL, "no sponge permutation for this hasher");
    }
}

}  // namespace ola
