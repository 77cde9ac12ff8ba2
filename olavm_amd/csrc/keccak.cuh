// Keccak-256 for the Merkle trees and the challenger of the reference's KeccakGoldilocksConfig
// (plonky2/plonky2/src/plonk/config.rs:145-151: Hasher = KeccakHash<25>, InnerHasher = PoseidonHash).
//
// Replaces (reference, relative to plonky2/plonky2/src/hash):
//   keccak.rs      KeccakHash<25>::hash_no_pad(field slice) = first 25 bytes of keccak(its bytes)  -> keccak_hash_words (one thread per leaf)
//   keccak.rs      two_to_one = first 25 bytes of keccak(left || right), 50 bytes                   -> keccak_node (one block)
//   keccak.rs      KeccakPermutation (the challenger's "onion" over full 32-byte hashes)            -> keccak_permutation_host
//   hash_types.rs:133-153  BytesHash<25>::to_vec: a digest is observed as 4 elements (7, 7, 7, 4 bytes) -> keccak_digest_elements
// The hash function is crate keccak-hash's `keccak`, which is not part of the reference tree; this is the published algorithm
// (the Keccak reference, sections 1.2 and 2: Keccak-f[1600] on 5 x 5 lanes of 64 bits, 24 rounds of theta, rho, pi, chi, iota; sponge with
// rate 1088 bits = 17 lanes and the ORIGINAL multi-rate padding 0x01 .. 0x80 -- not SHA3-256, whose domain byte is 0x06).  Field
// elements are hashed as canonical little-endian words, for the reason blake3.cuh gives.
// A digest is 25 bytes.  In memory it keeps the heap layout of every other digest, 4 little-endian u64 words: words 0..2 are bytes
// 0..23, word 3 holds byte 24 in its low byte and zeros above it.  It is bytes, not field elements, and is never reduced.  On the
// wire it is its 25 bytes (util/serialization.rs:89-97).
//
// The state is 25 lanes in registers: every lane index below is a compile-time constant (the loops over lanes are unrolled, the
// loop over the 24 rounds is not -- only the round constant is looked up by the round number, a wave-uniform load), so nothing
// goes to scratch.  Cost on gfx950 as tools/isa_count.py counts it on tools/ubench/keccak_leaf.hip: docs/EXPERIMENTS.md
// ("Keccak-256 leaves").  A 94-column leaf is 6 blocks of 17 words against 12 Blake3 compressions or 12 Poseidon permutations.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <utility>

#include "gl.cuh"

namespace ola {

#if defined(__HIPCC__)
#define KC_HD __host__ __device__ __forceinline__
#else
#define KC_HD inline
#endif

enum : int { KECCAK_RATE_WORDS = 17, KECCAK_DIGEST_BYTES = 25 };

KC_HD u64 keccak_rotl(u64 x, int n) { return n == 0 ? x : (x << n) | (x >> (64 - n)); }
// rotation of lane x + 5y (rho) and the lane it moves to (pi): B[y, 2x + 3y] = rot(A[x, y])
KC_HD constexpr int keccak_rho(int i) {
    constexpr int R[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    return R[i];
}
KC_HD constexpr int keccak_pi(int i) { return (i / 5) + 5 * ((2 * (i % 5) + 3 * (i / 5)) % 5); }
KC_HD u64 keccak_rc(int round) {
    constexpr u64 RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull,
                            0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull,
                            0x0000000080008009ull, 0x000000008000000Aull, 0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull,
                            0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
                            0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    return RC[round];
}

template <int I>
KC_HD void keccak_rho_pi_lane(const u64 (&a)[25], const u64 (&d)[5], u64 (&b)[25]) {
    b[keccak_pi(I)] = keccak_rotl(a[I] ^ d[I % 5], keccak_rho(I));
}
template <int... I>
KC_HD void keccak_rho_pi(const u64 (&a)[25], const u64 (&d)[5], u64 (&b)[25], std::integer_sequence<int, I...>) {
    (keccak_rho_pi_lane<I>(a, d, b), ...);
}

// Keccak-f[1600]
KC_HD void keccak_f1600(u64 (&a)[25]) {
#pragma unroll 1
    for (int round = 0; round < 24; round++) {
        u64 c[5], d[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ keccak_rotl(c[(x + 1) % 5], 1);
        keccak_rho_pi(a, d, b, std::make_integer_sequence<int, 25>());
#pragma unroll
        for (int y = 0; y < 25; y += 5) {
#pragma unroll
            for (int x = 0; x < 5; x++) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
        }
        a[0] ^= keccak_rc(round);
    }
}

// Sponge over `nwords` >= 0 words delivered by `word(i)` (the caller canonicalises), padded as Keccak-256 pads a message of
// 8 * nwords bytes: 0x01 into byte 0 of word nwords, 0x80 into the last byte of that block -- one word, 0x80..01, when nwords is
// 16 mod 17, and a block of padding alone when it is 0 mod 17.  Leaves the state after the last permutation; the hash is lanes 0..3.
// Control flow depends on nwords only, which is uniform over a launch.
template <class WordFn>
KC_HD void keccak_absorb_words(WordFn word, u32 nwords, u64 (&a)[25]) {
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = 0;
    const u32 full = nwords / KECCAK_RATE_WORDS;
    for (u32 b = 0; b < full; b++) {
#pragma unroll
        for (int i = 0; i < KECCAK_RATE_WORDS; i++) a[i] ^= word(KECCAK_RATE_WORDS * b + i);
        keccak_f1600(a);
    }
    const u32 w0 = KECCAK_RATE_WORDS * full, rest = nwords - w0;   // rest < 17
#pragma unroll
    for (int i = 0; i < KECCAK_RATE_WORDS; i++) {
        u64 x = (u32)i < rest ? word(w0 + i) : ((u32)i == rest ? 1ull : 0ull);
        if (i == KECCAK_RATE_WORDS - 1) x ^= 0x8000000000000000ull;
        a[i] ^= x;
    }
    keccak_f1600(a);
}
// KeccakHash<25>::hash_no_pad: the first 25 bytes of the hash as a digest of 4 words
template <class WordFn>
KC_HD void keccak_hash_words(WordFn word, u32 nwords, u64 (&d)[4]) {
    u64 a[25];
    keccak_absorb_words(word, nwords, a);
    d[0] = a[0]; d[1] = a[1]; d[2] = a[2]; d[3] = a[3] & 0xFFull;
}

// two_to_one: digest of the 50 bytes of two digests (children8 = left, right as 4-word digests).  The right digest starts at
// byte 25, so every one of its words straddles two message words; the 0x01 of the padding lands on byte 50 = byte 2 of word 6.
KC_HD void keccak_node(const u64* __restrict__ children8, u64* __restrict__ out4) {
    const u64 l3 = children8[3] & 0xFFull, r0 = children8[4], r1 = children8[5], r2 = children8[6], r3 = children8[7] & 0xFFull;
    u64 a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = 0;
    a[0] = children8[0]; a[1] = children8[1]; a[2] = children8[2];
    a[3] = l3 | (r0 << 8);
    a[4] = (r0 >> 56) | (r1 << 8);
    a[5] = (r1 >> 56) | (r2 << 8);
    a[6] = (r2 >> 56) | (r3 << 8) | (1ull << 16);
    a[KECCAK_RATE_WORDS - 1] = 0x8000000000000000ull;
    keccak_f1600(a);
    out4[0] = a[0]; out4[1] = a[1]; out4[2] = a[2]; out4[3] = a[3] & 0xFFull;
}

// ---- host side of the transcript ----
// Keccak-256 (all 32 bytes, as 4 words) of `nwords` little-endian words
static inline void keccak256_words_host(const u64* words, u32 nwords, u64 out4[4]) {
    u64 a[25];
    keccak_absorb_words([&](u32 i) { return words[i]; }, nwords, a);
    for (int i = 0; i < 4; i++) out4[i] = a[i];
}
// the selection rule of KeccakPermutation::permute over the stream of hash words h1 || h2 || ...: words >= p are dropped, the first
// twelve survivors are the new state.  `next()` yields the stream's next word.
template <class NextFn>
static inline void keccak_onion_collect(NextFn next, u64 state[12]) {
    for (int got = 0; got < 12;) {
        const u64 w = next();
        if (w < GL_P) state[got++] = w;
    }
}
// KeccakPermutation::permute (keccak.rs): h1 = H(96 bytes of the state), h_{k+1} = H(all 32 bytes of h_k), computed as they are needed
static inline void keccak_permutation_host(u64 state[12]) {
    u64 cur[12], h[4];
    for (int i = 0; i < 12; i++) cur[i] = gl_canon(state[i]);
    u32 nwords = 12;
    int at = 4;
    keccak_onion_collect([&]() {
        if (at == 4) {
            keccak256_words_host(cur, nwords, h);
            for (int i = 0; i < 4; i++) cur[i] = h[i];
            nwords = 4; at = 0;
        }
        return h[at++];
    }, state);
}
// BytesHash<25>::to_vec (hash_types.rs:142-152): bytes 0-6, 7-13, 14-20 and 21-24, each little-endian
static inline void keccak_digest_elements(const u64 h[4], u64 out[4]) {
    uint8_t b[KECCAK_DIGEST_BYTES];
    for (int k = 0; k < KECCAK_DIGEST_BYTES; k++) b[k] = (uint8_t)(h[k / 8] >> (8 * (k % 8)));
    for (int c = 0; c < 4; c++) {
        u64 x = 0;
        for (int k = 0; k < 7 && 7 * c + k < KECCAK_DIGEST_BYTES; k++) x |= (u64)b[7 * c + k] << (8 * k);
        out[c] = x;
    }
}

}  // namespace ola
