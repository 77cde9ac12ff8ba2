// Host-side Fiat-Shamir challenger (plonky2/plonky2/src/iop/challenger.rs:36-162): a few hundred permutations per proof, strictly
// sequential, so it stays on the CPU.  Host only (no HIP): the prover (fri.hip, stark.hip) and the verifier's host stage
// (verify_host.h) replay the same transcript with it.
#pragma once
#include <cstring>

#include "../../include/ola_gpu.h"
#include "blake3.cuh"
#include "gl.cuh"
#include "keccak.cuh"
#include "ola_error.h"
#include "poseidon2_host.h"
#include "poseidon_host.h"

namespace ola {

// bytes of a digest on the wire where the Hasher's digest is bytes (BytesHash<N>::to_bytes, util/serialization.rs:89-97: Blake3_256<32>,
// KeccakHash<25>), written as they are and never reduced; 0 for a HashOut, which is four canonical field words
inline int digest_wire_bytes(uint32_t hasher) { return hasher == OLA_HASH_BLAKE3 ? 32 : hasher == OLA_HASH_KECCAK ? KECCAK_DIGEST_BYTES : 0; }

// ------------------------------------------------------------------------------------------------ challenger
inline void challenger_duplex(OlaChallenger& ch) {
    for (uint32_t i = 0; i < ch.input_len; i++) ch.sponge_state[i] = ch.input_buffer[i];
    ch.input_len = 0;
    u64 s[12];
    for (int i = 0; i < 12; i++) s[i] = ch.sponge_state[i];
    switch (ch.hasher) {                                         // H::Permutation of Challenger<F, H> (challenger.rs:134-153)
        case OLA_HASH_POSEIDON: poseidon_permute_host(s); break;
        case OLA_HASH_BLAKE3: b3_permutation_host(s); break;
        case OLA_HASH_KECCAK: keccak_permutation_host(s); break;
        case OLA_HASH_POSEIDON2:
        case OLA_HASH_POSEIDON2_POW_POSEIDON: poseidon2_permute_host(s); break;
        default: throw OlaError(OLA_E_INTERNAL, "challenger of an unknown hasher");
    }
    for (int i = 0; i < 12; i++) ch.sponge_state[i] = s[i];
    for (int i = 0; i < 8; i++) ch.output_buffer[i] = s[i];
    ch.output_len = 8;
}
inline void challenger_observe(OlaChallenger& ch, const u64* e, size_t n) {
    for (size_t i = 0; i < n; i++) {
        ch.output_len = 0;
        ch.input_buffer[ch.input_len++] = gl_canon(e[i]);
        if (ch.input_len == 8) challenger_duplex(ch);
    }
}
// observe_cap (challenger.rs:75-84): GenericHashOut::to_vec of every digest
inline void challenger_observe_cap(OlaChallenger& ch, const u64* digests, size_t n) {
    // HashOut (Poseidon, Poseidon2): its four elements; Blake3's 32 bytes: five elements of 7 bytes (b3_digest_elements); Keccak's 25
    // bytes: four elements of 7, 7, 7 and 4 bytes (keccak_digest_elements)
    if (ch.hasher == OLA_HASH_KECCAK) {
        for (size_t i = 0; i < n; i++) {
            u64 e[4];
            keccak_digest_elements(digests + 4 * i, e);
            challenger_observe(ch, e, 4);
        }
        return;
    }
    if (ch.hasher != OLA_HASH_BLAKE3) { challenger_observe(ch, digests, 4 * n); return; }
    for (size_t i = 0; i < n; i++) {
        u64 e[5];
        b3_digest_elements(digests + 4 * i, e);
        challenger_observe(ch, e, 5);
    }
}
inline void challenger_init(OlaChallenger& ch, uint32_t hasher) {
    memset(&ch, 0, sizeof(ch));
    ch.hasher = hasher;
}
inline u64 challenger_get(OlaChallenger& ch) {
    if (ch.input_len != 0 || ch.output_len == 0) challenger_duplex(ch);
    return ch.output_buffer[--ch.output_len];
}
inline void challenger_compact(OlaChallenger& ch) {
    if (ch.input_len != 0) challenger_duplex(ch);
    ch.output_len = 0;
}
inline Ext2 challenger_get_ext(OlaChallenger& ch) {
    const u64 a = challenger_get(ch);
    const u64 b = challenger_get(ch);
    return ext_make(a, b);
}
inline void challenger_observe_ext(OlaChallenger& ch, Ext2 e) {
    u64 v[2] = {e.a, e.b};
    challenger_observe(ch, v, 2);
}

}  // namespace ola
