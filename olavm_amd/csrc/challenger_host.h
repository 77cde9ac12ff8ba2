// Host-side Fiat-Shamir challenger (plonky2/plonky2/src/iop/challenger.rs:36-162): a few hundred permutations per proof, strictly
// sequential, so it stays on the CPU.  Host only (no HIP): the prover (fri.hip, stark.hip) and the verifier's host stage
// (verify_host.h) replay the same transcript with it.
#pragma once
#include <cstring>

#include "../../include/ola_gpu.h"
#include "gl.cuh"
#include "hasher_host.h"
#include "ola_error.h"

namespace ola {

// bytes of a digest on the wire where the Hasher's digest is bytes (BytesHash<N>::to_bytes, util/serialization.rs:89-97: Blake3_256<32>,
// KeccakHash<25>), written as they are and never reduced; 0 for a HashOut, which is four canonical field words
inline int digest_wire_bytes(uint32_t hasher) { return hasher_row(hasher).wire_bytes; }

// ------------------------------------------------------------------------------------------------ challenger
inline void challenger_duplex(OlaChallenger& ch) {
    for (uint32_t i = 0; i < ch.input_len; i++) ch.sponge_state[i] = ch.input_buffer[i];
    ch.input_len = 0;
    u64 s[12];
    for (int i = 0; i < 12; i++) s[i] = ch.sponge_state[i];
    hasher_row(ch.hasher).permute(s);                           // H::Permutation of Challenger<F, H> (challenger.rs:134-153)
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
// observe_cap (challenger.rs:75-84): GenericHashOut::to_vec of every digest -- a HashOut's four elements, Blake3's 32 bytes as five
// elements of 7 bytes, Keccak's 25 bytes as four elements of 7, 7, 7 and 4 bytes
inline void challenger_observe_cap(OlaChallenger& ch, const u64* digests, size_t n) {
    const HasherInfo& h = hasher_row(ch.hasher);
    for (size_t i = 0; i < n; i++) {
        u64 e[5];
        h.cap_to_elements(digests + 4 * i, e);
        challenger_observe(ch, e, (size_t)h.cap_elements);
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
