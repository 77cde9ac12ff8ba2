// Host-side Poseidon2 permutation for the Fiat-Shamir transcript and the proof-of-work check of the Poseidon2 configurations
// (a few hundred permutations per proof, sequential: on the CPU, as poseidon_host.h).  Same function as poseidon2.cuh and as the
// reference's Poseidon2::poseidon2 (plonky2/plonky2/src/hash/poseidon2.rs:50), written as the reference writes it.
#pragma once
#include "gl.cuh"
#include "../../include/ola_poseidon2_constants.h"

namespace ola {

static inline void h_p2_external(u64 s[12]) {
    for (int g = 0; g < 12; g += 4) {   // matmul_m4 (poseidon2.rs:176)
        const u64 t0 = gl_add(s[g], s[g + 1]), t1 = gl_add(s[g + 2], s[g + 3]);
        const u64 t2 = gl_add(t1, gl_add(s[g + 1], s[g + 1])), t3 = gl_add(t0, gl_add(s[g + 3], s[g + 3]));
        const u64 t1x4 = gl_add(gl_add(t1, t1), gl_add(t1, t1)), t0x4 = gl_add(gl_add(t0, t0), gl_add(t0, t0));
        const u64 t4 = gl_add(t3, t1x4), t5 = gl_add(t2, t0x4);
        s[g] = gl_add(t3, t5); s[g + 1] = t5; s[g + 2] = gl_add(t2, t4); s[g + 3] = t4;
    }
    for (int l = 0; l < 4; l++) {       // matmul_external (:118): + the column sums over the three groups
        const u64 st = gl_add(gl_add(s[l], s[4 + l]), s[8 + l]);
        s[l] = gl_add(s[l], st); s[4 + l] = gl_add(s[4 + l], st); s[8 + l] = gl_add(s[8 + l], st);
    }
}

static inline void h_p2_internal(u64 s[12]) {   // matmul_internal (:155): out_i = (MAT_DIAG12_M_1[i] - 1) x_i + sum(x)
    u64 sum = 0;
    for (int i = 0; i < 12; i++) sum = gl_add(sum, s[i]);
    for (int i = 0; i < 12; i++) s[i] = gl_add(gl_mul(s[i], OLA_POSEIDON2_DIAG[i]), sum);
}

static inline u64 h_p2_sbox7(u64 x) {
    const u64 x2 = gl_mul(x, x), x4 = gl_mul(x2, x2), x3 = gl_mul(x, x2);
    return gl_mul(x3, x4);
}

// any u64 in, canonical out
static inline void poseidon2_permute_host(u64 s[12]) {
    for (int i = 0; i < 12; i++) s[i] = gl_canon(s[i]);
    h_p2_external(s);
    for (int r = 0; r < 8; r++) {
        if (r == 4) {
            for (int k = 0; k < 22; k++) {
                s[0] = h_p2_sbox7(gl_add(s[0], OLA_POSEIDON2_RC_MID[k]));
                h_p2_internal(s);
            }
        }
        for (int i = 0; i < 12; i++) s[i] = h_p2_sbox7(gl_add(s[i], OLA_POSEIDON2_RC[r * 12 + i]));
        h_p2_external(s);
    }
}

}  // namespace ola
