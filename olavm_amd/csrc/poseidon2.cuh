// Poseidon2-Goldilocks permutation (width 12, x^7, 4 + 22 + 4 rounds) for gfx950: the Merkle hasher and challenger permutation of
// Poseidon2GoldilocksConfig / Poseidon2GoldilocksConfig2, and the proof-of-work hash of the former.
//
// Computes the same function as the reference's Poseidon2::poseidon2 (plonky2/plonky2/src/hash/poseidon2.rs:50): matmul_external
// first, 4 external rounds (constants, 12 S-boxes, matmul_external), 22 internal rounds (RC12_MID on lane 0, S-box on lane 0,
// matmul_internal), 4 external rounds.  Parameters: include/ola_poseidon2_constants.h (tools/gen_poseidon2_tables.py).
//   matmul_external (:118): matmul_m4 (:176) on each group of four, then every element gets the sum of its column position over
//       the three groups -- a matrix of small integers (row sums <= 64): evaluated on the 32-bit halves of the weak state with
//       additions and shifts only, one fold per lane (poseidon.cuh fold_halves).
//   matmul_internal (:155): out_i = d_i x_i + sum(x), d_i = MAT_DIAG12_M_1[i] - 1 as the code computes it -- twelve products by
//       constants that are the same on every lane, plus one sum.
// Same two forms as poseidon.cuh: one state per thread, and quad-cooperative (4 lanes x 3 elements) for small batches.
#pragma once
#include "gl.cuh"
#include "poseidon.cuh"
#ifdef OLA_POSEIDON2_INTERNAL_ACC3
#include "airq.cuh"
#endif
#include "../../include/ola_poseidon2_constants.h"

namespace ola {

#if defined(__HIPCC__)
__constant__ u64 c_p2_rc[96];
__constant__ u64 c_p2_mid[22];
__constant__ u64 c_p2_diag[12];
#ifdef OLA_POSEIDON2_INTERNAL_ACC3
__constant__ u64 c_p2_limbs[36];
#endif

static inline void poseidon2_upload_constants() {
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_p2_rc), OLA_POSEIDON2_RC, sizeof(c_p2_rc)));
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_p2_mid), OLA_POSEIDON2_RC_MID, sizeof(c_p2_mid)));
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_p2_diag), OLA_POSEIDON2_DIAG, sizeof(c_p2_diag)));
#ifdef OLA_POSEIDON2_INTERNAL_ACC3
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_p2_limbs), OLA_POSEIDON2_DIAG_LIMBS, sizeof(c_p2_limbs)));
#endif
}

// matmul_external on twelve un-reduced integers (the 32-bit halves of a state: inputs < 2^32, outputs < 2^38)
__device__ __forceinline__ void p2_external_int(u64 (&a)[12]) {
#pragma unroll
    for (int g = 0; g < 12; g += 4) {   // matmul_m4 (poseidon2.rs:176): t2 = t1 + 2 x1, t3 = t0 + 2 x3, t4 = t3 + 4 t1, t5 = t2 + 4 t0
        const u64 t0 = a[g] + a[g + 1], t1 = a[g + 2] + a[g + 3];
        const u64 t2 = t1 + (a[g + 1] << 1), t3 = t0 + (a[g + 3] << 1);
        const u64 t4 = t3 + (t1 << 2), t5 = t2 + (t0 << 2);
        a[g] = t3 + t5; a[g + 1] = t5; a[g + 2] = t2 + t4; a[g + 3] = t4;
    }
#pragma unroll
    for (int l = 0; l < 4; l++) {
        const u64 st = a[l] + a[4 + l] + a[8 + l];
        a[l] += st; a[4 + l] += st; a[8 + l] += st;
    }
}

// weak state -> weak state
__device__ __forceinline__ void p2_external_weak(u64 (&s)[12]) {
    u64 l[12], h[12];
#pragma unroll
    for (int i = 0; i < 12; i++) { l[i] = (u32)s[i]; h[i] = s[i] >> 32; }
    p2_external_int(l);
    p2_external_int(h);
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = fold_halves(l[i], h[i]);
}

#ifdef OLA_POSEIDON2_INTERNAL_ACC3
// c0 + c1 2^22 + c2 2^44 (below 2^109) mod p, weak (acc3_reduce without the final canonicalisation)
__device__ __forceinline__ u64 acc3_reduce_weak(const Acc3& a) {
    const unsigned __int128 v = (unsigned __int128)a.c0 + ((unsigned __int128)a.c1 << 22) + ((unsigned __int128)a.c2 << 44);
    return gl_reduce128_weak_cc((u64)v, (u64)(v >> 64));
}
#endif

// matmul_internal, weak -> weak.  The sum is canonicalised once; each lane then costs one product by its uniform multiplier.
__device__ __forceinline__ void p2_internal_weak(u64 (&s)[12]) {
    u64 sl = 0, sh = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) { sl += (u32)s[i]; sh += s[i] >> 32; }
    const u64 sum = gl_canon(fold_halves(sl, sh));
#ifdef OLA_POSEIDON2_INTERNAL_ACC3
    // Measured and NOT adopted: the multipliers as 22-bit limbs through the scalar cache (airq.cuh Acc3), the
    // accumulator started from the sum -- six v_mad_u64_u32 per lane, but one product per reduction: assembling the 109-bit sum
    // costs more than the 64x64 product of mul_weak saves.
    const Acc3 a0 = acc3_init(sum);
#pragma unroll
    for (int i = 0; i < 12; i++) {
        Acc3 a = a0;
        acc3_mad(a, s[i], c_p2_limbs[3 * i], c_p2_limbs[3 * i + 1], c_p2_limbs[3 * i + 2]);
        s[i] = acc3_reduce_weak(a);
    }
#else
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = add_weak(mul_weak(s[i], c_p2_diag[i]), sum);
#endif
}

// Poseidon2::poseidon2 (poseidon2.rs:50) on one state per thread; any u64 in, canonical out
__device__ __forceinline__ void poseidon2_permute(u64 (&s)[12]) {
    p2_external_weak(s);
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = sbox7_weak(add_weak(s[i], c_p2_rc[r * 12 + i]));
        p2_external_weak(s);
    }
#pragma unroll 1
    for (int r = 0; r < 22; r++) {
        s[0] = sbox7_weak(add_weak(s[0], c_p2_mid[r]));
        p2_internal_weak(s);
    }
#pragma unroll 1
    for (int r = 4; r < 8; r++) {
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = sbox7_weak(add_weak(s[i], c_p2_rc[r * 12 + i]));
        p2_external_weak(s);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl_canon(s[i]);
}

// ------------------------------------------------------------------------------------------------ quad-cooperative form
// Lane q = lane & 3 of a DPP quad holds elements 3q, 3q+1, 3q+2 (as poseidon.cuh poseidon_permute_quad).  The groups of four of
// matmul_external straddle the lanes, so every lane fetches the halves of all twelve elements with quad_perm broadcasts, evaluates
// the whole small-integer layer and folds its own three outputs.  matmul_internal needs only the sum: two butterfly steps of
// quad_perm rotations over the lanes' partial sums.
template <int L>
__device__ __forceinline__ u32 quad_bcast(u32 v) {
    constexpr int ctrl = L | (L << 2) | (L << 4) | (L << 6);   // every lane of the quad reads lane L
    return (u32)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xF, 0xF, false);
}
template <int ROT>
__device__ __forceinline__ u64 quad_rot64(u64 v) { return ((u64)quad_rot<ROT>((u32)(v >> 32)) << 32) | quad_rot<ROT>((u32)v); }

__device__ __forceinline__ void p2_external_quad(u64 (&x)[3], int q) {
    u64 l[12], h[12];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const u32 lk = (u32)x[k], hk = (u32)(x[k] >> 32);
        l[k] = quad_bcast<0>(lk); h[k] = quad_bcast<0>(hk);
        l[3 + k] = quad_bcast<1>(lk); h[3 + k] = quad_bcast<1>(hk);
        l[6 + k] = quad_bcast<2>(lk); h[6 + k] = quad_bcast<2>(hk);
        l[9 + k] = quad_bcast<3>(lk); h[9 + k] = quad_bcast<3>(hk);
    }
    p2_external_int(l);
    p2_external_int(h);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const u64 al = q == 0 ? l[k] : q == 1 ? l[3 + k] : q == 2 ? l[6 + k] : l[9 + k];
        const u64 ah = q == 0 ? h[k] : q == 1 ? h[3 + k] : q == 2 ? h[6 + k] : h[9 + k];
        x[k] = fold_halves(al, ah);
    }
}

__device__ __forceinline__ void p2_internal_quad(u64 (&x)[3], const u64 (&d)[3]) {
    u64 sl = (u64)(u32)x[0] + (u32)x[1] + (u32)x[2], sh = (x[0] >> 32) + (x[1] >> 32) + (x[2] >> 32);   // < 2^34 each
    sl += quad_rot64<1>(sl); sh += quad_rot64<1>(sh);
    sl += quad_rot64<2>(sl); sh += quad_rot64<2>(sh);
    const u64 sum = gl_canon(fold_halves(sl, sh));
#pragma unroll
    for (int k = 0; k < 3; k++) x[k] = add_weak(mul_weak(x[k], d[k]), sum);
}

__device__ __forceinline__ void poseidon2_permute_quad(u64 (&x)[3], int q) {
    const u64 d[3] = {c_p2_diag[3 * q], c_p2_diag[3 * q + 1], c_p2_diag[3 * q + 2]};
    p2_external_quad(x, q);
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) x[k] = sbox7_weak(add_weak(x[k], c_p2_rc[r * 12 + 3 * q + k]));
        p2_external_quad(x, q);
    }
#pragma unroll 1
    for (int r = 0; r < 22; r++) {
        const u64 t = sbox7_weak(add_weak(x[0], c_p2_mid[r]));
        x[0] = (q == 0) ? t : x[0];
        p2_internal_quad(x, d);
    }
#pragma unroll 1
    for (int r = 4; r < 8; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) x[k] = sbox7_weak(add_weak(x[k], c_p2_rc[r * 12 + 3 * q + k]));
        p2_external_quad(x, q);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) x[k] = gl_canon(x[k]);
}
#endif  // __HIPCC__

}  // namespace ola
