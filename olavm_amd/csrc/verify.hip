// Device stage of the verifier (ola_verify_all_proof / ola_verify_opening): the Merkle paths and the FRI algebra of a proof, over the
// flat image the host stage wrote (verify_host.h: table headers, challenges, caps, opened rows, sibling lists, layer evaluations, then
// the two job lists in structure-of-arrays form).
//
// Replaces (reference paths relative to /root/reference/plonky2/plonky2/src):
//   hash/merkle_proofs.rs:52-80   verify_merkle_proof_to_cap       -> merkle_paths_check_kernel, one job per thread
//   fri/verifier.rs:109-151       fri_combine_initial              -> fri_query_check_kernel, one (table, query) per thread
//   fri/verifier.rs:19-45         compute_evaluation (barycentric interpolation on the layer's coset, field/src/interpolation.rs:31-66)
//   fri/verifier.rs:153-232       fri_verifier_query_round: consistency per layer, the final polynomial
// One upload, two launches, one read-back of flags per call, whatever the number of tables, queries and layers.  Both kernels are
// short and latency-bound (a 12-table proof is about 1 700 paths and 336 queries): one wave per workgroup so that the jobs spread
// over the CUs, job words read at consecutive addresses by consecutive lanes, Merkle jobs ordered so that a wave's lanes share
// leaf length and depth.  Every offset a job carries is checked against the size of the image before it is used.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "../../include/ola_gpu.h"
#include "device_ctx.h"
#include "gl.cuh"
#include "hasher.cuh"
#include "verify_host.h"

namespace ola {

// verify_merkle_proof_to_cap: hash the leaf, walk the siblings by the index bits, compare with cap[index >> depth].
// data_words: the part of the image the jobs may point into (the job lists lie behind it).
// H: the hash policy (hasher.cuh); the leaf's words are hashed as they lie in the image (the host stage read them as canonical words).
template <class H>
__global__ __launch_bounds__(64) void merkle_paths_check_kernel(const u64* __restrict__ image, size_t data_words, size_t jobs_off, u32 n_jobs,
                                                                u32* __restrict__ flags) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    const u64* w = image + jobs_off + j;
    const size_t n = n_jobs;
    const u64 leaf_off = w[vfy::MJ_LEAF_OFF * n], sib_off = w[vfy::MJ_SIB_OFF * n], cap_off = w[vfy::MJ_CAP_OFF * n];
    const u64 len_depth = w[vfy::MJ_LEN_DEPTH * n], cap_len = w[vfy::MJ_CAP_LEN * n];
    u64 index = w[vfy::MJ_INDEX * n];
    const u32 len = (u32)len_depth, depth = (u32)(len_depth >> 32);
    if (len == 0 || len > 4096u || depth > 64u || leaf_off > data_words || len > data_words - leaf_off || sib_off > data_words ||
        4 * (u64)depth > data_words - sib_off || cap_off > data_words || cap_len > (data_words - cap_off) / 4) {
        flags[j] = vfy::MF_BOUNDS;
        return;
    }
    alignas(16) u64 cur[4];
    const u64* leaf = image + leaf_off;
    H::leaf([&](u32 i) { return leaf[i]; }, len, cur);
    for (u32 d = 0; d < depth; d++) {
        const u64* s = image + sib_off + 4 * (size_t)d;
        const bool right = index & 1;      // this node is the right child: the sibling goes first
        alignas(16) u64 pair[8];
#pragma unroll
        for (int k = 0; k < 4; k++) { pair[k] = right ? s[k] : cur[k]; pair[4 + k] = right ? cur[k] : s[k]; }
        H::node(pair, cur);
        index >>= 1;
    }
    bool ok = index < cap_len;
    if (ok) {
        const u64* c = image + cap_off + 4 * (size_t)index;
        ok = c[0] == cur[0] && c[1] == cur[1] && c[2] == cur[2] && c[3] == cur[3];
    }
    flags[j] = ok ? vfy::MF_OK : vfy::MF_MISMATCH;
}

__device__ __forceinline__ Ext2 vfy_ext(const u64* p) { return ext_make(p[0], p[1]); }
// acc * alpha + v for a base-field v
__device__ __forceinline__ Ext2 vfy_horner_base(Ext2 acc, Ext2 alpha, u64 v) {
    acc = ext_mul(acc, alpha);
    acc.a = gl_add(acc.a, v);
    return acc;
}
// reduce_with_powers of row[from, to) behind what `acc` already holds of the batch's later values (Horner from the last value)
__device__ __forceinline__ Ext2 vfy_reduce_row(Ext2 acc, Ext2 alpha, const u64* __restrict__ row, u32 from, u32 to) {
    for (u32 k = to; k-- > from;) acc = vfy_horner_base(acc, alpha, row[k]);
    return acc;
}

// compute_evaluation (fri/verifier.rs:19-45): the layer's 2^ab values are those of a polynomial of degree < 2^ab on the coset
// x g^-rev(within) <g>, in bit-reversed order; its value at beta, by barycentric interpolation as the reference computes it.
__device__ Ext2 vfy_compute_evaluation(u64 x, u32 within, int ab, const u64* __restrict__ evals, Ext2 beta) {
    const u32 arity = 1u << ab;
    const u64 g = gl_root_of_unity(ab);
    const u64 start = gl_mul(x, gl_pow(g, arity - bitrev32(within, ab)));
    Ext2 lx = ext_make(1, 0), sum = ext_make(0, 0);
    u64 pk = start;
    for (u32 k = 0; k < arity; k++) {
        const Ext2 e = vfy_ext(evals + 2 * (size_t)bitrev32(k, ab));
        const Ext2 diff = ext_make(gl_sub(beta.a, pk), beta.b);       // beta - p_k
        if (diff.a == 0 && diff.b == 0) return e;
        lx = ext_mul(lx, diff);
        u64 den = 1, pj = start;                                      // prod over j != k of (p_k - p_j), in the base field
        for (u32 i = 0; i < arity; i++) {
            if (i != k) den = gl_mul(den, gl_sub(pk, pj));
            pj = gl_mul(pj, g);
        }
        sum = ext_add(sum, ext_mul(ext_scalar_mul(ext_inv(diff), gl_inv(den)), e));
        pk = gl_mul(pk, g);
    }
    return ext_mul(lx, sum);
}

// One (table, query): x from the query index, fri_combine_initial over the three opened rows, per layer the consistency check and
// compute_evaluation at that layer's beta, the final polynomial at the last point.  Writes the first failing kind and layer.
__global__ __launch_bounds__(64) void fri_query_check_kernel(const u64* __restrict__ image, size_t data_words, size_t jobs_off, u32 n_jobs,
                                                             u32* __restrict__ flags) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    const u64* w = image + jobs_off + j;
    const size_t n = n_jobs;
    const u64 tab_off = w[vfy::QJ_TAB_OFF * n], steps_off = w[vfy::QJ_STEPS_OFF * n];
    const u64 row_off[3] = {w[vfy::QJ_ROW0 * n], w[vfy::QJ_ROW1 * n], w[vfy::QJ_ROW2 * n]};
    u64 x_index = w[vfy::QJ_X_INDEX * n];
    if (tab_off > data_words || (u64)vfy::TAB_WORDS > data_words - tab_off) { flags[j] = vfy::QF_BOUNDS; return; }
    const u64* tab = image + tab_off;
    const u64 lde_bits = tab[vfy::TH_LDE_BITS], layers = tab[vfy::TH_LAYERS], arities_off = tab[vfy::TH_ARITIES_OFF];
    const u64 final_off = tab[vfy::TH_FINAL_OFF], final_len = tab[vfy::TH_FINAL_LEN], betas_off = tab[vfy::TH_BETAS_OFF];
    const u64 n0 = tab[vfy::TH_N0], n1 = tab[vfy::TH_N1], n2 = tab[vfy::TH_N2], nperm = tab[vfy::TH_NPERM];
    const u64 widths[3] = {n0, n1, n2};
    bool in_bounds = lde_bits <= (u64)vfy::MAX_LDE_BITS && layers <= 32 && nperm <= n1 &&
                     (x_index >> lde_bits) == 0;
    for (int o = 0; o < 3; o++) in_bounds = in_bounds && row_off[o] <= data_words && widths[o] <= data_words - row_off[o];
    // each layer's arity bits (a per-table list next to the betas): 1 .. MAX_ARITY_BITS, and the evaluations at their own widths
    in_bounds = in_bounds && arities_off <= data_words && layers <= data_words - arities_off;
    u64 steps_words = 0;
    if (in_bounds)
        for (u64 i = 0; i < layers; i++) {
            const u64 a = image[arities_off + i];
            if (a < 1 || a > (u64)vfy::MAX_ARITY_BITS) { in_bounds = false; break; }
            steps_words += 2ull << a;
        }
    in_bounds = in_bounds && steps_off <= data_words && steps_words <= data_words - steps_off;
    in_bounds = in_bounds && betas_off <= data_words && 2 * layers <= data_words - betas_off;
    in_bounds = in_bounds && final_off <= data_words && final_len <= (data_words - final_off) / 2;
    if (!in_bounds) { flags[j] = vfy::QF_BOUNDS; return; }
    const int log_n = (int)lde_bits;
    const Ext2 alpha = vfy_ext(tab + vfy::TH_ALPHA);
    const u64* r0 = image + row_off[0];
    const u64* r1 = image + row_off[1];
    const u64* r2 = image + row_off[2];

    u64 x = gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(log_n), (u64)bitrev32((u32)x_index, log_n)));
    // fri_combine_initial: the batches at zeta (trace, Zs, quotient), at g zeta (trace, Zs) and at g^-1 (the lookup Zs)
    const Ext2 zero = ext_make(0, 0);
    Ext2 reduced[3];
    reduced[0] = vfy_reduce_row(vfy_reduce_row(vfy_reduce_row(zero, alpha, r2, 0, (u32)n2), alpha, r1, 0, (u32)n1), alpha, r0, 0, (u32)n0);
    reduced[1] = vfy_reduce_row(vfy_reduce_row(zero, alpha, r1, 0, (u32)n1), alpha, r0, 0, (u32)n0);
    reduced[2] = vfy_reduce_row(zero, alpha, r1, (u32)nperm, (u32)n1);
    const Ext2 point[3] = {vfy_ext(tab + vfy::TH_ZETA), vfy_ext(tab + vfy::TH_ZETA_NEXT), ext_make(tab[vfy::TH_G_INV], 0)};
    Ext2 sum = zero;
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const Ext2 num = ext_sub(reduced[b], vfy_ext(tab + vfy::TH_REDUCED + 2 * b));
        const Ext2 den = ext_make(gl_sub(x, point[b].a), gl_neg(point[b].b));
        sum = ext_add(ext_mul(sum, vfy_ext(tab + vfy::TH_ALPHA_POW + 2 * b)), ext_mul(num, ext_inv(den)));
    }
    Ext2 old_eval = ext_scalar_mul(sum, x);       // the prover's final polynomial was multiplied by X (fri/oracle.rs:218)

    u32 verdict = vfy::QF_OK;
    const u64* evals = image + steps_off;
    for (u32 i = 0; i < (u32)layers; i++) {
        const int ab = (int)image[arities_off + i];
        const u32 within = (u32)x_index & ((1u << ab) - 1);
        if (!ext_eq(vfy_ext(evals + 2 * (size_t)within), old_eval)) { verdict = vfy::QF_CONSISTENCY | (i << 8); break; }
        old_eval = vfy_compute_evaluation(x, within, ab, evals, vfy_ext(image + betas_off + 2 * (size_t)i));
        for (int k = 0; k < ab; k++) x = gl_mul(x, x);
        x_index >>= ab;
        evals += 2u << ab;
    }
    if (verdict == vfy::QF_OK) {
        Ext2 fe = zero;
        const u64* fp = image + final_off;
        for (u64 k = final_len; k-- > 0;) {
            fe = ext_scalar_mul(fe, x);
            fe = ext_add(fe, vfy_ext(fp + 2 * k));
        }
        if (!ext_eq(fe, old_eval)) verdict = vfy::QF_FINAL_POLY;
    }
    flags[j] = verdict;
}

// ------------------------------------------------------------------------------------------------ host launcher
// Uploads the stage's image, runs the two kernels, reads the flags back and fills in the report.  No job: nothing runs.
void verify_on_device(DeviceCtx* ctx, const vfy::Stage& st, OlaVerifyReport* rep) {
    const size_t nm = st.merkle.size(), nq = st.queries.size();
    rep->merkle_jobs = (uint32_t)nm;
    rep->query_jobs = (uint32_t)nq;
    rep->kernel_launches = 0;
    rep->device_ms = 0;
    vfy::Verdict v = st.host;
    if (nm + nq > 0) {
        if (nm > 0xFFFFFFFFull || nq > 0xFFFFFFFFull) throw OlaError(OLA_E_INVALID_ARG, "proof too large for the verifier");
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> flags(nm + nq, 0xFFFFFFFFu);
        u64* d_image = (u64*)ctx->alloc(st.image.size() * 8);
        u32* d_flags = nullptr;
        try {
            d_flags = (u32*)ctx->alloc((nm + nq) * 4);
            HIP_CHECK(hipMemcpyAsync(d_image, st.image.data(), st.image.size() * 8, hipMemcpyHostToDevice, ctx->stream));
            HIP_CHECK(hipMemsetAsync(d_flags, 0xFF, (nm + nq) * 4, ctx->stream));
            const size_t data_words = st.merkle_off;      // the job lists lie behind the data
            if (nm) {
                const dim3 grid((unsigned)((nm + 63) / 64)), block(64);
                size_t leaf_words = 0;      // the widest leaf: Blake3's single-chunk form serves while none exceeds a chunk
                for (const vfy::MerkleJob& m : st.merkle) leaf_words = std::max(leaf_words, (size_t)m.leaf_len);
                with_hash((uint32_t)ctx->hasher, leaf_words, [&](auto tag) {
                    using H = typename decltype(tag)::type;
                    hipLaunchKernelGGL(merkle_paths_check_kernel<H>, grid, block, 0, ctx->stream, d_image, data_words, st.merkle_off, (u32)nm, d_flags);
                });
                rep->kernel_launches++;
            }
            if (nq) {
                hipLaunchKernelGGL(fri_query_check_kernel, dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, ctx->stream, d_image, data_words, st.query_off, (u32)nq,
                                   d_flags + nm);
                rep->kernel_launches++;
            }
            HIP_CHECK(hipMemcpyAsync(flags.data(), d_flags, (nm + nq) * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
        } catch (...) {
            (void)hipStreamSynchronize(ctx->stream);
            if (d_flags) ctx->free(d_flags);
            ctx->free(d_image);
            throw;
        }
        ctx->free(d_flags);
        ctx->free(d_image);
        for (uint32_t f : flags)
            if (f == 0xFFFFFFFFu) throw OlaError(OLA_E_HIP, "verifier: a kernel did not write its flag");
        v = vfy::resolve(st, flags.data());
        rep->device_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    rep->accepted = v.failed() ? 0u : 1u;
    rep->reason = v.reason;
    rep->table = v.table; rep->query = v.query; rep->oracle_or_layer = v.oracle_or_layer;
    vfy::describe(v, rep->message, sizeof(rep->message));
}

}  // namespace ola
