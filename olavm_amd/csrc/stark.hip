// Multi-table STARK prover on the device: CTL / permutation Z columns, constraint quotient, per-table proof assembly.
//
// Replaces (reference paths relative to /root/reference/circuits/src/stark):
//   prover.rs:79-327        prove_with_traces         -> prove_with_traces() below (host orchestration, device data)
//   prover.rs:330-567       prove_single_table
//   prover.rs:571-705       compute_quotient_polys    -> quotient_kernel (one thread per LDE point, constraint program
//                                                        interpreted out of an LDS register file) + coset iNTT
//   cross_table_lookup.rs:224-311  cross_table_lookup_data / partial_products -> ctl_factor_kernel + product scan
//   permutation.rs:103-155  compute_permutation_z_polys -> perm_factor_kernel + product scan
//   constraint_consumer.rs:34-78, vanishing_poly.rs:20-45, permutation.rs:302-360, cross_table_lookup.rs:380-421
//                           ConstraintConsumer / eval_vanishing_poly / permutation + CTL checks (inside quotient_kernel)
//   serialization.rs:349-358,377-393   write_proof / write_all_proof
// The table descriptions (constraint programs, permutation pairs, CTLs) are data: the AIR-set blob produced by
// olavm_amd/air/dsl.py.  The sequential prefix products of the reference become three-phase parallel scans; the
// quotient is evaluated directly on the resident LDE in leaf order (thread j <-> leaf j <-> natural LDE row bitrev(j)),
// which for a table of quotient-degree 2^qdb are exactly the first n*2^qdb leaves (cosets 0..2^qdb-1).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ola_gpu.h"
#include "device_ctx.h"
#include "gl.cuh"
#include "airset_host.h"
#include "air_interp.cuh"
#include "airq.cuh"
#include "dev_buf.h"
#include "scan.cuh"
#include "upload.h"

namespace ola {

static void push_lincol(std::vector<u64>& d, const HLinCol& c) {
    d.push_back(c.terms.size());
    for (auto& t : c.terms) { d.push_back(t.first); d.push_back(t.second); }
    d.push_back(c.constant);
}
// [beta, gamma, ncols, lincol*, has_filter, lincol?]
static void push_ctl_desc(std::vector<u64>& d, const HTwc& t, u64 beta, u64 gamma) {
    d.push_back(beta); d.push_back(gamma); d.push_back(t.columns.size());
    for (auto& c : t.columns) push_lincol(d, c);
    d.push_back(t.has_filter ? 1 : 0);
    if (t.has_filter) push_lincol(d, t.filter);
}


// FNV-1a over the little-endian bytes of the words a specialised kernel depends on (olavm_amd/air/dsl.py
// AirSet.signature_words): the table description and the static part of each of its CTL Z columns.
struct SigHasher {
    u64 h = 0xCBF29CE484222325ull;
    void word(u64 x) { for (int k = 0; k < 8; k++) { h ^= (x >> (8 * k)) & 0xFF; h *= 0x100000001B3ull; } }
    void lincol(const HLinCol& c) { word(c.terms.size()); for (auto& t : c.terms) { word(t.first); word(t.second); } word(c.constant); }
};
// nch: the challenge count the kernel is printed for.  Two is the reference's standard configuration and leaves the hash what it
// was; any other count is hashed in front (a table without lookups and permutation pairs has the same words at every count).
static u64 air_signature(const HTable& a, const std::vector<const HTwc*>& jobs, int nch) {
    SigHasher s;
    if (nch != 2) s.word((u64)nch);
    s.word((u64)a.ncols); s.word((u64)a.constraint_degree); s.word((u64)a.n_regs); s.word((u64)a.n_params);
    s.word(a.perm_pairs.size());
    for (auto& pr : a.perm_pairs) { s.word(pr.size()); for (auto& lr : pr) { s.word(lr.first); s.word(lr.second); } }
    s.word(a.ops.size() / 2);
    for (u64 w : a.ops) s.word(w);
    s.word(jobs.size());
    for (const HTwc* t : jobs) {
        s.word(t->columns.size());
        for (auto& c : t->columns) s.lincol(c);
        s.word(t->has_filter ? 1 : 0);
        if (t->has_filter) s.lincol(t->filter);
    }
    return s.h;
}

// ------------------------------------------------------------------------------------------------ device helpers
// evaluate a linear combination of columns at row `row` of a column-major table (stride `cs`); advances the cursor
__device__ __forceinline__ u64 dev_lincol(const u64* __restrict__ d, u32& p, const u64* __restrict__ tab, size_t cs, size_t row) {
    const u32 nt = (u32)d[p++];
    u64 s = 0;
    for (u32 i = 0; i < nt; i++) {
        const u64 c = d[p++], f = d[p++];
        const u64 v = gl_canon(tab[c * cs + row]);
        s = gl_add(s, f == 1 ? v : gl_mul(v, f));          // the coefficient is uniform: no divergence; most are 1
    }
    return gl_add(s, d[p++]);
}

// CTL factor columns: out[i] = filter(i) ? combine(i) : 1   (cross_table_lookup.rs:284-311)
// A table carries one Z column per (lookup side, challenge); the num_challenges columns of one side combine the SAME linear
// combinations of trace columns with different (beta, gamma).  One blockIdx.y handles such a group of G columns: descriptors at
// desc_all[offs[groups[G y + c]]], outputs at out_all + index*n.  The trace cells, the linear combinations and the filter are
// read / evaluated once for the whole group.
template <int G>
__global__ __launch_bounds__(256) void ctl_factor_kernel(const u64* __restrict__ trace, size_t n, const u64* __restrict__ desc_all,
                                                         const u64* __restrict__ offs, const u64* __restrict__ groups, u64* __restrict__ out_all,
                                                         unsigned* __restrict__ bad_filter) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 col[G], beta[G], acc[G], bp[G];
#pragma unroll
    for (int c = 0; c < G; c++) {
        col[c] = groups[(size_t)G * blockIdx.y + c];
        beta[c] = desc_all[offs[col[c]]];
        acc[c] = 0;
        bp[c] = 1;
    }
    const u64* __restrict__ desc = desc_all + offs[col[0]];      // the linear combinations: the same words in every member
    u32 p = 2;
    const u32 ncol = (u32)desc[p++];
    // combine = reduce_with_powers(evals, beta) + gamma = sum_k beta^k e_k + gamma
    for (u32 k = 0; k < ncol; k++) {
        const u64 e = dev_lincol(desc, p, trace, n, i);
#pragma unroll
        for (int c = 0; c < G; c++) {
            acc[c] = gl_add(acc[c], k == 0 ? e : gl_mul(bp[c], e));
            if (k + 1 < ncol) bp[c] = gl_mul(bp[c], beta[c]);
        }
    }
    u64 f = 1;
    if (desc[p++]) f = dev_lincol(desc, p, trace, n, i);
    if (f > 1) atomicOr(bad_filter, 1u);  // cross_table_lookup.rs:303-305 panics "Non-binary filter?"
#pragma unroll
    for (int c = 0; c < G; c++) out_all[col[c] * n + i] = (f == 1) ? gl_add(acc[c], desc_all[offs[col[c]] + 1]) : 1;
}

// permutation quotient column: out[i] = prod_inst (gamma + sum beta^k lhs_k) / prod_inst (gamma + sum beta^k rhs_k)
// desc: [n_inst, (beta, gamma, npairs, (lhs, rhs)*)*]
// A row whose denominator is zero has no quotient: the reference inverts the denominators in one batch_multiplicative_inverse and
// panics "Tried to invert zero" (permutation.rs:143).  Here gl_inv(0) = 0 and the row's factor is written as 0; the smallest `batch`
// with such a row is left in *zero_den (initialised to ~0u by the caller), who decides what a zero means for it.
__global__ __launch_bounds__(256) void perm_factor_kernel(const u64* __restrict__ trace, size_t n, const u64* __restrict__ desc,
                                                          u64* __restrict__ out, unsigned batch, unsigned* __restrict__ zero_den) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 p = 0;
    const u32 ninst = (u32)desc[p++];
    u64 num = 1, den = 1;
    for (u32 s = 0; s < ninst; s++) {
        const u64 beta = desc[p++], gamma = desc[p++];
        const u32 np = (u32)desc[p++];
        u64 l = gamma, r = gamma, w = 1;
        for (u32 k = 0; k < np; k++) {
            const u64 cl = desc[p++], cr = desc[p++];
            l = gl_add(l, gl_mul(gl_canon(trace[cl * n + i]), w));
            r = gl_add(r, gl_mul(gl_canon(trace[cr * n + i]), w));
            w = gl_mul(w, beta);
        }
        num = gl_mul(num, l);
        den = gl_mul(den, r);
    }
    if (den == 0) atomicMin(zero_den, batch);
    out[i] = gl_mul(num, gl_inv(den));
}

// exclusive form: out[0] = 1, out[i] = incl[i-1]
__global__ __launch_bounds__(256) void shift_right_kernel(const u64* __restrict__ incl, u64* __restrict__ out, size_t n) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    out[k] = k ? incl[k - 1] : 1;
}

// Lagrange selector polynomials in coefficient form: L_0 = (1/n) sum X^k ; L_{n-1} = (1/n) sum g^k X^k
__global__ __launch_bounds__(256) void lagrange_coeffs_kernel(u64* __restrict__ out, size_t n, u64 n_inv, const u64* __restrict__ g_lo,
                                                              const u64* __restrict__ g_hi, int g_h) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    out[k] = n_inv;
    const u64 gk = gl_mul(g_lo[k & (((size_t)1 << g_h) - 1)], g_hi[k >> g_h]);
    out[n + k] = gl_mul(n_inv, gk);
}

// any non-zero element in data[lo, hi)?
__global__ __launch_bounds__(256) void any_nonzero_kernel(const u64* __restrict__ data, size_t lo, size_t hi, unsigned* __restrict__ flag) {
    const size_t k = lo + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < hi && gl_canon(data[k]) != 0) atomicOr(flag, 1u);
}

// ------------------------------------------------------------------------------------------------ quotient kernel

// descriptor header (quotient_desc): 8 words of counts and offsets, the alphas, 1/Z_H per coset
constexpr int QD_ALPHA = 8, QD_ZH = QD_ALPHA + OLA_MAX_CHALLENGES, QD_HEAD = QD_ZH + 8;

template <int NCH>
__global__ __launch_bounds__(QW) void quotient_kernel(QuotParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u64* regs = reinterpret_cast<u64*>(smem_raw);
    const int lane = threadIdx.x;
    const size_t size = P.npoints ? P.npoints : P.out_plane;   // points this launch evaluates (the rank's cosets of the quotient domain)
    const size_t j = (size_t)blockIdx.x * QW + lane;
    const bool active = j < size;
    const size_t jj = active ? j : 0;
    // leaf j = c*n + r  <->  natural row m = bitrev3(c) + 8*bitrev_n(r); next row m + 8 -> r' = bitrev_n(bitrev_n(r) + 1)
    // (buffers hold cosets from P.coset_first on: `cl` indexes memory, `c` is the coset of the evaluation point)
    const size_t cl = jj >> P.log_n, r = jj & (P.n - 1);
    const size_t c = cl + P.coset_first;
    const u32 rr = bitrev32((u32)r, P.log_n);
    const size_t rn = bitrev32((rr + 1) & (u32)(P.n - 1), P.log_n);
    const size_t jn = (cl << P.log_n) + rn;
    const u64 m = ((u64)rr << (P.log_N - P.log_n)) + bitrev32((u32)c, P.log_N - P.log_n);
    const u64 x = gl_mul(GL_GENERATOR, gl_mul(P.gN_lo[m & (((u64)1 << P.gN_h) - 1)], P.gN_hi[m >> P.gN_h]));
    const u64 z_last = gl_sub(x, P.g_inv);
    const u64 lag_first = P.lag_lde[jj], lag_last = P.lag_lde[P.N + jj];

    const u64* __restrict__ D = P.desc;
    const u32 n_ops = (u32)D[0], ops_off = (u32)D[1], nperm = (u32)D[2], perm_off = (u32)D[3], nctl = (u32)D[4], ctl_off = (u32)D[5];
    const u32 params_off = (u32)D[7];
    const u64 zh_inv = D[QD_ZH + c];
    u64 alpha[NCH], acc[NCH];       // in registers: every loop over them is unrolled
#pragma unroll
    for (int a = 0; a < NCH; a++) { alpha[a] = D[QD_ALPHA + a]; acc[a] = 0; }
    auto emit = [&](int kind, u64 v) {
        if (kind == AK_TRANSITION) v = gl_mul(v, z_last);
        else if (kind == AK_FIRST) v = gl_mul(v, lag_first);
        else if (kind == AK_LAST) v = gl_mul(v, lag_last);
#pragma unroll
        for (int a = 0; a < NCH; a++) acc[a] = gl_add(gl_mul(acc[a], alpha[a]), v);
    };
    const size_t N = P.N;

    // ---- the table's constraint program ----
    air_interpret(D + ops_off, n_ops, D + params_off, regs, lane,
                  [&](u32 col, bool next) { return gl_canon(P.trace_lde[(size_t)col * N + (next ? jn : jj)]); }, emit);
    // ---- permutation checks (permutation.rs:302-360) ----
    {
        for (u32 i = 0; i < nperm; i++) emit(AK_FIRST, gl_sub(P.zs_lde[(size_t)i * N + jj], 1));
        u32 p = perm_off;
        for (u32 bI = 0; bI < nperm; bI++) {
            const u32 ninst = (u32)D[p++];
            u64 prod_l = 1, prod_r = 1;
            for (u32 s = 0; s < ninst; s++) {
                const u64 beta = D[p++], gamma = D[p++];
                const u32 np = (u32)D[p++];
                u64 l = 0, rr2 = 0, w = 1;
                for (u32 k = 0; k < np; k++) {
                    const u64 cl = D[p++], cr = D[p++];
                    l = gl_add(l, gl_mul(gl_canon(P.trace_lde[cl * N + jj]), w));
                    rr2 = gl_add(rr2, gl_mul(gl_canon(P.trace_lde[cr * N + jj]), w));
                    w = gl_mul(w, beta);
                }
                prod_l = gl_mul(prod_l, gl_add(l, gamma));
                prod_r = gl_mul(prod_r, gl_add(rr2, gamma));
            }
            const u64 zl = P.zs_lde[(size_t)bI * N + jj], zn = P.zs_lde[(size_t)bI * N + jn];
            emit(AK_ALL, gl_sub(gl_mul(zn, prod_r), gl_mul(zl, prod_l)));
        }
    }
    // ---- cross-table lookup checks (cross_table_lookup.rs:380-421) ----
    {
        u32 p = ctl_off;
        for (u32 i = 0; i < nctl; i++) {
            const u64 beta = D[p++], gamma = D[p++];
            const u32 ncol = (u32)D[p++];
            u64 cl = 0, cn = 0, bp = 1;
            for (u32 k = 0; k < ncol; k++) {
                u32 p2 = p;
                const u64 el = dev_lincol(D, p, P.trace_lde, N, jj);
                const u64 en = dev_lincol(D, p2, P.trace_lde, N, jn);
                cl = gl_add(cl, gl_mul(bp, el));
                cn = gl_add(cn, gl_mul(bp, en));
                bp = gl_mul(bp, beta);
            }
            cl = gl_add(cl, gamma);
            cn = gl_add(cn, gamma);
            u64 fl = 1, fn = 1;
            if (D[p++]) {
                u32 p2 = p;
                fl = dev_lincol(D, p, P.trace_lde, N, jj);
                fn = dev_lincol(D, p2, P.trace_lde, N, jn);
            }
            // select(f, x) = f*x + 1 - f
            const u64 sl = gl_sub(gl_add(gl_mul(fl, cl), 1), fl), sn = gl_sub(gl_add(gl_mul(fn, cn), 1), fn);
            const u64 zl = P.zs_lde[(size_t)(nperm + i) * N + jj], zn = P.zs_lde[(size_t)(nperm + i) * N + jn];
            emit(AK_FIRST, gl_sub(zl, sl));
            emit(AK_TRANSITION, gl_sub(zn, gl_mul(zl, sn)));
        }
    }
    if (active) {
#pragma unroll
        for (int a = 0; a < NCH; a++) P.out[(size_t)a * P.out_plane + j] = gl_mul(acc[a], zh_inv);
    }
}

// ------------------------------------------------------------------------------------------------ specialised quotient kernels
// (airq.cuh; one translation unit per table signature under gen/, printed by olavm_amd/air/codegen.py)
#include "gen/air_registry.inc"

static const AirKernelEntry* find_air_kernel(u64 sig) {
    for (const AirKernelEntry* e : AIR_KERNELS)
        if (e->signature == sig) return e;
    return nullptr;
}

// any element of a[0,len) != b[0,len)?
__global__ __launch_bounds__(256) void any_diff_kernel(const u64* __restrict__ a, const u64* __restrict__ b, size_t len, unsigned* __restrict__ flag) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < len && a[k] != b[k]) atomicOr(flag, 1u);
}

// ------------------------------------------------------------------------------------------------ host orchestration
struct GpChallenge { u64 beta, gamma; };

static GpChallenge get_gp(OlaChallenger& ch) { const u64 b = challenger_get(ch); const u64 g = challenger_get(ch); return {b, g}; }

struct CtlJob { const HTwc* twc; GpChallenge ch; };

// the instantiation of a kernel template for a challenge count (ola_gpu.hip resolve_config admits 1..OLA_MAX_CHALLENGES)
#define OLA_FOR_NCH(nch, F)                                                                       \
    switch (nch) {                                                                                \
        case 1: F(1); break; case 2: F(2); break; case 3: F(3); break; case 4: F(4); break;       \
        case 5: F(5); break; case 6: F(6); break; case 7: F(7); break; case 8: F(8); break;       \
        default: throw OlaError(OLA_E_INTERNAL, "challenge count out of range");                  \
    }

// `count` pairs (beta, gamma) as a caller hands them over, [count][2] words: reduced on entry
static std::vector<GpChallenge> read_challenges(const u64* words, size_t count) {
    std::vector<GpChallenge> out;
    for (size_t i = 0; i < count; i++) out.push_back({gl_canon(words[2 * i]), gl_canon(words[2 * i + 1])});
    return out;
}

// get_n_grand_product_challenge_sets (prover.rs:360-367): [permutation_batch_size][num_challenges], none for a table without
// permutation arguments -- from the transcript, or from a caller's words
using PermSets = std::vector<std::vector<GpChallenge>>;
static PermSets draw_perm_sets(const HTable& air, int nch, OlaChallenger& ch) {
    PermSets sets(air.perm_pairs.empty() ? 0 : air.permutation_batch_size());
    for (auto& s : sets)
        for (int c = 0; c < nch; c++) s.push_back(get_gp(ch));
    return sets;
}
static PermSets read_perm_sets(const HTable& air, int nch, const u64* words) {
    PermSets sets(air.perm_pairs.empty() ? 0 : air.permutation_batch_size());
    for (size_t i = 0; i < sets.size(); i++) sets[i] = read_challenges(words + i * nch * 2, nch);
    return sets;
}

// a table's public parameters, or the zero block for a caller that has none to give
static const u64* params_or_zero(const u64* params, size_t offset, const HTable& air) {
    static const u64 zero_block[64] = {};
    if (!params && air.n_params > 64) throw OlaError(OLA_E_INVALID_ARG, "params required");
    return params ? params + offset : zero_block;
}

static HAirSet parse_airset_with_table(const u64* airset, size_t airset_words, uint32_t table) {
    HAirSet set = parse_airset(airset, airset_words);
    if (table >= set.tables.size()) throw OlaError(OLA_E_INVALID_ARG, "table index out of range");
    return set;
}

// ---- descriptors of the Z columns, read by the factor kernels and, inside its own descriptor, by the quotient kernel ----
// The permutation batches of a table: per batch [instances, then per instance beta, gamma, pairs, (lhs column, rhs column) ...];
// batch_off[b]: where batch b starts.
struct PermDesc { std::vector<u64> words; std::vector<size_t> batch_off; int nperm() const { return (int)batch_off.size(); } };
static PermDesc build_perm_desc(const HTable& air, const PermSets& sets, int nch) {
    PermDesc d;
    const int nperm = air.num_permutation_batches(nch), bs = air.permutation_batch_size(), total = (int)air.perm_pairs.size() * nch;
    int inst = 0;
    for (int b = 0; b < nperm; b++) {
        const size_t at = d.words.size();
        d.batch_off.push_back(at);
        d.words.push_back(0);
        u64 cnt = 0;
        for (int i = 0; i < bs && inst < total; i++, inst++, cnt++) {
            const auto& pair = air.perm_pairs[inst / nch];
            const GpChallenge c = sets[i][inst % nch];
            d.words.push_back(c.beta); d.words.push_back(c.gamma); d.words.push_back(pair.size());
            for (auto& pr : pair) { d.words.push_back(pr.first); d.words.push_back(pr.second); }
        }
        d.words[at] = cnt;
    }
    return d;
}

// The lookup columns of a table: the push_ctl_desc words of its jobs, and what ctl_factor_kernel indexes them by -- index[j] for
// j < ncols: where job j starts; then the jobs in groups of `group`.  The columns of one lookup side under the challenges share
// their linear combinations, so they form a group: num_challenges columns each (ctl_jobs).
struct CtlDesc { std::vector<u64> words, index; size_t ncols = 0; int group = 1; size_t ngroups() const { return (index.size() - ncols) / (size_t)group; } };
static CtlDesc build_ctl_desc(const std::vector<CtlJob>& ctl, int nch) {
    CtlDesc d;
    d.ncols = ctl.size();
    d.group = nch;
    for (auto& j : ctl) { d.index.push_back(d.words.size()); push_ctl_desc(d.words, *j.twc, j.ch.beta, j.ch.gamma); }
    std::vector<char> taken(ctl.size(), 0);
    for (size_t a = 0; a < ctl.size(); a++) {
        if (taken[a]) continue;
        int members = 0;
        for (size_t c = a; c < ctl.size(); c++)
            if (!taken[c] && ctl[c].twc == ctl[a].twc) { taken[c] = 1; d.index.push_back(c); members++; }
        if (members != nch) throw OlaError(OLA_E_INTERNAL, "a lookup side does not carry one Z column per challenge");
    }
    return d;
}

struct BatchHolder {
    DeviceCtx* ctx;
    OlaBatch* b = nullptr;
    explicit BatchHolder(DeviceCtx* c) : ctx(c) {}
    ~BatchHolder() { if (b) { (void)hipStreamSynchronize(ctx->stream); batch_destroy(ctx, b); } }
};

// values of one table resident on the device (column-major, n per column)
struct DevTable { u64* vals = nullptr; uint32_t log_n = 0; size_t n() const { return (size_t)1 << log_n; } };

static void write_cap(ByteWriter& w, const std::vector<u64>& cap) { w.cap(cap.data(), cap.size() / 4); }

// PolynomialBatch::from_values / from_coeffs for the whole table, or -- under the coset partition -- this rank's share of
// it; either way `cap_full` receives the complete Merkle cap (all-gathered from the ranks' slices when sharded).
static OlaBatch* commit_shared(DeviceCtx* ctx, NttTables& t, const u64* dev_cols, uint32_t ncols, uint32_t log_n, const OlaGpuConfig& cfg,
                               bool from_values, bool sharded, const ColumnFeed* feed, std::vector<u64>& cap_full, bool lean = false) {
    const size_t len_cap = (size_t)1 << cfg.cap_height;
    cap_full.assign(len_cap * 4, 0);
    if (!sharded) {
        if (ctx->acct.shardable) acct_exchange(ctx, len_cap * 32);   // the cap slices a partitioned run gathers
        OlaBatch* b = batch_commit(ctx, t, nullptr, dev_cols, ncols, log_n, cfg.rate_bits, cfg.cap_height, from_values, 0, 0, feed, lean);
        try { batch_read_cap(ctx, *b, cap_full.data()); } catch (...) { batch_destroy(ctx, b); throw; }
        return b;
    }
    OlaBatch* b = batch_commit(ctx, t, nullptr, dev_cols, ncols, log_n, cfg.rate_bits, cfg.cap_height, from_values, ctx->shard.rank,
                               ctx->shard.log_world, feed);
    u64* d_full = nullptr;
    try {
        const size_t len_local = len_cap >> ctx->shard.log_world;   // the local tree's cap level (batch_read_cap)
        d_full = (u64*)ctx->alloc(len_cap * 32);
        shard_all_gather(ctx, b->heap + 4 * len_local, d_full, len_local * 32);
        HIP_CHECK(hipMemcpyAsync(cap_full.data(), d_full, len_cap * 32, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        ctx->free(d_full);
    } catch (...) { if (d_full) ctx->free(d_full); batch_destroy(ctx, b); throw; }
    return b;
}

// Which tables run on the coset partition: every table large enough to be worth the exchanges.  The COMMITMENTS of a table
// split over the 2^rate_bits LDE cosets whatever its constraint degree; its quotient lives on the first 2^qdb cosets of the
// leaf order and is evaluated by the ranks that own them (all ranks when 2^qdb = 2^rate_bits: CPU, memory, Poseidon tables).
static bool table_is_sharded(const DeviceCtx* ctx, const OlaGpuConfig& cfg, const HTable& air, uint32_t log_n) {
    (void)air;
    if (ctx->shard.world <= 1) return false;
    return log_n >= ctx->shard.min_log_n && ctx->shard.log_world <= cfg.rate_bits && ctx->shard.log_world <= cfg.cap_height;
}

// ---- steps of prove_single_table: each takes its memory from the caller's DevBuf and waits for nothing -----------------------
// host columns -> a table on the device, reduced
static DevTable upload_table(DeviceCtx* ctx, DevBuf& mem, const u64* const* cols, int ncols, uint32_t log_n) {
    DevTable tv{nullptr, log_n};
    const size_t n = tv.n();
    tv.vals = mem.alloc((size_t)ncols * n);
    for (int c = 0; c < ncols; c++) HIP_CHECK(hipMemcpyAsync(tv.vals + (size_t)c * n, cols[c], n * 8, hipMemcpyHostToDevice, ctx->stream));
    canonicalize(ctx, tv.vals, (size_t)ncols * n);
    return tv;
}

// What the Z steps find wrong with a trace, left on the device: a non-binary CTL filter, and the first permutation batch with a zero
// denominator (~0u: none).  The two words travel with the next read-back the host waits for anyway: fetch() after the steps,
// check() after that wait.  The reference meets the filter first (cross_table_lookup_data runs before any prove_single_table).
struct ZFlags {
    unsigned* dev; HostSpan host; int table_index;
    ZFlags(DeviceCtx* ctx, DevBuf& mem, int table) : dev((unsigned*)mem.alloc(1)), host(mem.host(1)), table_index(table) {
        HIP_CHECK(hipMemsetAsync(dev, 0, 4, ctx->stream));
        HIP_CHECK(hipMemsetAsync(dev + 1, 0xFF, 4, ctx->stream));
    }
    unsigned* bad_filter() const { return dev; }
    unsigned* zero_den() const { return dev + 1; }
    void fetch(DeviceCtx* ctx) const { HIP_CHECK(hipMemcpyAsync(&host[0], dev, 8, hipMemcpyDeviceToHost, ctx->stream)); }
    void check() const {
        if ((unsigned)host[0]) throw OlaError(OLA_E_INVALID_ARG, "Non-binary filter?");
        const unsigned zero_batch = (unsigned)(host[0] >> 32);
        if (zero_batch != ~0u)
            throw OlaError(OLA_E_INVALID_ARG, "Tried to invert zero: table " + std::to_string(table_index) + ", permutation batch " +
                                                  std::to_string(zero_batch) + " has a row whose denominator is zero");
    }
};

// One permutation batch (permutation.rs:103-187): num / den of every row, then their running product, in `col`; the batch's Z
// column is that product moved down one row.  tot: scan_tot_stride(n) words.
static void perm_z_batch(DeviceCtx* ctx, const DevTable& tv, const u64* d_batch, unsigned b, u64* col, u64* tot, unsigned* d_zero_den) {
    const size_t n = tv.n();
    hipLaunchKernelGGL(perm_factor_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, tv.vals, n, d_batch, col, b, d_zero_den);
    scan_inclusive<ScanProduct, false>(ctx->stream, col, n, 1, tot);
}

// compute_permutation_z_polys: zcols[nperm][n]
static void perm_z_columns(DeviceCtx* ctx, DevBuf& mem, const DevTable& tv, const PermDesc& pd, u64* zcols, u64* tot, unsigned* d_zero_den) {
    if (!pd.nperm()) return;
    const size_t n = tv.n();
    u64* tmpcol = mem.alloc(n);
    u64* d_pd = mem.upload(pd.words);
    for (int b = 0; b < pd.nperm(); b++) {
        perm_z_batch(ctx, tv, d_pd + pd.batch_off[b], (unsigned)b, tmpcol, tot, d_zero_den);
        hipLaunchKernelGGL(shift_right_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, tmpcol, zcols + (size_t)b * n, n);
    }
}

// The table's columns of cross_table_lookup_data (cross_table_lookup.rs:224-311), zcols[cd.ncols][n]: one launch per step for all
// of them.  tot: cd.ncols * scan_tot_stride(n) words.
static void ctl_z_columns(DeviceCtx* ctx, DevBuf& mem, const DevTable& tv, const CtlDesc& cd, u64* zcols, u64* tot, unsigned* d_bad_filter) {
    if (!cd.ncols) return;
    const size_t n = tv.n();
    u64* d_words = mem.upload(cd.words);
    u64* d_index = mem.upload(cd.index);
#define OLA_CTL_FACTOR(G)                                                                                                                      \
    hipLaunchKernelGGL(ctl_factor_kernel<G>, dim3((unsigned)((n + 255) / 256), (unsigned)cd.ngroups()), dim3(256), 0, ctx->stream, tv.vals, n, \
                       d_words, d_index, d_index + cd.ncols, zcols, d_bad_filter)
    OLA_FOR_NCH(cd.group, OLA_CTL_FACTOR)
#undef OLA_CTL_FACTOR
    scan_inclusive<ScanProduct, false>(ctx->stream, zcols, n, cd.ncols, tot);
}

// ---- quotient (prover.rs:571-705) ----
static int quotient_degree_bits(const HTable& air) { int qdb = 0; while ((1 << qdb) < air.quotient_degree_factor()) qdb++; return qdb; }

// what a table's quotient is computed from
struct QuotientIn {
    const HTable& air; const OlaBatch &trace_c, &zs_c;
    const PermSets& perm_sets; const PermDesc& pd; const std::vector<CtlJob>& ctl; const CtlDesc& cd;
    const u64* params; std::vector<u64> alpha;      // one alpha per challenge
};

// the descriptor quotient_kernel interprets: a header of QD_HEAD words, then the constraint program, the permutation and lookup
// descriptors and the parameters
static std::vector<u64> quotient_desc(const QuotientIn& in, int degree_bits, int qdb) {
    std::vector<u64> desc(QD_HEAD, 0);
    // Z_H(x)^-1 per coset (zero_poly_coset.rs:18-33): x^n = 7^n * v^i, i = natural index mod 2^qdb; coset c <-> i = bitrev
    u64 g_pow_n = GL_GENERATOR;
    for (int i = 0; i < degree_bits; i++) g_pow_n = gl_mul(g_pow_n, g_pow_n);
    const u64 v = gl_root_of_unity(qdb);
    for (int c = 0; c < (1 << qdb); c++) {
        const u32 i = bitrev32((u32)c, qdb);
        desc[QD_ZH + c] = gl_inv(gl_sub(gl_mul(g_pow_n, gl_pow(v, i)), 1));
    }
    desc[0] = in.air.ops.size() / 2;
    desc[1] = desc.size();
    desc.insert(desc.end(), in.air.ops.begin(), in.air.ops.end());
    desc[2] = (u64)in.pd.nperm();
    desc[3] = desc.size();
    desc.insert(desc.end(), in.pd.words.begin(), in.pd.words.end());
    desc[4] = in.ctl.size();
    desc[5] = desc.size();
    desc.insert(desc.end(), in.cd.words.begin(), in.cd.words.end());
    desc[6] = (u64)in.air.n_params;
    desc[7] = desc.size();
    for (int i = 0; i < in.air.n_params; i++) desc.push_back(gl_canon(in.params[i]));
    for (size_t a = 0; a < in.alpha.size(); a++) desc[QD_ALPHA + a] = in.alpha[a];
    return desc;
}

// the descriptor of a specialised kernel (airq.cuh): Z_H^-1 per coset, the alpha powers of its emits, the parameters, the challenges
// in the kernel's own order, then the limb forms of the uniform multipliers
static std::vector<u64> spec_quotient_desc(const QuotientIn& in, const AirKernelEntry& spec, const std::vector<u64>& desc, int qdb, int nch) {
    const int K = spec.n_emits, bs = in.air.permutation_batch_size();
    std::vector<u64> sd(8 + (size_t)nch * K, 0);
    for (int c = 0; c < (1 << qdb); c++) sd[c] = desc[QD_ZH + c];
    for (int c = 0; c < nch; c++) {
        u64 w = 1;
        for (int i = K - 1; i >= 0; i--) { sd[8 + (size_t)c * K + i] = w; w = gl_mul(w, in.alpha[c]); }
    }
    for (int i = 0; i < in.air.n_params; i++) sd.push_back(gl_canon(in.params[i]));
    for (int b = 0; b < in.pd.nperm(); b++)
        for (int i = 0; i < bs; i++)
            for (int k = 0; k < 2; k++) {
                const int inst = b * bs + i;
                const bool live = inst < (int)in.air.perm_pairs.size() * nch;
                sd.push_back(live ? (k ? in.perm_sets[i][inst % nch].gamma : in.perm_sets[i][inst % nch].beta) : 0);
            }
    for (auto& jb : in.ctl) {
        sd.push_back(jb.ch.gamma);
        u64 bp = 1;
        for (size_t k = 0; k < jb.twc->columns.size(); k++) { sd.push_back(bp); bp = gl_mul(bp, jb.ch.beta); }
    }
    // limb forms of the uniform multipliers (airq.cuh Acc3), one slot per use in the kernel's own order
    auto push_limbs = [&sd](u64 w) {
        w = gl_canon(w);
        const u64 v = gl_mul(w, (u64)1 << 32), M = 0x3FFFFF;
        sd.push_back((w & M) | (((w >> 22) & M) << 32));
        sd.push_back((w >> 44) | ((v & M) << 32));
        sd.push_back(((v >> 22) & M) | ((v >> 44) << 32));
    };
    const size_t u64_words = sd.size();
    sd.reserve(u64_words + 3 * (size_t)spec.n_limbs);
    for (int sl = 0; sl < spec.n_limbs; sl++) {
        if ((size_t)spec.limb_src[sl] >= u64_words) throw OlaError(OLA_E_INVALID_ARG, "generated kernel and descriptor disagree");
        push_limbs(sd[(size_t)spec.limb_src[sl]]);
    }
    return sd;
}

// The quotient polynomials (one per challenge) as coefficients over the 2^qdb-coset domain; of each only the first n * q may be non-zero, which
// the device has looked at: check() after the next wait of the host.
struct QuotientPolys {
    u64* coef; size_t n, size; int q, nch;
    HostSpan too_high; const DeviceCtx* ctx;
    void check() const {
#ifndef AIRQ_TIMING_ONLY_L2_LOADS      // (timing builds of airq.cuh's experiment produce garbage on purpose)
        if ((unsigned)too_high[0] && !ctx->priming) throw OlaError(OLA_E_QUOTIENT_DEGREE, "Quotient has failed, the vanishing polynomial is not divisible by Z_H");
#endif
    }
};

// compute_quotient_polys: the constraints on the LDE domain -- all of it, this rank's cosets (sharded) or coset by coset (a
// memory-lean table) --, then back to coefficients
static QuotientPolys quotient_polys(DeviceCtx* ctx, DevBuf& mem, NttTables& tables, const OlaGpuConfig& cfg, const QuotientIn& in, bool sharded) {
    const HTable& air = in.air;
    const OlaBatch &trace_c = in.trace_c, &zs_c = in.zs_c;
    const int degree_bits = (int)trace_c.log_n, rate_bits = (int)cfg.rate_bits;
    const size_t n = (size_t)1 << degree_bits, N = n << rate_bits;
    const bool lean = trace_c.lean;
    // this rank's part of the LDE domain (everything when not sharded)
    const uint32_t log_world = sharded ? ctx->shard.log_world : 0;
    const size_t coset_count = ((size_t)1 << rate_bits) >> log_world, coset_first = sharded ? ctx->shard.rank * coset_count : 0;
    const size_t N_loc = n * coset_count;
    const int q = air.quotient_degree_factor(), qdb = quotient_degree_bits(air);
    if (qdb > rate_bits) throw OlaError(OLA_E_INVALID_ARG, "Having constraints of degree higher than the rate is not supported yet.");
    const size_t size = n << qdb;
    const int nch = (int)cfg.num_challenges;
    // Lagrange first/last on the LDE domain (leaf order)
    u64* lag_coef = mem.alloc(2 * n);
    u64* lag_lde = mem.alloc(2 * (lean ? n : N_loc));
    {
        TwoLevel gt = get_two(tables, degree_bits, 0);
        const u64 n_inv = gl_inv(((u64)1 << degree_bits) % GL_P);
        hipLaunchKernelGGL(lagrange_coeffs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, lag_coef, n, n_inv, gt.lo, gt.hi, gt.h);
        WorkScope ws(ctx, rate_bits);
        if (!lean) ntt_lde_leaf_order(tables, lag_coef, lag_lde, degree_bits, rate_bits, 2, coset_first, coset_count);
    }
    const std::vector<u64> desc = quotient_desc(in, degree_bits, qdb);
    u64* d_desc = mem.upload(desc);
    u64* qv = mem.alloc((size_t)nch * size);
    // points this rank evaluates: the whole quotient domain, or (sharded) those of its cosets that belong to the quotient
    // domain -- the first 2^qdb cosets of the leaf order; a rank that owns none of them only takes part in the exchange
    const size_t plane = sharded ? N_loc : size;
    u64* qloc = sharded ? mem.alloc((size_t)nch * plane) : qv;
    const size_t q_cosets = (size_t)1 << qdb;
    const size_t my_q_cosets = !sharded ? q_cosets : (coset_first >= q_cosets ? 0 : std::min(coset_count, q_cosets - coset_first));
    {
        QuotParams P = {};
        P.trace_lde = trace_c.lde; P.zs_lde = zs_c.lde; P.lag_lde = lag_lde;
        P.N = N_loc; P.n = n; P.log_n = degree_bits; P.log_N = degree_bits + rate_bits; P.qdb = qdb;
        P.coset_first = (u32)coset_first; P.out_plane = plane;
        TwoLevel gN = get_two(tables, degree_bits + rate_bits, 0);
        P.gN_lo = gN.lo; P.gN_hi = gN.hi; P.gN_h = gN.h;
        P.desc = d_desc;
        P.g_inv = gl_inv(gl_root_of_unity(degree_bits));
        P.out = qloc;
        P.n_regs = air.n_regs;
        // OLA_AIR_KERNELS=interpreter forces the generic kernel, =crosscheck runs both and compares (tests)
        const char* mode = getenv("OLA_AIR_KERNELS");
        const bool force_interp = mode && !strcmp(mode, "interpreter"), crosscheck = mode && !strcmp(mode, "crosscheck");
        std::vector<const HTwc*> twcs;
        for (auto& jb : in.ctl) twcs.push_back(jb.twc);
        // the specialised kernels address rows as "workgroup base + lane": workgroups of min(AIRQ_THREADS, n) threads (airq.cuh)
        const AirKernelEntry* spec = force_interp ? nullptr : find_air_kernel(air_signature(air, twcs, nch));
        const unsigned spec_bs = (unsigned)std::min<size_t>(AIRQ_THREADS, n);
        // memory-lean: the trace and Z values of one coset at a time, re-derived from the coefficients; the quotient of a table
        // with 2^qdb < 2^rate_bits cosets lives on the first 2^qdb cosets of the leaf order
        u64 *slice_t = nullptr, *slice_z = nullptr;
        const size_t lean_cosets = lean ? ((size_t)1 << qdb) : 1;
        if (lean) {
            slice_t = mem.alloc((size_t)trace_c.ncols * n);
            slice_z = mem.alloc((size_t)zs_c.ncols * n);
            P.trace_lde = slice_t; P.zs_lde = slice_z; P.N = n; P.npoints = n;
        }
        u64* d_sd = spec ? mem.upload(spec_quotient_desc(in, *spec, desc, qdb, nch)) : nullptr;
        u64* qv2 = (spec && crosscheck) ? mem.alloc((size_t)nch * plane) : nullptr;
        WorkScope ws(ctx, qdb);   // the quotient lives on 2^qdb cosets: that many ranks share it
        // units: LDE points evaluated; bytes a point streams -- local and next row of the trace and Z batches, one plane per challenge written
        // (quotient row streaming is priced against HBM)
        const double q_points = (double)(sharded ? my_q_cosets * n : size);
        PhaseScope phq(ctx, PH_QUOTIENT, q_points, q_points * (8.0 * 2 * ((double)trace_c.ncols + (double)zs_c.ncols) + 8.0 * nch));
        if (!sharded && ctx->acct.shardable) for (int c = 0; c < nch; c++) acct_exchange(ctx, N * 8);   // the planes a partitioned run gathers
        for (size_t lc = 0; lc < lean_cosets; lc++) {
            u64* out = qloc;
            size_t points = sharded ? my_q_cosets * n : plane;
            if (sharded) { P.npoints = points; if (points == 0) break; }
            if (lean) {
                batch_lde_slice(ctx, tables, trace_c, lc, slice_t);
                batch_lde_slice(ctx, tables, zs_c, lc, slice_z);
                ntt_lde_leaf_order(tables, lag_coef, lag_lde, degree_bits, rate_bits, 2, lc, 1);
                P.coset_first = (u32)lc;
                out = qloc + lc * n;
                points = n;
            }
            auto run_interp_on = [&](u64* o) {
                P.out = o;
                const size_t lds = (size_t)air.n_regs * QW * 8;
                if (lds > 160 * 1024) throw OlaError(OLA_E_INVALID_ARG, "constraint program needs too many registers");
#define OLA_QUOTIENT_INTERP(NCH)                                                                                                          \
    if (lds > 48 * 1024)                                                                                                                  \
        HIP_CHECK(hipFuncSetAttribute((const void*)quotient_kernel<NCH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));         \
    hipLaunchKernelGGL(quotient_kernel<NCH>, dim3((unsigned)((points + QW - 1) / QW)), dim3(QW), lds, ctx->stream, P)
                OLA_FOR_NCH(nch, OLA_QUOTIENT_INTERP)
#undef OLA_QUOTIENT_INTERP
            };
            if (!spec) {
                run_interp_on(out);
            } else {
                QuotParams S = P;
                S.desc = d_sd;
                S.out = out;
                hipLaunchKernelGGL(spec->kernel, dim3((unsigned)((points + spec_bs - 1) / spec_bs)), dim3(spec_bs), 0, ctx->stream, S);
                if (crosscheck) run_interp_on(qv2 + (lean ? lc * n : 0));
            }
        }
        if (spec && crosscheck) {
            unsigned* d_flag = (unsigned*)mem.alloc(1);
            HIP_CHECK(hipMemsetAsync(d_flag, 0, 8, ctx->stream));
            const size_t evaluated = sharded ? my_q_cosets * n : plane;       // per plane
            for (int c = 0; c < nch && evaluated; c++)
                hipLaunchKernelGGL(any_diff_kernel, dim3((unsigned)((evaluated + 255) / 256)), dim3(256), 0, ctx->stream, qloc + (size_t)c * plane,
                                   qv2 + (size_t)c * plane, evaluated, d_flag);
            unsigned flag = 0;
            HIP_CHECK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            if (flag) throw OlaError(OLA_E_INTERNAL, std::string("specialised quotient kernel disagrees with the interpreter: ") + spec->name);
        }
    }
    if (sharded) {
        // every rank needs the whole quotient for the inverse transform: gather the ranks' planes (rank order = leaf order) and
        // keep the first n * 2^qdb values of each
        if (N == size) {
            for (int c = 0; c < nch; c++) shard_all_gather(ctx, qloc + (size_t)c * plane, qv + (size_t)c * size, plane * 8);
        } else {
            u64* gath = mem.alloc(N);
            for (int c = 0; c < nch; c++) {
                shard_all_gather(ctx, qloc + (size_t)c * plane, gath, plane * 8);
                HIP_CHECK(hipMemcpyAsync(qv + (size_t)c * size, gath, size * 8, hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
    }
    // qv is in bit-reversed order of the size-domain: un-reverse, coset iNTT (prover.rs:700-704)
    const int size_bits = degree_bits + qdb;
    u64* qnat = mem.alloc((size_t)nch * size);
    QuotientPolys qp = {mem.alloc((size_t)nch * size), n, size, q, nch, mem.host(1), ctx};
    u64* qscratch = size_bits > 13 ? mem.alloc((size_t)nch * size) : nullptr;
    launch_bitrev_rows(ctx, qv, qnat, size_bits, nch);
    ntt_coset_interpolate(tables, qnat, qp.coef, qscratch, size_bits, nch, GL_GENERATOR);
    // trim_to_len(n*q) (prover.rs:469-473): nothing may be left above
    qp.too_high[0] = 0;
    const size_t keep = n * (size_t)q;
    if (keep < size) {
        unsigned* d_flag = (unsigned*)mem.alloc(1);
        HIP_CHECK(hipMemsetAsync(d_flag, 0, 8, ctx->stream));
        for (int c = 0; c < nch; c++)
            hipLaunchKernelGGL(any_nonzero_kernel, dim3((unsigned)((size - keep + 255) / 256)), dim3(256), 0, ctx->stream, qp.coef + (size_t)c * size,
                               keep, size, d_flag);
        // read with the next read-back the host waits for (the quotient commitment's cap, or an entry point's copy): no wait of its own
        HIP_CHECK(hipMemcpyAsync(&qp.too_high[0], d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    return qp;
}

// chunks of n coefficients: [challenge][k] -> column challenge * q + k
static u64* split_quotient(DeviceCtx* ctx, DevBuf& mem, const QuotientPolys& qp) {
    const size_t keep = qp.n * (size_t)qp.q;
    u64* chunks = mem.alloc((size_t)qp.nch * keep);
    for (int c = 0; c < qp.nch; c++)
        HIP_CHECK(hipMemcpyAsync(chunks + (size_t)c * keep, qp.coef + (size_t)c * qp.size, keep * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return chunks;
}

// prove_single_table (prover.rs:330-567): the transcript, and the steps above between its draws and observations
static void prove_single_table(DeviceCtx* ctx, NttTables& tables, const OlaGpuConfig& cfg, const HTable& air, const DevTable& tv,
                               const OlaBatch& trace_c, const std::vector<u64>& trace_cap, const std::vector<CtlJob>& ctl,
                               const u64* params, OlaChallenger& ch, std::vector<uint8_t>& bytes, bool sharded, int table_index,
                               PowDefer* pow_defer = nullptr) {
    DevBuf mem(ctx);
    const int nch = (int)cfg.num_challenges;
    const size_t n = tv.n();
    challenger_compact(ch);
    // ---- permutation challenges + Z polys (prover.rs:360-377) ----
    const PermSets perm_sets = draw_perm_sets(air, nch, ch);
    const PermDesc pd = build_perm_desc(air, perm_sets, nch);
    const CtlDesc cd = build_ctl_desc(ctl, nch);
    const int nperm = pd.nperm(), nz = nperm + (int)ctl.size();
    if (nz == 0) throw OlaError(OLA_E_INVALID_ARG, "No CTL?");
    // OLA_TIMING scopes carry the reference's `timed!` names (prover.rs:374-544)
    // (the reference times only the permutation Z's, and only for tables that have permutation arguments, prover.rs:371-377; its
    // CTL Z's are computed untimed in cross_table_lookup_data, cross_table_lookup.rs:224-311 -- here both happen in this scope)
    std::unique_ptr<PhaseTimer> ph(new PhaseTimer(ctx, nperm > 0 ? "    compute permutation Z(x) polys" : "    compute CTL Z(x) polys"));
    u64* zvals = mem.alloc((size_t)nz * n);
    u64* tot = mem.alloc(scan_tot_stride(n) * std::max<size_t>(1, ctl.size()));
    const ZFlags zf(ctx, mem, table_index);
    perm_z_columns(ctx, mem, tv, pd, zvals, tot, zf.zero_den());
    ctl_z_columns(ctx, mem, tv, cd, zvals + (size_t)nperm * n, tot, zf.bad_filter());
    zf.fetch(ctx);
    // ---- Zs commitment ----
    ph.reset(); ph.reset(new PhaseTimer(ctx, "    compute Zs commitment"));
    const bool lean = trace_c.lean;   // the table is proven memory-lean: no LDE of its three batches is kept
    if (lean && sharded) throw OlaError(OLA_E_INTERNAL, "a memory-lean table cannot be on the coset partition");
    BatchHolder zs_c(ctx);
    std::vector<u64> zs_cap;
    zs_c.b = commit_shared(ctx, tables, zvals, (uint32_t)nz, tv.log_n, cfg, true, sharded, nullptr, zs_cap, lean);
    zf.check();                                          // commit_shared has waited for the cap
    challenger_observe_cap(ch, zs_cap.data(), zs_cap.size() / 4);
    std::vector<u64> alphas;                             // challenger.get_n_challenges (prover.rs:425)
    for (int c = 0; c < nch; c++) alphas.push_back(challenger_get(ch));

    ph.reset(); ph.reset(new PhaseTimer(ctx, "    compute quotient polys"));
    const QuotientIn qin = {air, trace_c, *zs_c.b, perm_sets, pd, ctl, cd, params, alphas};
    const QuotientPolys qp = quotient_polys(ctx, mem, tables, cfg, qin, sharded);
    ph.reset(); ph.reset(new PhaseTimer(ctx, "    split quotient polys"));
    u64* chunks = split_quotient(ctx, mem, qp);
    ph.reset(); ph.reset(new PhaseTimer(ctx, "    compute quotient commitment"));
    BatchHolder q_c(ctx);
    std::vector<u64> q_cap;
    q_c.b = commit_shared(ctx, tables, chunks, (uint32_t)(nch * qp.q), tv.log_n, cfg, false, sharded, nullptr, q_cap, lean);
    qp.check();                                          // commit_shared has waited for the cap
    challenger_observe_cap(ch, q_cap.data(), q_cap.size() / 4);

    // ---- write_proof (serialization.rs:349-358): caps, then opening set + FRI proof ----
    ByteWriter w{bytes, digest_wire_bytes((uint32_t)ctx->hasher)};
    write_cap(w, trace_cap);
    write_cap(w, zs_cap);
    write_cap(w, q_cap);
    size_t olen = 0;
    ph.reset(); ph.reset(new PhaseTimer(ctx, "    compute openings proof"));
    open_and_prove(ctx, tables, cfg, trace_c, *zs_c.b, *q_c.b, (uint32_t)nperm, ch, bytes, olen, pow_defer);
}

// Per table, the running products it must carry: one per (lookup it takes part in, challenge), looking sides before the
// looked side, lookups in declaration order (cross_table_lookup_data, cross_table_lookup.rs:224-311).
static std::vector<std::vector<CtlJob>> ctl_jobs(const HAirSet& set, const std::vector<GpChallenge>& ctl_ch) {
    std::vector<std::vector<CtlJob>> jobs(set.tables.size());
    for (const HCtl& ctl : set.ctls)
        for (const GpChallenge& c : ctl_ch) {
            for (const HTwc& twc : ctl.looking) jobs[twc.table].push_back({&twc, c});
            jobs[ctl.looked.table].push_back({&ctl.looked, c});
        }
    return jobs;
}

// One table's StarkProof with the trace commitment and the transcript supplied by the caller (ola_prove_single_table).
void prove_single_table_host(DeviceCtx* ctx, NttTables& tables, const OlaGpuConfig& cfg, const u64* airset, size_t airset_words,
                             uint32_t table, const u64* const* trace_cols, const OlaBatch& trace_c, const u64* trace_cap,
                             const u64* ctl_challenges, const u64* params, OlaChallenger& ch, std::vector<uint8_t>& bytes) {
    const HAirSet set = parse_airset_with_table(airset, airset_words, table);
    if (ctx->shard.world != 1) throw OlaError(OLA_E_INVALID_ARG, "per-table proving needs an unsharded context");
    const HTable& air = set.tables[table];
    if (trace_c.ncols != (uint32_t)air.ncols || trace_c.is_shard()) throw OlaError(OLA_E_INVALID_ARG, "trace commitment does not match the table");
    const std::vector<std::vector<CtlJob>> jobs = ctl_jobs(set, read_challenges(ctl_challenges, cfg.num_challenges));
    DevBuf mem(ctx);
    const DevTable tv = upload_table(ctx, mem, trace_cols, air.ncols, trace_c.log_n);
    const std::vector<u64> cap(trace_cap, trace_cap + 4 * ((size_t)1 << cfg.cap_height));
    prove_single_table(ctx, tables, cfg, air, tv, trace_c, cap, jobs[table], params_or_zero(params, 0, air), ch, bytes, false, (int)table);
}

// Widths of a table's three batches (trace, Z, quotient chunks)
struct TableWidths { size_t w, wz, wq; int qdb; };
static TableWidths table_widths(const HAirSet& set, size_t t, int nch) {
    const HTable& air = set.tables[t];
    size_t nctl = 0;
    for (const HCtl& c : set.ctls) { for (const HTwc& w2 : c.looking) nctl += ((size_t)w2.table == t) ? nch : 0; nctl += ((size_t)c.looked.table == t) ? nch : 0; }
    TableWidths r;
    r.w = (size_t)air.ncols; r.wz = air.num_permutation_batches(nch) + nctl; r.wq = (size_t)nch * air.quotient_degree_factor();
    r.qdb = quotient_degree_bits(air);
    return r;
}

// ---- phase-level entry points (one `timed!` scope of the reference at a time) --------------------------------
// out[6] = ncols, n_params, permutation Z columns, CTL Z columns, quotient_degree_factor, permutation batch size
void table_shape_host(const OlaGpuConfig& cfg, const u64* airset, size_t airset_words, uint32_t table, uint32_t out[6]) {
    const HAirSet set = parse_airset_with_table(airset, airset_words, table);
    const TableWidths tw = table_widths(set, table, (int)cfg.num_challenges);
    const HTable& air = set.tables[table];
    const uint32_t nperm = (uint32_t)air.num_permutation_batches((int)cfg.num_challenges);
    out[0] = (uint32_t)air.ncols; out[1] = (uint32_t)air.n_params; out[2] = nperm; out[3] = (uint32_t)tw.wz - nperm;
    out[4] = (uint32_t)air.quotient_degree_factor(); out[5] = (uint32_t)air.permutation_batch_size();
}

// after the steps of an entry point: one wait, what the device found wrong with the input, and only then the result into the
// caller's buffer -- a refused call leaves it untouched.  Staged in the scope's host memory (pinned while the arena has room).
template <class Finding>
static void hand_back(DeviceCtx* ctx, DevBuf& mem, u64* out, const u64* d_result, size_t words, const Finding& finding) {
    HostSpan staged = mem.host(words);
    HIP_CHECK(hipMemcpyAsync(staged.data(), d_result, words * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    finding.check();
    memcpy(out, staged.data(), words * 8);
}

// compute_permutation_z_polys (permutation.rs:103-187): the permutation Z columns as values over the trace domain (ola_perm_z)
void perm_z_host(DeviceCtx* ctx, const OlaGpuConfig& cfg, const u64* airset, size_t airset_words, uint32_t table, uint32_t log_n,
                 const u64* const* trace_cols, const u64* perm_challenges, u64* z_out) {
    const HAirSet set = parse_airset_with_table(airset, airset_words, table);
    const HTable& air = set.tables[table];
    const int nch = (int)cfg.num_challenges;
    if (table_widths(set, table, nch).wz == 0) throw OlaError(OLA_E_INVALID_ARG, "No CTL?");
    const PermDesc pd = build_perm_desc(air, read_perm_sets(air, nch, perm_challenges), nch);
    if (!pd.nperm()) return;
    DevBuf mem(ctx);
    PhaseTimer ph(ctx, "    compute permutation Z(x) polys");
    const DevTable tv = upload_table(ctx, mem, trace_cols, air.ncols, log_n);
    u64* z = mem.alloc((size_t)pd.nperm() * tv.n());
    const ZFlags zf(ctx, mem, (int)table);
    perm_z_columns(ctx, mem, tv, pd, z, mem.alloc(scan_tot_stride(tv.n())), zf.zero_den());
    zf.fetch(ctx);
    hand_back(ctx, mem, z_out, z, (size_t)pd.nperm() * tv.n(), zf);
}

// the table's share of cross_table_lookup_data (cross_table_lookup.rs:224-311): its CTL Z columns (ola_ctl_z)
void ctl_z_host(DeviceCtx* ctx, const OlaGpuConfig& cfg, const u64* airset, size_t airset_words, uint32_t table, uint32_t log_n,
                const u64* const* trace_cols, const u64* ctl_challenges, u64* z_out) {
    const HAirSet set = parse_airset_with_table(airset, airset_words, table);
    const HTable& air = set.tables[table];
    const int nch = (int)cfg.num_challenges;
    if (table_widths(set, table, nch).wz == 0) throw OlaError(OLA_E_INVALID_ARG, "No CTL?");
    const std::vector<std::vector<CtlJob>> jobs = ctl_jobs(set, read_challenges(ctl_challenges, nch));
    const CtlDesc cd = build_ctl_desc(jobs[table], nch);
    if (!cd.ncols) return;
    DevBuf mem(ctx);
    PhaseTimer ph(ctx, "    compute CTL Z(x) polys");
    const DevTable tv = upload_table(ctx, mem, trace_cols, air.ncols, log_n);
    u64* z = mem.alloc(cd.ncols * tv.n());
    const ZFlags zf(ctx, mem, (int)table);
    ctl_z_columns(ctx, mem, tv, cd, z, mem.alloc(cd.ncols * scan_tot_stride(tv.n())), zf.bad_filter());
    zf.fetch(ctx);
    hand_back(ctx, mem, z_out, z, cd.ncols * tv.n(), zf);
}

// compute_quotient_polys + the split into degree-n chunks (prover.rs:441-480, 571-705) on the caller's two commitments:
// coefficients of the num_challenges * q chunk polynomials, ready for PolynomialBatch::from_coeffs (ola_quotient)
void quotient_host(DeviceCtx* ctx, NttTables& tables, const OlaGpuConfig& cfg, const u64* airset, size_t airset_words, uint32_t table,
                   const OlaBatch& trace_c, const OlaBatch& zs_c, const u64* perm_challenges, const u64* ctl_challenges, const u64* alphas,
                   const u64* params, u64* chunks_out) {
    const HAirSet set = parse_airset_with_table(airset, airset_words, table);
    if (ctx->shard.world != 1) throw OlaError(OLA_E_INVALID_ARG, "per-phase proving needs an unsharded context");
    const HTable& air = set.tables[table];
    if (trace_c.ncols != (uint32_t)air.ncols || trace_c.is_shard()) throw OlaError(OLA_E_INVALID_ARG, "trace commitment does not match the table");
    if (!air.perm_pairs.empty() && !perm_challenges) throw OlaError(OLA_E_INVALID_ARG, "the table has permutation arguments: perm_challenges required");
    params = params_or_zero(params, 0, air);
    const int nch = (int)cfg.num_challenges;
    const std::vector<std::vector<CtlJob>> jobs = ctl_jobs(set, read_challenges(ctl_challenges, nch));
    const std::vector<CtlJob>& ctl = jobs[table];
    const PermSets perm_sets = read_perm_sets(air, nch, perm_challenges);
    const PermDesc pd = build_perm_desc(air, perm_sets, nch);
    const CtlDesc cd = build_ctl_desc(ctl, nch);
    const size_t nz = (size_t)pd.nperm() + ctl.size();
    if (nz == 0) throw OlaError(OLA_E_INVALID_ARG, "No CTL?");
    if (zs_c.ncols != nz || zs_c.log_n != trace_c.log_n || zs_c.lean != trace_c.lean || zs_c.is_shard())
        throw OlaError(OLA_E_INVALID_ARG, "Z commitment does not match the table");
    DevBuf mem(ctx);
    std::unique_ptr<PhaseTimer> ph(new PhaseTimer(ctx, "    compute quotient polys"));
    std::vector<u64> alpha;
    for (int c = 0; c < nch; c++) alpha.push_back(gl_canon(alphas[c]));
    const QuotientIn qin = {air, trace_c, zs_c, perm_sets, pd, ctl, cd, params, alpha};
    const QuotientPolys qp = quotient_polys(ctx, mem, tables, cfg, qin, false);
    ph.reset(); ph.reset(new PhaseTimer(ctx, "    split quotient polys"));
    hand_back(ctx, mem, chunks_out, split_quotient(ctx, mem, qp), (size_t)nch * qp.n * (size_t)qp.q, qp);
}

// Memory-lean tables (OLA_LEAN=1 forces, =0 forbids, default: when keeping every LDE resident would not fit): the LDEs of the
// large tables are streamed coset by coset instead of kept (batch_commit lean) -- a 2^24-row CPU table then proves on one GPU
// (fri/oracle.rs:66-99 holds all of it; the reference's GPU shim was sized for 2^24, cfft/ntt/mod.rs:13).
static std::vector<char> plan_lean_tables(DeviceCtx* ctx, const OlaGpuConfig& cfg, const HAirSet& set, const uint32_t* log_n) {
    const size_t nt = set.tables.size();
    const int nch = (int)cfg.num_challenges;
    std::vector<char> lean(nt, 0);
    const char* e = getenv("OLA_LEAN");
    const int mode = e ? atoi(e) : -1;
    size_t need = 0;
    for (size_t t = 0; t < nt; t++) {
        const TableWidths tw = table_widths(set, t, nch);
        const size_t n_t = (size_t)1 << log_n[t], w_all = tw.w + tw.wz + tw.wq;
        need += w_all * n_t * 8 * ((size_t)1 << cfg.rate_bits) + 3 * 2 * (n_t << cfg.rate_bits) * 32;   // LDEs + digest heaps
        need += (tw.w + w_all) * n_t * 8;                                                                // + values + coefficients
    }
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    // what the pool holds is available to the proof; blocks the reserver has not delivered yet are still part of free_b
    size_t cached;
    { std::lock_guard<std::mutex> lk(ctx->mu); cached = ctx->cached_bytes; }
    const size_t budget = (size_t)(0.80 * (double)(free_b + cached));
    const bool want = mode == 1 || (mode != 0 && need > budget);
    if (want && ctx->shard.world <= 1)
        for (size_t t = 0; t < nt; t++) lean[t] = (mode == 1) ? (log_n[t] >= 1) : (log_n[t] >= 20);
    if (ctx->timing) fprintf(stderr, "[ola-timing] resident proof would need about %.1f GB, %.1f GB available: %s\n", need / 1e9, budget / 1e9, want ? "memory-lean (coset-streamed) large tables" : "all LDEs resident");
    return lean;
}

// ola_gpu_reserve: the large device buffers prove_with_traces will ask for with these table heights, allocated by a helper
// thread into the context's pool while the caller is still busy elsewhere (reading the trace file, say).
void reserve_for_proof(DeviceCtx* ctx, const OlaGpuConfig& cfg, const u64* airset, size_t airset_words, const uint32_t* log_n) {
    HAirSet set = parse_airset(airset, airset_words);
    const size_t nt = set.tables.size();
    const int nch = (int)cfg.num_challenges;
    const std::vector<char> lean = plan_lean_tables(ctx, cfg, set, log_n);
    std::vector<size_t> sizes;
    auto batch_blocks = [&](size_t w, size_t n, bool is_lean) {
        const size_t N = n << cfg.rate_bits;
        sizes.push_back(w * n * 8);                      // coefficients
        sizes.push_back(2 * N * 32);                     // digest heap
        if (!is_lean) sizes.push_back(w * N * 8);        // LDE
    };
    // in the order the proof asks for them: the trace values of every large table (allocated before the upload starts), then the
    // commitment of each large table from the largest down (the order prove_with_traces commits in)
    std::vector<size_t> large;
    for (size_t t = 0; t < nt; t++)
        if (table_widths(set, t, nch).w * ((size_t)1 << log_n[t]) * 8 >= (64u << 20)) large.push_back(t);   // small tables allocate in microseconds
    for (size_t t : large) sizes.push_back(table_widths(set, t, nch).w * ((size_t)1 << log_n[t]) * 8);       // the trace values
    std::stable_sort(large.begin(), large.end(), [&](size_t a, size_t b) {
        return table_widths(set, a, nch).w << log_n[a] > table_widths(set, b, nch).w << log_n[b]; });
    for (size_t t : large) {
        const TableWidths tw = table_widths(set, t, nch);
        const size_t n = (size_t)1 << log_n[t];
        batch_blocks(tw.w, n, lean[t] != 0);
        if (lean[t]) sizes.push_back(tw.w * n * 8);      // the coset being hashed / transform scratch
    }
    // Z and quotient buffers go back to the pool when a table is done and are handed to the next table that asks for a size they
    // fit (alloc's rule: at most a quarter larger than wanted): reserve, in proving order, what no earlier table leaves behind
    std::vector<size_t> left_behind;
    std::sort(large.begin(), large.end());
    for (size_t t : large) {
        const TableWidths tw = table_widths(set, t, nch);
        const size_t n = (size_t)1 << log_n[t], size = n << tw.qdb;
        std::vector<size_t> mine;
        { std::vector<size_t> keep; keep.swap(sizes);
          sizes.push_back(tw.wz * n * 8);              // Z values
          batch_blocks(tw.wz, n, lean[t] != 0);
          for (int i = 0; i < 4; i++) sizes.push_back((size_t)nch * size * 8);   // quotient values, natural order, coefficients, scratch
          sizes.push_back(tw.wq * n * 8);              // chunks
          batch_blocks(tw.wq, n, lean[t] != 0);
          if (lean[t]) { sizes.push_back(tw.w * n * 8); sizes.push_back(tw.wz * n * 8); }
          mine.swap(sizes); sizes.swap(keep); }
        std::vector<size_t> avail = left_behind;
        for (size_t raw : mine) {
            const size_t want = DeviceCtx::round_size(raw);
            if (want < (32u << 20)) continue;
            size_t best = avail.size();
            for (size_t i = 0; i < avail.size(); i++)
                if (avail[i] >= want && avail[i] <= want + want / 4 && (best == avail.size() || avail[i] < avail[best])) best = i;
            if (best < avail.size()) { avail.erase(avail.begin() + (long)best); continue; }
            sizes.push_back(raw);
            left_behind.push_back(want);
        }
    }
    ctx->reserve_async(sizes);                            // delivered in this order
}

// prove_with_traces (prover.rs:79-327).  traces[t]: where table t's columns are -- one column-major ncols x 2^log_n[t] block, or one
// pointer per column (the reference's Vec<PolynomialValues<F>>, prover.rs:79-83) -- see upload.h.
void prove_with_traces(DeviceCtx* ctx, NttTables& tables, const OlaGpuConfig& cfg, const u64* airset, size_t airset_words,
                       const TraceSource* traces, const uint32_t* log_n, const u64* params, const u64* compress,
                       std::vector<uint8_t>& bytes) {
    HAirSet set = parse_airset(airset, airset_words);
    const size_t nt = set.tables.size();
    const int nch = (int)cfg.num_challenges;
    const size_t len_cap = (size_t)1 << cfg.cap_height;
    DevBuf mem(ctx);
    std::vector<DevTable> dev(nt);
    std::vector<std::unique_ptr<BatchHolder>> commits;
    std::vector<std::vector<u64>> caps(nt, std::vector<u64>(len_cap * 4));
    OlaChallenger ch;
    challenger_init(ch, (uint32_t)ctx->hasher);
    PhaseTimer t_all(ctx, "prove_with_traces total");
    // Coset partition: a sharded table's columns are uploaded 1/world per rank and all-gathered device to device (xGMI instead of
    // `world` copies of the trace over the host's PCIe links); cpr = columns per rank, the last ranks may hold fewer or none.
    const uint32_t world = ctx->shard.world, rank = ctx->shard.rank;
    std::vector<uint32_t> cpr(nt, 0);
    for (size_t t = 0; t < nt; t++) {
        if (log_n[t] + cfg.rate_bits > 32 || log_n[t] + cfg.rate_bits < cfg.cap_height) throw OlaError(OLA_E_INVALID_ARG, "table size out of range");
        dev[t].log_n = log_n[t];
        const uint32_t w = (uint32_t)set.tables[t].ncols;
        if (table_is_sharded(ctx, cfg, set.tables[t], log_n[t])) cpr[t] = (w + world - 1) / world;
        dev[t].vals = mem.alloc((size_t)(cpr[t] ? cpr[t] * world : w) << log_n[t]);
    }
    // The traces are pageable host memory: the uploader's threads push them to the device through a pinned staging ring on
    // their own stream while this thread already interpolates / extends / hashes what has arrived (upload.h).
    const std::vector<char> lean = plan_lean_tables(ctx, cfg, set, log_n);
    TraceUploader up(ctx, nt);
    std::vector<uint32_t> own_cols(nt, 0);
    for (size_t t = 0; t < nt; t++) {
        const size_t n_t = (size_t)1 << log_n[t];
        const uint32_t w = (uint32_t)set.tables[t].ncols;
        if (cpr[t]) {
            const uint32_t c0 = std::min(w, rank * cpr[t]), c1 = std::min(w, (rank + 1) * cpr[t]);
            own_cols[t] = c1 - c0;
            up.add(t, traces[t], c0, dev[t].vals + (size_t)c0 * n_t, own_cols[t], n_t);
        } else {
            up.add(t, traces[t], 0, dev[t].vals, w, n_t);
        }
    }
    // Order of upload and commitment (the caps enter the transcript in table order afterwards, prover.rs:139-142): the tables
    // below 64 MB first -- their commitments then run in the shadow of the large upload instead of after it --, then the large
    // ones from the largest down: what is left to do when the last byte arrives is one column group and the Merkle tree of
    // the smallest large table, and the largest tree (190 ms for the CPU table under Poseidon) overlaps the rest of the upload.
    std::vector<size_t> order(nt);
    for (size_t t = 0; t < nt; t++) order[t] = t;
    {
        auto bytes_of = [&](size_t t) { return ((size_t)set.tables[t].ncols << log_n[t]) * 8; };
        const size_t big = (size_t)64 << 20;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            const bool la = bytes_of(a) >= big, lb = bytes_of(b) >= big;
            if (la != lb) return lb;                       // small ones first
            return la && bytes_of(a) > bytes_of(b);        // large: descending; small: as numbered
        });
    }
    up.set_order(order);
    up.start();
    std::unique_ptr<PhaseTimer> t_commit(new PhaseTimer(ctx, "compute trace commitments"));
    commits.resize(nt);
    for (size_t t : order) {
        ctx->scopes.table = (int)t;
        PhaseTimer tt(ctx, "  table " + std::to_string(t) + " trace commitment (upload overlapped)");
        const size_t n_t = (size_t)1 << log_n[t];
        ctx->acct.shardable = log_n[t] >= ctx->shard.min_log_n;
        if (ctx->acct.shardable && !cpr[t]) acct_exchange(ctx, (size_t)set.tables[t].ncols * n_t * 8);   // the trace values a partitioned run gathers
        ColumnFeed feed;
        feed.chunk_cols = up.chunk_cols(t);
        feed.before_chunk = [&, t, n_t](uint32_t c0, uint32_t c1) {
            up.wait(t, c1);
            // columns that crossed the link as 32-bit words are canonical as they arrive: only runs of the others are reduced
            for (uint32_t c = c0; c < c1;) {
                if (up.column_is_narrow(t, c)) { c++; continue; }
                uint32_t e = c + 1;
                while (e < c1 && !up.column_is_narrow(t, e)) e++;
                canonicalize(ctx, dev[t].vals + (size_t)c * n_t, (size_t)(e - c) * n_t);
                c = e;
            }
        };
        commits[t].reset(new BatchHolder(ctx));
        if (cpr[t]) {
            // this rank's columns have to be on the device, then every rank receives everybody's
            up.wait(t, own_cols[t]);
            const size_t blk = (size_t)cpr[t] * n_t;
            DevBuf tmp(ctx);
            u64* send = tmp.alloc(blk);
            HIP_CHECK(hipMemcpyAsync(send, dev[t].vals + (size_t)rank * blk, blk * 8, hipMemcpyDeviceToDevice, ctx->stream));
            shard_all_gather(ctx, send, dev[t].vals, blk * 8);
            canonicalize(ctx, dev[t].vals, (size_t)set.tables[t].ncols * n_t);
            commits[t]->b = commit_shared(ctx, tables, dev[t].vals, (uint32_t)set.tables[t].ncols, log_n[t], cfg, true, true, nullptr, caps[t], false);
            continue;
        }
        commits[t]->b = commit_shared(ctx, tables, dev[t].vals, (uint32_t)set.tables[t].ncols, log_n[t], cfg, true,
                                      table_is_sharded(ctx, cfg, set.tables[t], log_n[t]), &feed, caps[t], lean[t] != 0);
    }
    up.finish();
    ctx->scopes.table = -1;
    t_commit.reset();
    for (size_t t = 0; t < nt; t++) challenger_observe_cap(ch, caps[t].data(), caps[t].size() / 4);
    // CTL challenges and per-table job lists, in cross_table_lookup_data order
    std::vector<GpChallenge> ctl_ch;
    for (int c = 0; c < nch; c++) ctl_ch.push_back(get_gp(ch));
    const std::vector<std::vector<CtlJob>> jobs = ctl_jobs(set, ctl_ch);
    ByteWriter w{bytes, digest_wire_bytes((uint32_t)ctx->hasher)};
    w.u32((uint32_t)nt);
    size_t poff = 0;
    // the proof-of-work searches of the tables run on the side stream and are collected at the end (fri.hip PowDefer); the
    // slots are this scope's, allocated before any inner scope exists (the pinned arena is a stack).  OLA_POW_DEFER=0: in line.
    PowDefer pow;
    static const bool pow_defer_on = [] { const char* e = getenv("OLA_POW_DEFER"); return !(e && *e == '0'); }();
    if (pow_defer_on) { pow.slots = (unsigned long long*)ctx->pinned_alloc(nt * 8); pow.nslots = pow.slots ? nt : 0; }
    struct PowGuard { DeviceCtx* c; PowDefer& p; ~PowGuard() { pow_abandon(c, p); } } pow_guard{ctx, pow};
    for (size_t t = 0; t < nt; t++) {
        const u64* pr = params_or_zero(params, poff, set.tables[t]);
        poff += set.tables[t].n_params;
        ctx->scopes.table = (int)t;
        PhaseTimer tt(ctx, "  table " + std::to_string(t) + " prove_single_table");
        ctx->acct.shardable = log_n[t] >= ctx->shard.min_log_n;
        prove_single_table(ctx, tables, cfg, set.tables[t], dev[t], *commits[t]->b, caps[t], jobs[t], pr, ch, bytes,
                           table_is_sharded(ctx, cfg, set.tables[t], log_n[t]), (int)t, &pow);
    }
    pow_finish(ctx, pow, bytes);
    ctx->acct.shardable = false;
    // compress_challenges (prover.rs:307-320) -- produced by trace generation, carried through
    w.u32((uint32_t)nt);
    for (size_t t = 0; t < nt; t++) w.field(compress ? compress[t] : 0);
    if (ctx->timing && ctx->adopted_blocks) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        fprintf(stderr, "[ola-timing] device allocator: %zu block(s), %.1f GB, taken over from idle contexts on this GPU so far\n", ctx->adopted_blocks, ctx->adopted_bytes / 1e9);
    }
}

// column counts of the tables of an AIR set (the whole-proof entry points validate their pointer arrays with it)
std::vector<size_t> airset_widths(const u64* airset, size_t airset_words) {
    HAirSet set = parse_airset(airset, airset_words);
    std::vector<size_t> w;
    for (const HTable& t : set.tables) w.push_back((size_t)t.ncols);
    return w;
}

// ola_air_kernels_available / ola_air_kernels_available_cfg: nch challenges
void air_kernels_available(const u64* airset, size_t airset_words, uint8_t* has_kernel, size_t ntables, int nch) {
    HAirSet set = parse_airset(airset, airset_words);
    if (ntables != set.tables.size()) throw OlaError(OLA_E_INVALID_ARG, "ntables does not match the AIR set");
    std::vector<std::vector<const HTwc*>> jobs(set.tables.size());
    for (const HCtl& ctl : set.ctls)
        for (int c = 0; c < nch; c++) {
            for (const HTwc& twc : ctl.looking) jobs[twc.table].push_back(&twc);
            jobs[ctl.looked.table].push_back(&ctl.looked);
        }
    for (size_t t = 0; t < set.tables.size(); t++) has_kernel[t] = find_air_kernel(air_signature(set.tables[t], jobs[t], nch)) ? 1 : 0;
}

}  // namespace ola
