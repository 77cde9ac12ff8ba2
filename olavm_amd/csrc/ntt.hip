// Batched Goldilocks NTT / iNTT / coset-LDE for gfx950 (MI355X).
//
// Replaces, for whole column batches resident in HBM, the reference's per-column CPU transforms
//   plonky2/field/src/cfft/mod.rs:22-231   evaluate_poly / evaluate_poly_with_offset / interpolate_poly(_with_offset)
//   plonky2/field/src/cfft/serial.rs:9-78  (index conventions: natural in, natural out; LDE point m = offset*g^m)
// and the dead CUDA hop plonky2/field/src/cfft/ntt/mod.rs:123-388.
//
// This file: the host-side tables every transform shares, and the ONE-TILE transform for 2^0 .. 2^13 points -- a whole column
// of one coset fits a workgroup's LDS, so a transform is one launch:
//   * copy in (canonicalise; a coset transform multiplies element k by s^k from a two-level table);
//   * the L bits in rounds of <= 4 bits held in registers (16 values per thread), decimation in frequency, top bits
//     first, one LDS exchange per round; LDS rows are padded by one element per 16 to stay bank-conflict free;
//   * copy out, bit-reversed as decimation in frequency leaves it -- precisely the order the commitment's Merkle leaves
//     want, so the LDE never needs a bit-reversal pass -- or through a bit-reversed LDS read in natural
//     order, times 2^-L for an inverse transform.
// Transforms of 2^14 points and more are cut into passes over HBM: ntt2.hip / ntt2t.cuh.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <tuple>
#include <vector>

#include "device_ctx.h"
#include "gl.cuh"

namespace ola {

struct NttPassParams {
    const u64* in;                         // every coset of a column reads the same input
    u64* out;
    size_t in_col_stride, out_col_stride;  // elements between consecutive columns
    size_t out_coset_stride;               // elements between consecutive cosets of one column (LDE), else 0
    int natural_out;                       // write natural order instead of bit-reversed
    const u64* tw_small;                   // w_{2^R}^j, j < 2^(R-1)
    const u64* sc_lo;                      // optional pre-scale tables s^j / s^(j<<sc_h), per coset
    const u64* sc_hi;
    int sc_h;
    size_t sc_coset_stride;
    u64 out_scale;                         // multiply every output by this (1 = skip)
};

template <int K, int S, int R>
__device__ __forceinline__ void dif_radix(u64 (&x)[1 << K], u32 m_below, const u64* __restrict__ tw) {
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        const int b = S + i;
#pragma unroll
        for (int j = 0; j < (1 << K); ++j) {
            if (j & (1 << i)) continue;
            const u32 e = ((u32)(j & ((1 << i) - 1)) << S) + m_below;  // m mod 2^b
            const u64 a = x[j], c = x[j | (1 << i)];
            x[j] = gl_add(a, c);
            u64 d = gl_sub(a, c);
            if (e != 0) d = gl_mul(d, tw[(size_t)e << (R - 1 - b)]);
            x[j | (1 << i)] = d;
        }
    }
}

__device__ __forceinline__ int lds_idx(int e) { return e + (e >> 4); }

// one round: bits [S, S+K) of the element index, 2^K values per group in registers
template <int R, int K, int S>
__device__ __forceinline__ void tile_round(u64* lds, const u64* __restrict__ tw, int tid, int nthreads) {
    constexpr int GROUPS = (1 << R) >> K;
    // group id g enumerates the other bits of the element index: bits [S, S+K) removed
    for (int g = tid; g < GROUPS; g += nthreads) {
        const int low = g & ((1 << S) - 1);
        const int high = g >> S;
        const int e0 = (high << (S + K)) | low;
        u64 x[1 << K];
#pragma unroll
        for (int j = 0; j < (1 << K); ++j) x[j] = lds[lds_idx(e0 + (j << S))];
        dif_radix<K, S, R>(x, (u32)low, tw);
#pragma unroll
        for (int j = 0; j < (1 << K); ++j) lds[lds_idx(e0 + (j << S))] = x[j];
    }
}

// rounds of as-even-as-possible width, top bits first; S = bits still to do, NR = rounds left
template <int R, int S, int NR>
struct TileRounds {
    static __device__ __forceinline__ void run(u64* lds, const u64* __restrict__ tw, int tid, int nthreads) {
        constexpr int K = (S + NR - 1) / NR;
        tile_round<R, K, S - K>(lds, tw, tid, nthreads);
        __syncthreads();
        TileRounds<R, S - K, NR - 1>::run(lds, tw, tid, nthreads);
    }
};
template <int R, int S>
struct TileRounds<R, S, 0> {
    static __device__ __forceinline__ void run(u64*, const u64* __restrict__, int, int) {}
};

template <int R>
__device__ __forceinline__ void tile_ntt(u64* lds, const u64* __restrict__ tw, int tid, int nthreads) {
    TileRounds<R, R, (R + 3) / 4>::run(lds, tw, tid, nthreads);
}

template <int R>
constexpr int ntt_threads() {
    return ((1 << R) / 16) < 64 ? 64 : (1 << R) / 16;  // 512 at R = 13
}

// One workgroup transforms column blockIdx.y for coset blockIdx.z: all 2^R points in LDS.
template <int R>
__global__ __launch_bounds__((ntt_threads<R>())) void ntt_pass_kernel(NttPassParams p) {
    constexpr int E = 1 << R;
    constexpr int NT = ntt_threads<R>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u64* lds = reinterpret_cast<u64*>(smem_raw);
    const int tid = threadIdx.x;
    const size_t col = blockIdx.y;
    const size_t coset = blockIdx.z;
    const u64* in = p.in + col * p.in_col_stride;
    u64* out = p.out + col * p.out_col_stride + coset * p.out_coset_stride;

    // ---- copy in (with optional pre-scale by s^index) ----
    const u64* sc_lo = p.sc_lo ? p.sc_lo + coset * p.sc_coset_stride : nullptr;
    const u64* sc_hi = p.sc_hi ? p.sc_hi + coset * p.sc_coset_stride : nullptr;
    for (int e = tid; e < E; e += NT) {
        u64 v = in[e];
        if (sc_lo) {
            const u64 s = gl_mul(sc_lo[e & ((1 << p.sc_h) - 1)], sc_hi[e >> p.sc_h]);
            v = gl_mul(gl_canon(v), s);
        } else {
            v = gl_canon(v);
        }
        lds[lds_idx(e)] = v;
    }
    __syncthreads();

    tile_ntt<R>(lds, p.tw_small, tid, NT);

    // ---- copy out (with scaling) ----
    for (int e = tid; e < E; e += NT) {
        u64 v = lds[lds_idx(p.natural_out ? (int)bitrev32((u32)e, R) : e)];
        if (p.out_scale != 1) v = gl_mul(v, p.out_scale);
        out[e] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// host side: tables, launcher
// ------------------------------------------------------------------------------------------------
struct TwoLevel {
    u64* lo = nullptr;
    u64* hi = nullptr;
    int h = 0;
};

struct NttTables {
    DeviceCtx* ctx;
    std::map<std::pair<int, int>, u64*> small;       // (R, inverse) -> w_{2^R}^j, j < 2^(R-1)
    std::map<std::pair<int, int>, TwoLevel> two;     // (k, inverse) -> two-level powers of w_{2^k}
    std::map<std::pair<int, int>, TwoLevel> coset;   // (log_n, rate_bits) -> per-coset scale tables (blowup cosets)
    std::map<std::pair<int, u64>, TwoLevel> shift;   // (log_n, shift) -> s^k tables (single coset, arbitrary shift)
    // ntt2.hip's per-coset tables: (log_n, rate_bits, e, shift) -> s^(2^e), and (log_n, rate_bits, 1000 + 16 lo + R, shift) ->
    // the pre-scale powers (s^(2^lo))^m of the T-form pass over index bits [lo, lo + R)
    std::map<std::tuple<int, int, int, u64>, const u64*> coset_steps;
    // ola_gpu_ntt_pass_times: every T-form pass launch bracketed by two events on the context's stream, summed per kernel
    // instantiation when read (the per-launch duration of the dominant kernel for bench.py's roofline; off by default)
    struct PassRec { int R, mode, lm; bool inv; size_t elems; hipEvent_t a, b; };
    bool pass_timing = false;
    std::vector<PassRec> pass_recs;
    ~NttTables() { for (PassRec& r : pass_recs) { if (r.a) (void)hipEventDestroy(r.a); if (r.b) (void)hipEventDestroy(r.b); } }
};

static u64* upload(DeviceCtx* ctx, const std::vector<u64>& v) {
    u64* d = (u64*)ctx->alloc_persistent(v.size() * 8);
    HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return d;
}

static std::vector<u64> powers(u64 base, size_t count) {
    std::vector<u64> v(count);
    u64 acc = 1;
    for (size_t i = 0; i < count; i++) { v[i] = acc; acc = gl_mul(acc, base); }
    return v;
}

static u64 root_for(int k, int inverse) {
    u64 w = gl_root_of_unity(k);
    return inverse ? gl_inv(w) : w;
}

static const u64* get_small(NttTables& t, int R, int inverse) {
    auto key = std::make_pair(R, inverse);
    auto it = t.small.find(key);
    if (it != t.small.end()) return it->second;
    std::vector<u64> v = powers(root_for(R, inverse), R ? ((size_t)1 << (R - 1)) : 1);
    return t.small[key] = upload(t.ctx, v);
}

static TwoLevel make_two_level(DeviceCtx* ctx, u64 w, int k) {
    TwoLevel tl;
    tl.h = (k + 1) / 2;
    std::vector<u64> lo = powers(w, (size_t)1 << tl.h);
    std::vector<u64> hi = powers(gl_pow(w, (u64)1 << tl.h), (size_t)1 << (k - tl.h));
    tl.lo = upload(ctx, lo);
    tl.hi = upload(ctx, hi);
    return tl;
}

static TwoLevel get_two(NttTables& t, int k, int inverse) {
    auto key = std::make_pair(k, inverse);
    auto it = t.two.find(key);
    if (it != t.two.end()) return it->second;
    return t.two[key] = make_two_level(t.ctx, root_for(k, inverse), k);
}

// the shifts of a coset transform: the LDE family 7 * g^bitrev(c), c < 2^rate_bits, g of order n * blowup
// (cfft/serial.rs:32-41), or for rate_bits < 0 the one shift given
static std::vector<u64> coset_shifts(int log_n, int rate_bits, u64 single_shift) {
    if (rate_bits < 0) return {single_shift};
    std::vector<u64> v;
    const u64 g = gl_root_of_unity(log_n + rate_bits);
    for (int c = 0; c < (1 << rate_bits); c++) v.push_back(gl_mul(gl_pow(g, bitrev32((u32)c, rate_bits)), GL_GENERATOR));
    return v;
}

// per-coset tables for the LDE: coset c scales coefficient k by s_c^k.  Layout: [coset][lo 2^h | hi 2^(log_n-h)] with a
// common stride.
static TwoLevel get_coset(NttTables& t, int log_n, int rate_bits, size_t* stride) {
    auto key = std::make_pair(log_n, rate_bits);
    const int h = (log_n + 1) / 2;
    const size_t nlo = (size_t)1 << h, nhi = (size_t)1 << (log_n - h);
    *stride = nlo + nhi;
    auto it = t.coset.find(key);
    if (it != t.coset.end()) return it->second;
    std::vector<u64> all;
    for (u64 s : coset_shifts(log_n, rate_bits, 0)) {
        const std::vector<u64> lo = powers(s, nlo), hi = powers(gl_pow(s, (u64)1 << h), nhi);
        all.insert(all.end(), lo.begin(), lo.end());
        all.insert(all.end(), hi.begin(), hi.end());
    }
    TwoLevel tl;
    tl.h = h;
    tl.lo = upload(t.ctx, all);
    tl.hi = tl.lo + nlo;
    return t.coset[key] = tl;
}

static TwoLevel get_shift(NttTables& t, int log_n, u64 shift) {
    auto key = std::make_pair(log_n, shift);
    auto it = t.shift.find(key);
    if (it != t.shift.end()) return it->second;
    return t.shift[key] = make_two_level(t.ctx, shift, log_n);
}

NttTables* ntt_tables_create(DeviceCtx* ctx) {
    NttTables* t = new NttTables();
    t->ctx = ctx;
    return t;
}
void ntt_tables_destroy(NttTables* t) { delete t; }  // device memory is owned by the ctx persistent pool

template <int R>
static void launch_tile(const NttPassParams& p, size_t cols, size_t cosets, hipStream_t stream) {
    constexpr int E = 1 << R;
    const size_t lds_bytes = (size_t)(E + (E >> 4) + 1) * 8;
    auto kern = ntt_pass_kernel<R>;
    // R = 13 needs more than 48 KB.  The attribute is a property of the kernel ON ONE DEVICE: a context that spans several GPUs
    // sets it once per device
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    if (lds_bytes > 48 * 1024 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && !attr_set[dev].load()) {
        HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        attr_set[dev].store(true);
    }
    hipLaunchKernelGGL(kern, dim3(1, (unsigned)cols, (unsigned)cosets), dim3(ntt_threads<R>()), lds_bytes, stream, p);
}

static std::vector<int> split_even(int total, int parts) {
    std::vector<int> v;
    for (int i = 0; i < parts; i++) {
        int k = (total + (parts - i) - 1) / (parts - i);
        v.push_back(k);
        total -= k;
    }
    return v;
}

// One-tile driver, L <= 13: one launch, a workgroup per column and coset.  `in` may equal `out` when cosets == 1 (a
// workgroup holds its whole column in LDS before it writes).
//   inverse:      use w^-1 and scale by 2^-L at the end
//   prescale:     nullptr, or two-level tables of s^k applied to input element k (coset transforms)
//   cosets:       number of output cosets (LDE); coset c writes at out + c * out_coset_stride and uses
//                 prescale tables at + c * sc_coset_stride
static void ntt_run(NttTables& t, const u64* in, size_t in_col_stride, u64* out, size_t out_col_stride, int L, size_t cols,
                    bool inverse, bool natural_out, const TwoLevel* prescale, size_t sc_coset_stride, size_t cosets,
                    size_t out_coset_stride) {
    if (cols == 0) return;
    NttPassParams p = {};
    p.in = in; p.in_col_stride = in_col_stride;
    p.out = out; p.out_col_stride = out_col_stride; p.out_coset_stride = out_coset_stride;
    p.natural_out = natural_out ? 1 : 0;
    p.tw_small = get_small(t, L, inverse);
    if (prescale) { p.sc_lo = prescale->lo; p.sc_hi = prescale->hi; p.sc_h = prescale->h; p.sc_coset_stride = sc_coset_stride; }
    p.out_scale = inverse ? gl_inv(((u64)1 << L) % GL_P) : 1;
    switch (L) {
#define OLA_CASE(r) case r: launch_tile<r>(p, cols, cosets, t.ctx->stream); break;
        OLA_CASE(0) OLA_CASE(1) OLA_CASE(2) OLA_CASE(3) OLA_CASE(4) OLA_CASE(5) OLA_CASE(6) OLA_CASE(7) OLA_CASE(8) OLA_CASE(9)
        OLA_CASE(10) OLA_CASE(11) OLA_CASE(12) OLA_CASE(13)
#undef OLA_CASE
        default: break;
    }
}

// ---- public (library-internal) entry points -----------------------------------------------------
// Transforms of 2^14 points and more run on the second-generation passes (ntt2.hip); smaller ones fit one tile here.
void ntt2_run(NttTables& t, const u64* in, size_t in_col_stride, u64* out, size_t out_col_stride, u64* scratch,
              size_t scratch_col_stride, int L, size_t cols, bool inverse, bool natural_out, int sc_rate_bits, u64 sc_shift,
              size_t cosets, size_t out_coset_stride, size_t coset_first = 0);
static const int NTT2_MIN_LOG = 14;

// values (natural) -> coefficients (natural), per column.  scratch must hold cols * 2^L elements when L > 13.
void ntt_interpolate(NttTables& t, const u64* values, u64* coeffs, u64* scratch, int L, size_t cols) {
    const size_t n = (size_t)1 << L;
    PhaseScope ph(t.ctx, PH_INTT, (double)cols * n * 16, (double)cols);
    if (L >= NTT2_MIN_LOG) { ntt2_run(t, values, n, coeffs, n, scratch, n, L, cols, true, true, -2, 0, 1, 0); return; }
    ntt_run(t, values, n, coeffs, n, L, cols, true, true, nullptr, 0, 1, 0);
}
// coefficients (natural) -> values at w^i (natural)
void ntt_evaluate(NttTables& t, const u64* coeffs, u64* values, u64* scratch, int L, size_t cols) {
    const size_t n = (size_t)1 << L;
    if (L >= NTT2_MIN_LOG) { ntt2_run(t, coeffs, n, values, n, scratch, n, L, cols, false, true, -2, 0, 1, 0); return; }
    ntt_run(t, coeffs, n, values, n, L, cols, false, true, nullptr, 0, 1, 0);
}
// coefficients (natural, n per column) -> LDE on 7*<g>, in commitment leaf order: out[col][c*n + r] =
// P(7 * g^bitrev(c) * w_n^bitrev_n(r)); equals natural LDE row bitrev_N(c*n + r).
void ntt_lde_leaf_order(NttTables& t, const u64* coeffs, u64* lde, int L, int rate_bits, size_t cols, size_t coset_first,
                        size_t coset_count, size_t in_col_stride = 0) {
    // cosets [coset_first, coset_first + coset_count) of the 2^rate_bits (leaf-order blocks of n); lde holds only those.
    // in_col_stride: distance between the coefficient columns (default n)
    const size_t n = (size_t)1 << L;
    if (!in_col_stride) in_col_stride = n;
    PhaseScope ph(t.ctx, PH_LDE, (double)cols * n * 8 * (1 + coset_count), (double)cols * coset_count);
    if (L >= NTT2_MIN_LOG) {
        ntt2_run(t, coeffs, in_col_stride, lde, n * coset_count, nullptr, 0, L, cols, false, false, rate_bits, 0, coset_count, n, coset_first);
        return;
    }
    size_t stride = 0;
    TwoLevel sc = get_coset(t, L, rate_bits, &stride);
    sc.lo += coset_first * stride;
    sc.hi += coset_first * stride;
    ntt_run(t, coeffs, in_col_stride, lde, n * coset_count, L, cols, false, false, &sc, stride, coset_count, n);
}
void ntt_lde_leaf_order(NttTables& t, const u64* coeffs, u64* lde, int L, int rate_bits, size_t cols) {
    ntt_lde_leaf_order(t, coeffs, lde, L, rate_bits, cols, 0, (size_t)1 << rate_bits);
}
// coefficients -> values on shift*<w_n> in natural order (coset_fft with blowup 1), or bit-reversed order
void ntt_coset_evaluate(NttTables& t, const u64* coeffs, u64* values, u64* scratch, int L, size_t cols, u64 shift,
                        bool natural_out) {
    const size_t n = (size_t)1 << L;
    if (L >= NTT2_MIN_LOG) { ntt2_run(t, coeffs, n, values, n, scratch, n, L, cols, false, natural_out, -1, shift, 1, 0); return; }
    TwoLevel sc = get_shift(t, L, shift);
    ntt_run(t, coeffs, n, values, n, L, cols, false, natural_out, &sc, 0, 1, 0);
}

}  // namespace ola
