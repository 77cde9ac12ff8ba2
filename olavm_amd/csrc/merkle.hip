// Merkle tree kernels for gfx950, one body per leaf shape and thread mapping, instantiated for the hash policies of hasher.cuh: the
// Poseidon and Poseidon2 sponges (poseidon.cuh, poseidon2.cuh: PoseidonGoldilocksConfig, Poseidon2GoldilocksConfig /
// Poseidon2GoldilocksConfig2 -- the same sponge and tree, hash/poseidon2.rs:500-512) and the byte hashes of Blake3GoldilocksConfig
// (blake3.cuh) and KeccakGoldilocksConfig (keccak.cuh).
//
// Replaces (reference, relative to plonky2/plonky2/src/hash):
//   hashing.rs:84-107            hash_n_to_m_no_pad  -- overwrite-mode sponge, rate 8, 4-element digest
//   hashing.rs:66-74             compress / two_to_one = permute(l || r || 0)[0..4]
//   merkle_tree/mod.rs:180-226   MerkleTree::new_v2: every leaf hashed with hash_no_pad; heap-ordered nodes;
//                                cap = level with 2^cap_height nodes
// Layout in HBM: `heap` holds 2N digests of 4 u64: heap[N + j] = digest of leaf j, heap[i] = H(heap[2i], heap[2i+1]),
// root at 1 (heap[0] unused).  Sibling paths for MerkleTree::prove (mod.rs:273-308) are read straight off the heap, so
// the reference's per-cap-subtree `digests` relayout (mod.rs:228-259) is never materialised.
// Leaves are read column-major ([col][leaf]) so consecutive lanes read consecutive addresses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "../../include/ola_gpu.h"
#include "device_ctx.h"
#include "gl.cuh"
#include "hasher.cuh"
#include "hasher_host.h"
#include "pow_batch.h"

namespace ola {

// batches up to this many states / nodes / leaves use the quad-cooperative (latency-oriented) kernels
static const size_t QUAD_MAX = 8192;

// ---- the three leaf shapes: words(j) delivers word i of leaf j.  Trace values are canonicalised as they are read; the extension
// planes only for the byte hashes (CANON), whose digest depends on the representative -- the sponge reduces whatever it absorbs.
// leaf j = (cols[0][j], cols[1][j], ...), column c at base + c*col_stride
struct ColMajorSrc {
    const u64* base; size_t col_stride; u32 ncols;
    __device__ __forceinline__ u32 nwords() const { return ncols; }
    __device__ __forceinline__ auto words(size_t j) const {
        return [b = base, stride = col_stride, j](u32 i) { return gl_canon(b[(size_t)i * stride + j]); };
    }
};
// leaf j = row j of a row-major matrix (rows of row_len elements)
struct RowMajorSrc {
    const u64* rows; size_t row_len;
    __device__ __forceinline__ u32 nwords() const { return (u32)row_len; }
    __device__ __forceinline__ auto words(size_t j) const {
        return [r = rows, at = j * row_len](u32 i) { return gl_canon(r[at + i]); };
    }
};
// FRI commit-phase leaves (fri/prover.rs:90-96): leaf j = flatten(`arity` consecutive bit-reversed extension values) =
// (a[arity j], b[arity j], a[arity j + 1], b[arity j + 1], ...) with the extension field stored as two planes.
template <bool CANON>
struct ExtSrc {
    const u64* plane_a; const u64* plane_b; u32 arity;
    __device__ __forceinline__ u32 nwords() const { return 2 * arity; }
    __device__ __forceinline__ auto words(size_t j) const {
        return [pa = plane_a, pb = plane_b, at = j * arity](u32 i) {
            const u64 v = ((i & 1) ? pb : pa)[at + (i >> 1)];
            return CANON ? gl_canon(v) : v;
        };
    }
};

// one lane per leaf
template <class H, class Src>
__global__ __launch_bounds__(256) void leaf_hash_kernel(Src src, size_t num_leaves, u64* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= num_leaves) return;
    H::leaf(src.words(j), src.nwords(), out + j * 4);
}

// ---- quad-cooperative variants (4 threads per leaf / node, poseidon.cuh): same digests, used when the batch is too small
// to fill the chip, where the latency of a permutation is what matters.  Lane q of a quad owns sponge lanes 3q..3q+2.
#define QUAD_PROLOGUE(count)                                            \
    const size_t g_ = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   \
    const size_t j_ = g_ >> 2;                                         \
    const int q = (int)(g_ & 3);                                       \
    const bool live = j_ < (count);                                    \
    const size_t j = live ? j_ : (count) - 1; /* surplus lanes redo the last item so that quads stay converged */
__device__ __forceinline__ void quad_store_digest(u64* __restrict__ out4, const u64 (&x)[3], int q, bool live) {
    if (!live) return;
    if (q == 0) { out4[0] = x[0]; out4[1] = x[1]; out4[2] = x[2]; }
    if (q == 1) out4[3] = x[0];
}

template <int PERM, class Src>
__global__ __launch_bounds__(256) void leaf_hash_quad_kernel(Src src, size_t num_leaves, u64* __restrict__ out) {
    QUAD_PROLOGUE(num_leaves)
    u64 x[3];
    sponge_quad_leaf<PERM>(src.words(j), src.nwords(), x, q);
    quad_store_digest(out + j * 4, x, q, live);
}

// node i = H(heap[2i] || heap[2i+1]) for i in [first, first + count)
template <int PERM>
__device__ __forceinline__ void quad_hash_node(u64* __restrict__ heap, size_t i, int q, bool live) {
    u64 x[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int e = 3 * q + k;
        x[k] = e < 8 ? heap[8 * i + e] : 0;   // the two child digests are adjacent
    }
    permute_quad<PERM>(x, q);
    quad_store_digest(heap + 4 * i, x, q, live);
}
template <int PERM>
__global__ __launch_bounds__(256) void merkle_level_quad_kernel(u64* __restrict__ heap, size_t first, size_t count) {
    QUAD_PROLOGUE(count)
    quad_hash_node<PERM>(heap, first + j, q, live);
}

// parents [first, first+count) of a heap-ordered digest array, one lane per node (children 2i, 2i+1 are adjacent)
template <class H>
__global__ __launch_bounds__(256) void merkle_level_kernel(u64* __restrict__ heap, size_t first, size_t count) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    H::node(heap + 8 * (first + t), heap + 4 * (first + t));
}

// The top of a tree in one launch: levels of `first` nodes and fewer (4 * first <= blockDim.x), down to the level of `last`
// nodes, one workgroup of quads, a barrier between levels.
template <int PERM>
__global__ __launch_bounds__(1024) void merkle_top_kernel(u64* __restrict__ heap, size_t first, size_t last) {
    const size_t t = threadIdx.x >> 2;
    const int q = threadIdx.x & 3;
    const size_t wave_first = (threadIdx.x & ~63u) >> 2;   // first node index of this wavefront's 16 quads
    for (size_t level = first; level >= last && level >= 1; level >>= 1) {
        if (wave_first < level) {   // wavefronts without a node of this level only wait at the barrier
            const bool live = t < level;
            quad_hash_node<PERM>(heap, level + (live ? t : level - 1), q, live);
        }
        __threadfence_block();
        __syncthreads();
    }
}

// Rows of the Poseidon STARK table (builtins/poseidon/columns.rs; layout of generation/poseidon.rs:5-80) from the
// permutation inputs: the reference's executor records the S-box inputs of every round (core/src/util/poseidon_utils.rs)
// and generate_poseidon_trace lays them out; here one thread recomputes them for its row.  Columns: 4 lookup filters,
// input[12], output[12], S-box inputs of full rounds 1..3 [3x12], of the 22 partial rounds (lane 0) [22], of full rounds
// 26..29 [4x12].  The S-box argument of a round does not depend on how the linear layers are factored, so the dense
// lane-0 form of poseidon.cuh yields exactly the values the reference's sparse form records.
// inputs / filters: n_live rows, column-major with `stride` words per column; rows n_live .. n of `out` are rows of all-zero inputs and
// filters (the table's padding, generation/poseidon.rs).
__global__ __launch_bounds__(256) void poseidon_trace_kernel(const u64* __restrict__ inputs, const u64* __restrict__ filters, size_t n_live,
                                                             size_t stride, size_t n, u64* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool live = i < n_live;
    auto col = [&](int c) -> u64& { return out[(size_t)c * n + i]; };
    for (int f = 0; f < 4; f++) col(f) = filters && live ? gl_canon(filters[(size_t)f * stride + i]) : 0;
    u64 s[12];
    for (int k = 0; k < 12; k++) { s[k] = live ? gl_canon(inputs[(size_t)k * stride + i]) : 0; col(4 + k) = s[k]; }
    for (int r = 0; r < 4; r++) {
        for (int k = 0; k < 12; k++) {
            s[k] = gl_add(gl_canon(s[k]), c_rc[r * 12 + k]);
            if (r > 0) col(28 + (r - 1) * 12 + k) = s[k];
            s[k] = sbox7_weak(s[k]);
        }
        mds_weak(s);
    }
    for (int r = 0; r < 22; r++) {
        const u64 a = gl_add(gl_canon(s[0]), c_lane0[r]);
        col(64 + r) = a;
        s[0] = sbox7_weak(a);
        mds_weak(s);
    }
    for (int r = 0; r < 4; r++) {
        for (int k = 0; k < 12; k++) {
            s[k] = gl_add(gl_canon(s[k]), r == 0 ? c_round26[k] : c_rc[(26 + r) * 12 + k]);
            col(86 + r * 12 + k) = s[k];
            s[k] = sbox7_weak(s[k]);
        }
        mds_weak(s);
    }
    for (int k = 0; k < 12; k++) col(16 + k) = gl_canon(s[k]);
}
void launch_poseidon_trace(DeviceCtx* ctx, const u64* inputs, const u64* filters, size_t n, u64* out) {
    if (n) hipLaunchKernelGGL(poseidon_trace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, inputs, filters, n, n, n, out);
}

// quad-cooperative permutation of whole states (4 threads per state); used for small n
template <int PERM>
__global__ __launch_bounds__(256) void poseidon_states_quad_kernel(u64* __restrict__ states, size_t n) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t t = g >> 2;
    const int q = (int)(g & 3);
    const size_t tt = t < n ? t : n - 1;   // keep whole quads converged; the surplus lanes redo the last state
    u64 x[3];
#pragma unroll
    for (int k = 0; k < 3; k++) x[k] = gl_canon(states[tt * 12 + 3 * q + k]);
    permute_quad<PERM>(x, q);
    if (t < n) {
#pragma unroll
        for (int k = 0; k < 3; k++) states[t * 12 + 3 * q + k] = x[k];
    }
}

template <int PERM>
__global__ __launch_bounds__(256) void poseidon_states_kernel(u64* __restrict__ states, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    u64 s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl_canon(states[t * 12 + i]);
    permute12<PERM>(s);
#pragma unroll
    for (int i = 0; i < 12; i++) states[t * 12 + i] = s[i];
}

// FRI proof of work (fri/prover.rs:126-148): each thread tries nonce = start + global id; the minimum satisfying
// nonce of the batch is kept with an atomicMin.
template <int PERM>
__global__ __launch_bounds__(256) void pow_kernel(u64 h0, u64 h1, u64 h2, u64 h3, u64 start, u32 bits,
                                                  unsigned long long* __restrict__ best) {
    const u64 nonce = start + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 s[12] = {h0, h1, h2, h3, nonce, 0, 0, 0, 0, 0, 0, 0};
    permute12<PERM>(s);
    if ((s[0] >> (64 - bits)) == 0) atomicMin(best, (unsigned long long)nonce);
}

// ---- kernels of the byte hashes alone (H::BYTES: one thread per leaf / node throughout, no quad forms)
// The extension leaves of arity 16, 8 and 4 (AB = 4, 3, 2: the default, and layers that FriReductionStrategy::Fixed and MinSize plan),
// through LDS (round 6).  A thread of leaf_hash_kernel<H, ExtSrc> at arity 16 reads 16 + 16 words 128 bytes apart from its neighbour's: a
// wave touches 64 lines per load and the lines are gone from the vector cache before their other words are asked for -- 17.1 GB
// fetched per 2^22-row proof for 1.2 GB of values (profiles/r05_proof_pmc_blake3.txt).  Here a workgroup copies its 128 leaves x
// 2^AB values of both planes with 16-byte loads on consecutive addresses and every thread hashes its leaf out of LDS.  Rows of
// S = 2^AB + 1 words: ds_read_b64 banks by (byte address / 4) mod 64 within each 32-lane half, lane l reads word l S + k, i.e. dwords
// 2 (l S + k) and the next -- the 32 lanes cover all 64 banks exactly once when l S mod 32 takes 32 values, that is for every odd S:
// 17, 9 and 5.
#define B3X_LEAVES 128
template <class H, int AB>
__global__ __launch_bounds__(B3X_LEAVES) void leaf_bytes_ext_tile_kernel(const u64* __restrict__ plane_a, const u64* __restrict__ plane_b, size_t num_leaves,
                                                                         u64* __restrict__ out) {
    static_assert(AB >= 2 && AB <= 4, "arity 2 needs no tile: leaf_bytes_ext2_kernel");
    constexpr int A = 1 << AB, S = A + 1;
    __shared__ u64 tile[2][B3X_LEAVES * S];
    const size_t j0 = (size_t)blockIdx.x * B3X_LEAVES;
    const size_t base = j0 * A;
    const size_t avail = (num_leaves - j0 < (size_t)B3X_LEAVES ? num_leaves - j0 : (size_t)B3X_LEAVES) * A;
#pragma unroll
    for (int i = 0; i < A / 2; i++) {
        const size_t e = 2 * ((size_t)threadIdx.x + B3X_LEAVES * i);
        if (e < avail) {
            const ulonglong2 va = *reinterpret_cast<const ulonglong2*>(plane_a + base + e);
            const ulonglong2 vb = *reinterpret_cast<const ulonglong2*>(plane_b + base + e);
            const size_t at = (e >> AB) * S + (e & (A - 1));
            tile[0][at] = va.x; tile[0][at + 1] = va.y;
            tile[1][at] = vb.x; tile[1][at + 1] = vb.y;
        }
    }
    __syncthreads();
    const size_t j = j0 + threadIdx.x;
    if (j >= num_leaves) return;
    H::leaf([&](u32 i) { return gl_canon(tile[i & 1][threadIdx.x * S + (i >> 1)]); }, (u32)(2 * A), out + j * 4);
}
// Arity 2: a thread's own leaf is 16 bytes per plane, and neighbouring lanes' loads are neighbours
template <class H>
__global__ __launch_bounds__(256) void leaf_bytes_ext2_kernel(const u64* __restrict__ plane_a, const u64* __restrict__ plane_b, size_t num_leaves,
                                                              u64* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= num_leaves) return;
    const ulonglong2 va = *reinterpret_cast<const ulonglong2*>(plane_a + 2 * j);
    const ulonglong2 vb = *reinterpret_cast<const ulonglong2*>(plane_b + 2 * j);
    // (selects, not an array: a run-time index would put it into scratch memory)
    H::leaf([&](u32 i) { return gl_canon((i & 2) ? ((i & 1) ? vb.y : va.y) : ((i & 1) ? vb.x : va.x)); }, 4u, out + j * 4);
}
// `nlev` (<= 8) consecutive levels in one launch (round 6): a workgroup computes 256 nodes of the level of `first` nodes from their
// children in the heap, then the 128, 64, ... nodes above them out of LDS -- every level is still written to the heap (sibling paths
// read it), but only the bottom one is read back.  Measured on the 2^22-row Blake3 proof (profiles/r06_merkle_levels_per_launch.txt,
// 314 level launches and 20.6 GB per proof before): eight levels per launch are SLOWER (6.3 -> 8.4 ms: the upper levels run on 128, 64,
// ... 1 lanes of a workgroup that keeps its slot for eight compressions in a row), two or three are a little faster (5.8 ms), four 6.0;
// the default is two (OLA_MERKLE_FUSED_LEVELS, 0 = one launch per level).
template <class H>
__global__ __launch_bounds__(256) void merkle_levels_bytes_kernel(u64* __restrict__ heap, size_t first, int nlev) {
    __shared__ u64 sh[2][256 * 4];
    const int t = threadIdx.x;
    alignas(16) u64 d[4];
    {
        const size_t node = first + (size_t)blockIdx.x * 256 + t;
        H::node(heap + 8 * node, d);
#pragma unroll
        for (int k = 0; k < 4; k++) { heap[4 * node + k] = d[k]; sh[0][4 * t + k] = d[k]; }
    }
    for (int l = 1; l < nlev; l++) {
        __syncthreads();
        const int count = 256 >> l;
        if (t < count) {
            const size_t node = (first >> l) + (size_t)blockIdx.x * count + t;
            H::node(&sh[(l - 1) & 1][8 * t], d);
#pragma unroll
            for (int k = 0; k < 4; k++) { heap[4 * node + k] = d[k]; sh[l & 1][4 * t + k] = d[k]; }
        }
    }
}
// levels of `first` nodes and fewer (first <= blockDim.x) down to the level of `last` nodes in one workgroup
template <class H>
__global__ __launch_bounds__(256) void merkle_top_bytes_kernel(u64* __restrict__ heap, size_t first, size_t last) {
    for (size_t level = first; level >= last && level >= 1; level >>= 1) {
        if (threadIdx.x < level) H::node(heap + 8 * (level + threadIdx.x), heap + 4 * (level + threadIdx.x));
        __threadfence_block();
        __syncthreads();
    }
}

// ---- host launchers ----
void poseidon_init(DeviceCtx*) {   // both permutations' constants on the calling thread's device, whatever the hasher
    poseidon_upload_constants();
    poseidon2_upload_constants();
}

// hash invocations per leaf of `words` field elements, for the phase accounting
static double leaf_hash_calls(const DeviceCtx* ctx, size_t words) { return hasher_row((uint32_t)ctx->hasher).leaf_calls(words); }

// the leaves of `src` under H: a quad per leaf for a small batch of sponge leaves, else a lane per leaf
template <class H, class Src>
static void launch_leaves(DeviceCtx* ctx, const Src& src, size_t words, size_t num_leaves, u64* out) {
    if (H::BYTES && (words == 0 || words > 4096)) throw OlaError(-1, "Blake3 and Keccak leaves hold 1..4096 field elements");
    if (num_leaves == 0) return;
    if constexpr (!H::BYTES) {
        if (num_leaves <= QUAD_MAX) {
            hipLaunchKernelGGL((leaf_hash_quad_kernel<H::perm, Src>), dim3((unsigned)((4 * num_leaves + 255) / 256)), dim3(256), 0, ctx->stream, src, num_leaves, out);
            return;
        }
    }
    hipLaunchKernelGGL((leaf_hash_kernel<H, Src>), dim3((unsigned)((num_leaves + 255) / 256)), dim3(256), 0, ctx->stream, src, num_leaves, out);
}
void launch_leaf_hash_colmajor(DeviceCtx* ctx, const u64* base, size_t col_stride, int ncols, size_t num_leaves,
                               u64* out) {
    PhaseScope ph(ctx, PH_LEAF_HASH, (double)num_leaves * leaf_hash_calls(ctx, (size_t)ncols), (double)num_leaves * ((size_t)ncols * 8 + 32));
    with_hash((uint32_t)ctx->hasher, (size_t)ncols, [&](auto tag) {
        using H = typename decltype(tag)::type;
        launch_leaves<H>(ctx, ColMajorSrc{base, col_stride, (u32)ncols}, (size_t)ncols, num_leaves, out);
    });
}
void launch_leaf_hash_rowmajor(DeviceCtx* ctx, const u64* rows, size_t row_len, size_t num_leaves, u64* out) {
    with_hash((uint32_t)ctx->hasher, row_len, [&](auto tag) {
        using H = typename decltype(tag)::type;
        launch_leaves<H>(ctx, RowMajorSrc{rows, row_len}, row_len, num_leaves, out);
    });
}
void launch_leaf_hash_ext(DeviceCtx* ctx, const u64* pa, const u64* pb, int arity, size_t num_leaves, u64* out) {
    const size_t words = (size_t)(2 * arity);
    PhaseScope ph(ctx, PH_LEAF_HASH, (double)num_leaves * leaf_hash_calls(ctx, words), (double)num_leaves * ((size_t)arity * 16 + 32));
    static const bool staged = !(getenv("OLA_LEAF_EXT_STAGED") && !strcmp(getenv("OLA_LEAF_EXT_STAGED"), "0"));
    with_hash((uint32_t)ctx->hasher, words, [&](auto tag) {
        using H = typename decltype(tag)::type;
        if constexpr (H::BYTES) {
            // every global load a 16-byte load on consecutive addresses (OLA_LEAF_EXT_STAGED=0: the plain kernel, for every arity)
            if (staged && num_leaves >= 1024 && (((uintptr_t)pa | (uintptr_t)pb) & 15) == 0 && (arity == 16 || arity == 8 || arity == 4 || arity == 2)) {
                using HS = typename H::Small;
                const dim3 tiles((unsigned)((num_leaves + B3X_LEAVES - 1) / B3X_LEAVES)), tile_block(B3X_LEAVES);
                switch (arity) {
                    case 16: hipLaunchKernelGGL((leaf_bytes_ext_tile_kernel<HS, 4>), tiles, tile_block, 0, ctx->stream, pa, pb, num_leaves, out); break;
                    case 8: hipLaunchKernelGGL((leaf_bytes_ext_tile_kernel<HS, 3>), tiles, tile_block, 0, ctx->stream, pa, pb, num_leaves, out); break;
                    case 4: hipLaunchKernelGGL((leaf_bytes_ext_tile_kernel<HS, 2>), tiles, tile_block, 0, ctx->stream, pa, pb, num_leaves, out); break;
                    default: hipLaunchKernelGGL(leaf_bytes_ext2_kernel<HS>, dim3((unsigned)((num_leaves + 255) / 256)), dim3(256), 0, ctx->stream, pa, pb, num_leaves, out); break;
                }
                return;
            }
        }
        launch_leaves<H>(ctx, ExtSrc<H::BYTES>{pa, pb, (u32)arity}, words, num_leaves, out);
    });
}
// heap[N..2N) must hold the leaf digests; fills heap[2^cap_height .. N): like the reference (merkle_tree/mod.rs:228-233)
// nothing above the cap is ever hashed
void launch_merkle_build(DeviceCtx* ctx, u64* heap, size_t num_leaves, uint32_t cap_height) {
    const size_t last = (size_t)1 << cap_height, top = 256;   // levels of <= `top` nodes share one launch
    PhaseScope ph(ctx, PH_MERKLE_LEVELS, num_leaves > last ? (double)(num_leaves - last) : 0.0, num_leaves > last ? (double)(num_leaves - last) * 96 : 0.0);
    static const int fused = getenv("OLA_MERKLE_FUSED_LEVELS") ? atoi(getenv("OLA_MERKLE_FUSED_LEVELS")) : 2;
    with_hash((uint32_t)ctx->hasher, 0, [&](auto tag) {
        using H = typename decltype(tag)::type::Small;
        size_t level = num_leaves / 2;
        if constexpr (H::BYTES) {
            if (fused > 1 && last <= top && (level & (level - 1)) == 0) {
                while (level > top) {          // level is a power of two >= 512: up to `fused` levels per launch, the last of them still above `top`
                    int nlev = 0;
                    while (nlev < fused && nlev < 8 && (level >> nlev) > top) nlev++;
                    hipLaunchKernelGGL(merkle_levels_bytes_kernel<H>, dim3((unsigned)(level / 256)), dim3(256), 0, ctx->stream, heap, level, nlev);
                    level >>= nlev;
                }
            }
        }
        for (; level >= last && level > top; level /= 2) {
            if constexpr (!H::BYTES) {
                if (level <= QUAD_MAX) {
                    hipLaunchKernelGGL(merkle_level_quad_kernel<H::perm>, dim3((unsigned)((4 * level + 255) / 256)), dim3(256), 0, ctx->stream, heap, level, level);
                    continue;
                }
            }
            hipLaunchKernelGGL(merkle_level_kernel<H>, dim3((unsigned)((level + 255) / 256)), dim3(256), 0, ctx->stream, heap, level, level);
        }
        if (level >= last && level >= 1) {   // the byte hashes with a lane per node (256 threads), the sponges with a quad per node (1024)
            if constexpr (H::BYTES) hipLaunchKernelGGL(merkle_top_bytes_kernel<H>, dim3(1), dim3(256), 0, ctx->stream, heap, level, last);
            else hipLaunchKernelGGL(merkle_top_kernel<H::perm>, dim3(1), dim3(1024), 0, ctx->stream, heap, level, last);
        }
    });
}
// `hasher` names the permutation (OLA_HASH_POSEIDON or OLA_HASH_POSEIDON2), not the context's configuration
void launch_poseidon_states(DeviceCtx* ctx, u64* states, size_t n, uint32_t hasher = OLA_HASH_POSEIDON) {
    if (n == 0) return;
    with_perm(hasher, [&](auto perm) {
        constexpr int PERM = decltype(perm)::value;
        if (n <= QUAD_MAX) {
            hipLaunchKernelGGL(poseidon_states_quad_kernel<PERM>, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, ctx->stream, states, n);
            return;
        }
        const unsigned blocks = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(poseidon_states_kernel<PERM>, dim3(blocks), dim3(256), 0, ctx->stream, states, n);
    });
}
// one batch of the proof-of-work search with the context's InnerHasher (fri/prover.rs:133 C::InnerHasher::hash_no_pad)
static void launch_pow_batch(DeviceCtx* ctx, hipStream_t stream, const u64 h[4], u64 start, u64 count, u32 bits, unsigned long long* best) {
    with_perm(hasher_row((uint32_t)ctx->hasher).inner, [&](auto perm) {
        constexpr int PERM = decltype(perm)::value;
        hipLaunchKernelGGL(pow_kernel<PERM>, dim3(pow_batch_blocks(count)), dim3((unsigned)POW_BLOCK), 0, stream, h[0], h[1], h[2], h[3], start, bits, best);
        HIP_CHECK(hipGetLastError());      // a refused launch throws: run_pow's loop would otherwise wait for a witness nobody looks for
    });
}
// minimal nonce with `bits` leading zeros; scans batches of pow_batch(bits) nonces (pow_batch.h) in increasing order
u64 run_pow(DeviceCtx* ctx, const u64 h[4], u32 bits) {
    unsigned long long* d_best = (unsigned long long*)ctx->alloc(8);
    const unsigned long long none = ~0ull;
    unsigned long long best = none;
    const u64 batch = pow_batch(bits);
    for (u64 start = 0; best == none; start += batch) {
        HIP_CHECK(hipMemcpyAsync(d_best, &none, 8, hipMemcpyHostToDevice, ctx->stream));
        launch_pow_batch(ctx, ctx->stream, h, start, batch, bits, d_best);
        HIP_CHECK(hipMemcpyAsync(&best, d_best, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    ctx->free(d_best);
    return best;
}

}  // namespace ola
