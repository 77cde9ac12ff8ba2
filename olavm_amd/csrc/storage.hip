// The account-storage tree and the storage-access table on the device (ola_generate_storage_trace), and the Poseidon table at its
// padded height (ola_generate_poseidon_table).  Part of ola_gpu.hip's translation unit, behind merkle.hip (the permutation and its
// constants) and dev_buf.h (DevBuf); tablegen_api.hip, further down in that unit, holds the two entry points with the other generators'.
//
// The tree is the one of builtins/storage/storage_access_stark.rs:110-334: 256 levels, the key's bits (four limbs, most significant
// first) choose the child, an inner node is Poseidon(left || right || 0,0,0,0)[0..4], the lowest level hashes the two 4-word values
// with capacity word 1, untouched leaves are zero.  A batch of accesses is 2 x 256 x n_access permutations with a dependency only
// from one level to the next, so a level is one launch: one thread per (access, version) hashes the child on the access's path with
// its sibling, for the tree after the access (version 0) and before it (version 1).
//
// Device scratch, all column-major over the accesses so that a wavefront reads consecutive words:
//   keyc  [4][n]        canonical keys
//   newn  [257][4][n]   node of the tree AFTER access a on a's path at layer L (256 = the leaf) -- what a later access's sibling is
//   oldn  [2][4][n]     the same for the tree BEFORE the access, two layers deep (layer L lives in half L & 1)
//   sibix [256][n]      self-contained mode: the access whose layer-L node is a's sibling at layer L = row + 1, or -1 (the empty tree's)
//   meta  [4][n]        from the host's validation pass: ordinal among the accesses with rows (~0 = silent), flags, psdn_row, and the
//                       list of the accesses with rows
#include "tablegen_storage_columns.h"

namespace ola {

namespace stg = olatgs;
static const u64 STORAGE_NO_ROWS = ~0ull;

// the empty tree's node per depth, [depth][4] (depth 256 = a leaf): 256 host permutations, once per process
static const u64* storage_default_nodes() {
    static u64 dflt[(stg::STORAGE_DEPTH + 1) * 4];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int w = 0; w < 4; w++) dflt[stg::STORAGE_DEPTH * 4 + w] = 0;
        for (int d = (int)stg::STORAGE_DEPTH - 1; d >= 0; d--) {
            const u64* c = dflt + (d + 1) * 4;
            u64 s[12] = {c[0], c[1], c[2], c[3], c[0], c[1], c[2], c[3], (u64)(d == (int)stg::STORAGE_DEPTH - 1), 0, 0, 0};
            poseidon_permute_host(s);
            for (int w = 0; w < 4; w++) dflt[d * 4 + w] = s[w];
        }
    });
    return dflt;
}

__global__ __launch_bounds__(256) void storage_keys_kernel(const u64* __restrict__ acc, u32 n, u64* __restrict__ keyc) {
    const u32 a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
#pragma unroll
    for (int w = 0; w < 4; w++) keyc[(size_t)w * n + a] = gl_canon(acc[(size_t)w * n + a]);
}

// Self-contained mode: thread i scans the accesses before it.  The number of leading bits two keys share is four XORs and a
// count-leading-zeros; the latest j per length is i's sibling source at layer length + 1, the latest WRITE of the same key gives the
// leaf before access i.  sibix was filled with -1 on the stream before this launch; a thread only ever rewrites its own column.
__global__ __launch_bounds__(64) void storage_resolve_kernel(const u64* __restrict__ keyc, const u64* __restrict__ meta, u32 n,
                                                             int32_t* __restrict__ sibix, int32_t* __restrict__ prev_write) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 k0 = keyc[i], k1 = keyc[(size_t)n + i], k2 = keyc[2 * (size_t)n + i], k3 = keyc[3 * (size_t)n + i];
    int32_t pw = -1;
    for (u32 j = 0; j < i; j++) {
        const u64 x0 = keyc[j] ^ k0, x1 = keyc[(size_t)n + j] ^ k1, x2 = keyc[2 * (size_t)n + j] ^ k2, x3 = keyc[3 * (size_t)n + j] ^ k3;
        if ((x0 | x1 | x2 | x3) == 0) {
            if (meta[(size_t)n + j] & OLA_STORAGE_WRITE) pw = (int32_t)j;
        } else {
            const u32 shared = x0 ? (u32)__clzll((long long)x0) : x1 ? 64u + (u32)__clzll((long long)x1) : x2 ? 128u + (u32)__clzll((long long)x2)
                                                                                                            : 192u + (u32)__clzll((long long)x3);
            sibix[(size_t)shared * n + i] = (int32_t)j;
        }
    }
    prev_write[i] = pw;
}

// the leaf after (newn, layer 256) and before (oldn, half 0) every access
__global__ __launch_bounds__(256) void storage_leaf_kernel(const u64* __restrict__ acc, const u64* __restrict__ meta,
                                                           const int32_t* __restrict__ prev_write, u32 n, u64* __restrict__ newn,
                                                           u64* __restrict__ oldn) {
    const u32 a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const bool write = meta[(size_t)n + a] & OLA_STORAGE_WRITE;
    const int32_t pw = prev_write ? prev_write[a] : -1;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const u64 value = gl_canon(acc[(size_t)(4 + w) * n + a]);
        // with the caller's siblings the leaf before is the caller's too, and a read's `value` is copied as given
        const u64 pre = prev_write ? (pw >= 0 ? gl_canon(acc[(size_t)(4 + w) * n + (u32)pw]) : 0) : gl_canon(acc[(size_t)(8 + w) * n + a]);
        newn[((size_t)stg::STORAGE_DEPTH * 4 + w) * n + a] = (write || !prev_write) ? value : pre;
        oldn[(size_t)w * n + a] = pre;
    }
}

// One level: thread t < n hashes layer L of the tree after access t, thread n + t of the tree before it.  Reads the child (its own
// column of newn / oldn) and the sibling, writes the node of layer L - 1, the table's PATH / SIB / HASH (after) or PRE_PATH / PRE_HASH
// (before) words of row 256 ordinal + L - 1, and the permutation's inputs and filters at Poseidon-table row psdn_row + 2 (L - 1) +
// version.  The host has checked every row index against the table's height and psdn_stride.
__global__ __launch_bounds__(64) void storage_level_kernel(u32 L, u32 n, const u64* __restrict__ keyc, const u64* __restrict__ meta,
                                                           const int32_t* __restrict__ sibix, const u64* __restrict__ siblings,
                                                           const u64* __restrict__ dflt, u64* __restrict__ newn, u64* __restrict__ oldn,
                                                           u64* __restrict__ out, size_t n_out, u64* __restrict__ psdn_in,
                                                           u64* __restrict__ psdn_f, size_t psdn_stride) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * n) return;
    const u32 v = t >= n ? 1u : 0u, a = t - v * n;
    const u32 bit = (u32)(keyc[(size_t)((L - 1) >> 6) * n + a] >> (63 - ((L - 1) & 63))) & 1u;
    const bool leaf_level = L == stg::STORAGE_DEPTH;
    u64 child[4], sib[4];
    const int32_t j = siblings ? -1 : sibix[(size_t)(L - 1) * n + a];
#pragma unroll
    for (int w = 0; w < 4; w++) {
        child[w] = v ? oldn[(size_t)((L & 1) * 4 + w) * n + a] : newn[((size_t)L * 4 + w) * n + a];
        sib[w] = siblings ? gl_canon(siblings[((size_t)(L - 1) * 4 + w) * n + a]) : j >= 0 ? newn[((size_t)L * 4 + w) * n + (u32)j] : dflt[L * 4 + w];
    }
    u64 s[12];
#pragma unroll
    for (int w = 0; w < 4; w++) { s[w] = bit ? sib[w] : child[w]; s[4 + w] = bit ? child[w] : sib[w]; }
    s[8] = leaf_level; s[9] = s[10] = s[11] = 0;
    const u64 ordinal = meta[a];
    if (psdn_in && ordinal != STORAGE_NO_ROWS) {
        const size_t row = (size_t)meta[2 * (size_t)n + a] + 2 * (L - 1) + v;
#pragma unroll
        for (int k = 0; k < 12; k++) psdn_in[(size_t)k * psdn_stride + row] = s[k];
        psdn_f[row] = 0; psdn_f[psdn_stride + row] = 0; psdn_f[2 * psdn_stride + row] = leaf_level; psdn_f[3 * psdn_stride + row] = !leaf_level;
    }
    poseidon_permute(s);
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (v) oldn[(size_t)(((L - 1) & 1) * 4 + w) * n + a] = s[w];
        else newn[((size_t)(L - 1) * 4 + w) * n + a] = s[w];
    }
    if (ordinal == STORAGE_NO_ROWS) return;
    const size_t r = (size_t)ordinal * stg::STORAGE_DEPTH + (L - 1);
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (v) {
            out[(size_t)(stg::COL_ST_PRE_PATH_RANGE_START + w) * n_out + r] = child[w];
            out[(size_t)(stg::COL_ST_PRE_HASH_RANGE_START + w) * n_out + r] = s[w];
        } else {
            out[(size_t)(stg::COL_ST_PATH_RANGE_START + w) * n_out + r] = child[w];
            out[(size_t)(stg::COL_ST_SIB_RANGE_START + w) * n_out + r] = sib[w];
            out[(size_t)(stg::COL_ST_HASH_RANGE_START + w) * n_out + r] = s[w];
        }
    }
}

// thread = row: every column the level launches do not write, and all 48 of the padding rows (generation/storage.rs:23-114)
__global__ __launch_bounds__(256) void storage_fill_kernel(u32 n, u32 m, const u64* __restrict__ keyc, const u64* __restrict__ meta,
                                                           const u64* __restrict__ newn, const u64* __restrict__ oldn, u64* __restrict__ out,
                                                           size_t n_out) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_out) return;
    auto col = [&](u32 c) -> u64& { return out[(size_t)c * n_out + r]; };
    const bool live = r < (size_t)m * stg::STORAGE_DEPTH;
    const u32 a = m ? (u32)meta[3 * (size_t)n + (live ? r / stg::STORAGE_DEPTH : m - 1)] : 0;
    const u32 L = (u32)(r % stg::STORAGE_DEPTH) + 1;
    const u64 flags = live ? meta[(size_t)n + a] : 0;
    const u64 limb = live ? keyc[(size_t)((L - 1) >> 6) * n + a] : 0;
    const u64 acc = limb >> (63 - ((L - 1) & 63));        // the limb's leading bits, the closed form of generation/storage.rs:44-50
    col(stg::COL_ST_ACCESS_IDX) = live ? r / stg::STORAGE_DEPTH + 1 : 0;
    col(stg::COL_ST_IS_WRITE) = live && (flags & OLA_STORAGE_WRITE);
    col(stg::COL_ST_LAYER) = live ? L : 0;
    col(stg::COL_ST_LAYER_BIT) = acc & 1;
    col(stg::COL_ST_ADDR_ACC) = acc;
    col(stg::COL_ST_HASH_TYPE) = live && L == 256;
    col(stg::COL_ST_IS_LAYER_1) = live && L == 1;
    col(stg::COL_ST_IS_LAYER_64) = live && L == 64;
    col(stg::COL_ST_IS_LAYER_128) = live && L == 128;
    col(stg::COL_ST_IS_LAYER_192) = live && L == 192;
    col(stg::COL_ST_IS_LAYER_256) = live && L == 256;
    col(stg::COL_ST_ACC_LAYER_MARKER) = live ? 1 + L / 64 : 0;
    col(stg::COL_ST_FILTER_IS_HASH_BIT_0) = live && !(acc & 1);
    col(stg::COL_ST_FILTER_IS_HASH_BIT_1) = live && (acc & 1);
    col(stg::COL_ST_FILTER_IS_FOR_PROG) = live && L == 256 && (flags & OLA_STORAGE_FOR_PROG);
    col(stg::COL_ST_IS_PADDING) = !live;
#pragma unroll
    for (u32 w = 0; w < 4; w++) {
        col(stg::COL_ST_ADDR_RANGE_START + w) = live ? keyc[(size_t)w * n + a] : 0;
        col(stg::COL_ST_PRE_ROOT_RANGE_START + w) = live ? oldn[(size_t)w * n + a] : 0;
        col(stg::COL_ST_ROOT_RANGE_START + w) = m ? newn[(size_t)w * n + a] : 0;     // padding repeats the last live row's root
        if (!live) {
            col(stg::COL_ST_PRE_PATH_RANGE_START + w) = 0; col(stg::COL_ST_PATH_RANGE_START + w) = 0; col(stg::COL_ST_SIB_RANGE_START + w) = 0;
            col(stg::COL_ST_PRE_HASH_RANGE_START + w) = 0; col(stg::COL_ST_HASH_RANGE_START + w) = 0;
        }
    }
}

// roots[0..4) = the root before the first access with rows (the root after the last access when none has rows), roots[4..8) = the
// root after the last access
__global__ void storage_roots_kernel(u32 n, u32 m, const u64* __restrict__ meta, const u64* __restrict__ newn, const u64* __restrict__ oldn,
                                     u64* __restrict__ roots) {
    const u32 w = threadIdx.x;
    if (w >= 4) return;
    roots[w] = m ? oldn[(size_t)w * n + (u32)meta[3 * (size_t)n]] : newn[(size_t)w * n + (n - 1)];
    roots[4 + w] = newn[(size_t)w * n + (n - 1)];
}

u32 storage_trace_log_n(u64 m) {
    u32 l = 3;
    while (((u64)1 << l) < m * stg::STORAGE_DEPTH) l++;
    return l;
}

// acc: device memory, 14 x n column-major; meta: HOST words 4 x n from the validation pass (ordinal or ~0, canonical flags, canonical
// psdn_row, the accesses with rows); siblings (1024 x n) / psdn_in (12 x stride) / psdn_f (4 x stride) / roots (8 words): device memory
// or null; out: 48 x 2^storage_trace_log_n(m).  Everything is enqueued on the context's stream: 6 launches and one per level.
void generate_storage_trace_dev(DeviceCtx* ctx, DevBuf& mem, const u64* acc, size_t n_access, const u64* meta_host, size_t m,
                                const u64* siblings, u64* out, u64* psdn_in, u64* psdn_f, size_t psdn_stride, u64* roots) {
    const u32 n = (u32)n_access;
    const size_t n_out = (size_t)1 << storage_trace_log_n(m);
    hipStream_t st = ctx->stream;
    const u64* dflt_host = storage_default_nodes();
    if (n == 0) {
        hipLaunchKernelGGL(storage_fill_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, 0u, 0u, nullptr, nullptr, nullptr, nullptr, out, n_out);
        if (roots) {     // no access: the empty tree's root, twice
            u64* h = mem.host(8).data();
            for (int w = 0; w < 8; w++) h[w] = dflt_host[w & 3];
            HIP_CHECK(hipMemcpyAsync(roots, h, 64, hipMemcpyHostToDevice, st));
        }
        return;
    }
    u64* meta = mem.alloc(4 * (size_t)n);
    u64* dflt = mem.alloc((stg::STORAGE_DEPTH + 1) * 4);
    u64* keyc = mem.alloc(4 * (size_t)n);
    u64* newn = mem.alloc((size_t)(stg::STORAGE_DEPTH + 1) * 4 * n);
    u64* oldn = mem.alloc(8 * (size_t)n);
    HIP_CHECK(hipMemcpyAsync(meta, meta_host, 4 * (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dflt, dflt_host, (stg::STORAGE_DEPTH + 1) * 4 * 8, hipMemcpyHostToDevice, st));
    const unsigned blocks256 = (n + 255) / 256;
    hipLaunchKernelGGL(storage_keys_kernel, dim3(blocks256), dim3(256), 0, st, acc, n, keyc);
    int32_t* sibix = nullptr;
    int32_t* prev_write = nullptr;
    if (!siblings) {
        sibix = (int32_t*)mem.alloc_bytes((size_t)stg::STORAGE_DEPTH * n * 4);
        prev_write = (int32_t*)mem.alloc_bytes((size_t)n * 4);
        HIP_CHECK(hipMemsetAsync(sibix, 0xFF, (size_t)stg::STORAGE_DEPTH * n * 4, st));
        hipLaunchKernelGGL(storage_resolve_kernel, dim3((n + 63) / 64), dim3(64), 0, st, keyc, meta, n, sibix, prev_write);
    }
    hipLaunchKernelGGL(storage_leaf_kernel, dim3(blocks256), dim3(256), 0, st, acc, meta, prev_write, n, newn, oldn);
    // one thread per state in 64-thread workgroups: a level is a few thousand states, which one wavefront per CU spreads widest
    for (u32 L = stg::STORAGE_DEPTH; L >= 1; L--)
        hipLaunchKernelGGL(storage_level_kernel, dim3((2 * n + 63) / 64), dim3(64), 0, st, L, n, keyc, meta, sibix, siblings, dflt, newn, oldn, out, n_out,
                           psdn_in, psdn_f, psdn_stride);
    hipLaunchKernelGGL(storage_fill_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, n, (u32)m, keyc, meta, newn, oldn, out, n_out);
    if (roots) hipLaunchKernelGGL(storage_roots_kernel, dim3(1), dim3(64), 0, st, n, (u32)m, meta, newn, oldn, roots);
}

// The Poseidon table at height n_out >= n_rows: rows n_rows .. n_out are rows of all-zero inputs (generation/poseidon.rs's ZERO-hash rows)
void generate_poseidon_table_dev(DeviceCtx* ctx, const u64* inputs, const u64* filters, size_t n_rows, size_t stride, size_t n_out, u64* out) {
    hipLaunchKernelGGL(poseidon_trace_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, ctx->stream, inputs, filters, n_rows, stride, n_out, out);
}

// ---- the small fills of ola_tables_from_records
// the four filter columns of the range-check table's input (cpu, memory sort, memory region, cmp; 4 x n_rows column-major) from the four
// segment lengths: the values lie as CPU, comparison, memory sort, memory region
__global__ __launch_bounds__(256) void rc_filters_kernel(u32 n_cpu, u32 n_cmp, u32 n_sort, u32 n_rows, u64* __restrict__ filters) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const u32 seg = i < n_cpu ? 0u : i < n_cpu + n_cmp ? 3u : i < n_cpu + n_cmp + n_sort ? 1u : 2u;
#pragma unroll
    for (u32 k = 0; k < 4; k++) filters[(size_t)k * n_rows + i] = k == seg ? 1 : 0;
}
// the SCCALL table of a run without cross-contract calls: IS_PADDING = 1, the rest 0
__global__ __launch_bounds__(256) void sccall_padding_kernel(u32 n, u64* __restrict__ out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= olatgx::NUM_COL_SCCALL * n) return;
    out[i] = i / n == olatgx::COL_SCCALL_IS_PADDING ? 1 : 0;
}
void rc_filters_dev(DeviceCtx* ctx, size_t n_cpu, size_t n_cmp, size_t n_sort, size_t n_rows, u64* filters) {
    if (n_rows) hipLaunchKernelGGL(rc_filters_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, ctx->stream, (u32)n_cpu, (u32)n_cmp, (u32)n_sort, (u32)n_rows, filters);
}
void sccall_padding_dev(DeviceCtx* ctx, u32 n, u64* out) {
    hipLaunchKernelGGL(sccall_padding_kernel, dim3((olatgx::NUM_COL_SCCALL * n + 255) / 256), dim3(256), 0, ctx->stream, n, out);
}

}  // namespace ola
