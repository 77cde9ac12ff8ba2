// Device-side `permuted_cols`: the permuted input / permuted table columns of the Halo2-style lookup
// argument that the range-check, bitwise and program tables carry (reference: circuits/src/stark/lookup.rs:68-132, called
// from generation/builtin.rs:121-200 and generation/prog.rs).  Own translation unit: rocPRIM (radix sort, scans) is only
// needed here.
//
// The reference walks the two SORTED columns with one sequential merge loop that keeps a stack of "unused" table values:
//   table value not wanted by any input  -> push;   repeated input (its table entry is already taken) -> pop, or, with
//   an empty stack, remember the slot;   at the end the remembered slots and the inputs left over when the table ran
//   out are filled, in order, with what is still on the stack (bottom first).
// Restated as data-parallel steps:
//   1. canonicalise and radix-sort both columns;
//   2. classify every element with binary searches: input i of value a with rank r among the inputs equal to a is MATCHED
//      iff r < (number of table entries equal to a); otherwise it is a POP if some table entry is > a (the merge loop is
//      still running when it is reached) and a TAIL slot if not.  Table entry j is matched iff its rank among equals is
//      below the number of inputs of that value, else it is a PUSH.  A value has surplus inputs or surplus table entries,
//      never both, so ordering the pushes and pops by (value, index) reproduces the order in which the loop meets them;
//      the position of an event in that sequence follows from two exclusive scans;
//   3. stack discipline = bracket matching: S = running sum of +1 / -1, m = running minimum of min(S, 0); a pop that
//      lowers m found the stack empty; the stack height after event k is d = S - m.  A stable sort of the events by the
//      height they push to / pop from puts every pop right behind the push it takes;
//   4. pushes nobody took (in event order) fill the slots of the unmatched pops (in event order) followed by the tail
//      slots (in index order).
#include <algorithm>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "device_ctx.h"
#include "gl.cuh"
#include "lookup.h"
#include "tablegen_columns.h"
#include "tablegen_cpu_columns.h"
#include "tablegen_mem_columns.h"
#include "tablegen_small_columns.h"

namespace ola {

namespace {

// A batch of pairs that share their height runs steps 2 - 4 together: every kernel below has the pair index in grid.y, the
// scans run once over the concatenation of the pairs' flag arrays (a pair's own prefix is the difference to the value at its
// first entry), the events of all pairs sit back to back (pair p at ev_base[p]) with the pair index as the key of the two
// segmented scans and as the high bits of the level key, so that one stable sort orders every pair's events.  The table
// generators further down fill a whole table and hand its lookup pairs to one such batch.
constexpr u32 kMaxBatch = 16;

struct PairArgs {                  // kernel argument (by value): pair p of the batch
    const u64* si[kMaxBatch];      // its inputs, canonical and sorted = permuted_inputs
    const u64* st[kMaxBatch];      // its table, canonical and sorted
    u64* pt[kMaxBatch];            // permuted_table
};

struct Scratch {
    DeviceCtx* ctx;
    std::vector<void*> ptrs;
    explicit Scratch(DeviceCtx* c) : ctx(c) {}
    template <typename T>
    T* alloc(size_t elems) {
        void* p = ctx->alloc(elems * sizeof(T));
        ptrs.push_back(p);
        return (T*)p;
    }
    ~Scratch() {
        (void)hipStreamSynchronize(ctx->stream);
        for (void* p : ptrs) ctx->free(p);
    }
};

// column y of a batch of columns: src[y] -> dst + y * n
struct CanonArgs { const u64* src[kMaxBatch]; };
__global__ __launch_bounds__(256) void canon_kernel(CanonArgs a, u64* __restrict__ dst, u32 n) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[(size_t)blockIdx.y * n + i] = gl_canon(a.src[blockIdx.y][i]);
}

__device__ __forceinline__ u32 lower_bound_u64(const u64* __restrict__ a, u32 n, u64 v) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ u32 upper_bound_u64(const u64* __restrict__ a, u32 n, u64 v) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Flags of a batch: three classes (FL_POP: input that pops, FL_PUSH: table entry that pushes, FL_TAIL: input reached after the
// table ran out) x pairs x (n + 1) entries, entry n of every run is 0 -- the exclusive scan over all of it then holds, at a run's
// entry n, the run's total on top of what came before.
enum : u32 { FL_POP = 0, FL_PUSH = 1, FL_TAIL = 2, FL_CLASSES = 3 };
__device__ __forceinline__ size_t flag_at(u32 cls, u32 pairs, u32 n, u32 p, u32 i) { return ((size_t)cls * pairs + p) * (n + 1) + i; }
__device__ __forceinline__ u32 before(const u32* __restrict__ sc, u32 cls, u32 pairs, u32 n, u32 p, u32 i) {
    const size_t b = flag_at(cls, pairs, n, p, 0);
    return sc[b + i] - sc[b];
}

// step 2: thread t < n classifies input t, thread n + t classifies table entry t.  other[t] = first position of the
// opposite column whose value is not below this one (where events of smaller values end).
__global__ __launch_bounds__(256) void classify_kernel(PairArgs a, u32 pairs, u32 n, u32* __restrict__ flags, u32* __restrict__ other_in,
                                                       u32* __restrict__ other_tab) {
    const u32 t = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    const u64* __restrict__ si = a.si[p];
    const u64* __restrict__ st = a.st[p];
    if (t < n) {
        const u64 v = si[t];
        const u32 rank = t - lower_bound_u64(si, n, v);
        const u32 lb = lower_bound_u64(st, n, v), ub = upper_bound_u64(st, n, v);
        other_in[(size_t)p * n + t] = lb;
        const bool matched = rank < ub - lb;
        if (matched) a.pt[p][t] = v;
        flags[flag_at(FL_POP, pairs, n, p, t)] = (!matched && ub < n) ? 1u : 0u;
        flags[flag_at(FL_TAIL, pairs, n, p, t)] = (!matched && ub >= n) ? 1u : 0u;
        if (t == 0)
            for (u32 c = 0; c < FL_CLASSES; c++) flags[flag_at(c, pairs, n, p, n)] = 0;
    } else if (t < 2 * n) {
        const u32 j = t - n;
        const u64 b = st[j];
        const u32 rank = j - lower_bound_u64(st, n, b);
        const u32 lb = lower_bound_u64(si, n, b), ub = upper_bound_u64(si, n, b);
        other_tab[(size_t)p * n + j] = lb;
        flags[flag_at(FL_PUSH, pairs, n, p, j)] = rank < ub - lb ? 0u : 1u;
    }
}

// ev_base[p] = where pair p's events start in the concatenated event list, ev_base[pairs] = their number
__global__ void event_base_kernel(const u32* __restrict__ sc, u32 pairs, u32 n, u32* __restrict__ ev_base) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    u32 acc = 0;
    for (u32 p = 0; p < pairs; p++) {
        ev_base[p] = acc;
        acc += before(sc, FL_POP, pairs, n, p, n) + before(sc, FL_PUSH, pairs, n, p, n);
    }
    ev_base[pairs] = acc;
}

// events in loop order: delta[e] = +1 (push) / -1 (pop), src[e] = table index / input index, ev_pair[e] = the pair
__global__ __launch_bounds__(256) void place_events_kernel(u32 pairs, u32 n, const u32* __restrict__ flags, const u32* __restrict__ sc,
                                                           const u32* __restrict__ other_in, const u32* __restrict__ other_tab,
                                                           const u32* __restrict__ ev_base, int* __restrict__ delta, u32* __restrict__ src,
                                                           u32* __restrict__ ev_pair) {
    const u32 t = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (t < n) {
        if (!flags[flag_at(FL_POP, pairs, n, p, t)]) return;
        const u32 e = ev_base[p] + before(sc, FL_POP, pairs, n, p, t) + before(sc, FL_PUSH, pairs, n, p, other_in[(size_t)p * n + t]);
        delta[e] = -1;
        src[e] = t;
        ev_pair[e] = p;
    } else if (t < 2 * n) {
        const u32 j = t - n;
        if (!flags[flag_at(FL_PUSH, pairs, n, p, j)]) return;
        const u32 e = ev_base[p] + before(sc, FL_PUSH, pairs, n, p, j) + before(sc, FL_POP, pairs, n, p, other_tab[(size_t)p * n + j]);
        delta[e] = 1;
        src[e] = j;
        ev_pair[e] = p;
    }
}

__global__ __launch_bounds__(256) void clamp_min_kernel(const int* __restrict__ s, u32 count, int* __restrict__ m) {
    const u32 e = blockIdx.x * 256 + threadIdx.x;
    if (e < count) m[e] = s[e] < 0 ? s[e] : 0;
}

// Flags of the events: two runs of count + 1 entries (empty pops, then free pushes), entry `count` of each is 0.
// level key of every event: pushes sort under the height they create, matched pops under the height they remove;
// pops that found the stack empty get level 0 and an `empty_pop` flag.  The pair index sits above the level.
__global__ __launch_bounds__(256) void level_kernel(const int* __restrict__ delta, const int* __restrict__ s, const int* __restrict__ runmin,
                                                    const u32* __restrict__ ev_pair, const u32* __restrict__ ev_base, u32 count, u32 level_bits,
                                                    u32* __restrict__ key, u32* __restrict__ ident, u32* __restrict__ empty_pop) {
    const u32 e = blockIdx.x * 256 + threadIdx.x;
    if (e > count) return;
    if (e == count) { empty_pop[e] = 0; return; }
    const u32 p = ev_pair[e];
    const int m = runmin[e], m_prev = e != ev_base[p] ? runmin[e - 1] : 0;
    const int height = s[e] - m;                      // stack height after the event
    const bool unmatched = delta[e] < 0 && s[e] < m_prev;
    ident[e] = e;
    empty_pop[e] = unmatched ? 1u : 0u;
    const u32 level = delta[e] > 0 ? (u32)height : (unmatched ? 0u : (u32)height + 1u);
    key[e] = (p << level_bits) | level;
}

// after the stable sort by (pair, level) a matched pop sits right behind its push
__global__ __launch_bounds__(256) void pair_kernel(PairArgs a, const u32* __restrict__ key_sorted, const u32* __restrict__ ev_sorted, u32 count,
                                                   u32 level_bits, const int* __restrict__ delta, const u32* __restrict__ src,
                                                   u32* __restrict__ free_push) {
    const u32 q = blockIdx.x * 256 + threadIdx.x;
    if (q > count) return;
    if (q == count) { free_push[count] = 0; return; }
    const u32 e = ev_sorted[q];
    if (delta[e] > 0) {
        const bool taken = q + 1 < count && key_sorted[q + 1] == key_sorted[q] && delta[ev_sorted[q + 1]] < 0;
        free_push[e] = taken ? 0u : 1u;
    } else {
        free_push[e] = 0;
        const u32 p = key_sorted[q] >> level_bits;
        if ((key_sorted[q] & ((1u << level_bits) - 1u)) != 0 && q > 0) a.pt[p][src[e]] = a.st[p][src[ev_sorted[q - 1]]];
    }
}

// step 4: slot list (unmatched pops, then tail inputs) and value list (free pushes) of every pair, then the fill.
// ev_sc: exclusive scan of the events' flags (empty pops at [0, count], free pushes at [count + 1, 2 count + 1]).
__global__ __launch_bounds__(256) void gather_lists_kernel(PairArgs a, u32 pairs, u32 n, u32 count, const u32* __restrict__ ev_base,
                                                           const u32* __restrict__ src, const u32* __restrict__ ev_flags,
                                                           const u32* __restrict__ ev_sc, const u32* __restrict__ flags,
                                                           const u32* __restrict__ sc, u32* __restrict__ slots, u64* __restrict__ values) {
    const u32 t = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    const u32 base = ev_base[p], mine = ev_base[p + 1] - base;
    const u32* __restrict__ free_flags = ev_flags + count + 1;
    const u32* __restrict__ free_sc = ev_sc + count + 1;
    if (t < mine) {
        const u32 g = base + t;
        if (ev_flags[g]) { const u32 k = ev_sc[g] - ev_sc[base]; if (k < n) slots[(size_t)p * n + k] = src[g]; }
        if (free_flags[g]) { const u32 k = free_sc[g] - free_sc[base]; if (k < n) values[(size_t)p * n + k] = a.st[p][src[g]]; }
    }
    if (t < n && flags[flag_at(FL_TAIL, pairs, n, p, t)]) {
        const u32 k = (ev_sc[base + mine] - ev_sc[base]) + before(sc, FL_TAIL, pairs, n, p, t);
        if (k < n) slots[(size_t)p * n + k] = t;
    }
}

__global__ __launch_bounds__(256) void fill_kernel(PairArgs a, u32 n, u32 count, const u32* __restrict__ ev_base, const u32* __restrict__ ev_sc,
                                                   const u32* __restrict__ slots, const u64* __restrict__ values) {
    const u32 k = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    const u32* __restrict__ free_sc = ev_sc + count + 1;
    const u32 free_total = free_sc[ev_base[p + 1]] - free_sc[ev_base[p]];
    if (k < n && k < free_total) {
        const u32 slot = slots[(size_t)p * n + k];
        if (slot < n) a.pt[p][slot] = values[(size_t)p * n + k];
    }
}

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

// radix sorts of one length share their temporary storage (everything runs on one stream)
struct SortU64 {
    size_t n, bytes = 0;
    void* tmp = nullptr;
    SortU64(Scratch& mem, hipStream_t stream, size_t n_) : n(n_) {
        HIP_CHECK(rocprim::radix_sort_keys(nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, n, 0, 64, stream));
        tmp = mem.alloc<unsigned char>(bytes);
    }
    void run(hipStream_t stream, const u64* in, u64* out) { HIP_CHECK(rocprim::radix_sort_keys(tmp, bytes, in, out, n, 0, 64, stream)); }
};

template <typename T, typename Op>
void scan_exclusive(Scratch& mem, hipStream_t stream, const T* in, T* out, T init, size_t n, Op op) {
    size_t bytes = 0;
    HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, out, init, n, op, stream));
    void* tmp = mem.alloc<unsigned char>(bytes);
    HIP_CHECK(rocprim::exclusive_scan(tmp, bytes, in, out, init, n, op, stream));
}
// inclusive scan that starts again wherever the key changes
template <typename T, typename Op>
void scan_inclusive_by_key(Scratch& mem, hipStream_t stream, const u32* keys, const T* in, T* out, size_t n, Op op) {
    size_t bytes = 0;
    HIP_CHECK(rocprim::inclusive_scan_by_key(nullptr, bytes, keys, in, out, n, op, rocprim::equal_to<u32>(), stream));
    void* tmp = mem.alloc<unsigned char>(bytes);
    HIP_CHECK(rocprim::inclusive_scan_by_key(tmp, bytes, keys, in, out, n, op, rocprim::equal_to<u32>(), stream));
}

u32 bit_length(u64 v) { u32 b = 0; while (v) { b++; v >>= 1; } return b; }

// One batch of at most kMaxBatch pairs of n rows.  tables[k]: the distinct table columns (any words), sorted once each;
// table_of[p]: which of them pair p looks into.  Enqueued on the context's stream; `mem` is released by the caller.
void permuted_batch(DeviceCtx* ctx, Scratch& mem, u32 n, const u64* const* tables, u32 n_tables, const PermutedPair* pairs_in,
                    const u32* table_of, u32 pairs) {
    hipStream_t stream = ctx->stream;
    // ---- 1. canonical, sorted: every distinct table once, every pair's inputs into its permuted_inputs
    u64* canon = mem.alloc<u64>((size_t)std::max(pairs, n_tables) * n);
    u64* st = mem.alloc<u64>((size_t)n_tables * n);
    SortU64 sort(mem, stream, n);
    CanonArgs ca = {};
    for (u32 k = 0; k < n_tables; k++) ca.src[k] = tables[k];
    hipLaunchKernelGGL(canon_kernel, dim3(blocks(n), n_tables), dim3(256), 0, stream, ca, canon, n);
    for (u32 k = 0; k < n_tables; k++) sort.run(stream, canon + (size_t)k * n, st + (size_t)k * n);
    PairArgs a = {};
    for (u32 p = 0; p < pairs; p++) {
        ca.src[p] = pairs_in[p].inputs;
        a.si[p] = pairs_in[p].permuted_inputs;
        a.st[p] = st + (size_t)table_of[p] * n;
        a.pt[p] = pairs_in[p].permuted_table;
    }
    hipLaunchKernelGGL(canon_kernel, dim3(blocks(n), pairs), dim3(256), 0, stream, ca, canon, n);
    for (u32 p = 0; p < pairs; p++) sort.run(stream, canon + (size_t)p * n, pairs_in[p].permuted_inputs);
    // ---- 2. classify, order the events
    const size_t n_flags = (size_t)FL_CLASSES * pairs * (n + 1);
    u32* flags = mem.alloc<u32>(n_flags);
    u32* sc = mem.alloc<u32>(n_flags);
    u32* other_in = mem.alloc<u32>((size_t)pairs * n);
    u32* other_tab = mem.alloc<u32>((size_t)pairs * n);
    u32* ev_base = mem.alloc<u32>(kMaxBatch + 1);
    hipLaunchKernelGGL(classify_kernel, dim3(blocks(2 * (size_t)n), pairs), dim3(256), 0, stream, a, pairs, n, flags, other_in, other_tab);
    scan_exclusive(mem, stream, flags, sc, 0u, n_flags, rocprim::plus<u32>());
    hipLaunchKernelGGL(event_base_kernel, dim3(1), dim3(64), 0, stream, sc, pairs, n, ev_base);
    u32 base_host[kMaxBatch + 1];
    HIP_CHECK(hipMemcpyAsync(base_host, ev_base, (pairs + 1) * sizeof(u32), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const u32 count = base_host[pairs];
    if (count == 0) return;        // every input found its table entry: no push, hence nothing left to place
    u32 most = 0;
    for (u32 p = 0; p < pairs; p++) most = std::max(most, base_host[p + 1] - base_host[p]);
    // ---- 3. the stack, as bracket matching
    const u32 level_bits = bit_length(2 * (u64)n), pair_bits = bit_length(pairs - 1);
    int* delta = mem.alloc<int>(count);
    u32* src = mem.alloc<u32>(count);
    u32* ev_pair = mem.alloc<u32>(count);
    int* s = mem.alloc<int>(count);
    int* runmin = mem.alloc<int>(count);
    int* clamped = mem.alloc<int>(count);
    u32* key = mem.alloc<u32>(count);
    u32* ident = mem.alloc<u32>(count);
    u32* key_sorted = mem.alloc<u32>(count);
    u32* ev_sorted = mem.alloc<u32>(count);
    u32* ev_flags = mem.alloc<u32>(2 * ((size_t)count + 1));
    u32* ev_sc = mem.alloc<u32>(2 * ((size_t)count + 1));
    hipLaunchKernelGGL(place_events_kernel, dim3(blocks(2 * (size_t)n), pairs), dim3(256), 0, stream, pairs, n, flags, sc, other_in, other_tab,
                       ev_base, delta, src, ev_pair);
    scan_inclusive_by_key(mem, stream, ev_pair, delta, s, count, rocprim::plus<int>());
    hipLaunchKernelGGL(clamp_min_kernel, dim3(blocks(count)), dim3(256), 0, stream, s, count, clamped);
    scan_inclusive_by_key(mem, stream, ev_pair, clamped, runmin, count, rocprim::minimum<int>());
    hipLaunchKernelGGL(level_kernel, dim3(blocks((size_t)count + 1)), dim3(256), 0, stream, delta, s, runmin, ev_pair, ev_base, count, level_bits,
                       key, ident, ev_flags);
    {
        size_t bytes = 0;
        HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, key, key_sorted, ident, ev_sorted, count, 0, level_bits + pair_bits, stream));
        void* tmp = mem.alloc<unsigned char>(bytes);
        HIP_CHECK(rocprim::radix_sort_pairs(tmp, bytes, key, key_sorted, ident, ev_sorted, count, 0, level_bits + pair_bits, stream));
    }
    hipLaunchKernelGGL(pair_kernel, dim3(blocks((size_t)count + 1)), dim3(256), 0, stream, a, key_sorted, ev_sorted, count, level_bits, delta, src,
                       ev_flags + count + 1);
    scan_exclusive(mem, stream, ev_flags, ev_sc, 0u, 2 * ((size_t)count + 1), rocprim::plus<u32>());
    // ---- 4. leftovers
    u32* slots = mem.alloc<u32>((size_t)pairs * n);
    u64* values = mem.alloc<u64>((size_t)pairs * n);
    // both lists of a pair have free_total entries (two columns of one height: the loop ends with as many open slots as unused
    // values); the kernels bound every index by n all the same, a compare per store
    hipLaunchKernelGGL(gather_lists_kernel, dim3(blocks(std::max<size_t>(n, most)), pairs), dim3(256), 0, stream, a, pairs, n, count, ev_base, src,
                       ev_flags, ev_sc, flags, sc, slots, values);
    hipLaunchKernelGGL(fill_kernel, dim3(blocks(n), pairs), dim3(256), 0, stream, a, n, count, ev_base, ev_sc, slots, values);
}

}  // namespace

void permuted_cols_batch_dev(DeviceCtx* ctx, size_t n_, const u64* const* tables, size_t n_tables, const PermutedPair* pairs, size_t n_pairs) {
    if (n_ == 0 || n_pairs == 0) return;
    if (n_ >= ((size_t)1 << 30)) throw OlaError(-2, "permuted_cols: more than 2^30 rows");
    const u32 n = (u32)n_;
    for (size_t p = 0; p < n_pairs; p++)
        if (pairs[p].table >= n_tables) throw OlaError(-1, "permuted_cols: a pair names a table beyond the list");
    // a group: as many pairs as the kernel argument holds, the level key has bits for and the 32-bit prefix sums can count
    const u32 level_bits = bit_length(2 * (u64)n);
    size_t group = kMaxBatch;
    while (group > 1 && (bit_length(group - 1) + level_bits > 32 || (size_t)FL_CLASSES * group * ((size_t)n + 1) >= ((size_t)1 << 32))) group >>= 1;
    for (size_t first = 0; first < n_pairs; first += group) {
        const u32 count = (u32)std::min(group, n_pairs - first);
        // the distinct tables of this group
        const u64* tabs[kMaxBatch];
        u32 table_of[kMaxBatch], n_tabs = 0;
        for (u32 p = 0; p < count; p++) {
            const u64* t = tables[pairs[first + p].table];
            u32 k = 0;
            while (k < n_tabs && tabs[k] != t) k++;
            if (k == n_tabs) tabs[n_tabs++] = t;
            table_of[p] = k;
        }
        Scratch mem(ctx);
        permuted_batch(ctx, mem, n, tabs, n_tabs, pairs + first, table_of, count);
        HIP_CHECK(hipGetLastError());
    }
}

void permuted_cols_dev(DeviceCtx* ctx, const u64* inputs, const u64* table, size_t n, u64* permuted_inputs, u64* permuted_table) {
    const PermutedPair pair = {inputs, 0, permuted_inputs, permuted_table};
    permuted_cols_batch_dev(ctx, n, &table, 1, &pair, 1);
}

// ------------------------------------------------------------------------------------------------ sort / scan for check.hip
// the key + payload variant of SortU64 (rocPRIM's radix sort is stable: equal keys keep the order of their payloads)
size_t sort_pairs_tmp_bytes(size_t n) {
    size_t bytes = 0;
    HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, n, 0, 64, (hipStream_t) nullptr));
    return std::max<size_t>(bytes, 8);
}
void sort_pairs_dev(hipStream_t stream, void* tmp, size_t tmp_bytes, const u64* keys_in, u64* keys_out, const u32* payload_in, u32* payload_out,
                    size_t n) {
    HIP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, payload_in, payload_out, n, 0, 64, stream));
}
size_t exclusive_sum_tmp_bytes(size_t n) {
    size_t bytes = 0;
    HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, (const u32*)nullptr, (u32*)nullptr, 0u, n, rocprim::plus<u32>(), (hipStream_t) nullptr));
    return std::max<size_t>(bytes, 8);
}
void exclusive_sum_dev(hipStream_t stream, void* tmp, size_t tmp_bytes, const u32* in, u32* out, size_t n) {
    HIP_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0u, n, rocprim::plus<u32>(), stream));
}

// ------------------------------------------------------------------------------------------------ table generators
// The range-check, bitwise and program tables from their primary columns (generation/builtin.rs:35-206, 249-316,
// generation/prog.rs:18-156): one fill kernel per table writes every column that is not a permuted one -- thread = row, so
// every column is stored along rows, and rows beyond the live inputs get their zeros in the same pass -- then the table's
// lookup pairs go through one batch of permuted_cols, straight into their columns of `out`.
namespace {

namespace tg = olatg;
namespace tc = olatgc;
namespace tm = olatgm;
namespace tx = olatgx;

__global__ __launch_bounds__(256) void rc_fill_kernel(const u64* __restrict__ vals, const u64* __restrict__ filters, u32 n_rows, u32 range_bits,
                                                      u32 n, u64* __restrict__ out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool live = i < n_rows;
    const u64 v = live ? gl_canon(vals[i]) : 0;
    const u32 filter_cols[4] = {tg::RC_CPU_FILTER, tg::RC_MEMORY_SORT_FILTER, tg::RC_MEMORY_REGION_FILTER, tg::RC_CMP_FILTER};
#pragma unroll
    for (u32 k = 0; k < 4; k++) out[(size_t)filter_cols[k] * n + i] = (live && filters) ? gl_canon(filters[(size_t)k * n_rows + i]) : 0;
    const u64 top = ((u64)1 << range_bits) - 1;
    out[(size_t)tg::RC_VAL * n + i] = v;
    out[(size_t)tg::RC_LIMB_LO * n + i] = v & top;
    out[(size_t)tg::RC_LIMB_HI * n + i] = v >> range_bits;
    out[(size_t)tg::RC_FIX_RANGE_CHECK_U16 * n + i] = i < top ? i : top;
}

__device__ __forceinline__ u64 compress4(u64 tag, u64 a, u64 b, u64 c, u64 beta) {
    return gl_add(gl_mul(gl_add(gl_mul(gl_add(gl_mul(c, beta), b), beta), a), beta), tag);     // tag + a B + b B^2 + c B^3
}

// ops: filter, tag, op0, op1, res (n_ops each).  skip_limb3: the reference's generator leaves the three limb-3 columns zero.
__global__ __launch_bounds__(256) void bitwise_fill_kernel(const u64* __restrict__ ops, u32 n_ops, u32 limb_bits, u64 beta, u32 skip_limb3,
                                                           u32 n, u64* __restrict__ out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool live = i < n_ops;
    const u64 mask = ((u64)1 << limb_bits) - 1;
    u64 w[5];
#pragma unroll
    for (u32 k = 0; k < 5; k++) w[k] = live ? gl_canon(ops[(size_t)k * n_ops + i]) : 0;
    out[(size_t)tg::BW_FILTER * n + i] = w[0];
    out[(size_t)tg::BW_TAG * n + i] = w[1];
    out[(size_t)tg::BW_OP0 * n + i] = w[2];
    out[(size_t)tg::BW_OP1 * n + i] = w[3];
    out[(size_t)tg::BW_RES * n + i] = w[4];
#pragma unroll
    for (u32 l = 0; l < 4; l++) {
        const bool keep = !(skip_limb3 && l == 3);
        const u64 a = keep ? (w[2] >> (limb_bits * l)) & mask : 0;
        const u64 b = keep ? (w[3] >> (limb_bits * l)) & mask : 0;
        const u64 c = keep ? (w[4] >> (limb_bits * l)) & mask : 0;
        out[(size_t)(tg::BW_OP0_LIMBS_START + l) * n + i] = a;
        out[(size_t)(tg::BW_OP1_LIMBS_START + l) * n + i] = b;
        out[(size_t)(tg::BW_RES_LIMBS_START + l) * n + i] = c;
        out[(size_t)(tg::BW_COMPRESS_LIMBS_START + l) * n + i] = compress4(w[1], a, b, c, beta);
    }
    // the fixed tables: 0 .. 2^limb_bits - 1 then zeros; AND, OR, XOR of every operand pair, one operation after the other
    const u64 per = (u64)1 << (2 * limb_bits);
    const u32 which = (u32)(i / per);
    const u64 index = i % per;
    const bool fixed = which < 3;
    const u64 x = fixed ? index >> limb_bits : 0, y = fixed ? index & mask : 0;
    const u64 z = !fixed ? 0 : which == 0 ? (x & y) : which == 1 ? (x | y) : (x ^ y);
    const u64 tag = !fixed ? 0 : which == 0 ? tg::OP_MASK_AND : which == 1 ? tg::OP_MASK_OR : tg::OP_MASK_XOR;
    out[(size_t)tg::BW_FIX_RANGE_CHECK_U8 * n + i] = i <= mask ? i : 0;
    out[(size_t)tg::BW_FIX_TAG * n + i] = tag;
    out[(size_t)tg::BW_FIX_BITWSIE_OP0 * n + i] = x;
    out[(size_t)tg::BW_FIX_BITWSIE_OP1 * n + i] = y;
    out[(size_t)tg::BW_FIX_BITWSIE_RES * n + i] = z;
    out[(size_t)tg::BW_FIX_COMPRESS * n + i] = compress4(tag, x, y, z, beta);
}

// side: a0 .. a3, pc, inst, filter (n each) -> its six data columns, its compress column, its filter column
__device__ __forceinline__ void prog_side(const u64* __restrict__ side, u32 i, u32 n, u64 beta, u32 addr_start, u32 pc_col, u32 inst_col,
                                          u32 comp_col, u32 filter_col, u64* __restrict__ out) {
    u64 w[7];
#pragma unroll
    for (u32 k = 0; k < 7; k++) w[k] = gl_canon(side[(size_t)k * n + i]);
#pragma unroll
    for (u32 k = 0; k < 4; k++) out[(size_t)(addr_start + k) * n + i] = w[k];
    out[(size_t)pc_col * n + i] = w[4];
    out[(size_t)inst_col * n + i] = w[5];
    out[(size_t)filter_col * n + i] = w[6];
    u64 acc = w[5];                                     // a0 + a1 B + a2 B^2 + a3 B^3 + pc B^4 + inst B^5
#pragma unroll
    for (int k = 4; k >= 0; k--) acc = gl_add(gl_mul(acc, beta), w[k]);
    out[(size_t)comp_col * n + i] = acc;
}
__global__ __launch_bounds__(256) void prog_fill_kernel(const u64* __restrict__ exec, const u64* __restrict__ prog, u32 n, u64 beta,
                                                        u64* __restrict__ out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    prog_side(exec, i, n, beta, tg::COL_PROG_EXEC_CODE_ADDR_RANGE_START, tg::COL_PROG_EXEC_PC, tg::COL_PROG_EXEC_INST, tg::COL_PROG_EXEC_COMP_PROG,
              tg::COL_PROG_FILTER_EXEC, out);
    prog_side(prog, i, n, beta, tg::COL_PROG_CODE_ADDR_RANGE_START, tg::COL_PROG_PC, tg::COL_PROG_INST, tg::COL_PROG_COMP_PROG,
              tg::COL_PROG_FILTER_PROG_CHUNK, out);
}

// ---- the CPU table and the program table's executed side from step records (generation/cpu.rs:11-218, generation/prog.rs:31-108)
// A step record is what cpu.rs copies from one `Step`: tc::STEP_COPIED_COLS words = CPU columns COL_ENV_IDX .. the last register
// selector (cpu.rs:64-105), then filter_tape_looking; records are column-major tc::STEP_WORDS x n_steps.
__device__ __forceinline__ u64 step_word(const u64* __restrict__ steps, u32 n_steps, u32 col, u32 i) {
    return gl_canon(steps[(size_t)(col - tc::STEP_FIRST_COL) * n_steps + i]);
}
__device__ __forceinline__ bool is_op(u64 opcode, u32 shift) { return opcode == (u64)1 << shift; }

// cpu.rs:20-60, the column of the opcode's selector; 0 (no selector column) for a word that is none of the 25 masks
__device__ __forceinline__ u32 opcode_selector(u64 opcode) {
    if (opcode == 0 || (opcode & (opcode - 1)) != 0 || (opcode >> 32) != 0) return 0;
    switch ((u32)__ffsll((unsigned long long)opcode) - 1u) {
        case tc::OP_SHIFT_ADD: case tc::OP_SHIFT_MUL: case tc::OP_SHIFT_EQ: case tc::OP_SHIFT_ASSERT: case tc::OP_SHIFT_NEQ:
            return tc::COL_S_SIMPLE_ARITHMATIC_OP;
        case tc::OP_SHIFT_MOV: return tc::COL_S_MOV;
        case tc::OP_SHIFT_JMP: return tc::COL_S_JMP;
        case tc::OP_SHIFT_CJMP: return tc::COL_S_CJMP;
        case tc::OP_SHIFT_CALL: return tc::COL_S_CALL;
        case tc::OP_SHIFT_RET: return tc::COL_S_RET;
        case tc::OP_SHIFT_MLOAD: return tc::COL_S_MLOAD;
        case tc::OP_SHIFT_MSTORE: return tc::COL_S_MSTORE;
        case tc::OP_SHIFT_END: return tc::COL_S_END;
        case tc::OP_SHIFT_RC: return tc::COL_S_RC;
        case tc::OP_SHIFT_AND: case tc::OP_SHIFT_OR: case tc::OP_SHIFT_XOR: return tc::COL_S_BITWISE;
        case tc::OP_SHIFT_NOT: return tc::COL_S_NOT;
        case tc::OP_SHIFT_GTE: return tc::COL_S_GTE;
        case tc::OP_SHIFT_POSEIDON: return tc::COL_S_PSDN;
        case tc::OP_SHIFT_SLOAD: return tc::COL_S_SLOAD;
        case tc::OP_SHIFT_SSTORE: return tc::COL_S_SSTORE;
        case tc::OP_SHIFT_TLOAD: return tc::COL_S_TLOAD;
        case tc::OP_SHIFT_TSTORE: return tc::COL_S_TSTORE;
        case tc::OP_SHIFT_SCCALL: return tc::COL_S_CALL_SC;
        default: return 0;
    }
}

// thread = row: the record is loaded along rows, all 94 columns are stored along rows; rows n_steps .. n are cpu.rs:180-208's padding
__global__ __launch_bounds__(256) void cpu_fill_kernel(const u64* __restrict__ steps, u32 n_steps, u32 n, u64* __restrict__ out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool live = i < n_steps;
    const u32 r = live ? i : n_steps - 1;                                     // padding carries INST and IDX_STORAGE of the last live row
    const u64 end_mask = (u64)1 << tc::OP_SHIFT_END;
    out[(size_t)tc::COL_TX_IDX * n + i] = 0;
    u64 opcode = end_mask, env_idx = 0, is_ext = 0, ext_cnt = 0, op1_imm = 0, op0 = 0, op1 = 0;
#pragma unroll
    for (u32 c = tc::STEP_FIRST_COL; c < tc::STEP_FIRST_COL + tc::STEP_COPIED_COLS; c++) {
        u64 v = 0;
        if (live) v = step_word(steps, n_steps, c, i);
        else if (c == tc::COL_OPCODE) v = end_mask;
        else if (c == tc::COL_INST) v = n_steps ? step_word(steps, n_steps, c, r) : (u64)1048576;
        else if (c == tc::COL_IDX_STORAGE) v = n_steps ? step_word(steps, n_steps, c, r) : 0;
        out[(size_t)c * n + i] = v;
        if (c == tc::COL_OPCODE) opcode = v;
        if (c == tc::COL_ENV_IDX) env_idx = v;
        if (c == tc::COL_IS_EXT_LINE) is_ext = v;
        if (c == tc::COL_EXT_CNT) ext_cnt = v;
        if (c == tc::COL_OP1_IMM) op1_imm = v;
        if (c == tc::COL_OP0) op0 = v;
        if (c == tc::COL_OP1) op1 = v;
    }
    const u32 sel = opcode_selector(opcode);
#pragma unroll
    for (u32 c = tc::COL_S_SIMPLE_ARITHMATIC_OP; c <= tc::COL_S_CALL_SC; c++) out[(size_t)c * n + i] = c == sel ? 1 : 0;
    const bool entry = env_idx == 0;
    const bool end = is_op(opcode, tc::OP_SHIFT_END), sload = is_op(opcode, tc::OP_SHIFT_SLOAD), sstore = is_op(opcode, tc::OP_SHIFT_SSTORE);
    const bool sccall = is_op(opcode, tc::OP_SHIFT_SCCALL), mem = is_op(opcode, tc::OP_SHIFT_MLOAD) || is_op(opcode, tc::OP_SHIFT_MSTORE);
    // cpu.rs:119-132 ext_length; TLOAD's op0 * op1 + (1 - op0) in the field
    u64 ext_length = 0;
    if (sload || sstore || sccall || (end && !entry)) ext_length = 1;
    else if (is_op(opcode, tc::OP_SHIFT_TLOAD)) ext_length = gl_add(gl_mul(op0, op1), gl_sub(1, op0));
    else if (is_op(opcode, tc::OP_SHIFT_TSTORE)) ext_length = op1;
    out[(size_t)tc::COL_IS_ENTRY_SC * n + i] = entry ? 1 : 0;
    out[(size_t)tc::COL_IS_NEXT_LINE_DIFF_INST * n + i] = (!live || ext_length == ext_cnt) ? 1 : 0;
    out[(size_t)tc::COL_IS_NEXT_LINE_SAME_TX * n + i] = (!live || (entry && end)) ? 0 : 1;
    out[(size_t)tc::COL_FILTER_TAPE_LOOKING * n + i] = live ? gl_canon(steps[(size_t)tc::STEP_FILTER_TAPE_LOOKING * n_steps + i]) : 0;
    out[(size_t)tc::IS_SCCALL_EXT_LINE * n + i] = (live && sccall && ext_cnt == 1) ? 1 : 0;
    out[(size_t)tc::COL_IS_STORAGE_EXT_LINE * n + i] = (live && (sload || sstore) && is_ext == 1) ? 1 : 0;
    out[(size_t)tc::COL_FILTER_SCCALL_END * n + i] = (live && end && is_ext == 1) ? 1 : 0;
    out[(size_t)tc::COL_FILTER_LOOKING_PROG_IMM * n + i] = (live && is_ext != 1 && (mem || op1_imm == 1)) ? 1 : 0;
    out[(size_t)tc::COL_IS_PADDING * n + i] = live ? 0 : 1;
}

// prog.rs:31-44: rows a step gives to the executed side -- none for an extension line, two when an immediate word follows
__device__ __forceinline__ u32 step_exec_rows(const u64* __restrict__ steps, u32 n_steps, u32 i) {
    if (step_word(steps, n_steps, tc::COL_IS_EXT_LINE, i) == 1) return 0;
    const u64 opcode = step_word(steps, n_steps, tc::COL_OPCODE, i);
    const bool two = step_word(steps, n_steps, tc::COL_OP1_IMM, i) == 1 || is_op(opcode, tc::OP_SHIFT_MLOAD) || is_op(opcode, tc::OP_SHIFT_MSTORE);
    return two ? 2 : 1;
}
// counts[n_steps] = 0: the exclusive scan then ends with the total
__global__ __launch_bounds__(256) void exec_count_kernel(const u64* __restrict__ steps, u32 n_steps, u32* __restrict__ counts) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i <= n_steps) counts[i] = i < n_steps ? step_exec_rows(steps, n_steps, i) : 0;
}
// prog.rs:59-108 into a side of ola_generate_prog_trace: a0 .. a3, pc, inst, filter (n each); every row written is below n
__global__ __launch_bounds__(256) void exec_scatter_kernel(const u64* __restrict__ steps, u32 n_steps, const u32* __restrict__ at, u32 n,
                                                           u64* __restrict__ exec) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_steps) return;
    const u32 rows = at[i + 1] - at[i], row = at[i];
    if (rows == 0 || row + rows > n) return;
    const u64 pc = step_word(steps, n_steps, tc::COL_PC, i);
    for (u32 k = 0; k < rows; k++) {
#pragma unroll
        for (u32 j = 0; j < 4; j++) exec[(size_t)j * n + row + k] = step_word(steps, n_steps, tc::COL_ADDR_CODE_RANGE_START + j, i);
        exec[(size_t)4 * n + row + k] = k ? gl_add(pc, 1) : pc;
        exec[(size_t)5 * n + row + k] = step_word(steps, n_steps, k ? tc::COL_IMM_VAL : tc::COL_INST, i);
        exec[(size_t)6 * n + row + k] = 1;
    }
}
// rows total .. n: executed row 0 again with filter 0 (this project's filler, which keeps the lookup's inputs inside the listing), or zeros
__global__ __launch_bounds__(256) void exec_filler_kernel(u32 total, u32 repeat_row0, u32 n, u64* __restrict__ exec) {
    const u32 i = total + blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (u32 j = 0; j < 6; j++) exec[(size_t)j * n + i] = repeat_row0 ? exec[(size_t)j * n] : 0;
    exec[(size_t)6 * n + i] = 0;
}

// ---- the memory table from raw cells and the comparison table from operand pairs (ola_generate_memory_trace / ola_generate_cmp_trace;
// olavm_amd/air/miniexec.py memory_trace, tracegen.py generate_cmp_trace; generation/memory.rs:5-153, generation/builtin.rs:208-247)
// A cell is tm::MEM_CELL_WORDS words, column-major: address, clock, op (the opcode's one-hot word), value, is_write.
enum : u32 { CELL_ADDR = 0, CELL_CLK = 1, CELL_OP = 2, CELL_VALUE = 3, CELL_IS_WRITE = 4 };

// the op's place in the row order: the rank of one of the nine ops (`sel`: its selector column), else -- behind them, in word order --
// MEM_OPS + the canonical word (below 2^64: p + 9 is), and no selector (0)
__device__ __forceinline__ u64 mem_op_key(u64 op, u32& sel) {
    sel = 0;
    switch (op) {
        case tm::MEM_OP_MASK_CALL: sel = tm::COL_MEM_S_CALL; return tm::MEM_OP_RANK_CALL;
        case tm::MEM_OP_MASK_MLOAD: sel = tm::COL_MEM_S_MLOAD; return tm::MEM_OP_RANK_MLOAD;
        case tm::MEM_OP_MASK_MSTORE: sel = tm::COL_MEM_S_MSTORE; return tm::MEM_OP_RANK_MSTORE;
        case tm::MEM_OP_MASK_POSEIDON: sel = tm::COL_MEM_S_POSEIDON; return tm::MEM_OP_RANK_POSEIDON;
        case tm::MEM_OP_MASK_RET: sel = tm::COL_MEM_S_RET; return tm::MEM_OP_RANK_RET;
        case tm::MEM_OP_MASK_SLOAD: sel = tm::COL_MEM_S_SLOAD; return tm::MEM_OP_RANK_SLOAD;
        case tm::MEM_OP_MASK_SSTORE: sel = tm::COL_MEM_S_SSTORE; return tm::MEM_OP_RANK_SSTORE;
        case tm::MEM_OP_MASK_TLOAD: sel = tm::COL_MEM_S_TLOAD; return tm::MEM_OP_RANK_TLOAD;
        case tm::MEM_OP_MASK_TSTORE: sel = tm::COL_MEM_S_TSTORE; return tm::MEM_OP_RANK_TSTORE;
        default: return tm::MEM_OPS + op;
    }
}
__device__ __forceinline__ u64 mem_sort_key(const u64* __restrict__ canon, u32 n_cells, u32 field, u32 r) {
    const u64 v = canon[(size_t)field * n_cells + r];
    u32 sel;
    return field == CELL_OP ? mem_op_key(v, sel) : v;
}

// What the host reads before it sorts: stats[f], f < 5 = the OR of every cell's sort key of field f (a pass of the sort covers the bits
// set there, and a field whose keys are all 0 needs none), stats[MS_BELOW_HEAP] = cells below the heap region -- sorted by address the heap
// rows are a suffix, so this is the index of the first heap row.
enum : u32 { MS_BELOW_HEAP = tm::MEM_CELL_WORDS, MS_WORDS };
// canonical cells, the identity index, and the statistics: reduced over the wave, then one atomic per wave and word
__global__ __launch_bounds__(256) void mem_key_kernel(const u64* __restrict__ cells, u32 n_cells, u64* __restrict__ canon, u32* __restrict__ idx,
                                                      unsigned long long* __restrict__ stats) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n_cells;
    unsigned long long r[MS_WORDS] = {};
    if (live) {
        u32 sel;
#pragma unroll
        for (u32 f = 0; f < tm::MEM_CELL_WORDS; f++) {
            const u64 w = gl_canon(cells[(size_t)f * n_cells + i]);
            canon[(size_t)f * n_cells + i] = w;
            r[f] = f == CELL_OP ? mem_op_key(w, sel) : w;
        }
        idx[i] = i;
        r[MS_BELOW_HEAP] = r[CELL_ADDR] < tm::ADDR_HEAP_PTR ? 1 : 0;
    }
#pragma unroll
    for (u32 f = 0; f < MS_WORDS; f++)
        for (int off = warpSize / 2; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(r[f], off);
            r[f] = f == MS_BELOW_HEAP ? r[f] + other : r[f] | other;
        }
    if ((threadIdx.x & (warpSize - 1)) != 0) return;
#pragma unroll
    for (u32 f = 0; f < tm::MEM_CELL_WORDS; f++)
        if (r[f]) atomicOr(&stats[f], r[f]);
    if (r[MS_BELOW_HEAP]) atomicAdd(&stats[MS_BELOW_HEAP], r[MS_BELOW_HEAP]);
}
// the keys of one pass, in the order the passes before it left
__global__ __launch_bounds__(256) void mem_pass_key_kernel(const u64* __restrict__ canon, u32 n_cells, const u32* __restrict__ idx, u32 field,
                                                           u64* __restrict__ keys) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_cells) keys[i] = mem_sort_key(canon, n_cells, field, idx[i]);
}

// thread = row: row i < n_cells reads its cell and its predecessor's address and clock through the sorted index, all 29 columns are stored
// along rows, the prophet-region padding comes in the same pass.  The range-checked values go to their final places in rc_out (when given):
// the sort values of rows 1 .. n_cells - 1 without the first heap row behind a stack row (generation/memory.rs:77-86), then the region
// values of the heap rows.  Heap rows being a suffix, a sort value's place is i - 1, one less behind that boundary row, and a region
// value's is i - first_heap behind the sort values.
__global__ __launch_bounds__(256) void mem_fill_kernel(const u64* __restrict__ canon, const u32* __restrict__ idx, u32 n_cells, u32 first_heap,
                                                       u32 quirks, u32 n, u64* __restrict__ out, u64* __restrict__ rc_out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 prophet_base = gl_neg(0xFFFFFFFFull);                    // p - (2^32 - 1): where the prophet region starts
    const bool boundary_exists = first_heap > 0 && first_heap < n_cells;
    u64 addr = 0, clk = 0, op = 0, value = 0, is_write = 0, d_addr = 0, d_clk = 0, cond = 0, rc = 0;
    u32 sel = 0;
    bool rw = false, heap = false, prophet = false, unchanged = false, looking = false;
    if (i < n_cells) {
        const u32 r = idx[i];
        addr = canon[(size_t)CELL_ADDR * n_cells + r];
        clk = canon[(size_t)CELL_CLK * n_cells + r];
        op = canon[(size_t)CELL_OP * n_cells + r];
        value = canon[(size_t)CELL_VALUE * n_cells + r];
        is_write = canon[(size_t)CELL_IS_WRITE * n_cells + r];
        (void)mem_op_key(op, sel);
        rw = true;
        heap = i >= first_heap;
        if (heap) cond = gl_sub(prophet_base, addr);                   // 0 - (2^32 - 1) - address
        if (i > 0) {
            const u32 q = idx[i - 1];
            const u64 prev_addr = canon[(size_t)CELL_ADDR * n_cells + q], prev_clk = canon[(size_t)CELL_CLK * n_cells + q];
            d_addr = addr - prev_addr;
            if (i != first_heap) {                                     // the first heap row behind a stack row gets DIFF_ADDR and its inverse only
                unchanged = addr == prev_addr;
                d_clk = unchanged ? clk - prev_clk : 0;
                rc = unchanged ? d_clk : d_addr;
                looking = true;
            }
        }
        if (rc_out) {
            const u32 n_sort = n_cells - 1 - (boundary_exists ? 1u : 0u);
            if (looking) rc_out[i - 1 - ((boundary_exists && first_heap < i) ? 1u : 0u)] = rc;
            if (heap) rc_out[(size_t)n_sort + (i - first_heap)] = cond;
        }
    } else if (quirks) {                                               // n_cells == 0: generation/memory.rs:95-153 as it is, every row a prophet row
        addr = gl_add(prophet_base, i);
        is_write = 1; prophet = true;
        cond = rc = gl_neg(addr);
        if (i) { sel = tm::COL_MEM_S_PROPHET; d_addr = 1; }
    } else {
        const u32 start = n_cells ? n_cells : 1;                       // a table without cells: row 0 carries S_PROPHET and IS_WRITE only
        sel = tm::COL_MEM_S_PROPHET;
        is_write = 1;
        if (i >= start) {
            addr = gl_add(prophet_base, i - start);
            prophet = true;
            // the first padding row continues from the last live address, the others step by 1
            d_addr = i != start ? 1 : gl_sub(addr, n_cells ? canon[(size_t)CELL_ADDR * n_cells + idx[n_cells - 1]] : 0);
            cond = rc = gl_neg(addr);
        }
    }
    const u64 d_inv = d_addr <= 1 ? d_addr : gl_inv(d_addr);          // the inverse of 0 is 0
    auto put = [&](u32 c, u64 v) { out[(size_t)c * n + i] = v; };
    put(tm::COL_MEM_TX_IDX, 0);
    put(tm::COL_MEM_ENV_IDX, 0);
    put(tm::COL_MEM_IS_RW, rw ? 1 : 0);
    put(tm::COL_MEM_ADDR, addr);
    put(tm::COL_MEM_CLK, clk);
    put(tm::COL_MEM_OP, op);
#pragma unroll
    for (u32 c = tm::COL_MEM_S_MLOAD; c <= tm::COL_MEM_S_PROPHET; c++) put(c, c == sel ? 1 : 0);
    put(tm::COL_MEM_IS_WRITE, is_write);
    put(tm::COL_MEM_VALUE, value);
    put(tm::COL_MEM_DIFF_ADDR, d_addr);
    put(tm::COL_MEM_DIFF_ADDR_INV, d_inv);
    put(tm::COL_MEM_DIFF_CLK, d_clk);
    put(tm::COL_MEM_DIFF_ADDR_COND, cond);
    put(tm::COL_MEM_RW_ADDR_UNCHANGED, unchanged ? 1 : 0);
    put(tm::COL_MEM_REGION_PROPHET, prophet ? 1 : 0);
    put(tm::COL_MEM_REGION_HEAP, heap ? 1 : 0);
    put(tm::COL_MEM_RC_VALUE, rc);
    put(tm::COL_MEM_FILTER_LOOKING_RC, looking ? 1 : 0);
    put(tm::COL_MEM_FILTER_LOOKING_RC_COND, heap ? 1 : 0);
}
static_assert(tm::COL_MEM_S_PROPHET - tm::COL_MEM_S_MLOAD == 10 && tm::COL_MEM_S_MLOAD == tm::COL_MEM_OP + 1 && tm::COL_MEM_IS_WRITE == tm::COL_MEM_S_PROPHET + 1,
              "the eleven selector columns of the memory table lie between OP and IS_WRITE");

// ops: op0, op1 (n_ops each); rows n_ops .. n are generation/builtin.rs:240-245's padding
__global__ __launch_bounds__(256) void cmp_fill_kernel(const u64* __restrict__ ops, u32 n_ops, u32 n, u64* __restrict__ out,
                                                       u64* __restrict__ abs_diff_out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool live = i < n_ops;
    const u64 a = live ? gl_canon(ops[i]) : 1, b = live ? gl_canon(ops[(size_t)n_ops + i]) : 0;
    const u64 d = a >= b ? a - b : b - a;
    out[(size_t)tm::COL_CMP_OP0 * n + i] = a;
    out[(size_t)tm::COL_CMP_OP1 * n + i] = b;
    out[(size_t)tm::COL_CMP_GTE * n + i] = a >= b ? 1 : 0;
    out[(size_t)tm::COL_CMP_ABS_DIFF * n + i] = d;
    out[(size_t)tm::COL_CMP_ABS_DIFF_INV * n + i] = d <= 1 ? d : gl_inv(d);
    out[(size_t)tm::COL_CMP_FILTER_LOOKING_RC * n + i] = live ? 1 : 0;
    if (live && abs_diff_out) abs_diff_out[i] = d;
}

// ---- the tape, Poseidon-chunk and program-chunk tables (ola_generate_tape_trace / _poseidon_chunk_trace / _prog_chunk_trace;
// olavm_amd/air/miniexec.py tape_trace, poseidon_chunk_trace, prog_chunk_and_poseidon).  Narrow tables whose hashes are all output words
// of rows of the resident Poseidon table, so a row is a gather: thread = row, every column stored along rows.

// canonical tape addresses as sort keys, the identity index, and the OR of the keys (the bits the sort has to cover)
__global__ __launch_bounds__(256) void tape_key_kernel(const u64* __restrict__ cells, u32 n_cells, u64* __restrict__ keys, u32* __restrict__ idx,
                                                       unsigned long long* __restrict__ stats) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long r = 0;
    if (i < n_cells) {
        r = gl_canon(cells[i]);
        keys[i] = r;
        idx[i] = i;
    }
    for (int off = warpSize / 2; off > 0; off >>= 1) r |= __shfl_xor(r, off);
    if ((threadIdx.x & (warpSize - 1)) == 0 && r) atomicOr(stats, r);
}

// idx: the cells in row order (null: they are in it already).  Rows n_cells .. n repeat the last sorted cell as an unfiltered TLOAD;
// without cells every row is tracegen.tape_padding_trace's.
__global__ __launch_bounds__(256) void tape_fill_kernel(const u64* __restrict__ cells, const u32* __restrict__ idx, u32 n_cells, u32 n,
                                                        u64* __restrict__ out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool live = i < n_cells;
    u64 addr = 0, op = tx::OP_MASK_TLOAD, value = 0;
    if (n_cells) {
        const u32 at = live ? i : n_cells - 1;
        const u32 c = idx ? idx[at] : at;
        addr = gl_canon(cells[c]);
        if (live) op = gl_canon(cells[(size_t)n_cells + c]);
        value = gl_canon(cells[2 * (size_t)n_cells + c]);
    }
    out[(size_t)tx::COL_TAPE_TX_IDX * n + i] = 0;
    out[(size_t)tx::COL_TAPE_IS_INIT_SEG * n + i] = 0;
    out[(size_t)tx::COL_TAPE_OPCODE * n + i] = op;
    out[(size_t)tx::COL_TAPE_ADDR * n + i] = addr;
    out[(size_t)tx::COL_TAPE_VALUE * n + i] = value;
    out[(size_t)tx::COL_TAPE_FILTER_LOOKED * n + i] = live ? 1 : 0;
}
static_assert(tx::NUM_COL_TAPE == 6, "tape_fill_kernel writes six columns");

// a POSEIDON call record, column-major over the calls
enum : u32 { PCALL_CLK = 0, PCALL_SRC = 1, PCALL_LEN = 2, PCALL_DST = 3, PCALL_PSDN_ROW = 4 };

// rows per call (1 + len / 8) for the exclusive scan; entry n_calls is 0 so that the scan's last word is the total
__global__ __launch_bounds__(256) void pchunk_count_kernel(const u64* __restrict__ calls, u32 n_calls, u32* __restrict__ counts) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i > n_calls) return;
    counts[i] = i < n_calls ? 1u + (u32)(gl_canon(calls[(size_t)PCALL_LEN * n_calls + i]) >> 3) : 0u;
}

// the last c < n with a[c] <= v (a ascending, a[0] = 0)
__device__ __forceinline__ u32 last_at_or_below(const u32* __restrict__ a, u32 n, u32 v) {
    u32 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (a[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// at[c]: the header row of call c (the scan), rows = at[n_calls].  The host has checked every psdn_row + len / 8 against n_psdn; the
// row index is clamped all the same, so that records changed behind the host's back cannot read outside the table.
__global__ __launch_bounds__(256) void pchunk_fill_kernel(const u64* __restrict__ calls, u32 n_calls, const u32* __restrict__ at, u32 rows,
                                                          const u64* __restrict__ psdn, u32 n_psdn, u32 n, u64* __restrict__ out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u64 v[tx::NUM_POSEIDON_CHUNK_COLS];
#pragma unroll
    for (u32 c = 0; c < tx::NUM_POSEIDON_CHUNK_COLS; c++) v[c] = 0;
    if (i >= rows) {
        v[tx::COL_POSEIDON_CHUNK_IS_PADDING_LINE] = 1;
    } else {
        const u32 c = last_at_or_below(at, n_calls, i), j = i - at[c];
        const u64 src = gl_canon(calls[(size_t)PCALL_SRC * n_calls + c]), len = gl_canon(calls[(size_t)PCALL_LEN * n_calls + c]);
        v[tx::COL_POSEIDON_CHUNK_CLK] = gl_canon(calls[(size_t)PCALL_CLK * n_calls + c]);
        v[tx::COL_POSEIDON_CHUNK_OPCODE] = tx::OP_MASK_POSEIDON;
        v[tx::COL_POSEIDON_CHUNK_OP1] = len;
        v[tx::COL_POSEIDON_CHUNK_DST] = gl_canon(calls[(size_t)PCALL_DST * n_calls + c]);
        if (j == 0) {
            v[tx::COL_POSEIDON_CHUNK_OP0] = src;
            v[tx::COL_POSEIDON_CHUNK_FILTER_LOOKED_CPU] = 1;
        } else {
            const u64 first = gl_canon(calls[(size_t)PCALL_PSDN_ROW * n_calls + c]) + (j - 1);
            const size_t pr = first < n_psdn ? (size_t)first : n_psdn - 1;
            v[tx::COL_POSEIDON_CHUNK_OP0] = gl_add(src, 8ull * (j - 1));
            v[tx::COL_POSEIDON_CHUNK_ACC_CNT] = 8ull * j;
#pragma unroll
            for (u32 k = 0; k < 8; k++) v[tx::COL_POSEIDON_CHUNK_VALUE_RANGE_START + k] = gl_canon(psdn[(size_t)(tx::COL_POSEIDON_INPUT_RANGE_START + k) * n_psdn + pr]);
#pragma unroll
            for (u32 k = 0; k < 4; k++) v[tx::COL_POSEIDON_CHUNK_CAP_RANGE_START + k] = gl_canon(psdn[(size_t)(tx::COL_POSEIDON_INPUT_RANGE_START + 8 + k) * n_psdn + pr]);
#pragma unroll
            for (u32 k = 0; k < 12; k++) v[tx::COL_POSEIDON_CHUNK_HASH_RANGE_START + k] = gl_canon(psdn[(size_t)(tx::COL_POSEIDON_OUTPUT_RANGE_START + k) * n_psdn + pr]);
            v[tx::COL_POSEIDON_CHUNK_IS_EXT_LINE] = 1;
            v[tx::COL_POSEIDON_CHUNK_IS_RESULT_LINE] = 8ull * j == len ? 1 : 0;
#pragma unroll
            for (u32 k = 0; k < 8; k++) v[tx::COL_POSEIDON_CHUNK_FILTER_LOOKING_MEM_RANGE_START + k] = 1;
            v[tx::COL_POSEIDON_CHUNK_FILTER_LOOKING_POSEIDON] = 1;
        }
    }
#pragma unroll
    for (u32 c = 0; c < tx::NUM_POSEIDON_CHUNK_COLS; c++) out[(size_t)c * n + i] = v[c];
}

struct CodeAddr { u64 w[4]; };     // canonical, by value

// row i < n_chunks: listing words 8 i .. 8 i + 7 with row i of the Poseidon table, which hashed them
__global__ __launch_bounds__(256) void prog_chunk_fill_kernel(const u64* __restrict__ words, u32 n_chunks, CodeAddr code_addr, u32 result_line,
                                                              const u64* __restrict__ psdn, u32 n_psdn, u32 n, u64* __restrict__ out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u64 v[tx::NUM_PROG_CHUNK_COLS];
#pragma unroll
    for (u32 c = 0; c < tx::NUM_PROG_CHUNK_COLS; c++) v[c] = 0;
    if (i >= n_chunks) {
        v[tx::COL_PROG_CHUNK_IS_PADDING_LINE] = 1;
    } else {
#pragma unroll
        for (u32 k = 0; k < 4; k++) v[tx::COL_PROG_CHUNK_CODE_ADDR_RANGE_START + k] = code_addr.w[k];
        v[tx::COL_PROG_CHUNK_START_PC] = 8ull * i;
#pragma unroll
        for (u32 k = 0; k < 8; k++) v[tx::COL_PROG_CHUNK_INST_RANGE_START + k] = gl_canon(words[8 * (size_t)i + k]);
#pragma unroll
        for (u32 k = 0; k < 4; k++) v[tx::COL_PROG_CHUNK_CAP_RANGE_START + k] = gl_canon(psdn[(size_t)(tx::COL_POSEIDON_INPUT_RANGE_START + 8 + k) * n_psdn + i]);
#pragma unroll
        for (u32 k = 0; k < 12; k++) v[tx::COL_PROG_CHUNK_HASH_RANGE_START + k] = gl_canon(psdn[(size_t)(tx::COL_POSEIDON_OUTPUT_RANGE_START + k) * n_psdn + i]);
        v[tx::COL_PROG_CHUNK_IS_FIRST_LINE] = i == 0 ? 1 : 0;
        v[tx::COL_PROG_CHUNK_IS_RESULT_LINE] = (result_line && i == n_chunks - 1) ? 1 : 0;
#pragma unroll
        for (u32 k = 0; k < 8; k++) v[tx::COL_PROG_CHUNK_FILTER_LOOKING_PROG_RANGE_START + k] = 1;
    }
#pragma unroll
    for (u32 c = 0; c < tx::NUM_PROG_CHUNK_COLS; c++) out[(size_t)c * n + i] = v[c];
}

u32 log2_rows(u64 rows) {            // next power of two, at least 2 (the reference's ext_trace_len)
    u32 log_n = 1;
    while (((u64)1 << log_n) < rows) log_n++;
    return log_n;
}

}  // namespace

u32 rc_trace_log_n(u64 n_rows, u32 range_bits) { return log2_rows(std::max<u64>(n_rows, (u64)1 << range_bits)); }
u32 bitwise_trace_log_n(u64 n_ops, u32 limb_bits) { return log2_rows(std::max<u64>(n_ops, std::max<u64>((u64)1 << limb_bits, (u64)3 << (2 * limb_bits)))); }

void generate_rc_trace_dev(DeviceCtx* ctx, const u64* vals, const u64* filters, size_t n_rows, u32 range_bits, u64* out) {
    const u32 n = 1u << rc_trace_log_n(n_rows, range_bits);
    hipLaunchKernelGGL(rc_fill_kernel, dim3(blocks(n)), dim3(256), 0, ctx->stream, vals, filters, (u32)n_rows, range_bits, n, out);
    const u64* table = out + (size_t)tg::RC_FIX_RANGE_CHECK_U16 * n;
    const PermutedPair pairs[2] = {
        {out + (size_t)tg::RC_LIMB_LO * n, 0, out + (size_t)tg::RC_LIMB_LO_PERMUTED * n, out + (size_t)tg::RC_FIX_RANGE_CHECK_U16_PERMUTED_LO * n},
        {out + (size_t)tg::RC_LIMB_HI * n, 0, out + (size_t)tg::RC_LIMB_HI_PERMUTED * n, out + (size_t)tg::RC_FIX_RANGE_CHECK_U16_PERMUTED_HI * n}};
    permuted_cols_batch_dev(ctx, n, &table, 1, pairs, 2);
}

void generate_bitwise_trace_dev(DeviceCtx* ctx, const u64* ops, size_t n_ops, u32 limb_bits, u64 beta, bool reference_quirks, u64* out) {
    const u32 n = 1u << bitwise_trace_log_n(n_ops, limb_bits);
    hipLaunchKernelGGL(bitwise_fill_kernel, dim3(blocks(n)), dim3(256), 0, ctx->stream, ops, (u32)n_ops, limb_bits, gl_canon(beta),
                       reference_quirks ? 1u : 0u, n, out);
    auto col = [&](u32 c) { return out + (size_t)c * n; };
    const u64* tables[2] = {col(tg::BW_FIX_RANGE_CHECK_U8), col(tg::BW_FIX_COMPRESS)};
    PermutedPair pairs[16];
    // generation/builtin.rs:161-195: limb l of op0 / op1 / res against the range table (permuted table columns l, 4 + l, 8 + l), its
    // compress column against the compressed operation table
    const u32 limb_cols[3][2] = {{tg::BW_OP0_LIMBS_START, tg::BW_OP0_LIMBS_PERMUTED_START}, {tg::BW_OP1_LIMBS_START, tg::BW_OP1_LIMBS_PERMUTED_START},
                                 {tg::BW_RES_LIMBS_START, tg::BW_RES_LIMBS_PERMUTED_START}};
    u32 k = 0;
    for (u32 g = 0; g < 3; g++)
        for (u32 l = 0; l < 4; l++)
            pairs[k++] = {col(limb_cols[g][0] + l), 0, col(limb_cols[g][1] + l), col(tg::BW_FIX_RANGE_CHECK_U8_PERMUTED_START + 4 * g + l)};
    for (u32 l = 0; l < 4; l++)
        pairs[k++] = {col(tg::BW_COMPRESS_LIMBS_START + l), 1, col(tg::BW_COMPRESS_PERMUTED_START + l), col(tg::BW_FIX_COMPRESS_PERMUTED_START + l)};
    permuted_cols_batch_dev(ctx, n, tables, 2, pairs, 16);
}

void generate_prog_trace_dev(DeviceCtx* ctx, const u64* exec, const u64* prog, u32 log_n, u64 beta, u64* out) {
    const u32 n = 1u << log_n;
    hipLaunchKernelGGL(prog_fill_kernel, dim3(blocks(n)), dim3(256), 0, ctx->stream, exec, prog, n, gl_canon(beta), out);
    const u64* table = out + (size_t)tg::COL_PROG_COMP_PROG * n;
    const PermutedPair pair = {out + (size_t)tg::COL_PROG_EXEC_COMP_PROG * n, 0, out + (size_t)tg::COL_PROG_EXEC_COMP_PROG_PERM * n,
                               out + (size_t)tg::COL_PROG_COMP_PROG_PERM * n};
    permuted_cols_batch_dev(ctx, n, &table, 1, &pair, 1);
}

void generate_cpu_trace_dev(DeviceCtx* ctx, const u64* steps, size_t n_steps, u32 log_n, u64* out) {
    const u32 n = 1u << log_n;
    hipLaunchKernelGGL(cpu_fill_kernel, dim3(blocks(n)), dim3(256), 0, ctx->stream, steps, (u32)n_steps, n, out);
    HIP_CHECK(hipGetLastError());
}

bool generate_prog_trace_steps_dev(DeviceCtx* ctx, const u64* steps, size_t n_steps_, const u64* prog, u32 log_n, u64 beta, bool zero_filler,
                                   u64* out, u64* exec_rows) {
    const u32 n = 1u << log_n, n_steps = (u32)n_steps_;
    hipStream_t stream = ctx->stream;
    Scratch mem(ctx);
    u32 total = 0;
    u32* at = nullptr;
    if (n_steps) {
        u32* counts = mem.alloc<u32>((size_t)n_steps + 1);
        at = mem.alloc<u32>((size_t)n_steps + 1);
        hipLaunchKernelGGL(exec_count_kernel, dim3(blocks((size_t)n_steps + 1)), dim3(256), 0, stream, steps, n_steps, counts);
        HIP_CHECK(hipGetLastError());
        scan_exclusive(mem, stream, counts, at, 0u, (size_t)n_steps + 1, rocprim::plus<u32>());
        HIP_CHECK(hipMemcpyAsync(&total, at + n_steps, sizeof(u32), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    *exec_rows = total;
    if (total > n) return false;
    u64* exec = mem.alloc<u64>((size_t)7 * n);
    if (total) hipLaunchKernelGGL(exec_scatter_kernel, dim3(blocks(n_steps)), dim3(256), 0, stream, steps, n_steps, at, n, exec);
    if (total < n)
        hipLaunchKernelGGL(exec_filler_kernel, dim3(blocks(n - total)), dim3(256), 0, stream, total, (total && !zero_filler) ? 1u : 0u, n, exec);
    HIP_CHECK(hipGetLastError());          // scatter, filler
    generate_prog_trace_dev(ctx, exec, prog, log_n, beta, out);
    HIP_CHECK(hipGetLastError());
    return true;
}

u32 memory_trace_log_n(u64 n_cells) { return log2_rows(std::max<u64>(n_cells + 1, 8)); }
u32 cmp_trace_log_n(u64 n_ops) { return log2_rows(n_ops); }

void generate_memory_trace_dev(DeviceCtx* ctx, const u64* cells, size_t n_cells_, bool reference_quirks, u64* out, u64* rc_out, u64 counts[2]) {
    const u32 n = 1u << memory_trace_log_n(n_cells_), n_cells = (u32)n_cells_;
    hipStream_t stream = ctx->stream;
    counts[0] = counts[1] = 0;
    if (n_cells == 0) {
        hipLaunchKernelGGL(mem_fill_kernel, dim3(blocks(n)), dim3(256), 0, stream, nullptr, nullptr, 0u, 0u, reference_quirks ? 1u : 0u, n, out, nullptr);
        HIP_CHECK(hipGetLastError());
        return;
    }
    Scratch mem(ctx);
    u64* canon = mem.alloc<u64>((size_t)tm::MEM_CELL_WORDS * n_cells);
    u64* keys = mem.alloc<u64>(2 * (size_t)n_cells);                       // a pass's keys, and where the sort leaves them
    u32* idx[2] = {mem.alloc<u32>(n_cells), mem.alloc<u32>(n_cells)};
    unsigned long long* stats = mem.alloc<unsigned long long>(MS_WORDS);
    HIP_CHECK(hipMemsetAsync(stats, 0, MS_WORDS * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(mem_key_kernel, dim3(blocks(n_cells)), dim3(256), 0, stream, cells, n_cells, canon, idx[0], stats);
    HIP_CHECK(hipGetLastError());
    unsigned long long host_stats[MS_WORDS];
    HIP_CHECK(hipMemcpyAsync(host_stats, stats, sizeof(host_stats), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    // least significant key first; rocPRIM's radix sort is stable, so each pass keeps the order of the ones before it
    const u32 order[tm::MEM_CELL_WORDS] = {CELL_IS_WRITE, CELL_VALUE, CELL_OP, CELL_CLK, CELL_ADDR};
    // one temporary buffer for every pass: the largest any of their bit ranges asks for
    u32 bits[tm::MEM_CELL_WORDS];
    size_t tmp_bytes = 8;
    for (u32 field : order) {
        bits[field] = bit_length(host_stats[field]);
        size_t bytes = 0;
        if (bits[field]) HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, keys, keys + n_cells, idx[0], idx[1], n_cells, 0, bits[field], stream));
        tmp_bytes = std::max(tmp_bytes, bytes);
    }
    void* tmp = mem.alloc<unsigned char>(tmp_bytes);
    u32 cur = 0;
    for (u32 field : order) {
        if (bits[field] == 0) continue;                                     // every key of this field is 0
        hipLaunchKernelGGL(mem_pass_key_kernel, dim3(blocks(n_cells)), dim3(256), 0, stream, canon, n_cells, idx[cur], field, keys);
        HIP_CHECK(hipGetLastError());
        size_t bytes = tmp_bytes;
        HIP_CHECK(rocprim::radix_sort_pairs(tmp, bytes, keys, keys + n_cells, idx[cur], idx[cur ^ 1], n_cells, 0, bits[field], stream));
        cur ^= 1;
    }
    const u32 first_heap = (u32)host_stats[MS_BELOW_HEAP];
    hipLaunchKernelGGL(mem_fill_kernel, dim3(blocks(n)), dim3(256), 0, stream, canon, idx[cur], n_cells, first_heap, 0u, n, out, rc_out);
    HIP_CHECK(hipGetLastError());
    counts[0] = n_cells - 1 - ((first_heap > 0 && first_heap < n_cells) ? 1 : 0);
    counts[1] = n_cells - first_heap;
}

void generate_cmp_trace_dev(DeviceCtx* ctx, const u64* ops, size_t n_ops, u64* out, u64* abs_diff_out) {
    const u32 n = 1u << cmp_trace_log_n(n_ops);
    hipLaunchKernelGGL(cmp_fill_kernel, dim3(blocks(n)), dim3(256), 0, ctx->stream, ops, (u32)n_ops, n, out, abs_diff_out);
    HIP_CHECK(hipGetLastError());
}

u32 small_trace_log_n(u64 rows) { return log2_rows(std::max<u64>(rows, 8)); }

// One host wait: the OR of the canonical addresses sizes the sort's bit range (no pass at all when every address is 0).  rocPRIM's radix
// sort is stable and the index goes in ascending, so cells of one address keep execution order.
void generate_tape_trace_dev(DeviceCtx* ctx, const u64* cells, size_t n_cells_, u64* out) {
    const u32 n = 1u << small_trace_log_n(n_cells_), n_cells = (u32)n_cells_;
    hipStream_t stream = ctx->stream;
    if (n_cells == 0) {
        hipLaunchKernelGGL(tape_fill_kernel, dim3(blocks(n)), dim3(256), 0, stream, nullptr, nullptr, 0u, n, out);
        HIP_CHECK(hipGetLastError());
        return;
    }
    Scratch mem(ctx);
    u64* keys = mem.alloc<u64>(2 * (size_t)n_cells);
    u32* idx = mem.alloc<u32>(2 * (size_t)n_cells);
    unsigned long long* stats = mem.alloc<unsigned long long>(1);
    HIP_CHECK(hipMemsetAsync(stats, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(tape_key_kernel, dim3(blocks(n_cells)), dim3(256), 0, stream, cells, n_cells, keys, idx, stats);
    HIP_CHECK(hipGetLastError());
    unsigned long long host_stats = 0;
    HIP_CHECK(hipMemcpyAsync(&host_stats, stats, sizeof(host_stats), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const u32 bits = bit_length(host_stats);
    const u32* order = nullptr;
    if (bits) {
        size_t bytes = 0;
        HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, keys, keys + n_cells, idx, idx + n_cells, n_cells, 0, bits, stream));
        void* tmp = mem.alloc<unsigned char>(std::max<size_t>(bytes, 8));
        HIP_CHECK(rocprim::radix_sort_pairs(tmp, bytes, keys, keys + n_cells, idx, idx + n_cells, n_cells, 0, bits, stream));
        order = idx + n_cells;
    }
    hipLaunchKernelGGL(tape_fill_kernel, dim3(blocks(n)), dim3(256), 0, stream, cells, order, n_cells, n, out);
    HIP_CHECK(hipGetLastError());
}

// The caller's validation pass read the lengths and gave `rows`: count, exclusive scan, fill; one host wait, before the scan's work
// space goes back to the pool.
void generate_poseidon_chunk_trace_dev(DeviceCtx* ctx, const u64* calls, size_t n_calls_, u64 rows, const u64* psdn, u32 psdn_log_n, u64* out) {
    const u32 n = 1u << small_trace_log_n(rows), n_calls = (u32)n_calls_;
    hipStream_t stream = ctx->stream;
    Scratch mem(ctx);
    u32* at = nullptr;
    if (n_calls) {
        u32* counts = mem.alloc<u32>((size_t)n_calls + 1);
        at = mem.alloc<u32>((size_t)n_calls + 1);
        hipLaunchKernelGGL(pchunk_count_kernel, dim3(blocks((size_t)n_calls + 1)), dim3(256), 0, stream, calls, n_calls, counts);
        HIP_CHECK(hipGetLastError());
        scan_exclusive(mem, stream, counts, at, 0u, (size_t)n_calls + 1, rocprim::plus<u32>());
    }
    hipLaunchKernelGGL(pchunk_fill_kernel, dim3(blocks(n)), dim3(256), 0, stream, calls, n_calls, at, (u32)rows, psdn, 1u << psdn_log_n, n, out);
    HIP_CHECK(hipGetLastError());
}

// One launch, no host wait.
void generate_prog_chunk_trace_dev(DeviceCtx* ctx, const u64* words, size_t n_chunks, const u64 code_addr[4], bool result_line, const u64* psdn,
                                   u32 psdn_log_n, u64* out) {
    const u32 n = 1u << small_trace_log_n(n_chunks);
    CodeAddr ca;
    for (int k = 0; k < 4; k++) ca.w[k] = gl_canon(code_addr[k]);
    hipLaunchKernelGGL(prog_chunk_fill_kernel, dim3(blocks(n)), dim3(256), 0, ctx->stream, words, (u32)n_chunks, ca, result_line ? 1u : 0u, psdn,
                       1u << psdn_log_n, n, out);
    HIP_CHECK(hipGetLastError());
}

}  // namespace ola
