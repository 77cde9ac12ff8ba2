// Device-side `permuted_cols`: the permuted input / permuted table columns of the Halo2-style lookup
// argument that the range-check, bitwise and program tables carry (reference: circuits/src/stark/lookup.rs:68-132, called
// from generation/builtin.rs:121-200 and generation/prog.rs).  Own translation unit: rocPRIM (radix sort, scans) is needed
// here and in tablegen.hip only; what the two share of it is rocprim_ops.h.
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

#include "lookup.h"
#include "rocprim_ops.h"

namespace ola {

namespace {

// A batch of pairs that share their height runs steps 2 - 4 together: every kernel below has the pair index in grid.y, the
// scans run once over the concatenation of the pairs' flag arrays (a pair's own prefix is the difference to the value at its
// first entry), the events of all pairs sit back to back (pair p at ev_base[p]) with the pair index as the key of the two
// segmented scans and as the high bits of the level key, so that one stable sort orders every pair's events.  The table
// generators (tablegen.hip) fill a whole table and hand its lookup pairs to one such batch.
constexpr u32 kMaxBatch = 16;

struct PairArgs {                  // kernel argument (by value): pair p of the batch
    const u64* si[kMaxBatch];      // its inputs, canonical and sorted = permuted_inputs
    const u64* st[kMaxBatch];      // its table, canonical and sorted
    u64* pt[kMaxBatch];            // permuted_table
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

// One batch of at most kMaxBatch pairs of n rows.  tables[k]: the distinct table columns (any words), sorted once each;
// table_of[p]: which of them pair p looks into.  Enqueued on the context's stream; `mem` is released by the caller.
void permuted_batch(DeviceCtx* ctx, DevBuf& mem, u32 n, const u64* const* tables, u32 n_tables, const PermutedPair* pairs_in,
                    const u32* table_of, u32 pairs) {
    hipStream_t stream = ctx->stream;
    // ---- 1. canonical, sorted: every distinct table once, every pair's inputs into its permuted_inputs
    u64* canon = mem.alloc<u64>((size_t)std::max(pairs, n_tables) * n);
    u64* st = mem.alloc<u64>((size_t)n_tables * n);
    SortU64 sort(mem, n);
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
    ExclusiveSum<u32>(mem, n_flags).run(stream, flags, sc, n_flags);
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
    ScanInclusiveByKey<int> scan_events(mem, count);
    scan_events.run(stream, ev_pair, delta, s, rocprim::plus<int>());
    hipLaunchKernelGGL(clamp_min_kernel, dim3(blocks(count)), dim3(256), 0, stream, s, count, clamped);
    scan_events.run(stream, ev_pair, clamped, runmin, rocprim::minimum<int>());
    hipLaunchKernelGGL(level_kernel, dim3(blocks((size_t)count + 1)), dim3(256), 0, stream, delta, s, runmin, ev_pair, ev_base, count, level_bits,
                       key, ident, ev_flags);
    SortPairs<u32>(mem, count, level_bits + pair_bits).run(stream, key, key_sorted, ident, ev_sorted, level_bits + pair_bits);
    hipLaunchKernelGGL(pair_kernel, dim3(blocks((size_t)count + 1)), dim3(256), 0, stream, a, key_sorted, ev_sorted, count, level_bits, delta, src,
                       ev_flags + count + 1);
    ExclusiveSum<u32>(mem, 2 * ((size_t)count + 1)).run(stream, ev_flags, ev_sc, 2 * ((size_t)count + 1));
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
        DevBuf mem(ctx);
        permuted_batch(ctx, mem, n, tabs, n_tabs, pairs + first, table_of, count);
        HIP_CHECK(hipGetLastError());
    }
}

void permuted_cols_dev(DeviceCtx* ctx, const u64* inputs, const u64* table, size_t n, u64* permuted_inputs, u64* permuted_table) {
    const PermutedPair pair = {inputs, 0, permuted_inputs, permuted_table};
    permuted_cols_batch_dev(ctx, n, &table, 1, &pair, 1);
}

// ------------------------------------------------------------------------------------------------ sort / scan for check.hip
// the shape of rocprim_ops.h with external linkage: the pair sort over all 64 key bits, the 32-bit exclusive sum
SortPairsU64::SortPairsU64(DevBuf& mem, size_t n_) : n(n_) {
    HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, n, 0, 64, mem.ctx->stream));
    tmp = mem.alloc_bytes(bytes);
}
void SortPairsU64::run(hipStream_t stream, const u64* keys_in, u64* keys_out, const u32* payload_in, u32* payload_out) {
    HIP_CHECK(rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, payload_in, payload_out, n, 0, 64, stream));
}
ExclusiveSumU32::ExclusiveSumU32(DevBuf& mem, size_t max_n) {
    HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, (const u32*)nullptr, (u32*)nullptr, 0u, max_n, rocprim::plus<u32>(), mem.ctx->stream));
    tmp = mem.alloc_bytes(bytes);
}
void ExclusiveSumU32::run(hipStream_t stream, const u32* in, u32* out, size_t n) {
    HIP_CHECK(rocprim::exclusive_scan(tmp, bytes, in, out, 0u, n, rocprim::plus<u32>(), stream));
}

}  // namespace ola
