// Constraint check on the trace domain: which constraint of which table fails at which row (ola_check_constraints).
//
// Replaces (reference paths relative to circuits/src):
//   stark/prover.rs:711-819              check_constraints            -> check_constraints_kernel (one thread per trace row, the
//                                                                       table's constraint program interpreted as in quotient_kernel,
//                                                                       failures recorded per emit instead of folded by alphas)
//   stark/cross_table_lookup.rs:551-584  verify_cross_table_lookups   -> the last values of the CTL Z columns (ctl_factor_kernel +
//                                                                       product scan), compared on the host
//   test_utils.rs:152-195                the per-table recipe         -> check_constraints() below
//   generation/ctl_test/ (one file per lookup: filter both sides, project the data columns, print two lists to diff;
//   debug_trace_print.rs:64-88)          -> check_lookup(): the exact multiset difference of a lookup's two sides (lk_*_kernel)
// Included by ola_gpu.hip after stark.hip (AIR-set parser, Z-column kernels, trace uploader).
#include <hip/hip_runtime.h>

namespace ola {

// Thread i <-> row i of the column-major trace (natural order), next row (i + 1) mod n; consecutive lanes take consecutive rows,
// so a column load of a wave is one 512-byte run.  rec[2e] = smallest failing row of emit e (starts at ~0), rec[2e + 1] = number
// of failing rows.  The lanes of a wave are joined by a ballot: a failing emit costs the wave two atomics, a row that satisfies
// everything none.
// NEIGHBOUR: a `next` cell is the neighbouring lane's `local` cell for 63 of 64 lanes.  true takes it from there (the local cell is
// loaded, moved down one lane through the LDS crossbar, and the wave's last lane reads its own next cell); false reads it from
// memory -- the same 512-byte run shifted by one word, whose lines the local load of that column has in cache.  An interpreter
// does not know whether the local cell is in a register already, so `true` saves no load and adds the move (static count per `next`
// op: +10 VALU, +2 ds_bpermute, +1 load instruction): `false` is what the library runs.
template <bool NEIGHBOUR>
__global__ __launch_bounds__(QW) void check_constraints_kernel(const u64* __restrict__ trace, size_t n, const u64* __restrict__ D,
                                                               unsigned long long* __restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u64* regs = reinterpret_cast<u64*>(smem_raw);
    const int lane = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * QW + lane;
    const bool active = i < n;
    const size_t row = active ? i : 0;
    const size_t nxt = (row + 1) & (n - 1);
    const u32 n_ops = (u32)D[0], ops_off = (u32)D[1], params_off = (u32)D[2];
    u32 e = 0;
    auto load = [&](u32 col, bool next) {
        if (!next) return gl_canon(trace[(size_t)col * n + row]);
        if (!NEIGHBOUR) return gl_canon(trace[(size_t)col * n + nxt]);
        u64 v = __shfl_down(trace[(size_t)col * n + row], 1, QW);
        if (lane == QW - 1 || nxt == 0) v = trace[(size_t)col * n + nxt];
        return gl_canon(v);
    };
    auto emit = [&](int kind, u64 v) {
        // where z_last and the Lagrange selectors are non-zero on H (constraint_consumer.rs:34-78).  | and & on purpose: the kind is
        // uniform and the row tests are loop invariants, so this is a few scalar selects; && and || became branches per emit
        // (profiles/airset_one_description_ab.txt)
        const bool applies = (kind == AK_ALL) | ((kind == AK_TRANSITION) & (row != n - 1)) | ((kind == AK_FIRST) & (row == 0)) |
                             ((kind == AK_LAST) & (row == n - 1));
        const bool fail = active & applies & (gl_canon(v) != 0);
        const unsigned long long m = __ballot(fail);
        if (m) {
            const int first = __ffsll((long long)m) - 1;       // lanes are rows in order: the lowest failing lane is the smallest row
            if (lane == first) {
                atomicMin(&rec[2 * e], (unsigned long long)i);
                atomicAdd(&rec[2 * e + 1], (unsigned long long)__popcll(m));
            }
        }
        e++;
    };
    air_interpret(D + ops_off, n_ops, D + params_off, regs, lane, load, emit);
}

// rows a lookup side selects: filter(row) == 1, as ctl_factor_kernel decides it (every row without a filter).  desc: push_ctl_desc.
__global__ __launch_bounds__(256) void ctl_selected_rows_kernel(const u64* __restrict__ trace, size_t n, const u64* __restrict__ desc,
                                                                unsigned long long* __restrict__ count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    u32 p = 2;
    const u32 ncol = (u32)desc[p++];
    for (u32 k = 0; k < ncol; k++) p += 2 * (u32)desc[p] + 2;
    bool sel = i < n;
    if (sel && desc[p++]) sel = dev_lincol(desc, p, trace, n, i) == 1;
    const unsigned long long m = __ballot(sel);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(count, (unsigned long long)__popcll(m));
}

// OLA_CHECK_NEXT=neighbour selects the NEIGHBOUR instantiation (the experiment of DESIGN.md, kept measurable: tools/bench_check_constraints.py)
static bool check_neighbour_variant() {
    const char* e = getenv("OLA_CHECK_NEXT");
    return e && !strcmp(e, "neighbour");
}

// the AIR section of one table whose values are on the device (canonical or not): K emits -> rec_host[2K]
static void launch_check_constraints(DeviceCtx* ctx, DevBuf& mem, const HTable& air, const u64* vals, size_t n, const u64* params,
                                     size_t n_emits, unsigned long long* d_rec) {
    std::vector<u64> desc(3, 0);
    desc[0] = air.ops.size() / 2;
    desc[1] = desc.size();
    desc.insert(desc.end(), air.ops.begin(), air.ops.end());
    desc[2] = desc.size();
    for (int i = 0; i < air.n_params; i++) desc.push_back(gl_canon(params[i]));
    u64* d_desc = mem.upload(desc);
    std::vector<u64> init(2 * std::max<size_t>(1, n_emits), 0);
    for (size_t e = 0; e < n_emits; e++) init[2 * e] = ~0ull;
    HostSpan h = mem.host(init.size());
    std::copy(init.begin(), init.end(), h.begin());
    HIP_CHECK(hipMemcpyAsync(d_rec, h.data(), init.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    const size_t lds = (size_t)air.n_regs * QW * 8;
    if (lds > 160 * 1024) throw OlaError(OLA_E_INVALID_ARG, "constraint program needs too many registers");
    const unsigned blocks = (unsigned)((n + QW - 1) / QW);
    if (check_neighbour_variant()) {
        if (lds > 48 * 1024) HIP_CHECK(hipFuncSetAttribute((const void*)check_constraints_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(check_constraints_kernel<true>, dim3(blocks), dim3(QW), lds, ctx->stream, vals, n, d_desc, d_rec);
    } else {
        if (lds > 48 * 1024) HIP_CHECK(hipFuncSetAttribute((const void*)check_constraints_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(check_constraints_kernel<false>, dim3(blocks), dim3(QW), lds, ctx->stream, vals, n, d_desc, d_rec);
    }
}

static std::vector<int> emit_kinds(const HTable& air) {
    std::vector<int> k;
    for (size_t i = 0; i + 1 < air.ops.size(); i += 2) {
        const AirOp o = air_op(air.ops[i], air.ops[i + 1]);
        if (o.op == AOP_EMIT) k.push_back(o.kind);
    }
    return k;
}

// test_utils.rs:152-195 for the tables of `mask`.  OLA_TIMING=1 prints the device time of each table's check kernel alone
// (tools/bench_check_constraints.py reads it).
void check_constraints(DeviceCtx* ctx, const OlaGpuConfig& cfg, const u64* airset, size_t airset_words, const TraceSource* traces,
                       const uint32_t* log_n, const u64* params, const u64* ctl_challenges, uint32_t mask,
                       std::vector<OlaConstraintFailure>& out) {
    const bool timing = ctx->timing;
    HAirSet set = parse_airset(airset, airset_words);
    const size_t nt = set.tables.size();
    const int nch = (int)cfg.num_challenges;
    // challenges: a fresh transcript that has observed nothing (include/ola_gpu.h states the order)
    OlaChallenger ch;
    challenger_init(ch, (uint32_t)ctx->hasher);
    std::vector<GpChallenge> ctl_ch;
    for (int c = 0; c < nch; c++) ctl_ch.push_back(get_gp(ch));
    if (ctl_challenges) ctl_ch = read_challenges(ctl_challenges, nch);
    std::vector<PermSets> perm_sets;
    for (const HTable& air : set.tables) perm_sets.push_back(draw_perm_sets(air, nch, ch));
    const std::vector<std::vector<CtlJob>> jobs = ctl_jobs(set, ctl_ch);
    std::vector<size_t> poffs(nt, 0);
    { size_t p = 0; for (size_t t = 0; t < nt; t++) { poffs[t] = p; p += (size_t)set.tables[t].n_params; } }

    DevBuf mem(ctx);
    std::vector<DevTable> dev(nt);
    const UploadStats saved_upload = ctx->upload;         // ola_gpu_upload_stats keeps describing the last whole proof
    TraceUploader up(ctx, nt);
    for (size_t t = 0; t < nt; t++) {
        dev[t].log_n = log_n[t];
        const size_t n_t = (size_t)1 << log_n[t];
        if (!(mask >> t & 1)) { up.add(t, traces[t], 0, nullptr, 0, n_t); continue; }
        dev[t].vals = mem.alloc((size_t)set.tables[t].ncols << log_n[t]);
        up.add(t, traces[t], 0, dev[t].vals, (uint32_t)set.tables[t].ncols, n_t);
    }
    up.start();
    std::vector<std::vector<u64>> z_last(nt);              // last value of each CTL Z column of a table, in ctl_jobs order
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct EvGuard { hipEvent_t& a; hipEvent_t& b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev_guard{ev0, ev1};
    if (timing) { HIP_CHECK(hipEventCreate(&ev0)); HIP_CHECK(hipEventCreate(&ev1)); }
    for (size_t t = 0; t < nt; t++) {
        if (!(mask >> t & 1)) continue;
        const HTable& air = set.tables[t];
        const size_t n = dev[t].n();
        const uint32_t w = (uint32_t)air.ncols;
        DevBuf tm(ctx);                                    // this table's scratch goes back to the pool before the next table
        up.wait(t, w);
        // the check kernel canonicalises on load; the Z builders read the cells several times: reduce what did not arrive reduced
        for (uint32_t c = 0; c < w;) {
            if (up.column_is_narrow(t, c)) { c++; continue; }
            uint32_t e = c + 1;
            while (e < w && !up.column_is_narrow(t, e)) e++;
            canonicalize(ctx, dev[t].vals + (size_t)c * n, (size_t)(e - c) * n);
            c = e;
        }
        // ---- AIR: the table's constraint program on H ----
        const std::vector<int> kinds = emit_kinds(air);
        const size_t K = kinds.size();
        const u64* table_params = params_or_zero(params, poffs[t], air);
        unsigned long long* d_rec = (unsigned long long*)tm.alloc(2 * std::max<size_t>(1, K));
        if (timing) HIP_CHECK(hipEventRecord(ev0, ctx->stream));
        launch_check_constraints(ctx, tm, air, dev[t].vals, n, table_params, K, d_rec);
        if (timing) HIP_CHECK(hipEventRecord(ev1, ctx->stream));
        HostSpan rec = tm.host(2 * std::max<size_t>(1, K));
        HIP_CHECK(hipMemcpyAsync(rec.data(), d_rec, 2 * std::max<size_t>(1, K) * 8, hipMemcpyDeviceToHost, ctx->stream));
        // ---- PERMUTATION: the running product of num / den over all rows is Z[n-1] num(n-1) / den(n-1) with Z[0] = 1 ----
        const PermDesc pd = build_perm_desc(air, perm_sets[t], nch);
        const int nperm = pd.nperm();
        HostSpan perm_tot = tm.host(std::max(1, nperm));
        u64* tot = tm.alloc(scan_tot_stride(n) * std::max<size_t>(1, jobs[t].size()));
        if (nperm) {
            u64* tmpcol = tm.alloc(n);
            u64* d_pd = tm.upload(pd.words);
            // a row with a zero denominator gets the factor 0 (perm_factor_kernel): the batch's product is then 0, not 1, and the
            // batch is reported below like any other failing permutation argument -- the kernel's own flag is not read here
            unsigned* d_zero_den = (unsigned*)tm.alloc(1);
            HIP_CHECK(hipMemsetAsync(d_zero_den, 0xFF, 8, ctx->stream));
            for (int b = 0; b < nperm; b++) {
                perm_z_batch(ctx, dev[t], d_pd + pd.batch_off[b], (unsigned)b, tmpcol, tot, d_zero_den);
                HIP_CHECK(hipMemcpyAsync(&perm_tot[b], tmpcol + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
            }
        }
        // ---- the table's CTL Z columns (cross_table_lookup.rs:224-311), of which verify_cross_table_lookups reads the last values ----
        const std::vector<CtlJob>& ctl = jobs[t];
        HostSpan zl = tm.host(std::max<size_t>(1, ctl.size()));
        if (!ctl.empty()) {
            unsigned* d_bad = (unsigned*)tm.alloc(1);      // a non-binary filter selects nothing here; the AIR section names the cell
            HIP_CHECK(hipMemsetAsync(d_bad, 0, 8, ctx->stream));
            u64* zc = tm.alloc(ctl.size() * n);
            ctl_z_columns(ctx, tm, dev[t], build_ctl_desc(ctl, nch), zc, tot, d_bad);
            for (size_t j = 0; j < ctl.size(); j++)
                HIP_CHECK(hipMemcpyAsync(&zl[j], zc + j * n + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (timing) {
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
            fprintf(stderr, "[ola-timing] check_constraints_kernel: table %zu, %zu rows x %d columns, %zu emits: %.4f ms = %.4f ns per row\n", t, n, air.ncols, K, ms, ms * 1e6 / (double)n);
        }
        for (size_t e = 0; e < K; e++)
            if (rec[2 * e + 1]) out.push_back({(uint32_t)t, OLA_CHECK_AIR, (uint32_t)e, (uint32_t)kinds[e], rec[2 * e], rec[2 * e + 1]});
        for (int b = 0; b < nperm; b++)
            if (perm_tot[b] != 1) out.push_back({(uint32_t)t, OLA_CHECK_PERMUTATION, (uint32_t)b, 0u, (uint64_t)(n - 1), 1});
        z_last[t].assign(zl.begin(), zl.begin() + ctl.size());
    }
    up.finish();
    ctx->upload = saved_upload;
    // ---- LOOKUP: verify_cross_table_lookups (cross_table_lookup.rs:551-584) ----
    // ctl_jobs order within a table: lookups in declaration order, challenge-minor, looking sides before the looked side
    std::vector<size_t> cursor(nt, 0);
    for (size_t li = 0; li < set.ctls.size(); li++) {
        const HCtl& ctl = set.ctls[li];
        bool all_in = (mask >> ctl.looked.table & 1) != 0;
        for (const HTwc& twc : ctl.looking) all_in = all_in && (mask >> twc.table & 1);
        for (int c = 0; c < nch; c++) {
            u64 looking = 1, looked = 0;
            for (const HTwc& twc : ctl.looking) { const size_t k = cursor[twc.table]++; if (all_in) looking = gl_mul(looking, z_last[twc.table][k]); }
            { const size_t k = cursor[ctl.looked.table]++; if (all_in) looked = z_last[ctl.looked.table][k]; }
            if (!all_in || looking == looked) continue;
            // the diagnosis: how many rows each side selects
            DevBuf tm(ctx);
            unsigned long long* d_cnt = (unsigned long long*)tm.alloc(2);
            HIP_CHECK(hipMemsetAsync(d_cnt, 0, 16, ctx->stream));
            auto count = [&](const HTwc& twc, unsigned long long* d_dst) {
                std::vector<u64> d;
                push_ctl_desc(d, twc, 0, 0);
                u64* d_d = tm.upload(d);
                const size_t n = dev[twc.table].n();
                hipLaunchKernelGGL(ctl_selected_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dev[twc.table].vals, n, d_d, d_dst);
            };
            for (const HTwc& twc : ctl.looking) count(twc, d_cnt);
            count(ctl.looked, d_cnt + 1);
            HostSpan h = tm.host(2);
            HIP_CHECK(hipMemcpyAsync(h.data(), d_cnt, 16, hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            out.push_back({(uint32_t)ctl.looked.table, OLA_CHECK_LOOKUP, (uint32_t)li, (uint32_t)c, h[0], h[1]});
        }
    }
    std::sort(out.begin(), out.end(), [](const OlaConstraintFailure& a, const OlaConstraintFailure& b) {
        if (a.table != b.table) return a.table < b.table;
        if (a.section != b.section) return a.section < b.section;
        if (a.index != b.index) return a.index < b.index;
        return a.kind < b.kind;
    });
}

// ------------------------------------------------------------------------------------------------ ola_check_lookup
// The exact multiset difference of the two sides of one cross-table lookup: what generation/ctl_test/*.rs prints for a person to
// diff (filter the looking and looked rows, project the data columns), computed next to the data.
//   1. count + scan + extract: every selected row of every side becomes a RECORD; records are numbered in (looking before looked,
//      entry position, row) order -- a deterministic compaction (ballot, wave prefix, block offsets from a scan; no atomic
//      cursor), because that order is the tie-break of the report.  A record's tuple is stored word-major (`width` planes of N
//      words), its origin word packs (side, entry, row) so that unsigned order is record order.
//   2. a stable LSD sort of the record numbers over the planes, last word first: full-tuple order, no hashing anywhere.
//   3. run boundaries from full-tuple comparison of neighbours; with the stable sort a run holds its looking records first, in
//      record order, then its looked records: counts and first carriers follow from one prefix sum of "is a looking record".
//   4. the mismatching runs, already in tuple order, are compacted into OlaLookupMismatch records on the device.
// Entry table `ent` (5 words per entry, the looked side last): trace pointer, rows, offset of its push_ctl_desc descriptor, first
// block of its rows in the block-count array, table index.
constexpr u32 LK_ENT_WORDS = 5;
constexpr u32 LK_ROW_BITS = 40, LK_ENTRY_BITS = 23;            // origin = side << 63 | entry << 40 | row
constexpr u32 LK_REC_WORDS = 5 + OLA_LOOKUP_MAX_VALUES;        // OlaLookupMismatch as 64-bit words
static_assert(sizeof(OlaLookupMismatch) == LK_REC_WORDS * 8, "OlaLookupMismatch is written word by word");

// filter(row) == 1 as ctl_factor_kernel decides it; leaves nothing behind but the verdict
__device__ __forceinline__ bool lk_selected(const u64* __restrict__ desc, const u64* __restrict__ trace, size_t n, size_t i) {
    u32 p = 2;
    const u32 ncol = (u32)desc[p++];
    for (u32 k = 0; k < ncol; k++) p += 2 * (u32)desc[p] + 2;
    if (!desc[p++]) return true;
    return dev_lincol(desc, p, trace, n, i) == 1;
}

// selected rows of a block -> *total, and this thread's rank among them (rows in order); every thread of the block calls it
__device__ __forceinline__ u32 lk_block_rank(bool sel, u32* __restrict__ wave_counts, u32* total) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(sel);
    if (lane == 0) wave_counts[wave] = (u32)__popcll(m);
    __syncthreads();
    u32 before = 0, all = 0;
    for (u32 w = 0; w < 4; w++) { const u32 c = wave_counts[w]; if (w < wave) before += c; all += c; }
    *total = all;
    return before + (u32)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(256) void lk_count_kernel(const u64* __restrict__ ent, const u64* __restrict__ desc_all, u32* __restrict__ block_counts) {
    __shared__ u32 wave_counts[4];
    const u64* __restrict__ e = ent + (size_t)blockIdx.y * LK_ENT_WORDS;
    const size_t n = (size_t)e[1], i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if ((size_t)blockIdx.x * 256 >= n) return;                 // the grid is as wide as the lookup's tallest table
    const bool sel = i < n && lk_selected(desc_all + e[2], reinterpret_cast<const u64*>(e[0]), n, i);
    u32 total;
    (void)lk_block_rank(sel, wave_counts, &total);
    if (threadIdx.x == 0) block_counts[e[3] + blockIdx.x] = total;
}

// thread = row.  block_offs: exclusive sum of the block counts; records beyond N cannot exist, the stores are bounded all the same.
__global__ __launch_bounds__(256) void lk_extract_kernel(const u64* __restrict__ ent, const u64* __restrict__ desc_all, const u32* __restrict__ block_offs,
                                                         u32 n_looking_entries, u32 N, u64* __restrict__ planes, u64* __restrict__ origin,
                                                         u32* __restrict__ ident) {
    __shared__ u32 wave_counts[4];
    const u64* __restrict__ e = ent + (size_t)blockIdx.y * LK_ENT_WORDS;
    const size_t n = (size_t)e[1], i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if ((size_t)blockIdx.x * 256 >= n) return;
    const u64* __restrict__ desc = desc_all + e[2];
    const u64* __restrict__ trace = reinterpret_cast<const u64*>(e[0]);
    const bool sel = i < n && lk_selected(desc, trace, n, i);
    u32 total;
    const u32 rank = lk_block_rank(sel, wave_counts, &total);
    if (!sel) return;
    const size_t pos = (size_t)block_offs[e[3] + blockIdx.x] + rank;
    if (pos >= N) return;
    u32 p = 2;
    const u32 ncol = (u32)desc[p++];
    for (u32 k = 0; k < ncol; k++) planes[(size_t)k * N + pos] = dev_lincol(desc, p, trace, n, i);
    const u64 looked = blockIdx.y >= n_looking_entries ? 1 : 0;
    origin[pos] = looked << 63 | (looked ? 0 : (u64)blockIdx.y) << LK_ROW_BITS | (u64)i;
    ident[pos] = (u32)pos;
}

__global__ __launch_bounds__(256) void lk_gather_kernel(const u64* __restrict__ plane, const u32* __restrict__ idx, u32 N, u64* __restrict__ keys) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const u32 r = idx[i];
    keys[i] = r < N ? plane[r] : 0;
}

// flags: two runs of N + 1 words (entry N of each is 0): "a run starts here" (the full tuple differs from the predecessor's), and
// "a looking record"; their exclusive sum `sc` then holds the number of runs at sc[N] and sc[N + 1].
__global__ __launch_bounds__(256) void lk_boundary_kernel(const u64* __restrict__ planes, const u32* __restrict__ idx, u32 N, u32 width, u32 n_looking,
                                                          u32* __restrict__ flags) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i > N) return;
    if (i == N) { flags[N] = 0; flags[(size_t)2 * N + 1] = 0; return; }
    const u32 r = idx[i];
    bool starts = i == 0;
    if (i > 0 && r < N) {
        const u32 q = idx[i - 1];
        if (q < N)
            for (u32 k = 0; k < width; k++) starts = starts || planes[(size_t)k * N + r] != planes[(size_t)k * N + q];
    }
    flags[i] = starts ? 1u : 0u;
    flags[(size_t)N + 1 + i] = r < n_looking ? 1u : 0u;
}

__global__ __launch_bounds__(256) void lk_run_start_kernel(const u32* __restrict__ flags, const u32* __restrict__ sc, u32 N, u32* __restrict__ run_start) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < N && flags[i] && sc[i] < N) run_start[sc[i]] = i;
}

// run r = sorted positions [s, e): its looking records are the first lk of them
__device__ __forceinline__ void lk_run(const u32* __restrict__ sc, const u32* __restrict__ run_start, u32 N, u32 R, u32 r, u32& s, u32& lk, u32& ld) {
    s = run_start[r];
    u32 e = r + 1 < R ? run_start[r + 1] : N;
    if (s > N) s = N;
    if (e > N || e < s) e = s;
    const u32* __restrict__ lsum = sc + N + 1;
    lk = lsum[e] - lsum[s];
    ld = (e - s) - lk;
}

// mism[r] = run r mismatches (N + 1 words, 0 from the number of runs on); totals[3] += |looking - looked|
__global__ __launch_bounds__(256) void lk_mismatch_kernel(const u32* __restrict__ sc, const u32* __restrict__ run_start, u32 N, u32* __restrict__ mism,
                                                          unsigned long long* __restrict__ totals) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    const u32 R = sc[N];
    unsigned long long diff = 0;
    if (r < R) {
        u32 s, lk, ld;
        lk_run(sc, run_start, N, R, r, s, lk, ld);
        diff = lk > ld ? lk - ld : ld - lk;
    }
    if (r <= N) mism[r] = diff ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) diff += __shfl_down(diff, off, 64);
    if ((threadIdx.x & 63) == 0 && diff) atomicAdd(&totals[3], diff);
}

// ent_tables[e]: table of looking entry e.  out: cap records of LK_REC_WORDS words.
__global__ __launch_bounds__(256) void lk_emit_kernel(const u32* __restrict__ sc, const u32* __restrict__ run_start, const u32* __restrict__ mism,
                                                      const u32* __restrict__ mpos, const u32* __restrict__ idx, const u64* __restrict__ planes,
                                                      const u64* __restrict__ origin, const u64* __restrict__ ent, u32 n_looking_entries, u32 N,
                                                      u32 width, u32 n_looking, u32 cap, u64* __restrict__ out,
                                                      unsigned long long* __restrict__ totals) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    const u32 R = sc[N];
    if (r == 0) { totals[0] = n_looking; totals[1] = N - n_looking; totals[2] = mpos[N]; }
    if (r >= R || !mism[r]) return;
    const u32 k = mpos[r];
    if (k >= cap) return;
    u32 s, lk, ld;
    lk_run(sc, run_start, N, R, r, s, lk, ld);
    if (s >= N) return;
    u64* __restrict__ o = out + (size_t)k * LK_REC_WORDS;
    o[0] = lk;
    o[1] = ld;
    u64 who = ~0ull, looking_row = ~0ull, looked_row = ~0ull;
    if (lk) {
        const u32 rec = idx[s];
        if (rec < N) {
            const u64 og = origin[rec];
            const u64 entry = (og >> LK_ROW_BITS) & ((1ull << LK_ENTRY_BITS) - 1);
            looking_row = og & ((1ull << LK_ROW_BITS) - 1);
            if (entry < n_looking_entries) who = entry | ent[entry * LK_ENT_WORDS + 4] << 32;     // looking_entry, looking_table (little-endian pair)
        }
    }
    if (ld && s + lk < N) {
        const u32 rec = idx[s + lk];
        if (rec < N) looked_row = origin[rec] & ((1ull << LK_ROW_BITS) - 1);
    }
    o[2] = who;
    o[3] = looking_row;
    o[4] = looked_row;
    const u32 first = idx[s];
    for (u32 w = 0; w < (u32)OLA_LOOKUP_MAX_VALUES; w++) o[5 + w] = (w < width && first < N) ? planes[(size_t)w * N + first] : 0;
}

struct LookupReport {
    uint64_t totals[4] = {0, 0, 0, 0};
    uint32_t width = 0;
    std::vector<OlaLookupMismatch> entries;                    // the first min(cap, totals[2])
};

// What can be said about `lookup` of a parsed set before a device is touched -> the tables it names (bit t = table t)
static uint32_t check_lookup_tables(const HAirSet& set, uint32_t lookup) {
    if (lookup >= set.ctls.size()) throw OlaError(OLA_E_INVALID_ARG, "lookup index beyond the AIR set's cross-table lookups");
    if (set.tables.size() > 32) throw OlaError(OLA_E_INVALID_ARG, "more than 32 tables");
    const HCtl& ctl = set.ctls[lookup];
    const size_t width = ctl.looked.columns.size();
    if (width == 0 || width > OLA_LOOKUP_MAX_VALUES)
        throw OlaError(OLA_E_INVALID_ARG, "the lookup has " + std::to_string(width) + " data columns: 1 .. OLA_LOOKUP_MAX_VALUES (" +
                                              std::to_string(OLA_LOOKUP_MAX_VALUES) + ") are supported");
    if (ctl.looking.size() >= ((size_t)1 << LK_ENTRY_BITS)) throw OlaError(OLA_E_INVALID_ARG, "too many looking entries");
    uint32_t mask = 0;
    auto side = [&](const HTwc& s) {
        if (s.columns.size() != width) throw OlaError(OLA_E_INVALID_ARG, "AIR-set blob: the sides of a lookup differ in width");
        mask |= 1u << s.table;
    };
    for (const HTwc& s : ctl.looking) side(s);
    side(ctl.looked);
    return mask;
}

// OLA_TIMING=1 prints the call's device time and its launch count (tools/bench_check_lookup.py reads the line)
void check_lookup(DeviceCtx* ctx, const u64* airset, size_t airset_words, const TraceSource* traces, const uint32_t* log_n, uint32_t lookup,
                  uint32_t cap, LookupReport& rep) {
    HAirSet set = parse_airset(airset, airset_words);
    const size_t nt = set.tables.size();
    const uint32_t mask = check_lookup_tables(set, lookup);
    const HCtl& ctl = set.ctls[lookup];
    const u32 width = (u32)ctl.looked.columns.size(), n_lk = (u32)ctl.looking.size();
    std::vector<const HTwc*> sides;
    for (const HTwc& t : ctl.looking) sides.push_back(&t);
    sides.push_back(&ctl.looked);
    size_t rows = 0;
    for (const HTwc* s : sides) {
        if (log_n[s->table] > 30) throw OlaError(OLA_E_INVALID_ARG, "table size out of range");
        rows += (size_t)1 << log_n[s->table];
    }
    // record numbers and the prefix sums are 32-bit
    if (rows >= ((size_t)1 << 31)) throw OlaError(OLA_E_INVALID_ARG, "check_lookup: more than 2^31 rows on the two sides together");
    rep.width = width;
    const bool timing = ctx->timing;
    u32 launches = 0, library_calls = 0;                       // kernels of this file / rocPRIM sorts and scans (several launches each)

    DevBuf mem(ctx);
    // ---- the tables the lookup names
    std::vector<DevTable> dev(nt);
    const UploadStats saved_upload = ctx->upload;              // ola_gpu_upload_stats keeps describing the last whole proof
    {
        TraceUploader up(ctx, nt);
        for (size_t t = 0; t < nt; t++) {
            if (!(mask >> t & 1)) { up.add(t, TraceSource{}, 0, nullptr, 0, 2); continue; }
            dev[t].log_n = log_n[t];
            dev[t].vals = mem.alloc((size_t)set.tables[t].ncols << log_n[t]);
            up.add(t, traces[t], 0, dev[t].vals, (uint32_t)set.tables[t].ncols, dev[t].n());
        }
        up.start();
        for (size_t t = 0; t < nt; t++)
            if (mask >> t & 1) up.wait(t, (uint32_t)set.tables[t].ncols);
        up.finish();
    }
    ctx->upload = saved_upload;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct EvGuard { hipEvent_t& a; hipEvent_t& b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev_guard{ev0, ev1};
    if (timing) { HIP_CHECK(hipEventCreate(&ev0)); HIP_CHECK(hipEventCreate(&ev1)); HIP_CHECK(hipEventRecord(ev0, ctx->stream)); }

    // ---- 1. count, scan
    std::vector<u64> desc, ent;
    size_t n_blocks = 0, widest = 0;
    for (const HTwc* s : sides) {
        const size_t n = dev[s->table].n(), b = (n + 255) / 256;
        ent.push_back((u64)(uintptr_t)dev[s->table].vals); ent.push_back(n); ent.push_back(desc.size()); ent.push_back(n_blocks); ent.push_back((u64)s->table);
        push_ctl_desc(desc, *s, 0, 0);
        n_blocks += b;
        widest = std::max(widest, b);
    }
    const u64 looked_block0 = ent[(size_t)n_lk * LK_ENT_WORDS + 3];
    u64* d_desc = mem.upload(desc);
    u64* d_ent = mem.upload(ent);
    u32* d_counts = (u32*)mem.alloc_bytes((n_blocks + 1) * 4);
    u32* d_offs = (u32*)mem.alloc_bytes((n_blocks + 1) * 4);
    HIP_CHECK(hipMemsetAsync(d_counts + n_blocks, 0, 4, ctx->stream));
    const dim3 grid((unsigned)widest, (unsigned)sides.size());
    hipLaunchKernelGGL(lk_count_kernel, grid, dim3(256), 0, ctx->stream, d_ent, d_desc, d_counts);
    launches++;
    ExclusiveSumU32(mem, n_blocks + 1).run(ctx->stream, d_counts, d_offs, n_blocks + 1);
    library_calls++;
    HostSpan h = mem.host(2);
    HIP_CHECK(hipMemcpyAsync(h.data(), d_offs + looked_block0, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(h.data() + 1, d_offs + n_blocks, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));              // the one synchronisation that sizes the second half
    const u64 n_looking64 = h[0] & 0xffffffffull, N64 = h[1] & 0xffffffffull;
    rep.totals[0] = n_looking64;
    rep.totals[1] = N64 - n_looking64;
    if (N64 == 0) return;
    const u32 N = (u32)N64, n_looking = (u32)n_looking64;

    // ---- extract
    u64* planes = mem.alloc((size_t)width * N);
    u64* origin = mem.alloc(N);
    u32* idx_a = (u32*)mem.alloc_bytes((size_t)N * 4);
    u32* idx_b = (u32*)mem.alloc_bytes((size_t)N * 4);
    hipLaunchKernelGGL(lk_extract_kernel, grid, dim3(256), 0, ctx->stream, d_ent, d_desc, d_offs, n_lk, N, planes, origin, idx_a);
    launches++;
    // ---- 2. the stable LSD sort: the last word first; the first pass sorts the records as they lie
    const unsigned nb = (unsigned)((N + 255) / 256), nb1 = (unsigned)(((size_t)N + 1 + 255) / 256);
    {
        u64* keys = mem.alloc(N);
        u64* keys_sorted = mem.alloc(N);
        SortPairsU64 sort(mem, N);
        for (u32 w = width; w-- > 0;) {
            const u64* in = planes + (size_t)w * N;
            if (w + 1 != width) {
                hipLaunchKernelGGL(lk_gather_kernel, dim3(nb), dim3(256), 0, ctx->stream, in, idx_a, N, keys);
                launches++;
                in = keys;
            }
            sort.run(ctx->stream, in, keys_sorted, idx_a, idx_b);
            library_calls++;
            std::swap(idx_a, idx_b);
        }
    }
    const u32* idx = idx_a;
    // ---- 3. runs
    u32* flags = (u32*)mem.alloc_bytes(2 * ((size_t)N + 1) * 4);
    u32* sc = (u32*)mem.alloc_bytes(2 * ((size_t)N + 1) * 4);
    u32* run_start = (u32*)mem.alloc_bytes((size_t)N * 4);
    u32* mism = (u32*)mem.alloc_bytes(((size_t)N + 1) * 4);
    u32* mpos = (u32*)mem.alloc_bytes(((size_t)N + 1) * 4);
    unsigned long long* d_totals = (unsigned long long*)mem.alloc(4);
    HIP_CHECK(hipMemsetAsync(d_totals, 0, 32, ctx->stream));
    ExclusiveSumU32 scan(mem, 2 * ((size_t)N + 1));                // both scans below, the second over half as many words
    hipLaunchKernelGGL(lk_boundary_kernel, dim3(nb1), dim3(256), 0, ctx->stream, planes, idx, N, width, n_looking, flags);
    scan.run(ctx->stream, flags, sc, 2 * ((size_t)N + 1));
    hipLaunchKernelGGL(lk_run_start_kernel, dim3(nb), dim3(256), 0, ctx->stream, flags, sc, N, run_start);
    hipLaunchKernelGGL(lk_mismatch_kernel, dim3(nb1), dim3(256), 0, ctx->stream, sc, run_start, N, mism, d_totals);
    scan.run(ctx->stream, mism, mpos, (size_t)N + 1);
    // ---- 4. the report
    const u32 cap_dev = std::min(cap, N);
    u64* d_out = mem.alloc(std::max<size_t>(1, (size_t)cap_dev * LK_REC_WORDS));
    hipLaunchKernelGGL(lk_emit_kernel, dim3(nb), dim3(256), 0, ctx->stream, sc, run_start, mism, mpos, idx, planes, origin, d_ent, n_lk, N, width,
                       n_looking, cap_dev, d_out, d_totals);
    launches += 4;
    library_calls += 2;
    HostSpan tot = mem.host(4);
    HIP_CHECK(hipMemcpyAsync(tot.data(), d_totals, 32, hipMemcpyDeviceToHost, ctx->stream));
    if (timing) HIP_CHECK(hipEventRecord(ev1, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));              // the synchronisation at the end
    HIP_CHECK(hipGetLastError());
    for (int k = 0; k < 4; k++) rep.totals[k] = tot[k];
    const size_t take = (size_t)std::min<u64>(cap_dev, tot[2]);
    if (take) {                                                // only a mismatching lookup pays for this copy
        rep.entries.resize(take);
        HIP_CHECK(hipMemcpy(rep.entries.data(), d_out, take * sizeof(OlaLookupMismatch), hipMemcpyDeviceToHost));
    }
    if (timing) {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
        fprintf(stderr, "[ola-timing] check_lookup: lookup %u, width %u, %u looking entries, %u selected rows: %u kernel launches + %u sort / scan calls, %.4f ms = %.4f ns per selected row\n",
                lookup, width, n_lk, N, launches, library_calls, ms, ms * 1e6 / (double)N);
    }
}

}  // namespace ola
