// Constraint check on the trace domain: which constraint of which table fails at which row (ola_check_constraints).
//
// Replaces (reference paths relative to circuits/src):
//   stark/prover.rs:711-819              check_constraints            -> check_constraints_kernel (one thread per trace row, the
//                                                                       table's constraint program interpreted as in quotient_kernel,
//                                                                       failures recorded per emit instead of folded by alphas)
//   stark/cross_table_lookup.rs:551-584  verify_cross_table_lookups   -> the last values of the CTL Z columns (ctl_factor_kernel +
//                                                                       product scan), compared on the host
//   test_utils.rs:152-195                the per-table recipe         -> check_constraints() below
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
// op: +8 VALU, +2 ds_bpermute, +1 load instruction): `false` is what the library runs.
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
    for (u32 k = 0; k < n_ops; k++) {
        const u64 w0 = D[ops_off + 2 * k], w1 = D[ops_off + 2 * k + 1];
        const int op = (int)(w0 & 0xff), kind = (int)((w0 >> 8) & 0xff);
        const u32 dst = (u32)((w0 >> 16) & 0xffff), a = (u32)((w0 >> 32) & 0xffff), b = (u32)((w0 >> 48) & 0xffff);
        u64 v;
        switch (op) {
            case AOP_LOCAL: v = gl_canon(trace[(size_t)a * n + row]); break;
            case AOP_NEXT:
                if (NEIGHBOUR) {
                    const u64 loc = trace[(size_t)a * n + row];
                    v = __shfl_down(loc, 1, QW);
                    if (lane == QW - 1 || nxt == 0) v = trace[(size_t)a * n + nxt];
                    v = gl_canon(v);
                } else {
                    v = gl_canon(trace[(size_t)a * n + nxt]);
                }
                break;
            case AOP_CONST: v = w1; break;
            case AOP_PARAM: v = D[params_off + a]; break;
            case AOP_ADD: v = gl_add(regs[a * QW + lane], regs[b * QW + lane]); break;
            case AOP_SUB: v = gl_sub(regs[a * QW + lane], regs[b * QW + lane]); break;
            case AOP_MUL: v = gl_mul(regs[a * QW + lane], regs[b * QW + lane]); break;
            case AOP_ISZERO: v = (regs[a * QW + lane] == 0) ? 1 : 0; break;
            default: {
                // where z_last and the Lagrange selectors are non-zero on H (constraint_consumer.rs:34-78)
                const bool applies = kind == AK_ALL || (kind == AK_TRANSITION && row != n - 1) || (kind == AK_FIRST && row == 0) ||
                                     (kind == AK_LAST && row == n - 1);
                const bool fail = active && applies && gl_canon(regs[a * QW + lane]) != 0;
                const unsigned long long m = __ballot(fail);
                if (m) {
                    const int first = __ffsll((long long)m) - 1;       // lanes are rows in order: the lowest failing lane is the smallest row
                    if (lane == first) {
                        atomicMin(&rec[2 * e], (unsigned long long)i);
                        atomicAdd(&rec[2 * e + 1], (unsigned long long)__popcll(m));
                    }
                }
                e++;
                continue;
            }
        }
        regs[dst * QW + lane] = v;
    }
}

// rows a lookup side selects: filter(row) == 1, as ctl_factor_kernel decides it (every row without a filter).  desc: push_ctl_desc.
__global__ __launch_bounds__(256) void ctl_selected_rows_kernel(const u64* __restrict__ trace, size_t n, const u64* __restrict__ desc,
                                                                unsigned long long* __restrict__ count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    u32 p = 2;
    const u32 ncol = (u32)desc[p++];
    for (u32 k = 0; k < ncol; k++) p += 2 * (u32)desc[p] + 2;
    bool sel = i < n;
    if (sel && desc[p++]) sel = dev_lincol_fast(desc, p, trace, n, i) == 1;
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
    // the kernel indexes the trace, its register file and the parameters with what the program says: hold it to the table's shape
    for (size_t k = 0; k + 1 < air.ops.size(); k += 2) {
        const u64 w0 = air.ops[k];
        const int op = (int)(w0 & 0xff);
        const u64 dst = (w0 >> 16) & 0xffff, a = (w0 >> 32) & 0xffff, b = (w0 >> 48) & 0xffff;
        bool ok = op <= AOP_ISZERO && (int)((w0 >> 8) & 0xff) <= AK_LAST;
        if (op != AOP_EMIT) ok = ok && dst < (u64)air.n_regs;
        if (op == AOP_LOCAL || op == AOP_NEXT) ok = ok && a < (u64)air.ncols;
        if (op == AOP_PARAM) ok = ok && a < (u64)air.n_params;
        if (op == AOP_ADD || op == AOP_SUB || op == AOP_MUL) ok = ok && a < (u64)air.n_regs && b < (u64)air.n_regs;
        if (op == AOP_EMIT || op == AOP_ISZERO) ok = ok && a < (u64)air.n_regs;
        if (!ok) throw OlaError(OLA_E_INVALID_ARG, "AIR-set blob: constraint program refers outside its table");
    }
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
    for (size_t i = 0; i + 1 < air.ops.size(); i += 2)
        if ((int)(air.ops[i] & 0xff) == AOP_EMIT) k.push_back((int)((air.ops[i] >> 8) & 0xff));
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
    if (nch != 2) throw OlaError(OLA_E_INVALID_ARG, "num_challenges must be 2");
    // challenges: a fresh transcript that has observed nothing (include/ola_gpu.h states the order)
    OlaChallenger ch;
    challenger_init(ch, (uint32_t)ctx->hasher);
    std::vector<GpChallenge> ctl_ch;
    for (int c = 0; c < nch; c++) {
        const GpChallenge drawn = get_gp(ch);
        ctl_ch.push_back(ctl_challenges ? GpChallenge{gl_canon(ctl_challenges[2 * c]), gl_canon(ctl_challenges[2 * c + 1])} : drawn);
    }
    std::vector<std::vector<std::vector<GpChallenge>>> perm_sets(nt);
    for (size_t t = 0; t < nt; t++)
        if (!set.tables[t].perm_pairs.empty())
            for (int i = 0; i < set.tables[t].permutation_batch_size(); i++) {
                std::vector<GpChallenge> s;
                for (int c = 0; c < nch; c++) s.push_back(get_gp(ch));
                perm_sets[t].push_back(s);
            }
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
    std::vector<u64> zero_params(64, 0);
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
        if (!params && air.n_params > 64) throw OlaError(OLA_E_INVALID_ARG, "params required");
        unsigned long long* d_rec = (unsigned long long*)tm.alloc(2 * std::max<size_t>(1, K));
        if (timing) HIP_CHECK(hipEventRecord(ev0, ctx->stream));
        launch_check_constraints(ctx, tm, air, dev[t].vals, n, params ? params + poffs[t] : zero_params.data(), K, d_rec);
        if (timing) HIP_CHECK(hipEventRecord(ev1, ctx->stream));
        HostSpan rec = tm.host(2 * std::max<size_t>(1, K));
        HIP_CHECK(hipMemcpyAsync(rec.data(), d_rec, 2 * std::max<size_t>(1, K) * 8, hipMemcpyDeviceToHost, ctx->stream));
        // ---- PERMUTATION: the running product of num / den over all rows is Z[n-1] num(n-1) / den(n-1) with Z[0] = 1 ----
        const int nperm = air.num_permutation_batches(nch), bs = air.permutation_batch_size();
        HostSpan perm_tot = tm.host(std::max(1, nperm));
        u64* tot = tm.alloc(pscan_tot_stride(n) * std::max<size_t>(1, jobs[t].size()));
        if (nperm) {
            u64* tmpcol = tm.alloc(n);
            const int total = (int)air.perm_pairs.size() * nch;
            int inst = 0;
            for (int b = 0; b < nperm; b++) {
                std::vector<u64> pd(1, 0);
                u64 cnt = 0;
                for (int i = 0; i < bs && inst < total; i++, inst++, cnt++) {
                    const auto& pair = air.perm_pairs[inst / nch];
                    const GpChallenge c = perm_sets[t][i][inst % nch];
                    pd.push_back(c.beta); pd.push_back(c.gamma); pd.push_back(pair.size());
                    for (auto& pr : pair) { pd.push_back(pr.first); pd.push_back(pr.second); }
                }
                pd[0] = cnt;
                u64* d_pd = tm.upload(pd);
                hipLaunchKernelGGL(perm_factor_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dev[t].vals, n, d_pd, tmpcol);
                product_scan_inclusive(ctx, tmpcol, n, tot);
                HIP_CHECK(hipMemcpyAsync(&perm_tot[b], tmpcol + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
            }
        }
        // ---- the table's CTL Z columns (cross_table_lookup.rs:224-311), of which verify_cross_table_lookups reads the last values ----
        const std::vector<CtlJob>& ctl = jobs[t];
        HostSpan zl = tm.host(std::max<size_t>(1, ctl.size()));
        if (!ctl.empty()) {
            std::vector<u64> ctl_desc, offs;
            for (auto& j : ctl) { offs.push_back(ctl_desc.size()); push_ctl_desc(ctl_desc, *j.twc, j.ch.beta, j.ch.gamma); }
            std::vector<u64> pairs;
            std::vector<char> taken(ctl.size(), 0);
            for (size_t a = 0; a < ctl.size(); a++) {
                if (taken[a]) continue;
                size_t b = a;
                for (size_t c = a + 1; c < ctl.size(); c++)
                    if (!taken[c] && ctl[c].twc == ctl[a].twc) { b = c; break; }
                taken[a] = taken[b] = 1;
                pairs.push_back(a); pairs.push_back(b);
            }
            const size_t n_offs = offs.size();
            offs.insert(offs.end(), pairs.begin(), pairs.end());
            u64* d_cd = tm.upload(ctl_desc);
            u64* d_offs = tm.upload(offs);
            unsigned* d_bad = (unsigned*)tm.alloc(1);      // a non-binary filter selects nothing here; the AIR section names the cell
            HIP_CHECK(hipMemsetAsync(d_bad, 0, 8, ctx->stream));
            u64* zc = tm.alloc(ctl.size() * n);
            hipLaunchKernelGGL(ctl_factor_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)(pairs.size() / 2)), dim3(256), 0, ctx->stream,
                               dev[t].vals, n, d_cd, d_offs, d_offs + n_offs, zc, d_bad);
            product_scan_inclusive(ctx, zc, n, tot, ctl.size());
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

}  // namespace ola
