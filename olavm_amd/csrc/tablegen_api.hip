// The table generators' entry points (include/ola_gpu.h: the twelve ola_generate_*, ola_tables_*, ola_prove_from_records).  Part of
// ola_gpu.hip's translation unit, behind storage.hip (DevBuf, the storage tree and the Poseidon table); the kernels of the other nine
// tables are tablegen.hip, a unit of its own.
//
// Every generator is two functions that throw OlaError.  *_check does the argument checks that need no context and returns the table's
// height (a null input with a non-zero count is refused only when `fill` says that a table is wanted); *_fill takes that height and the
// caller's host or device pointers and leaves the finished table in `out`.  An ola_generate_* is check, *log_n_out, and -- when `out` is
// given -- fill on the context's device; tables_from_records runs the same pair once per table.

// device memory must be the context's GPU's: the kernels run there
static bool pointer_on_device(OlaCtx* ctx, const void* p) {
    int device = -1;
    if (!is_device_pointer(p, &device)) return false;
    require(device == ctx->dev.device, "a device buffer is not memory of the context's GPU");
    return true;
}
// input of `words` words wherever the caller has it -> device memory (a copy on the context's stream when it is host memory)
static const u64* table_input(OlaCtx* ctx, DevBuf& mem, const uint64_t* src, size_t words) {
    if (!src || words == 0 || pointer_on_device(ctx, src)) return (const u64*)src;
    u64* d = mem.alloc(words);
    HIP_CHECK(hipMemcpyAsync(d, src, words * 8, hipMemcpyHostToDevice, ctx->dev.stream));
    return d;
}
// the generated table: in place when `out` is device memory, else through a device buffer
struct TableOutput {
    OlaCtx* ctx;
    uint64_t* out;
    u64* dev;
    size_t words;
    TableOutput(OlaCtx* c, DevBuf& mem, uint64_t* out_, size_t words_) : ctx(c), out(out_), words(words_) {
        dev = pointer_on_device(ctx, out) ? (u64*)out : mem.alloc(words);
    }
    void finish() {
        if (dev != (u64*)out) HIP_CHECK(hipMemcpyAsync(out, dev, words * 8, hipMemcpyDeviceToHost, ctx->dev.stream));
        HIP_CHECK(hipStreamSynchronize(ctx->dev.stream));
    }
};

// ---- the range-check, bitwise and program tables from their primary columns
static uint32_t rc_check(const uint64_t* vals, size_t n_rows, uint32_t range_bits, bool fill) {
    require(range_bits >= 1 && range_bits <= 24, "range_bits out of range (1 .. 24)");
    require(n_rows <= ((size_t)1 << 28), "more than 2^28 rows");
    require(!fill || vals || n_rows == 0, "null pointer");
    return rc_trace_log_n(n_rows, range_bits);
}
static void rc_fill(OlaCtx* ctx, const uint64_t* vals, const uint64_t* filters, size_t n_rows, uint32_t range_bits, uint64_t* out, uint32_t log_n) {
    const size_t n = (size_t)1 << log_n;
    DevBuf mem(&ctx->dev);
    const u64* d_vals = table_input(ctx, mem, vals, n_rows);
    const u64* d_filters = table_input(ctx, mem, filters, 4 * n_rows);
    TableOutput t(ctx, mem, out, (size_t)olatg::COL_NUM_RC * n);
    generate_rc_trace_dev(&ctx->dev, d_vals, d_filters, n_rows, range_bits, t.dev);
    t.finish();
}
int32_t ola_generate_rc_trace(OlaCtx* ctx, const uint64_t* vals, const uint64_t* filters, size_t n_rows, uint32_t range_bits, uint64_t* out,
                              uint32_t* log_n_out) {
    OLA_TRY
    require(log_n_out, "null pointer");
    *log_n_out = rc_check(vals, n_rows, range_bits, out != nullptr);
    if (!out) return OLA_OK;       // the sizing call
    require_context(ctx);
    OLA_ON_DEVICE(ctx);
    rc_fill(ctx, vals, filters, n_rows, range_bits, out, *log_n_out);
    OLA_CATCH
}

static uint32_t bitwise_check(const uint64_t* ops, size_t n_ops, uint32_t limb_bits, uint32_t flags, bool fill) {
    require(limb_bits >= 1 && limb_bits <= 12, "limb_bits out of range (1 .. 12)");
    require((flags & ~(uint32_t)OLA_TABLEGEN_REFERENCE_QUIRKS) == 0, "unknown flag");
    require(n_ops <= ((size_t)1 << 26), "more than 2^26 operations");
    require(!fill || ops || n_ops == 0, "null pointer");
    return bitwise_trace_log_n(n_ops, limb_bits);
}
static void bitwise_fill(OlaCtx* ctx, const uint64_t* ops, size_t n_ops, uint32_t limb_bits, uint64_t beta, uint32_t flags, uint64_t* out,
                         uint32_t log_n) {
    const size_t n = (size_t)1 << log_n;
    DevBuf mem(&ctx->dev);
    const u64* d_ops = table_input(ctx, mem, ops, 5 * n_ops);
    TableOutput t(ctx, mem, out, (size_t)olatg::COL_NUM_BITWISE * n);
    generate_bitwise_trace_dev(&ctx->dev, d_ops, n_ops, limb_bits, beta, (flags & OLA_TABLEGEN_REFERENCE_QUIRKS) != 0, t.dev);
    t.finish();
}
int32_t ola_generate_bitwise_trace(OlaCtx* ctx, const uint64_t* ops, size_t n_ops, uint32_t limb_bits, uint64_t beta, uint32_t flags,
                                   uint64_t* out, uint32_t* log_n_out) {
    OLA_TRY
    require(log_n_out, "null pointer");
    *log_n_out = bitwise_check(ops, n_ops, limb_bits, flags, out != nullptr);
    if (!out) return OLA_OK;       // the sizing call
    require_context(ctx);
    OLA_ON_DEVICE(ctx);
    bitwise_fill(ctx, ops, n_ops, limb_bits, beta, flags, out, *log_n_out);
    OLA_CATCH
}

// the CPU table and the two program-table generators get their height from the caller: nothing to return
static void prog_check(const uint64_t* exec, const uint64_t* prog, uint32_t log_n) {
    require(exec && prog, "null pointer");
    require(log_n >= 1 && log_n <= 26, "log_n out of range (1 .. 26)");
}
static void prog_fill(OlaCtx* ctx, const uint64_t* exec, const uint64_t* prog, uint32_t log_n, uint64_t beta, uint64_t* out) {
    const size_t n = (size_t)1 << log_n;
    DevBuf mem(&ctx->dev);
    const u64* d_exec = table_input(ctx, mem, exec, 7 * n);
    const u64* d_prog = table_input(ctx, mem, prog, 7 * n);
    TableOutput t(ctx, mem, out, (size_t)olatg::NUM_PROG_COLS * n);
    generate_prog_trace_dev(&ctx->dev, d_exec, d_prog, log_n, beta, t.dev);
    t.finish();
}
int32_t ola_generate_prog_trace(OlaCtx* ctx, const uint64_t* exec, const uint64_t* prog, uint32_t log_n, uint64_t beta, uint64_t* out) {
    OLA_TRY
    require(out, "null pointer");
    prog_check(exec, prog, log_n);
    require_context(ctx);
    OLA_ON_DEVICE(ctx);
    prog_fill(ctx, exec, prog, log_n, beta, out);
    OLA_CATCH
}

// ---- the CPU table and the program table's executed side from step records
static_assert(OLA_CPU_STEP_WORDS == olatgc::STEP_WORDS, "include/ola_gpu.h and tablegen_cpu_columns.h disagree on the step record");
static void cpu_check(const uint64_t* steps, size_t n_steps, uint32_t log_n) {
    require(steps || n_steps == 0, "null pointer");
    require(log_n >= 1 && log_n <= 26, "log_n out of range (1 .. 26)");
    require(n_steps <= ((size_t)1 << log_n), "more steps than 2^log_n rows");
}
static void cpu_fill(OlaCtx* ctx, const uint64_t* steps, size_t n_steps, uint32_t log_n, uint64_t* out) {
    DevBuf mem(&ctx->dev);
    const u64* d_steps = table_input(ctx, mem, steps, (size_t)OLA_CPU_STEP_WORDS * n_steps);
    TableOutput t(ctx, mem, out, (size_t)olatgc::NUM_CPU_COLS << log_n);
    generate_cpu_trace_dev(&ctx->dev, d_steps, n_steps, log_n, t.dev);
    t.finish();
}
int32_t ola_generate_cpu_trace(OlaCtx* ctx, const uint64_t* steps, size_t n_steps, uint32_t log_n, uint64_t* out) {
    OLA_TRY
    require(out, "null pointer");
    cpu_check(steps, n_steps, log_n);
    require_context(ctx);
    OLA_ON_DEVICE(ctx);
    cpu_fill(ctx, steps, n_steps, log_n, out);
    OLA_CATCH
}

static void prog_steps_check(const uint64_t* steps, size_t n_steps, const uint64_t* prog, uint32_t log_n, uint32_t flags) {
    require(prog && (steps || n_steps == 0), "null pointer");
    require(log_n >= 1 && log_n <= 26, "log_n out of range (1 .. 26)");
    require((flags & ~(uint32_t)OLA_TABLEGEN_ZERO_FILLER) == 0, "unknown flag");
    require(n_steps < ((size_t)1 << 31), "2^31 steps or more");
}
static void prog_steps_fill(OlaCtx* ctx, const uint64_t* steps, size_t n_steps, const uint64_t* prog, uint32_t log_n, uint64_t beta, uint32_t flags,
                            uint64_t* out, uint64_t* exec_rows_out) {
    const size_t n = (size_t)1 << log_n;
    DevBuf mem(&ctx->dev);
    const u64* d_steps = table_input(ctx, mem, steps, (size_t)OLA_CPU_STEP_WORDS * n_steps);
    const u64* d_prog = table_input(ctx, mem, prog, 7 * n);
    TableOutput t(ctx, mem, out, (size_t)olatg::NUM_PROG_COLS * n);
    u64 exec_rows = 0;
    const bool fits = generate_prog_trace_steps_dev(&ctx->dev, d_steps, n_steps, d_prog, log_n, beta, (flags & OLA_TABLEGEN_ZERO_FILLER) != 0, t.dev,
                                                    &exec_rows);
    *exec_rows_out = exec_rows;
    require(fits, "the steps give more executed rows than 2^log_n (the count is in *exec_rows_out)");
    t.finish();
}
int32_t ola_generate_prog_trace_steps(OlaCtx* ctx, const uint64_t* steps, size_t n_steps, const uint64_t* prog, uint32_t log_n, uint64_t beta,
                                      uint32_t flags, uint64_t* out, uint64_t* exec_rows_out) {
    OLA_TRY
    require(out && exec_rows_out, "null pointer");
    prog_steps_check(steps, n_steps, prog, log_n, flags);
    require_context(ctx);
    OLA_ON_DEVICE(ctx);
    prog_steps_fill(ctx, steps, n_steps, prog, log_n, beta, flags, out, exec_rows_out);
    OLA_CATCH
}

// ---- the memory table from raw cells and the comparison table from operand pairs
static_assert(OLA_MEM_CELL_WORDS == olatgm::MEM_CELL_WORDS, "include/ola_gpu.h and tablegen_mem_columns.h disagree on the memory cell");
static uint32_t memory_check(const uint64_t* cells, size_t n_cells, uint32_t flags, bool fill) {
    require((flags & ~(uint32_t)OLA_TABLEGEN_REFERENCE_QUIRKS) == 0, "unknown flag");
    require(n_cells < ((size_t)1 << 31), "2^31 cells or more");
    require(!fill || cells || n_cells == 0, "null pointer");
    return memory_trace_log_n(n_cells);
}
static void memory_fill(OlaCtx* ctx, const uint64_t* cells, size_t n_cells, uint32_t flags, uint64_t* out, uint32_t log_n, uint64_t* rc_out,
                        uint64_t rc_counts[2]) {
    DevBuf mem(&ctx->dev);
    const u64* d_cells = table_input(ctx, mem, cells, (size_t)OLA_MEM_CELL_WORDS * n_cells);
    TableOutput t(ctx, mem, out, (size_t)olatgm::NUM_MEM_COLS << log_n);
    // the value lists: in place when rc_out is device memory, else through a device buffer; only the words the counts name are written
    const bool rc_on_device = rc_out && n_cells && pointer_on_device(ctx, rc_out);
    u64* d_rc = !rc_out || !n_cells ? nullptr : rc_on_device ? (u64*)rc_out : mem.alloc(2 * n_cells);
    u64 counts[2] = {0, 0};
    generate_memory_trace_dev(&ctx->dev, d_cells, n_cells, (flags & OLA_TABLEGEN_REFERENCE_QUIRKS) != 0, t.dev, d_rc, counts);
    if (d_rc && !rc_on_device && counts[0] + counts[1])
        HIP_CHECK(hipMemcpyAsync(rc_out, d_rc, (counts[0] + counts[1]) * 8, hipMemcpyDeviceToHost, ctx->dev.stream));
    t.finish();
    rc_counts[0] = counts[0]; rc_counts[1] = counts[1];
}
int32_t ola_generate_memory_trace(OlaCtx* ctx, const uint64_t* cells, size_t n_cells, uint32_t flags, uint64_t* out, uint32_t* log_n_out,
                                  uint64_t* rc_out, uint64_t rc_counts[2]) {
    OLA_TRY
    require(log_n_out && rc_counts, "null pointer");
    *log_n_out = memory_check(cells, n_cells, flags, out != nullptr);
    if (!out) return OLA_OK;       // the sizing call
    require_context(ctx);
    OLA_ON_DEVICE(ctx);
    memory_fill(ctx, cells, n_cells, flags, out, *log_n_out, rc_out, rc_counts);
    OLA_CATCH
}

static uint32_t cmp_check(const uint64_t* ops, size_t n_ops, bool fill) {
    require(n_ops < ((size_t)1 << 31), "2^31 operand pairs or more");
    require(!fill || ops || n_ops == 0, "null pointer");
    return cmp_trace_log_n(n_ops);
}
static void cmp_fill(OlaCtx* ctx, const uint64_t* ops, size_t n_ops, uint64_t* out, uint32_t log_n, uint64_t* abs_diff_out) {
    DevBuf mem(&ctx->dev);
    const u64* d_ops = table_input(ctx, mem, ops, 2 * n_ops);
    TableOutput t(ctx, mem, out, (size_t)olatgm::COL_NUM_CMP << log_n);
    const bool diff_on_device = abs_diff_out && n_ops && pointer_on_device(ctx, abs_diff_out);
    u64* d_diff = !abs_diff_out || !n_ops ? nullptr : diff_on_device ? (u64*)abs_diff_out : mem.alloc(n_ops);
    generate_cmp_trace_dev(&ctx->dev, d_ops, n_ops, t.dev, d_diff);
    if (d_diff && !diff_on_device) HIP_CHECK(hipMemcpyAsync(abs_diff_out, d_diff, n_ops * 8, hipMemcpyDeviceToHost, ctx->dev.stream));
    t.finish();
}
int32_t ola_generate_cmp_trace(OlaCtx* ctx, const uint64_t* ops, size_t n_ops, uint64_t* out, uint32_t* log_n_out, uint64_t* abs_diff_out) {
    OLA_TRY
    require(log_n_out, "null pointer");
    *log_n_out = cmp_check(ops, n_ops, out != nullptr);
    if (!out) return OLA_OK;       // the sizing call
    require_context(ctx);
    OLA_ON_DEVICE(ctx);
    cmp_fill(ctx, ops, n_ops, out, *log_n_out, abs_diff_out);
    OLA_CATCH
}

// words [first, first + count) of a caller's buffer, wherever it lives, into host memory (the validation passes, which run
// before there has to be a context)
static void fetch_words(OlaCtx* ctx, u64* dst, const uint64_t* src, size_t count) {
    if (count == 0) return;
    const bool dev = ctx ? pointer_on_device(ctx, src) : is_device_pointer(src);
    if (dev) HIP_CHECK(hipMemcpy(dst, src, count * 8, hipMemcpyDeviceToHost));
    else memcpy(dst, src, count * 8);
}

// ---- the storage-access table and the Poseidon table (storage.hip)
static_assert(OLA_STORAGE_ACCESS_WORDS == olatgs::STORAGE_ACCESS_WORDS, "include/ola_gpu.h and tablegen_storage_columns.h disagree on the access record");
// the validation pass: flags and Poseidon rows of every record, read on the host before any work.  m = the accesses with rows; meta is
// storage.hip's [4][n]
struct StorageChecked { uint32_t log_n; size_t m; std::vector<u64> meta; };
static StorageChecked storage_check(OlaCtx* ctx, const uint64_t* accesses, size_t n, const uint64_t* siblings, const uint64_t* psdn_inputs,
                                    const uint64_t* psdn_filters, size_t psdn_stride, bool fill) {
    require(n < ((size_t)1 << 23), "2^23 accesses or more");
    require((psdn_inputs == nullptr) == (psdn_filters == nullptr), "psdn_inputs and psdn_filters go together");
    require(accesses || n == 0 || !fill, "null pointer");
    StorageChecked c = {0, 0, std::vector<u64>(4 * n + 1, 0)};
    std::vector<u64>& meta = c.meta;
    size_t m = 0;
    if (accesses && n) {
        fetch_words(ctx, meta.data() + n, accesses + 12 * n, 2 * n);
        for (size_t a = 0; a < n; a++) {
            const u64 flags = gl_canon(meta[n + a]), row = gl_canon(meta[2 * n + a]);
            require((flags & ~(u64)(OLA_STORAGE_WRITE | OLA_STORAGE_FOR_PROG | OLA_STORAGE_SILENT)) == 0, "unknown flag in an access record");
            const bool silent = flags & OLA_STORAGE_SILENT;
            require(!(silent && siblings), "OLA_STORAGE_SILENT in a batch with the caller's siblings");
            if (psdn_inputs && !silent)
                require(row < psdn_stride && psdn_stride - row >= 2 * olatgs::STORAGE_DEPTH, "psdn_row + 512 is beyond psdn_stride");
            meta[a] = silent ? ~0ull : m;
            meta[n + a] = flags; meta[2 * n + a] = row;
            if (!silent) meta[3 * n + m++] = a;
        }
    } else {
        m = n;       // a sizing call without records: no access is taken to be silent
    }
    c.m = m;
    c.log_n = storage_trace_log_n(m);
    return c;
}
static void storage_fill(OlaCtx* ctx, const uint64_t* accesses, size_t n, const uint64_t* siblings, const StorageChecked& c, uint64_t* out,
                         uint64_t* psdn_inputs, uint64_t* psdn_filters, size_t psdn_stride, uint64_t roots_out[8]) {
    const size_t m = c.m, n_out = (size_t)1 << c.log_n;
    DevBuf mem(&ctx->dev);
    const u64* d_acc = table_input(ctx, mem, accesses, (size_t)OLA_STORAGE_ACCESS_WORDS * n);
    const u64* d_sib = n ? table_input(ctx, mem, siblings, (size_t)4 * olatgs::STORAGE_DEPTH * n) : nullptr;
    TableOutput t(ctx, mem, out, (size_t)olatgs::NUM_COL_ST * n_out);
    // the Poseidon inputs: rows the call does not own must survive, so a host buffer travels to the device and back whole
    const bool psdn = psdn_inputs && m;
    const bool psdn_on_device = psdn && pointer_on_device(ctx, psdn_inputs);
    if (psdn) require(pointer_on_device(ctx, psdn_filters) == psdn_on_device, "psdn_inputs and psdn_filters: one in host memory, one on the device");
    u64* d_pin = !psdn ? nullptr : psdn_on_device ? (u64*)psdn_inputs : mem.alloc(12 * psdn_stride);
    u64* d_pf = !psdn ? nullptr : psdn_on_device ? (u64*)psdn_filters : mem.alloc(4 * psdn_stride);
    if (psdn && !psdn_on_device) {
        HIP_CHECK(hipMemcpyAsync(d_pin, psdn_inputs, 12 * psdn_stride * 8, hipMemcpyHostToDevice, ctx->dev.stream));
        HIP_CHECK(hipMemcpyAsync(d_pf, psdn_filters, 4 * psdn_stride * 8, hipMemcpyHostToDevice, ctx->dev.stream));
    }
    const bool roots_on_device = roots_out && pointer_on_device(ctx, roots_out);
    u64* d_roots = !roots_out ? nullptr : roots_on_device ? (u64*)roots_out : mem.alloc(8);
    generate_storage_trace_dev(&ctx->dev, mem, d_acc, n, c.meta.data(), m, d_sib, t.dev, d_pin, d_pf, psdn_stride, d_roots);
    if (psdn && !psdn_on_device) {
        HIP_CHECK(hipMemcpyAsync(psdn_inputs, d_pin, 12 * psdn_stride * 8, hipMemcpyDeviceToHost, ctx->dev.stream));
        HIP_CHECK(hipMemcpyAsync(psdn_filters, d_pf, 4 * psdn_stride * 8, hipMemcpyDeviceToHost, ctx->dev.stream));
    }
    if (d_roots && !roots_on_device) HIP_CHECK(hipMemcpyAsync(roots_out, d_roots, 64, hipMemcpyDeviceToHost, ctx->dev.stream));
    t.finish();
}
// the check reads the records, which may be device memory: the context's device, when there is one, is current before it
int32_t ola_generate_storage_trace(OlaCtx* ctx, const uint64_t* accesses, size_t n_access, const uint64_t* siblings, uint64_t* out,
                                   uint32_t* log_n_out, uint64_t* psdn_inputs, uint64_t* psdn_filters, size_t psdn_stride, uint64_t roots_out[8]) {
    OLA_TRY
    require(log_n_out, "null pointer");
    OLA_ON_DEVICE(ctx);
    const StorageChecked c = storage_check(ctx, accesses, n_access, siblings, psdn_inputs, psdn_filters, psdn_stride, out != nullptr);
    *log_n_out = c.log_n;
    if (!out) return OLA_OK;       // the sizing call
    require_context(ctx);
    storage_fill(ctx, accesses, n_access, siblings, c, out, psdn_inputs, psdn_filters, psdn_stride, roots_out);
    OLA_CATCH
}

static uint32_t poseidon_table_check(const uint64_t* inputs, size_t n_rows, size_t stride, bool fill) {
    require(n_rows <= ((size_t)1 << 26), "more than 2^26 rows");
    require(stride >= n_rows, "stride is smaller than n_rows");
    require(!fill || inputs || n_rows == 0, "null pointer");
    uint32_t log_n = 3;
    while (((size_t)1 << log_n) < n_rows) log_n++;
    return log_n;
}
static void poseidon_table_fill(OlaCtx* ctx, const uint64_t* inputs, const uint64_t* filters, size_t n_rows, size_t stride, uint64_t* out,
                                uint32_t log_n) {
    DevBuf mem(&ctx->dev);
    const u64* d_in = n_rows ? table_input(ctx, mem, inputs, 12 * stride) : nullptr;
    const u64* d_f = n_rows ? table_input(ctx, mem, filters, 4 * stride) : nullptr;
    TableOutput t(ctx, mem, out, (size_t)olatgs::NUM_POSEIDON_COLS << log_n);
    generate_poseidon_table_dev(&ctx->dev, d_in, d_f, n_rows, stride, (size_t)1 << log_n, t.dev);
    t.finish();
}
int32_t ola_generate_poseidon_table(OlaCtx* ctx, const uint64_t* inputs, const uint64_t* filters, size_t n_rows, size_t stride, uint64_t* out,
                                    uint32_t* log_n_out) {
    OLA_TRY
    require(log_n_out, "null pointer");
    *log_n_out = poseidon_table_check(inputs, n_rows, stride, out != nullptr);
    if (!out) return OLA_OK;       // the sizing call
    require_context(ctx);
    OLA_ON_DEVICE(ctx);
    poseidon_table_fill(ctx, inputs, filters, n_rows, stride, out, *log_n_out);
    OLA_CATCH
}

// ---- the tape, Poseidon-chunk and program-chunk tables
static_assert(OLA_TAPE_CELL_WORDS == olatgx::TAPE_CELL_WORDS && OLA_POSEIDON_CALL_WORDS == olatgx::POSEIDON_CALL_WORDS,
              "include/ola_gpu.h and tablegen_small_columns.h disagree on the tape cell or the POSEIDON call record");
static uint32_t tape_check(const uint64_t* cells, size_t n_cells, bool fill) {
    require(n_cells < ((size_t)1 << 31), "2^31 cells or more");
    require(!fill || cells || n_cells == 0, "null pointer");
    return small_trace_log_n(n_cells);
}
static void tape_fill(OlaCtx* ctx, const uint64_t* cells, size_t n_cells, uint64_t* out, uint32_t log_n) {
    DevBuf mem(&ctx->dev);
    const u64* d_cells = table_input(ctx, mem, cells, (size_t)OLA_TAPE_CELL_WORDS * n_cells);
    TableOutput t(ctx, mem, out, (size_t)olatgx::NUM_COL_TAPE << log_n);
    generate_tape_trace_dev(&ctx->dev, d_cells, n_cells, t.dev);
    t.finish();
}
int32_t ola_generate_tape_trace(OlaCtx* ctx, const uint64_t* cells, size_t n_cells, uint64_t* out, uint32_t* log_n_out) {
    OLA_TRY
    require(log_n_out, "null pointer");
    *log_n_out = tape_check(cells, n_cells, out != nullptr);
    if (!out) return OLA_OK;       // the sizing call
    require_context(ctx);
    OLA_ON_DEVICE(ctx);
    tape_fill(ctx, cells, n_cells, out, *log_n_out);
    OLA_CATCH
}

// the validation pass: len and psdn_row of every call, read on the host before any work
struct PoseidonChunkChecked { uint32_t log_n; u64 rows; };
static PoseidonChunkChecked poseidon_chunk_check(OlaCtx* ctx, const uint64_t* calls, size_t n, const uint64_t* poseidon_table, uint32_t psdn_log_n,
                                                 bool fill) {
    require(calls || n == 0, "null pointer");
    require(n < ((size_t)1 << 26), "2^26 calls or more");
    require(psdn_log_n >= 3 && psdn_log_n <= 26, "psdn_log_n out of range (3 .. 26)");
    require(poseidon_table || !fill, "null pointer");
    std::vector<u64> len(n), row(n);
    fetch_words(ctx, len.data(), calls + 2 * n, n);
    if (poseidon_table) fetch_words(ctx, row.data(), calls + 4 * n, n);
    u64 rows = 0;
    for (size_t c = 0; c < n; c++) {
        const u64 l = gl_canon(len[c]);
        require(l != 0, "a POSEIDON call of length 0");
        require(l % 8 == 0, "a POSEIDON call whose length is no multiple of 8");
        require(l / 8 <= ((u64)1 << 26), "a POSEIDON call of more than 2^26 blocks");
        if (poseidon_table) {
            const u64 r = gl_canon(row[c]);
            require(r <= ((u64)1 << psdn_log_n) && l / 8 <= ((u64)1 << psdn_log_n) - r, "psdn_row + len / 8 is beyond the Poseidon table");
        }
        rows += 1 + l / 8;
        require(rows <= ((u64)1 << 26), "more than 2^26 rows");
    }
    return {small_trace_log_n(rows), rows};
}
static void poseidon_chunk_fill(OlaCtx* ctx, const uint64_t* calls, size_t n, const uint64_t* poseidon_table, uint32_t psdn_log_n,
                                const PoseidonChunkChecked& c, uint64_t* out) {
    DevBuf mem(&ctx->dev);
    const u64* d_calls = table_input(ctx, mem, calls, (size_t)OLA_POSEIDON_CALL_WORDS * n);
    const u64* d_psdn = table_input(ctx, mem, poseidon_table, (size_t)olatgx::NUM_POSEIDON_COLS << psdn_log_n);
    TableOutput t(ctx, mem, out, (size_t)olatgx::NUM_POSEIDON_CHUNK_COLS << c.log_n);
    generate_poseidon_chunk_trace_dev(&ctx->dev, d_calls, n, c.rows, d_psdn, psdn_log_n, t.dev);
    t.finish();
}
// like the storage-access table: the device is current before the check reads the records
int32_t ola_generate_poseidon_chunk_trace(OlaCtx* ctx, const uint64_t* calls, size_t n_calls, const uint64_t* poseidon_table,
                                          uint32_t psdn_log_n, uint64_t* out, uint32_t* log_n_out) {
    OLA_TRY
    require(log_n_out, "null pointer");
    OLA_ON_DEVICE(ctx);
    const PoseidonChunkChecked c = poseidon_chunk_check(ctx, calls, n_calls, poseidon_table, psdn_log_n, out != nullptr);
    *log_n_out = c.log_n;
    if (!out) return OLA_OK;       // the sizing call
    require_context(ctx);
    poseidon_chunk_fill(ctx, calls, n_calls, poseidon_table, psdn_log_n, c, out);
    OLA_CATCH
}

static uint32_t prog_chunk_check(const uint64_t* words, size_t n_words, const uint64_t* code_addr, uint32_t flags, const uint64_t* poseidon_table,
                                 uint32_t psdn_log_n, bool fill) {
    require((flags & ~(uint32_t)OLA_PROG_CHUNK_RESULT_LINE) == 0, "unknown flag");
    require(psdn_log_n >= 3 && psdn_log_n <= 26, "psdn_log_n out of range (3 .. 26)");
    require(n_words <= ((size_t)1 << 29), "more than 2^29 listing words");
    require(n_words % 8 == 0, "the listing is not padded to whole 8-word chunks");
    require(n_words / 8 <= ((size_t)1 << psdn_log_n), "more chunks than the Poseidon table has rows");
    require(!fill || (poseidon_table && code_addr && (words || n_words == 0)), "null pointer");
    return small_trace_log_n(n_words / 8);
}
static void prog_chunk_fill(OlaCtx* ctx, const uint64_t* words, size_t n_words, const uint64_t* code_addr, uint32_t flags,
                            const uint64_t* poseidon_table, uint32_t psdn_log_n, uint64_t* out, uint32_t log_n) {
    u64 ca[4];
    fetch_words(ctx, ca, code_addr, 4);
    DevBuf mem(&ctx->dev);
    const u64* d_words = table_input(ctx, mem, words, n_words);
    const u64* d_psdn = table_input(ctx, mem, poseidon_table, (size_t)olatgx::NUM_POSEIDON_COLS << psdn_log_n);
    TableOutput t(ctx, mem, out, (size_t)olatgx::NUM_PROG_CHUNK_COLS << log_n);
    generate_prog_chunk_trace_dev(&ctx->dev, d_words, n_words / 8, ca, (flags & OLA_PROG_CHUNK_RESULT_LINE) != 0, d_psdn, psdn_log_n, t.dev);
    t.finish();
}
int32_t ola_generate_prog_chunk_trace(OlaCtx* ctx, const uint64_t* words, size_t n_words, const uint64_t* code_addr, uint32_t flags,
                                      const uint64_t* poseidon_table, uint32_t psdn_log_n, uint64_t* out, uint32_t* log_n_out) {
    OLA_TRY
    require(log_n_out, "null pointer");
    *log_n_out = prog_chunk_check(words, n_words, code_addr, flags, poseidon_table, psdn_log_n, out != nullptr);
    if (!out) return OLA_OK;       // the sizing call
    require_context(ctx);
    OLA_ON_DEVICE(ctx);
    prog_chunk_fill(ctx, words, n_words, code_addr, flags, poseidon_table, psdn_log_n, out, *log_n_out);
    OLA_CATCH
}

// ---- from the executor's records to the twelve tables (include/ola_gpu.h, the last block of the table generators)
struct OlaTableSet {
    OlaCtx* ctx = nullptr;
    uint64_t* table[12] = {};
    uint32_t log_n[12] = {};
    uint64_t params[2] = {0, 0};
    std::vector<void*> scratch;          // the Poseidon inputs' copies and the range-check value buffer: freed before the set is handed out
    uint64_t* take(size_t words) { return (uint64_t*)ctx->dev.alloc((words ? words : 1) * 8); }
    void drop_scratch() { for (void* p : scratch) ctx->dev.free(p); scratch.clear(); }
    ~OlaTableSet() {
        if (!ctx) return;
        DeviceGuard guard(ctx);
        drop_scratch();
        for (uint64_t* t : table) if (t) ctx->dev.free(t);
    }
};
enum { TBL_CPU, TBL_MEMORY, TBL_BITWISE, TBL_CMP, TBL_RANGECHECK, TBL_POSEIDON, TBL_POSEIDON_CHUNK, TBL_STORAGE, TBL_TAPE, TBL_SCCALL, TBL_PROGRAM,
       TBL_PROG_CHUNK };

// One table of the records path, judged like an entry point of its own: HIP's stale error goes before it, its launches' error is read
// after it, and whatever it throws comes out with its code behind the name of the table.
static void records_table(const char* name, const std::function<void()>& body) {
    try {
        clear_stale_errors();
        body();
        check_launch_errors();
    }
    catch (const OlaError& e) { throw OlaError(e.code, std::string(name) + ": " + e.what()); }
    catch (const std::bad_alloc&) { throw OlaError(OLA_E_OOM, std::string(name) + ": host out of memory"); }
    catch (const std::exception& e) { throw OlaError(OLA_E_INTERNAL, std::string(name) + ": " + e.what()); }
}
// generation/builtin.rs:120-131 as backend.bitwise_beta restates it: a fresh Poseidon challenger observes the twelve limb columns (op0,
// op1, res limbs 0..3) at the table's full height and draws one challenge
static u64 draw_bitwise_beta(OlaCtx* ctx, const uint64_t* ops, size_t n_ops, uint32_t limb_bits, uint32_t log_n, bool quirks) {
    std::vector<u64> host(5 * n_ops);
    fetch_words(ctx, host.data(), ops, 5 * n_ops);
    const size_t n = (size_t)1 << log_n;
    const u64 mask = ((u64)1 << limb_bits) - 1;
    OlaChallenger ch;
    challenger_init(ch, OLA_HASH_POSEIDON);
    std::vector<u64> col(n, 0);
    for (size_t k = 2; k < 5; k++)
        for (uint32_t i = 0; i < 4; i++) {
            for (size_t r = 0; r < n_ops; r++) col[r] = (quirks && i == 3) ? 0 : (gl_canon(host[k * n_ops + r]) >> (limb_bits * i)) & mask;
            challenger_observe(ch, col.data(), n);
        }
    return challenger_get(ch);
}

static void tables_from_records(OlaCtx* ctx, const OlaExecRecords* r, OlaTableSet& s) {
    s.ctx = ctx;
    hipStream_t st = ctx->dev.stream;
    const bool quirks = r->flags & OLA_RECORDS_REFERENCE_QUIRKS, explicit_betas = r->flags & OLA_RECORDS_EXPLICIT_BETAS;
    const uint32_t tq = quirks ? OLA_TABLEGEN_REFERENCE_QUIRKS : 0u;
    uint32_t* L = s.log_n;
    // the storage tree hashed, with the accesses' rows of the Poseidon inputs; the inputs are copies, the caller's are not written
    const size_t stride = r->psdn_stride;
    uint64_t* pin = s.take(12 * stride); s.scratch.push_back(pin);
    uint64_t* pf = s.take(4 * stride); s.scratch.push_back(pf);
    if (stride) {
        HIP_CHECK(hipMemcpyAsync(pin, r->psdn_inputs, 12 * stride * 8, hipMemcpyDefault, st));
        HIP_CHECK(hipMemcpyAsync(pf, r->psdn_filters, 4 * stride * 8, hipMemcpyDefault, st));
        HIP_CHECK(hipStreamSynchronize(st));     // the caller's host buffers are read before the call goes on
    }
    uint64_t roots[8];
    records_table("storage-access table", [&] {
        const StorageChecked c = storage_check(ctx, r->accesses, r->n_access, r->siblings, stride ? pin : nullptr, stride ? pf : nullptr, stride, true);
        L[TBL_STORAGE] = c.log_n;
        s.table[TBL_STORAGE] = s.take((size_t)olatgs::NUM_COL_ST << c.log_n);
        storage_fill(ctx, r->accesses, r->n_access, r->siblings, c, s.table[TBL_STORAGE], stride ? pin : nullptr, stride ? pf : nullptr, stride, roots);
    });
    records_table("Poseidon table", [&] {
        L[TBL_POSEIDON] = poseidon_table_check(pin, r->psdn_rows, stride, true);
        s.table[TBL_POSEIDON] = s.take((size_t)olatgs::NUM_POSEIDON_COLS << L[TBL_POSEIDON]);
        poseidon_table_fill(ctx, pin, pf, r->psdn_rows, stride, s.table[TBL_POSEIDON], L[TBL_POSEIDON]);
    });
    // the two chunk tables gather from it
    records_table("Poseidon-chunk table", [&] {
        const PoseidonChunkChecked c = poseidon_chunk_check(ctx, r->psdn_calls, r->n_psdn_calls, s.table[TBL_POSEIDON], L[TBL_POSEIDON], true);
        L[TBL_POSEIDON_CHUNK] = c.log_n;
        s.table[TBL_POSEIDON_CHUNK] = s.take((size_t)olatgx::NUM_POSEIDON_CHUNK_COLS << c.log_n);
        poseidon_chunk_fill(ctx, r->psdn_calls, r->n_psdn_calls, s.table[TBL_POSEIDON], L[TBL_POSEIDON], c, s.table[TBL_POSEIDON_CHUNK]);
    });
    records_table("program-chunk table", [&] {
        const uint32_t cflags = (r->flags & OLA_RECORDS_RESULT_LINE) ? OLA_PROG_CHUNK_RESULT_LINE : 0u;
        L[TBL_PROG_CHUNK] = prog_chunk_check(r->listing_words, r->n_listing_words, r->code_addr, cflags, s.table[TBL_POSEIDON], L[TBL_POSEIDON], true);
        s.table[TBL_PROG_CHUNK] = s.take((size_t)olatgx::NUM_PROG_CHUNK_COLS << L[TBL_PROG_CHUNK]);
        prog_chunk_fill(ctx, r->listing_words, r->n_listing_words, r->code_addr, cflags, s.table[TBL_POSEIDON], L[TBL_POSEIDON], s.table[TBL_PROG_CHUNK],
                        L[TBL_PROG_CHUNK]);
    });
    // the comparison and memory tables, their value lists behind the CPU's in one buffer
    const size_t n_cpu = r->n_cpu_rc, n_cmp = r->n_cmp_ops, n_cells = r->n_mem_cells;
    uint64_t* vals = s.take(n_cpu + n_cmp + 2 * n_cells); s.scratch.push_back(vals);
    if (n_cpu) { HIP_CHECK(hipMemcpyAsync(vals, r->cpu_rc, n_cpu * 8, hipMemcpyDefault, st)); HIP_CHECK(hipStreamSynchronize(st)); }
    records_table("comparison table", [&] {
        L[TBL_CMP] = cmp_check(r->cmp_ops, n_cmp, true);
        s.table[TBL_CMP] = s.take((size_t)olatgm::COL_NUM_CMP << L[TBL_CMP]);
        cmp_fill(ctx, r->cmp_ops, n_cmp, s.table[TBL_CMP], L[TBL_CMP], n_cmp ? vals + n_cpu : nullptr);
    });
    uint64_t counts[2] = {0, 0};
    records_table("memory table", [&] {
        L[TBL_MEMORY] = memory_check(r->mem_cells, n_cells, tq, true);
        s.table[TBL_MEMORY] = s.take((size_t)olatgm::NUM_MEM_COLS << L[TBL_MEMORY]);
        memory_fill(ctx, r->mem_cells, n_cells, tq, s.table[TBL_MEMORY], L[TBL_MEMORY], n_cells ? vals + n_cpu + n_cmp : nullptr, counts);
    });
    // the range-check table from that buffer and four filter columns filled from the segment lengths
    const size_t n_rows = n_cpu + n_cmp + counts[0] + counts[1];
    records_table("range-check table", [&] {
        L[TBL_RANGECHECK] = rc_check(vals, n_rows, r->range_bits, true);
        uint64_t* filters = s.take(4 * n_rows); s.scratch.push_back(filters);
        rc_filters_dev(&ctx->dev, n_cpu, n_cmp, counts[0], n_rows, (u64*)filters);
        s.table[TBL_RANGECHECK] = s.take((size_t)olatg::COL_NUM_RC << L[TBL_RANGECHECK]);
        rc_fill(ctx, n_rows ? vals : nullptr, n_rows ? filters : nullptr, n_rows, r->range_bits, s.table[TBL_RANGECHECK], L[TBL_RANGECHECK]);
    });
    // CPU, tape, SCCALL, bitwise
    records_table("CPU table", [&] {
        cpu_check(r->steps, r->n_steps, r->cpu_log_n);
        L[TBL_CPU] = r->cpu_log_n;
        s.table[TBL_CPU] = s.take((size_t)olatgc::NUM_CPU_COLS << L[TBL_CPU]);
        cpu_fill(ctx, r->steps, r->n_steps, L[TBL_CPU], s.table[TBL_CPU]);
    });
    records_table("tape table", [&] {
        L[TBL_TAPE] = tape_check(r->tape_cells, r->n_tape_cells, true);
        s.table[TBL_TAPE] = s.take((size_t)olatgx::NUM_COL_TAPE << L[TBL_TAPE]);
        tape_fill(ctx, r->tape_cells, r->n_tape_cells, s.table[TBL_TAPE], L[TBL_TAPE]);
    });
    L[TBL_SCCALL] = 3;
    s.table[TBL_SCCALL] = s.take((size_t)olatgx::NUM_COL_SCCALL << 3);
    sccall_padding_dev(&ctx->dev, 8, (u64*)s.table[TBL_SCCALL]);
    records_table("bitwise table", [&] {
        L[TBL_BITWISE] = bitwise_check(r->bitwise_ops, r->n_bitwise_ops, r->limb_bits, tq, true);
        s.params[0] = explicit_betas ? gl_canon(r->bitwise_beta) : draw_bitwise_beta(ctx, r->bitwise_ops, r->n_bitwise_ops, r->limb_bits, L[TBL_BITWISE], quirks);
        s.table[TBL_BITWISE] = s.take((size_t)olatg::COL_NUM_BITWISE << L[TBL_BITWISE]);
        bitwise_fill(ctx, r->bitwise_ops, r->n_bitwise_ops, r->limb_bits, s.params[0], tq, s.table[TBL_BITWISE], L[TBL_BITWISE]);
    });
    // the program table, its challenge from the two state roots (generation/prog.rs:23-29)
    if (explicit_betas) {
        s.params[1] = gl_canon(r->program_beta);
    } else {
        OlaChallenger ch;
        challenger_init(ch, OLA_HASH_POSEIDON);
        for (int i = 0; i < 4; i++) { const u64 pair[2] = {gl_canon(roots[i]), gl_canon(roots[4 + i])}; challenger_observe(ch, pair, 2); }
        s.params[1] = challenger_get(ch);
    }
    records_table("program table", [&] {
        const uint32_t pflags = (r->flags & OLA_RECORDS_ZERO_FILLER) ? OLA_TABLEGEN_ZERO_FILLER : 0u;
        prog_steps_check(r->steps, r->n_steps, r->prog_listing, r->prog_log_n, pflags);
        L[TBL_PROGRAM] = r->prog_log_n;
        s.table[TBL_PROGRAM] = s.take((size_t)olatg::NUM_PROG_COLS << L[TBL_PROGRAM]);
        uint64_t exec_rows = 0;
        prog_steps_fill(ctx, r->steps, r->n_steps, r->prog_listing, L[TBL_PROGRAM], s.params[1], pflags, s.table[TBL_PROGRAM], &exec_rows);
    });
    HIP_CHECK(hipStreamSynchronize(st));          // the two fills
    s.drop_scratch();
}

static void require_records(OlaCtx* ctx, const OlaExecRecords* rec) {
    require(rec != nullptr, "null pointer");
    require(rec->size >= sizeof(OlaExecRecords), "OlaExecRecords.size is smaller than this library's struct");
    require((rec->flags & ~(uint32_t)(OLA_RECORDS_REFERENCE_QUIRKS | OLA_RECORDS_ZERO_FILLER | OLA_RECORDS_RESULT_LINE | OLA_RECORDS_EXPLICIT_BETAS)) == 0,
            "unknown flag");
    require(rec->psdn_stride <= ((uint64_t)1 << 26) && rec->psdn_rows <= rec->psdn_stride, "psdn_rows / psdn_stride out of range");
    require((rec->psdn_inputs && rec->psdn_filters) || rec->psdn_stride == 0, "null pointer");
    require(rec->n_cpu_rc < ((uint64_t)1 << 31) && rec->n_bitwise_ops <= ((uint64_t)1 << 26), "too many range-check values or bitwise operations");
    require((rec->cpu_rc || !rec->n_cpu_rc) && (rec->bitwise_ops || !rec->n_bitwise_ops), "null pointer");
    require_context(ctx);
}

int32_t ola_tables_from_records(OlaCtx* ctx, const OlaExecRecords* rec, OlaTableSet** out) {
    OLA_TRY
    require(out != nullptr, "null pointer");
    *out = nullptr;
    require_records(ctx, rec);
    OLA_ON_DEVICE(ctx);
    std::unique_ptr<OlaTableSet> set(new OlaTableSet());
    tables_from_records(ctx, rec, *set);
    *out = set.release();
    OLA_CATCH
}

int32_t ola_tables_get(const OlaTableSet* set, const uint64_t* ptrs[12], uint32_t log_n[12], uint64_t params[2], uint64_t compress[12]) {
    OLA_TRY
    require(set != nullptr, "null pointer");
    for (int t = 0; t < 12; t++) {
        if (ptrs) ptrs[t] = set->table[t];
        if (log_n) log_n[t] = set->log_n[t];
        if (compress) compress[t] = t == TBL_BITWISE ? set->params[0] : t == TBL_PROGRAM ? set->params[1] : 0;
    }
    if (params) { params[0] = set->params[0]; params[1] = set->params[1]; }
    OLA_CATCH
}

int32_t ola_tables_free(OlaTableSet* set) {
    OLA_TRY
    delete set;
    OLA_CATCH
}

int32_t ola_prove_from_records(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, const OlaExecRecords* rec, uint8_t* out, size_t cap,
                               size_t* out_len) {
    OLA_TRY
    require(airset && out_len, "null pointer");
    require_records(ctx, rec);
    OLA_ON_DEVICE(ctx);
    require(airset_widths((const u64*)airset, airset_words).size() == 12, "the AIR set does not have the twelve tables of the records");
    std::unique_ptr<OlaTableSet> set(new OlaTableSet());
    tables_from_records(ctx, rec, *set);
    const uint64_t* ptrs[12];
    uint64_t compress[12];
    for (int t = 0; t < 12; t++) { ptrs[t] = set->table[t]; compress[t] = t == TBL_BITWISE ? set->params[0] : t == TBL_PROGRAM ? set->params[1] : 0; }
    const int32_t rc = ola_prove_with_traces(ctx, airset, airset_words, ptrs, set->log_n, set->params, compress, out, cap, out_len);
    if (rc != OLA_OK) throw OlaError(rc, g_last_error);
    OLA_CATCH
}
