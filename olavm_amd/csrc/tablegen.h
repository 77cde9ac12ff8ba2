// Device-side table generators (tablegen.hip, its own translation unit; called from tablegen_api.hip).
#pragma once
#include <cstddef>
#include <cstdint>

#include "device_ctx.h"
#include "gl.cuh"

namespace ola {

// Whole tables from their primary columns (ola_generate_rc_trace / _bitwise_trace / _prog_trace of include/ola_gpu.h): all
// pointers are device memory, `out` is column-major ncols x 2^log_n with log_n as the *_log_n functions give it (the
// program table: as passed).  Every column of `out` is written; complete when the call returns.
u32 rc_trace_log_n(u64 n_rows, u32 range_bits);
u32 bitwise_trace_log_n(u64 n_ops, u32 limb_bits);
void generate_rc_trace_dev(DeviceCtx* ctx, const u64* vals, const u64* filters, size_t n_rows, u32 range_bits, u64* out);
void generate_bitwise_trace_dev(DeviceCtx* ctx, const u64* ops, size_t n_ops, u32 limb_bits, u64 beta, bool reference_quirks, u64* out);
void generate_prog_trace_dev(DeviceCtx* ctx, const u64* exec, const u64* prog, u32 log_n, u64 beta, u64* out);

// The CPU table (94 x 2^log_n) and the program table with its executed side built on the device, both from step records
// (ola_generate_cpu_trace / ola_generate_prog_trace_steps): steps is device memory, OLA_CPU_STEP_WORDS x n_steps column-major,
// n_steps <= 2^log_n and < 2^31.  generate_prog_trace_steps_dev returns false, with the count in *exec_rows and nothing written,
// when the steps give more than 2^log_n executed rows; otherwise it ends in generate_prog_trace_dev.
void generate_cpu_trace_dev(DeviceCtx* ctx, const u64* steps, size_t n_steps, u32 log_n, u64* out);
bool generate_prog_trace_steps_dev(DeviceCtx* ctx, const u64* steps, size_t n_steps, const u64* prog, u32 log_n, u64 beta, bool zero_filler,
                                   u64* out, u64* exec_rows);

// The memory table (29 x 2^memory_trace_log_n) from raw cells and the comparison table (6 x 2^cmp_trace_log_n) from operand pairs
// (ola_generate_memory_trace / ola_generate_cmp_trace): cells is device memory, 5 x n_cells column-major in any order, n_cells < 2^31;
// ops is 2 x n_ops, n_ops < 2^31.  rc_out (device memory of 2 n_cells words, or null) receives counts[0] range-checked sort values and
// behind them counts[1] region values, nothing else of it is written; abs_diff_out (n_ops words, or null) ABS_DIFF of the live rows.
// The memory table waits for the stream once (the key statistics that size the sort passes) and is complete on return; the
// comparison table is one launch and returns when it is enqueued.
u32 memory_trace_log_n(u64 n_cells);
u32 cmp_trace_log_n(u64 n_ops);
void generate_memory_trace_dev(DeviceCtx* ctx, const u64* cells, size_t n_cells, bool reference_quirks, u64* out, u64* rc_out, u64 counts[2]);
void generate_cmp_trace_dev(DeviceCtx* ctx, const u64* ops, size_t n_ops, u64* out, u64* abs_diff_out);

// The tape table (6 columns) from cells in execution order, the Poseidon-chunk table (53) from POSEIDON call records and the program-chunk
// table (40) from the zero-padded listing (ola_generate_tape_trace / _poseidon_chunk_trace / _prog_chunk_trace): all pointers but code_addr
// are device memory, every table is 2^small_trace_log_n(rows) high with rows = n_cells, the sum of 1 + len / 8 over the calls (the
// caller's validation pass computed it, and checked every psdn_row + len / 8 against the Poseidon table's height), n_chunks.  psdn is the
// resident Poseidon table, 134 x 2^psdn_log_n; n_chunks <= 2^psdn_log_n.  The tape table waits for the stream once (the address bits
// that size the sort) and once more, like the Poseidon-chunk table with calls, before its work space goes back to the pool (DevBuf's
// destructor); the program-chunk table only enqueues.
u32 small_trace_log_n(u64 rows);
void generate_tape_trace_dev(DeviceCtx* ctx, const u64* cells, size_t n_cells, u64* out);
void generate_poseidon_chunk_trace_dev(DeviceCtx* ctx, const u64* calls, size_t n_calls, u64 rows, const u64* psdn, u32 psdn_log_n, u64* out);
void generate_prog_chunk_trace_dev(DeviceCtx* ctx, const u64* words, size_t n_chunks, const u64 code_addr[4], bool result_line, const u64* psdn,
                                   u32 psdn_log_n, u64* out);

}  // namespace ola
