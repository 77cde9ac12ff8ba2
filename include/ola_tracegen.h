/* Native trace generator: runs a small OlaVM program on the host and fills the 12 STARK tables so that every
 * constraint and cross-table lookup of OlaStark holds -- the job of the reference's Rust executor + circuits/src/generation
 * for the instructions it supports: MOV NOT ADD MUL EQ NEQ ASSERT JMP CJMP CALL RET MLOAD MSTORE RC AND OR XOR GTE POSEIDON
 * TSTORE TLOAD SSTORE SLOAD END -- everything but cross-contract calls (for which the reference AIR admits no trace, see
 * DESIGN.md) and SIGCHECK.  It reproduces the Python executor olavm_amd/air/miniexec.py word for word.  Host-only C ABI,
 * libola_tracegen.so; the traces go straight into ola_prove_with_traces.
 *
 * Restates: core/src/vm/opcodes.rs:81-114 (opcode masks), circuits/src/cpu/cpu_stark.rs:529-581 (instruction encoding),
 * executor/src/lib.rs (instruction semantics), circuits/src/generation/{cpu,memory,builtin,poseidon,poseidon_chunk,prog}.rs
 * (row layouts and padding), circuits/src/stark/lookup.rs:68-132 (permuted columns). */
#ifndef OLA_TRACEGEN_H
#define OLA_TRACEGEN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* One instruction: op = bit position of the opcode mask (core/src/vm/opcodes.rs: ADD 31, MUL 30, EQ 29, ASSERT 28, MOV 27,
 * JMP 26, CJMP 25, CALL 24, RET 23, MLOAD 22, MSTORE 21, END 20, RC 19, AND 18, OR 17, XOR 16, NOT 15, NEQ 14, GTE 13,
 * POSEIDON 12, SLOAD 11, SSTORE 10, TLOAD 9, TSTORE 8); dst / op0 / op1 = register index 0..9 or -1; op1_is_imm != 0: the second operand is `imm` (a two-word
 * instruction). */
typedef struct OlaInstr {
    uint32_t op;
    int32_t dst, op0, op1;
    uint32_t op1_is_imm;
    uint64_t imm;
} OlaInstr;

typedef struct OlaTraceSet OlaTraceSet;

/* flags: close the program-hash chain with a result line and a state-tree proof that the hash is the leaf at the code
 * address (256 storage rows, 512 Poseidon rows) */
#define OLA_TRACEGEN_PROVE_PROGRAM_HASH 1u
/* flags: take the compress challenges of the bitwise and program tables from the bitwise_beta / program_beta arguments (tests).
 * Without it they are derived as the reference derives them -- a Fiat-Shamir transcript observes the limb columns of the bitwise
 * table (generation/builtin.rs:120-131) and the state roots before and after the run (generation/prog.rs:23-29) -- and the two
 * arguments are ignored; ola_tracegen_betas returns the values used (they are the proof's compress_challenges). */
#define OLA_TRACEGEN_EXPLICIT_BETAS 2u
/* flags: reproduce the two places where the reference's generators write rows its own AIR rejects, for comparing whole pipelines with
 * a build of the reference (integration/pin/) -- not for proving: (a) the fourth limb of a bitwise operand / result is left zero
 * (generation/builtin.rs:66,71,76 store it at `OP*_LIMBS.end`, the exclusive end of the column range, and the next write replaces it);
 * (b) the memory table of a run without memory cells is generation/memory.rs:95-153's: every row a prophet-region row, row 0 without
 * its selector (default: one stack-region row first, so that memory_stark.rs:265-270 hold on the wrap-around). */
#define OLA_TRACEGEN_REFERENCE_QUIRKS 4u
/* flags: do not build the CPU table and the program table -- the two that are per-row functions of the executed steps and that the
 * GPU generates from them (include/ola_gpu.h ola_generate_cpu_trace, ola_generate_prog_trace_steps).  ola_tracegen_table answers the
 * two with their shape and data = NULL; ola_tracegen_cpu_steps and ola_tracegen_prog_listing return what the GPU calls take. */
#define OLA_TRACEGEN_STEPS_ONLY 8u
/* flags: OLA_TRACEGEN_STEPS_ONLY (implied), and the memory, comparison and range-check tables are not built either -- no sort, no field
 * inversions, no permuted columns on the host: the GPU makes the first two from raw cells and operand pairs (include/ola_gpu.h
 * ola_generate_memory_trace, ola_generate_cmp_trace) and the third from the value lists those calls leave in HBM behind the CPU's
 * (ola_generate_rc_trace).  ola_tracegen_table answers the three with their shape and data = NULL as well; ola_tracegen_mem_cells,
 * ola_tracegen_cmp_ops and ola_tracegen_cpu_rc_values return what the GPU calls take.  A range-checked value too wide for two limbs,
 * which the table path refuses, is not looked for. */
#define OLA_TRACEGEN_CELLS_ONLY 16u
/* flags: OLA_TRACEGEN_CELLS_ONLY (implied), and neither the storage-access table nor the Poseidon table is built: the state tree is
 * bypassed -- a key -> value map serves SLOAD, no node is hashed -- and the GPU hashes it from the access records (include/ola_gpu.h
 * ola_generate_storage_trace, ola_generate_poseidon_table).  ola_tracegen_table answers the two with their shape and data = NULL;
 * ola_tracegen_storage_accesses and ola_tracegen_poseidon_inputs return what the GPU calls take.  The program table's challenge needs
 * the state roots before and after the run, which only the device's tree has: ola_tracegen_betas answers ~0 (-1) for it unless
 * OLA_TRACEGEN_EXPLICIT_BETAS is set, and ola_tracegen_program_beta draws it from the roots the GPU call returns. */
#define OLA_TRACEGEN_HASHES_ONLY 32u
/* flags: OLA_TRACEGEN_HASHES_ONLY (implied), and no table at all is built: ola_tracegen_table answers every table with its shape and
 * data = NULL.  The bitwise, tape, Poseidon-chunk and program-chunk tables are the GPU's to make as well (include/ola_gpu.h
 * ola_generate_bitwise_trace, ola_generate_tape_trace, ola_generate_poseidon_chunk_trace, ola_generate_prog_chunk_trace; the SCCALL table is
 * the 26 x 8 padding table): ola_tracegen_bitwise_ops, ola_tracegen_tape_cells, ola_tracegen_poseidon_calls and ola_tracegen_listing_words
 * return what those calls take.  The Poseidon inputs keep coming from ola_tracegen_poseidon_inputs -- the host hashes the listing and the
 * POSEIDON instructions' blocks anyway in order to execute.  The bitwise table's challenge observes that table's limb columns, which
 * only the device has then: ola_tracegen_betas answers ~0 (-1) for it, as for the program table's, unless OLA_TRACEGEN_EXPLICIT_BETAS
 * is set. */
#define OLA_TRACEGEN_RECORDS_ONLY 64u

/* Executes the program (at most max_steps CPU rows) and builds the 12 tables of ola_stark(range_bits, limb_bits) in
 * `enum Table` order.  range_bits / limb_bits are 16 / 8 in the reference; smaller values give structurally identical
 * miniature fixed tables.  Returns 0, or a negative code with a message in ola_tracegen_last_error(). */
int32_t ola_tracegen_run(const OlaInstr* program, size_t n_instr, const uint64_t code_addr[4], const uint64_t storage_addr[4],
                         uint32_t range_bits, uint32_t limb_bits, uint64_t bitwise_beta, uint64_t program_beta, uint64_t max_steps,
                         uint32_t flags, OlaTraceSet** out);
/* Table t: column-major ncols x 2^log_n words, owned by the set (data = NULL for a table OLA_TRACEGEN_STEPS_ONLY, _CELLS_ONLY, _HASHES_ONLY or _RECORDS_ONLY left out). */
int32_t ola_tracegen_table(const OlaTraceSet* set, uint32_t table, uint32_t* ncols, uint32_t* log_n, const uint64_t** data);
/* OLA_TRACEGEN_STEPS_ONLY sets only (-1 otherwise): the step records, OLA_CPU_STEP_WORDS x n_steps column-major, and the program
 * table's listing side, 7 x 2^log_n column-major (four code-address words, pc, inst, filter); both owned by the set. */
int32_t ola_tracegen_cpu_steps(const OlaTraceSet* set, uint64_t* n_steps, const uint64_t** data);
int32_t ola_tracegen_prog_listing(const OlaTraceSet* set, uint32_t* log_n, const uint64_t** data);
/* OLA_TRACEGEN_CELLS_ONLY sets only (-1 otherwise), all owned by the set: the memory cells in execution order, OLA_MEM_CELL_WORDS x
 * n_cells column-major (address, clock, the op's one-hot word, value, is_write); the comparison operands, 2 x n_ops column-major (op0,
 * op1); the values of the CPU's RC instructions, the first segment of the range-check table's input. */
int32_t ola_tracegen_mem_cells(const OlaTraceSet* set, uint64_t* n_cells, const uint64_t** data);
int32_t ola_tracegen_cmp_ops(const OlaTraceSet* set, uint64_t* n_ops, const uint64_t** data);
int32_t ola_tracegen_cpu_rc_values(const OlaTraceSet* set, uint64_t* n_values, const uint64_t** data);
/* OLA_TRACEGEN_HASHES_ONLY sets only (-1 otherwise), owned by the set: the access records in execution order, OLA_STORAGE_ACCESS_WORDS x
 * n_access column-major (tree key, value = the leaf after the access, pre_value = 0, flags, psdn_row) -- the silent write of the
 * program hash first and its OLA_STORAGE_FOR_PROG read last when OLA_TRACEGEN_PROVE_PROGRAM_HASH is set; and the Poseidon table's
 * inputs (12 x 2^log_n) and filters (4 x 2^log_n), column-major at full table height, with the program-chunk, POSEIDON-instruction and
 * tree-key rows filled and the 512 rows of every access left zero, their first row in the record's psdn_row. */
int32_t ola_tracegen_storage_accesses(const OlaTraceSet* set, uint64_t* n_access, const uint64_t** data);
int32_t ola_tracegen_poseidon_inputs(const OlaTraceSet* set, uint32_t* log_n, const uint64_t** inputs, const uint64_t** filters);
/* OLA_TRACEGEN_RECORDS_ONLY sets only (-1 otherwise), all owned by the set, column-major in execution order: the bitwise operations,
 * 5 x n_ops (filter = 1, the opcode's one-hot word, op0, op1, res); the tape cells, OLA_TAPE_CELL_WORDS x n_cells (tape address, the
 * opcode's one-hot word, value); the POSEIDON calls, OLA_POSEIDON_CALL_WORDS x n_calls (clk, src, len, dst, psdn_row -- the row of the
 * call's first block in the numbering ola_tracegen_poseidon_inputs uses: the program chunks first, then the calls' blocks); the
 * listing zero-padded to whole 8-word chunks, with the code address in code_addr[0..3]. */
int32_t ola_tracegen_bitwise_ops(const OlaTraceSet* set, uint64_t* n_ops, const uint64_t** data);
int32_t ola_tracegen_tape_cells(const OlaTraceSet* set, uint64_t* n_cells, const uint64_t** data);
int32_t ola_tracegen_poseidon_calls(const OlaTraceSet* set, uint64_t* n_calls, const uint64_t** data);
int32_t ola_tracegen_listing_words(const OlaTraceSet* set, uint64_t* n_words, const uint64_t** data, uint64_t code_addr[4]);
/* The program table's compress challenge from roots[0..3] = the state root before the run and roots[4..7] = after it
 * (generation/prog.rs:23-29; the roots_out of ola_generate_storage_trace).  Host only. */
int32_t ola_tracegen_program_beta(const uint64_t roots[8], uint64_t* beta);
/* Number of executed CPU rows (before padding). */
uint64_t ola_tracegen_cpu_rows(const OlaTraceSet* set);
/* out[0] = the bitwise table's compress challenge, out[1] = the program table's. */
int32_t ola_tracegen_betas(const OlaTraceSet* set, uint64_t out[2]);
void ola_tracegen_free(OlaTraceSet* set);
const char* ola_tracegen_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* OLA_TRACEGEN_H */
