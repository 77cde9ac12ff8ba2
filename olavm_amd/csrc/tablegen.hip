// Device-side table generators (tablegen.h): kernels and launchers of nine tables.  Own translation unit, the second that pulls in
// rocPRIM (sorts and scans, rocprim_ops.h); the entry points that call it are tablegen_api.hip.
//
// The range-check, bitwise and program tables from their primary columns (generation/builtin.rs:35-206, 249-316,
// generation/prog.rs:18-156): one fill kernel per table writes every column that is not a permuted one -- thread = row, so
// every column is stored along rows, and rows beyond the live inputs get their zeros in the same pass -- then the table's
// lookup pairs go through one batch of permuted_cols (lookup.hip), straight into their columns of `out`.
#include <algorithm>

#include "lookup.h"
#include "rocprim_ops.h"
#include "tablegen.h"
#include "tablegen_columns.h"
#include "tablegen_cpu_columns.h"
#include "tablegen_mem_columns.h"
#include "tablegen_small_columns.h"

namespace ola {

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
    DevBuf mem(ctx);
    u32 total = 0;
    u32* at = nullptr;
    if (n_steps) {
        u32* counts = mem.alloc<u32>((size_t)n_steps + 1);
        at = mem.alloc<u32>((size_t)n_steps + 1);
        hipLaunchKernelGGL(exec_count_kernel, dim3(blocks((size_t)n_steps + 1)), dim3(256), 0, stream, steps, n_steps, counts);
        HIP_CHECK(hipGetLastError());
        ExclusiveSum<u32>(mem, (size_t)n_steps + 1).run(stream, counts, at, (size_t)n_steps + 1);
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
    DevBuf mem(ctx);
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
    // one sort for every pass, sized for the widest of their bit ranges (rocPRIM's temporary storage grows with the number of digit
    // places, ceil(bits / radix bits), so the widest range asks for the most)
    u32 bits[tm::MEM_CELL_WORDS], widest = 0;
    for (u32 field : order) widest = std::max(widest, bits[field] = bit_length(host_stats[field]));
    SortPairs<u64> sort(mem, n_cells, std::max(widest, 1u));
    u32 cur = 0;
    for (u32 field : order) {
        if (bits[field] == 0) continue;                                     // every key of this field is 0
        hipLaunchKernelGGL(mem_pass_key_kernel, dim3(blocks(n_cells)), dim3(256), 0, stream, canon, n_cells, idx[cur], field, keys);
        HIP_CHECK(hipGetLastError());
        sort.run(stream, keys, keys + n_cells, idx[cur], idx[cur ^ 1], bits[field]);
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
    DevBuf mem(ctx);
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
        SortPairs<u64>(mem, n_cells, bits).run(stream, keys, keys + n_cells, idx, idx + n_cells, bits);
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
    DevBuf mem(ctx);
    u32* at = nullptr;
    if (n_calls) {
        u32* counts = mem.alloc<u32>((size_t)n_calls + 1);
        at = mem.alloc<u32>((size_t)n_calls + 1);
        hipLaunchKernelGGL(pchunk_count_kernel, dim3(blocks((size_t)n_calls + 1)), dim3(256), 0, stream, calls, n_calls, counts);
        HIP_CHECK(hipGetLastError());
        ExclusiveSum<u32>(mem, (size_t)n_calls + 1).run(stream, counts, at, (size_t)n_calls + 1);
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
