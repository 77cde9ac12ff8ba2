"""generation/cpu.rs:11-218 and generation/prog.rs:31-108 restated in plain Python over step records (olavm_amd/air/cpu_steps.py):
the reference the tests of ola_generate_cpu_trace / ola_generate_prog_trace_steps compare with, itself compared with the reference's
own output (tests/golden/ref_cpu_steps.json) and with the tables of olavm_amd/air/miniexec.py in tests/test_ref_cpu_steps.py."""
import numpy as np

from olavm_amd.air import cpu_steps as S, ola_tables as T, tracegen as TG
from olavm_amd.air.dsl import P

# cpu.rs:20-60
SELECTOR = {"ADD": T.COL_S_SIMPLE_ARITHMATIC_OP, "MUL": T.COL_S_SIMPLE_ARITHMATIC_OP, "EQ": T.COL_S_SIMPLE_ARITHMATIC_OP,
            "ASSERT": T.COL_S_SIMPLE_ARITHMATIC_OP, "NEQ": T.COL_S_SIMPLE_ARITHMATIC_OP, "MOV": T.COL_S_MOV, "JMP": T.COL_S_JMP,
            "CJMP": T.COL_S_CJMP, "CALL": T.COL_S_CALL, "RET": T.COL_S_RET, "MLOAD": T.COL_S_MLOAD, "MSTORE": T.COL_S_MSTORE,
            "END": T.COL_S_END, "RC": T.COL_S_RC, "AND": T.COL_S_BITWISE, "OR": T.COL_S_BITWISE, "XOR": T.COL_S_BITWISE, "NOT": T.COL_S_NOT,
            "GTE": T.COL_S_GTE, "POSEIDON": T.COL_S_PSDN, "SLOAD": T.COL_S_SLOAD, "SSTORE": T.COL_S_SSTORE, "TLOAD": T.COL_S_TLOAD,
            "TSTORE": T.COL_S_TSTORE, "SCCALL": T.COL_S_CALL_SC}
assert len(SELECTOR) == 25
MASK = {name: T.op_mask(name) for name in SELECTOR}


def canonical(words):
    w = np.asarray(words, dtype=np.uint64)
    return np.where(w >= np.uint64(P), w - np.uint64(P), w)


def field(steps, col):
    """CPU column `col` of every record, as Python integers"""
    return [int(x) for x in steps[col - S.STEP_FIRST_COL]]


def cpu_table(steps, log_n):
    steps = canonical(steps).reshape(S.STEP_WORDS, -1)
    k, n = steps.shape[1], 1 << log_n
    assert k <= n
    t = np.zeros((T.NUM_CPU_COLS, n), dtype=np.uint64)
    t[S.STEP_FIRST_COL:S.STEP_FIRST_COL + S.STEP_COPIED_COLS, :k] = steps[:S.STEP_COPIED_COLS]
    t[T.COL_FILTER_TAPE_LOOKING, :k] = steps[S.STEP_COPIED_COLS]
    opcode, env, ext, cnt = (field(steps, c) for c in (T.COL_OPCODE, T.COL_ENV_IDX, T.COL_IS_EXT_LINE, T.COL_EXT_CNT))
    imm, op0, op1 = (field(steps, c) for c in (T.COL_OP1_IMM, T.COL_OP0, T.COL_OP1))
    by_mask = {MASK[name]: col for name, col in SELECTOR.items()}
    for i in range(k):
        o = opcode[i]
        if o in by_mask:
            t[by_mask[o], i] = 1
        entry = env[i] == 0
        if o in (MASK["SLOAD"], MASK["SSTORE"], MASK["SCCALL"]) or (o == MASK["END"] and not entry):
            ext_length = 1
        elif o == MASK["TLOAD"]:
            ext_length = (op0[i] * op1[i] + 1 - op0[i]) % P
        elif o == MASK["TSTORE"]:
            ext_length = op1[i]
        else:
            ext_length = 0
        t[T.COL_IS_ENTRY_SC, i] = int(entry)
        t[T.COL_IS_NEXT_LINE_DIFF_INST, i] = int(ext_length == cnt[i])
        t[T.COL_IS_NEXT_LINE_SAME_TX, i] = int(not (entry and o == MASK["END"]))
        t[T.IS_SCCALL_EXT_LINE, i] = int(o == MASK["SCCALL"] and cnt[i] == 1)
        t[T.COL_IS_STORAGE_EXT_LINE, i] = int(o in (MASK["SLOAD"], MASK["SSTORE"]) and ext[i] == 1)
        t[T.COL_FILTER_SCCALL_END, i] = int(o == MASK["END"] and ext[i] == 1)
        t[T.COL_FILTER_LOOKING_PROG_IMM, i] = int(ext[i] != 1 and (o in (MASK["MLOAD"], MASK["MSTORE"]) or imm[i] == 1))
    # cpu.rs:180-208
    t[T.COL_INST, k:] = t[T.COL_INST, k - 1] if k else 1048576
    t[T.COL_IDX_STORAGE, k:] = t[T.COL_IDX_STORAGE, k - 1] if k else 0
    t[T.COL_OPCODE, k:] = MASK["END"]
    for c in (T.COL_S_END, T.COL_IS_ENTRY_SC, T.COL_IS_NEXT_LINE_DIFF_INST, T.COL_IS_PADDING):
        t[c, k:] = 1
    return t


def executed_rows(steps):
    """prog.rs:31-44, 59-108 -> [(addr_code[4], pc, word)]"""
    steps = canonical(steps).reshape(S.STEP_WORDS, -1)
    cols = [field(steps, c) for c in list(T.COL_ADDR_CODE_RANGE) + [T.COL_PC, T.COL_INST, T.COL_IMM_VAL, T.COL_IS_EXT_LINE, T.COL_OP1_IMM, T.COL_OPCODE]]
    rows = []
    for a0, a1, a2, a3, pc, inst, imm_val, ext, imm, o in zip(*cols):
        if ext == 1:
            continue
        rows.append(((a0, a1, a2, a3), pc, inst))
        if imm == 1 or o in (MASK["MLOAD"], MASK["MSTORE"]):
            rows.append(((a0, a1, a2, a3), (pc + 1) % P, imm_val))
    return rows


def exec_side(steps, log_n, zero_filler=False):
    """the executed side as ola_generate_prog_trace takes it (7 x n), filler rows included"""
    rows, n = executed_rows(steps), 1 << log_n
    assert len(rows) <= n
    side = np.zeros((7, n), dtype=np.uint64)
    for i in range(n):
        if i < len(rows) or (rows and not zero_filler):
            addr, pc, w = rows[i] if i < len(rows) else rows[0]
            side[:4, i], side[4, i], side[5, i], side[6, i] = addr, pc, w, int(i < len(rows))
    return side, len(rows)


def prog_table(steps, listing, log_n, beta, zero_filler=False):
    """-> (18 x n table, executed rows); listing: 7 x n"""
    n, b = 1 << log_n, int(beta) % P
    ex, count = exec_side(steps, log_n, zero_filler)
    pr = canonical(listing).reshape(7, n)
    t = np.zeros((T.NUM_PROG_COLS, n), dtype=np.uint64)
    for side, addr, pc, inst, comp, filt in ((ex, T.COL_PROG_EXEC_CODE_ADDR_RANGE, T.COL_PROG_EXEC_PC, T.COL_PROG_EXEC_INST, T.COL_PROG_EXEC_COMP_PROG,
                                              T.COL_PROG_FILTER_EXEC),
                                             (pr, T.COL_PROG_CODE_ADDR_RANGE, T.COL_PROG_PC, T.COL_PROG_INST, T.COL_PROG_COMP_PROG,
                                              T.COL_PROG_FILTER_PROG_CHUNK)):
        t[list(addr)], t[pc], t[inst], t[filt] = side[:4], side[4], side[5], side[6]
        t[comp] = [sum(int(side[k, i]) * b ** k for k in range(6)) % P for i in range(n)]
    t[T.COL_PROG_EXEC_COMP_PROG_PERM], t[T.COL_PROG_COMP_PROG_PERM] = TG.permuted_cols([int(x) for x in t[T.COL_PROG_EXEC_COMP_PROG]],
                                                                                        [int(x) for x in t[T.COL_PROG_COMP_PROG]])
    return t, count
