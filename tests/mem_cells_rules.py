"""Memory cells as ola_generate_memory_trace (include/ola_gpu.h) takes them, and its contract restated over cells whose op is a WORD:
miniexec.memory_trace is the specification but knows its ops by name, so it cannot be given an op word that is none of the nine.
tests/test_mem_tablegen_abi.py holds `table` equal to miniexec.memory_trace wherever both apply; tests/test_gpu_mem_tablegen.py compares
the device with miniexec.memory_trace directly and uses `table` only for the op words memory_trace has no name for."""
import numpy as np

from olavm_amd.air import dump, miniexec as M, ola_tables as T, tracegen as TG
from olavm_amd.air.dsl import P

SPAN = 2**32 - 1
PROPHET = P - SPAN                     # where the prophet region (and the padding) starts; the heap region ends below it
HEAP = T.ADDR_HEAP_PTR
RANK = {T.op_mask(op): k for k, op in enumerate(dump.MEM_OPS)}
SELECTOR = {T.op_mask(op): getattr(T, "COL_MEM_S_" + op) for op in dump.MEM_OPS}


def words(cells):
    """named cells [(address, clock, op name or word, value, is_write)] -> 5 x n uint64, column-major as the entry point takes them"""
    a = np.zeros((5, len(cells)), dtype=np.uint64)
    for i, (addr, clk, op, value, is_write) in enumerate(cells):
        a[:, i] = [addr, clk, T.op_mask(op) if isinstance(op, str) else op, value, is_write]
    return a


def sort_key(cell):
    addr, clk, op, value, is_write = (int(x) % P for x in cell)
    return (addr, clk, RANK[op] if op in RANK else len(RANK) + op, value, is_write)


def table(cell_words, patch=False):
    """5 x n words (any order, words >= p allowed) -> (29 x n table, sort values, region values), as include/ola_gpu.h states it.
    patch: take the way of the op words without a name also when every op has one (tests/test_mem_tablegen_abi.py compares the two)."""
    cells = sorted(([int(x) % P for x in c] for c in np.asarray(cell_words, dtype=np.uint64).reshape(5, -1).T), key=sort_key)
    if not patch and all(c[2] in RANK for c in cells):
        name = {T.op_mask(op): op for op in dump.MEM_OPS}
        return M.memory_trace([(a, c, name[o], v, w) for a, c, o, v, w in cells])
    # an op without a name: the rows of memory_trace with that cell under another op, then its own word and no selector
    t, rc, cond = M.memory_trace([(a, c, "MLOAD", v, w) for a, c, o, v, w in cells])
    order = sorted(range(len(cells)), key=lambda i: (cells[i][0], cells[i][1], "MLOAD", cells[i][3], cells[i][4]))
    # memory_trace sorted by (address, clock, value, is_write); within one (address, clock) every derived column is the same for
    # every order, so the five copied words and the selector can be put back in the order the contract asks for
    assert [cells[i][:2] for i in order] == [c[:2] for c in cells]
    for i, (a, c, o, v, w) in enumerate(cells):
        t[T.COL_MEM_OP, i], t[T.COL_MEM_VALUE, i], t[T.COL_MEM_IS_WRITE, i] = o, v, w
        t[T.COL_MEM_S_MLOAD:T.COL_MEM_S_PROPHET + 1, i] = 0
        if o in SELECTOR:
            t[SELECTOR[o], i] = 1
    return t, rc, cond


def pattern(count, base=1):
    """memory_program's pattern: every address stored once and loaded three times, the loads in reverse order"""
    cells = [(base + i, 10 + 2 * i, "MSTORE", 1000 + i, 1) for i in range(count)]
    for rep in range(3):
        cells += [(base + i, 10 + 2 * count + (rep * count + (count - 1 - i)) * 3, "MLOAD", 1000 + i, 0) for i in range(count)]
    return cells


def hand_made():
    """name -> named cells, at the sizes where a height or a branch changes"""
    stack = [(3 + 2 * i, 5 + i, "MSTORE" if i % 2 == 0 else "MLOAD", 100 + i, int(i % 2 == 0)) for i in range(9)]
    heap = [(HEAP + 7 * i, 40 + i, "MSTORE" if i % 3 == 0 else "MLOAD", 7 + i, int(i % 3 == 0)) for i in range(9)]
    out = {"stack_%d" % k: stack[:k] for k in (0, 1, 2, 6, 7, 8, 9)}                    # 7 fills 8 rows with one padding row, 8 forces 16
    out.update({"heap_%d" % k: heap[:k] for k in (1, 2, 7, 8)})
    out["stack_then_heap"] = stack[:4] + heap[:3]                                       # the first heap row takes the boundary branch
    out["one_stack_then_heap"] = stack[:1] + heap[:6]
    out["stack_then_one_heap"] = stack[:6] + heap[:1]
    out["one_address"] = [(77, 3 * i, "MSTORE" if i == 0 else "MLOAD", 5, int(i == 0)) for i in range(11)]
    out["rising_with_gaps"] = [(10 + i * i * 1000, 1 + i, "MSTORE", i, 1) for i in range(12)]
    out["last_cell_high"] = stack[:3] + [(PROPHET - 1, 99, "MSTORE", 1, 1)]             # the padding continues one above the last heap address
    out["last_cell_low"] = [(0, 1, "MSTORE", 1, 1)]                                     # ... and from address 0: a difference of p - 2^32 + 1
    out["last_stack_cell_high"] = [(HEAP - 1, 1, "MSTORE", 1, 1), (HEAP - 1, 2, "MLOAD", 1, 0)]
    out["heap_top_and_bottom"] = [(HEAP, 1, "MSTORE", 1, 1), (PROPHET - 1, 2, "MSTORE", 2, 1), (HEAP - 1, 3, "MSTORE", 3, 1)]
    out["every_op"] = [(20 + k, 5, op, k, int(op in ("CALL", "MSTORE", "POSEIDON", "SLOAD", "TLOAD"))) for k, op in enumerate(dump.MEM_OPS)]
    return out


def ties():
    """cells that share (address, clock) and differ in op, in value, or in is_write only; op WORDS, four of them outside the nine"""
    m = T.op_mask
    return words([
        (50, 7, "TSTORE", 1, 0), (50, 7, "CALL", 9, 1), (50, 7, "RET", 5, 0), (50, 7, "POSEIDON", 5, 0), (50, 7, "MLOAD", 2, 0),      # in op
        (50, 8, "POSEIDON", 9, 0), (50, 8, "POSEIDON", 3, 1), (50, 8, "POSEIDON", 4, 0),                                             # in value
        (51, 8, "SLOAD", 6, 1), (51, 8, "SLOAD", 6, 0), (51, 8, "SLOAD", 6, 1),                                                       # in is_write (one twice)
        (52, 1, m("ADD"), 0, 0), (52, 1, 3, 9, 0), (52, 1, "TSTORE", 8, 0), (52, 1, m("ADD"), 0, 1), (52, 1, 0, 1, 0),                 # op words without a name:
        (52, 1, P - 1, 0, 0), (52, 1, "CALL", 7, 0),                                                                                 # behind the nine, by word
        (HEAP + 1, 4, "MLOAD", 6, 0), (HEAP + 1, 4, "CALL", 6, 0), (HEAP + 1, 4, "CALL", 5, 0),
    ])


def big():
    """2^12 + 3 cells: memory_program's pattern on 1000 addresses, then heap cells -- more than one workgroup, more than one block of the sort"""
    cells = pattern(1000)
    cells += [(HEAP + 3 * (i % 50), 20000 + i, "MSTORE" if i < 50 else "MLOAD", i % 50, int(i < 50)) for i in range((1 << 12) + 3 - len(cells))]
    assert len(cells) == (1 << 12) + 3
    return cells


def cmp_rows(ops):
    """2 x n operand words -> the rows tracegen.generate_cmp_trace takes: (op0, op1, gte, abs_diff, inverse, filter)"""
    rows = []
    for a, b in np.asarray(ops, dtype=np.uint64).reshape(2, -1).T:
        a, b = int(a) % P, int(b) % P
        d = abs(a - b)
        rows.append((a, b, int(a >= b), d, pow(d, P - 2, P) if d else 0, 1))
    return rows


def cmp_table(ops):
    rows = cmp_rows(ops)
    return TG.generate_cmp_trace(rows), [r[3] for r in rows]
