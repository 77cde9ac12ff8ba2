"""Writes the AIR-set blob of the reference's 12-table OlaStark (what `ola_prove_with_traces` takes as `airset`) to a file of
little-endian u64 words, for a host binding that embeds it.  usage: python -m olavm_amd.air.dump out.bin
python -m olavm_amd.air.dump --lookup-max-values prints the OLA_LOOKUP_MAX_VALUES line of include/ola_gpu.h."""
import sys

from . import ola_tables


def lookup_max_values():
    """the widest cross-table lookup of ola_stark(): data columns per side"""
    return max(len(c.looked_table.columns) for c in ola_tables.ola_stark().ctls)


def main(argv):
    if len(argv) > 1 and argv[1] == "--lookup-max-values":
        print("#define OLA_LOOKUP_MAX_VALUES %d" % lookup_max_values())
        return
    path = argv[1] if len(argv) > 1 else "ola_airset.bin"
    blob = ola_tables.ola_stark().blob()
    blob.astype("<u8").tofile(path)
    print("%s: %d words, %d tables, %d cross-table lookups" % (path, blob.size, int(blob[2]), int(blob[3])))


if __name__ == "__main__":
    main(sys.argv)


def columns_header():
    """C++ header with every column index / table width of olavm_amd/air/ola_tables.py (ranges as NAME_START / NAME_END),
    the opcode bit positions and the memory-region constants -- what the native trace generator
    (olavm_amd/csrc/host/tracegen.cpp) shares with the Python table descriptions.  Written at build time."""
    from . import ola_tables as T
    out = ["// generated from olavm_amd/air/ola_tables.py by olavm_amd.air.dump.columns_header() -- do not edit",
           "#pragma once", "#include <cstdint>", "namespace olacols {"]
    for name in sorted(n for n in dir(T) if n.isupper()):
        v = getattr(T, name)
        if isinstance(v, bool):
            continue
        if isinstance(v, int):
            out.append("constexpr uint64_t %s = %dull;" % (name, v % (1 << 64)))
        elif isinstance(v, range):
            out.append("constexpr uint64_t %s_START = %dull, %s_END = %dull;" % (name, v.start, name, v.stop))
    for op, sh in sorted(T.OPCODE_SHIFT.items()):
        out.append("constexpr uint32_t OP_%s = %d;" % (op, sh))
    out.append("}  // namespace olacols")
    return "\n".join(out) + "\n"


TABLEGEN_COLUMNS_H = "olavm_amd/csrc/tablegen_columns.h"


def tablegen_columns_header():
    """The checked header olavm_amd/csrc/tablegen_columns.h: column indices of the range-check, bitwise and program tables and the three
    bitwise opcode masks, for the device-side table generators in olavm_amd/csrc/tablegen.hip.  The file is committed (tablegen.hip is compiled
    before anything is generated); tests/test_tablegen_abi.py compares it with this text.  Regenerate:
        python -c "from olavm_amd.air import dump; print(dump.tablegen_columns_header(), end='')" > olavm_amd/csrc/tablegen_columns.h"""
    from . import ola_tables as T
    out = ["// generated from olavm_amd/air/ola_tables.py by olavm_amd.air.dump.tablegen_columns_header() -- do not edit",
           "#pragma once", "#include <cstdint>", "namespace olatg {"]
    wanted = lambda n: n.startswith(("RC_", "BW_")) or n in ("COL_NUM_RC", "COL_NUM_BITWISE", "NUM_PROG_COLS") or (
        n.startswith("COL_PROG_") and not n.startswith("COL_PROG_CHUNK_"))
    for name in sorted(n for n in dir(T) if n.isupper() and wanted(n)):
        v = getattr(T, name)
        if isinstance(v, bool):
            continue
        if isinstance(v, int):
            out.append("constexpr uint32_t %s = %du;" % (name, v))
        elif isinstance(v, range):
            out.append("constexpr uint32_t %s_START = %du, %s_END = %du;" % (name, v.start, name, v.stop))
    for op in ("AND", "OR", "XOR"):
        out.append("constexpr uint64_t OP_MASK_%s = %dull;" % (op, T.op_mask(op)))
    out.append("}  // namespace olatg")
    return "\n".join(out) + "\n"


TABLEGEN_CPU_COLUMNS_H = "olavm_amd/csrc/tablegen_cpu_columns.h"
CPU_STEP_WORDS = 66      # include/ola_gpu.h OLA_CPU_STEP_WORDS; olavm_amd/air/cpu_steps.py STEP_WORDS


def tablegen_cpu_columns_header():
    """The checked header olavm_amd/csrc/tablegen_cpu_columns.h: every column index of the CPU table, the bit position of every opcode
    mask and the layout of a step record, for ola_generate_cpu_trace / ola_generate_prog_trace_steps in olavm_amd/csrc/tablegen.hip (the
    program table's indices are in tablegen_columns.h).  Committed like its sibling; tests/test_cpu_tablegen_abi.py compares it with
    this text.  Regenerate:
        python -c "from olavm_amd.air import dump; print(dump.tablegen_cpu_columns_header(), end='')" > olavm_amd/csrc/tablegen_cpu_columns.h"""
    from . import ola_tables as T
    out = ["// generated from olavm_amd/air/ola_tables.py by olavm_amd.air.dump.tablegen_cpu_columns_header() -- do not edit",
           "#pragma once", "#include <cstdint>", "namespace olatgc {"]
    # cpu/columns.rs: the COL_* names that carry no other table's prefix, and IS_SCCALL_EXT_LINE
    others = ("COL_MEM_", "COL_CMP_", "COL_SCCALL_", "COL_TAPE_", "COL_PROG_", "COL_POSEIDON_", "COL_ST_", "COL_NUM_")
    cpu = [n for n in dir(T) if n.isupper() and ((n.startswith("COL_") and not n.startswith(others)) or n == "IS_SCCALL_EXT_LINE")]
    for name in sorted(cpu):
        v = getattr(T, name)
        if isinstance(v, range):
            out.append("constexpr uint32_t %s_START = %du, %s_END = %du;" % (name, v.start, name, v.stop))
        else:
            out.append("constexpr uint32_t %s = %du;" % (name, v))
    out.append("constexpr uint32_t NUM_CPU_COLS = %du;" % T.NUM_CPU_COLS)
    for op, sh in sorted(T.OPCODE_SHIFT.items()):
        out.append("constexpr uint32_t OP_SHIFT_%s = %du;" % (op, sh))
    # a step record: the columns cpu.rs copies from a Step (COL_ENV_IDX .. the last register-selector column), then filter_tape_looking
    out.append("constexpr uint32_t STEP_FIRST_COL = %du, STEP_COPIED_COLS = %du;" % (T.COL_ENV_IDX, T.COL_S_DST.stop - T.COL_ENV_IDX))
    out.append("constexpr uint32_t STEP_FILTER_TAPE_LOOKING = %du;" % (T.COL_S_DST.stop - T.COL_ENV_IDX))
    out.append("constexpr uint32_t STEP_WORDS = %du;" % CPU_STEP_WORDS)
    out.append("}  // namespace olatgc")
    return "\n".join(out) + "\n"


TABLEGEN_MEM_COLUMNS_H = "olavm_amd/csrc/tablegen_mem_columns.h"
MEM_CELL_WORDS = 5       # include/ola_gpu.h OLA_MEM_CELL_WORDS: address, clock, op, value, is_write
# the ops a memory cell can carry, in the order ties of (address, clock) sort by: alphabetical, as miniexec.memory_trace's sorted(cells)
# and enum MemOp of olavm_amd/csrc/host/tracegen.cpp have it; the rank of an op is its position here
MEM_OPS = ("CALL", "MLOAD", "MSTORE", "POSEIDON", "RET", "SLOAD", "SSTORE", "TLOAD", "TSTORE")


def tablegen_mem_columns_header():
    """The checked header olavm_amd/csrc/tablegen_mem_columns.h: the column indices of the memory and comparison tables, the start of the
    heap region and the nine op masks of a memory cell with their ranks, for ola_generate_memory_trace / ola_generate_cmp_trace in
    olavm_amd/csrc/tablegen.hip.  Committed like its siblings; tests/test_mem_tablegen_abi.py compares it with this text.  Regenerate:
        python -c "from olavm_amd.air import dump; print(dump.tablegen_mem_columns_header(), end='')" > olavm_amd/csrc/tablegen_mem_columns.h"""
    from . import ola_tables as T
    assert list(MEM_OPS) == sorted(MEM_OPS)
    out = ["// generated from olavm_amd/air/ola_tables.py by olavm_amd.air.dump.tablegen_mem_columns_header() -- do not edit",
           "#pragma once", "#include <cstdint>", "namespace olatgm {"]
    for name in sorted(n for n in dir(T) if n.startswith(("COL_MEM_", "COL_CMP_"))):
        out.append("constexpr uint32_t %s = %du;" % (name, getattr(T, name)))
    out.append("constexpr uint32_t NUM_MEM_COLS = %du, COL_NUM_CMP = %du;" % (T.NUM_MEM_COLS, T.COL_NUM_CMP))
    out.append("constexpr uint64_t ADDR_HEAP_PTR = %dull;" % T.ADDR_HEAP_PTR)
    for rank, op in enumerate(MEM_OPS):
        out.append("constexpr uint64_t MEM_OP_MASK_%s = %dull; constexpr uint32_t MEM_OP_RANK_%s = %du;" % (op, T.op_mask(op), op, rank))
    out.append("constexpr uint32_t MEM_OPS = %du, MEM_CELL_WORDS = %du;" % (len(MEM_OPS), MEM_CELL_WORDS))
    out.append("}  // namespace olatgm")
    return "\n".join(out) + "\n"


TABLEGEN_STORAGE_COLUMNS_H = "olavm_amd/csrc/tablegen_storage_columns.h"
STORAGE_ACCESS_WORDS = 14    # include/ola_gpu.h OLA_STORAGE_ACCESS_WORDS: key[4], value[4], pre_value[4], flags, psdn_row
STORAGE_DEPTH = 256          # levels of the state tree (builtins/storage/storage_access_stark.rs)


def tablegen_storage_columns_header():
    """The checked header olavm_amd/csrc/tablegen_storage_columns.h: the column indices of the storage-access table, the Poseidon table's
    column groups and the layout of an access record, for ola_generate_storage_trace / ola_generate_poseidon_table in
    olavm_amd/csrc/storage.hip.  Committed like its siblings; tests/test_storage_tablegen_abi.py compares it with this text.  Regenerate:
        python -c "from olavm_amd.air import dump; print(dump.tablegen_storage_columns_header(), end='')" > olavm_amd/csrc/tablegen_storage_columns.h"""
    from . import ola_tables as T
    out = ["// generated from olavm_amd/air/ola_tables.py by olavm_amd.air.dump.tablegen_storage_columns_header() -- do not edit",
           "#pragma once", "#include <cstdint>", "namespace olatgs {"]
    for name in sorted(n for n in dir(T) if n.startswith("COL_ST_")):
        v = getattr(T, name)
        if isinstance(v, range):
            out.append("constexpr uint32_t %s_START = %du, %s_END = %du;" % (name, v.start, name, v.stop))
        else:
            out.append("constexpr uint32_t %s = %du;" % (name, v))
    out.append("constexpr uint32_t NUM_COL_ST = %du, NUM_POSEIDON_COLS = %du;" % (T.NUM_COL_ST, T.NUM_POSEIDON_COLS))
    out.append("constexpr uint32_t STORAGE_ACCESS_WORDS = %du, STORAGE_DEPTH = %du;" % (STORAGE_ACCESS_WORDS, STORAGE_DEPTH))
    out.append("}  // namespace olatgs")
    return "\n".join(out) + "\n"


TABLEGEN_SMALL_COLUMNS_H = "olavm_amd/csrc/tablegen_small_columns.h"
TAPE_CELL_WORDS = 3          # include/ola_gpu.h OLA_TAPE_CELL_WORDS: tape address, the opcode's one-hot word, value
POSEIDON_CALL_WORDS = 5      # include/ola_gpu.h OLA_POSEIDON_CALL_WORDS: clk, src, len, dst, psdn_row


def tablegen_small_columns_header():
    """The checked header olavm_amd/csrc/tablegen_small_columns.h: the column indices of the tape, Poseidon-chunk, program-chunk and SCCALL
    tables, where the Poseidon table keeps a permutation's inputs and outputs, the two opcode masks and the layout of a tape cell and of
    a POSEIDON call record, for ola_generate_tape_trace / _poseidon_chunk_trace / _prog_chunk_trace in olavm_amd/csrc/tablegen.hip.
    Committed like its siblings; tests/test_small_tablegen_abi.py compares it with this text.  Regenerate:
        python -c "from olavm_amd.air import dump; print(dump.tablegen_small_columns_header(), end='')" > olavm_amd/csrc/tablegen_small_columns.h"""
    from . import ola_tables as T
    out = ["// generated from olavm_amd/air/ola_tables.py by olavm_amd.air.dump.tablegen_small_columns_header() -- do not edit",
           "#pragma once", "#include <cstdint>", "namespace olatgx {"]
    for name in sorted(n for n in dir(T) if n.startswith(("COL_TAPE_", "COL_POSEIDON_CHUNK_", "COL_PROG_CHUNK_", "COL_SCCALL_"))
                       or n in ("COL_POSEIDON_INPUT_RANGE", "COL_POSEIDON_OUTPUT_RANGE")):
        v = getattr(T, name)
        if isinstance(v, range):
            out.append("constexpr uint32_t %s_START = %du, %s_END = %du;" % (name, v.start, name, v.stop))
        else:
            out.append("constexpr uint32_t %s = %du;" % (name, v))
    out.append("constexpr uint32_t NUM_COL_TAPE = %du, NUM_POSEIDON_CHUNK_COLS = %du, NUM_PROG_CHUNK_COLS = %du, NUM_COL_SCCALL = %du;"
               % (T.NUM_COL_TAPE, T.NUM_POSEIDON_CHUNK_COLS, T.NUM_PROG_CHUNK_COLS, T.NUM_COL_SCCALL))
    out.append("constexpr uint32_t NUM_POSEIDON_COLS = %du;" % T.NUM_POSEIDON_COLS)
    for op in ("TLOAD", "POSEIDON"):
        out.append("constexpr uint64_t OP_MASK_%s = %dull;" % (op, T.op_mask(op)))
    out.append("constexpr uint32_t TAPE_CELL_WORDS = %du, POSEIDON_CALL_WORDS = %du;" % (TAPE_CELL_WORDS, POSEIDON_CALL_WORDS))
    out.append("}  // namespace olatgx")
    return "\n".join(out) + "\n"
