"""Step records: what ola_generate_cpu_trace and ola_generate_prog_trace_steps (include/ola_gpu.h) take in place of the CPU table --
per executed row the columns generation/cpu.rs:64-105 copies from a `Step` (COL_ENV_IDX .. the last register-selector column), then
filter_tape_looking; column-major STEP_WORDS x n_steps.  Everything else of the CPU table, and the executed side of the program table,
is a function of these words."""
import numpy as np

from . import ola_tables as T

STEP_FIRST_COL = T.COL_ENV_IDX
STEP_COPIED_COLS = T.COL_S_DST.stop - T.COL_ENV_IDX
STEP_WORDS = STEP_COPIED_COLS + 1


def live_rows(cpu_table):
    """Executed rows of a CPU table: the rows before the first padding row."""
    pad = np.flatnonzero(np.asarray(cpu_table)[T.COL_IS_PADDING])
    return int(pad[0]) if pad.size else int(np.asarray(cpu_table).shape[1])


def from_table(cpu_table, live_rows):
    """The step records of the first live_rows rows of a CPU table (94 x n, any generator's) -> STEP_WORDS x live_rows."""
    t = np.asarray(cpu_table, dtype=np.uint64)
    assert t.ndim == 2 and t.shape[0] == T.NUM_CPU_COLS and 0 <= live_rows <= t.shape[1]
    steps = np.empty((STEP_WORDS, live_rows), dtype=np.uint64)
    steps[:STEP_COPIED_COLS] = t[STEP_FIRST_COL:STEP_FIRST_COL + STEP_COPIED_COLS, :live_rows]
    steps[STEP_COPIED_COLS] = t[T.COL_FILTER_TAPE_LOOKING, :live_rows]
    return steps


def prog_listing(prog_table):
    """The listing side of a program table (18 x n) as the generators take it: 7 x n (code address, pc, inst, filter)."""
    t = np.asarray(prog_table, dtype=np.uint64)
    return np.ascontiguousarray(t[list(T.COL_PROG_CODE_ADDR_RANGE) + [T.COL_PROG_PC, T.COL_PROG_INST, T.COL_PROG_FILTER_PROG_CHUNK]])
