"""Traces whose words are not the canonical representatives, and what they cost on the link (tests/test_noncanonical_cases.py,
tests/test_gpu_noncanonical_traces.py; not collected by pytest, imports neither the backend nor torch).

The reference's trace generator itself writes words >= p: generation/memory.rs:104-112,137 stores `p - addr`, the literal word
0xFFFFFFFF00000001 for addr = 0, and GoldilocksField compares canonical values (goldilocks_field.rs:32-37), so a trace with such words
is the same trace.  shift_words() re-represents chosen words of a canonical trace as w + p; link_bytes_model() restates the staging plan
of olavm_amd/csrc/upload.h, so that a test can tell from upload_stats()["link_bytes"] that a pattern reached the path it is named for."""
import numpy as np

P = 0xFFFFFFFF00000001
# w + p < 2^64 exactly for w <= 2^32 - 2, and w + p is then the only other 64-bit word of w's residue class
ELIGIBLE_MAX = (1 << 32) - 2
FRACTION = 1.0 / 3.0
SEED = 20                                                         # of the generator the GPU module hands to every pattern
# memory table and the two columns generation/memory.rs fills with `p - x` (asserted against olavm_amd.air.ola_tables by the CPU tests)
MEMORY_TABLE = 1
COL_MEM_DIFF_ADDR_COND, COL_MEM_RC_VALUE = 22, 26

# rows of the `single` patterns: the block edges of pack_low_bytes / pack_low_halves (4096 words), the seam between the two pieces
# of a column cut in half, the first and the last word
SINGLE_ROWS = {"0": lambda n: 0, "4095": lambda n: 4095, "4096": lambda n: 4096, "n/2-1": lambda n: n // 2 - 1, "n/2": lambda n: n // 2,
               "n-1": lambda n: n - 1}
PATTERNS = ["all", "odd_columns", "even_columns", "first_half", "second_half"] + ["single(%s)" % r for r in SINGLE_ROWS] + ["zeros_to_p"]


def _third(t, rng):
    """a seeded third of the eligible words of every column, plus the first eligible word of every column that has one (no filter,
    permuted-lookup or limb column is left out, however sparse)"""
    eligible = t <= np.uint64(ELIGIBLE_MAX)
    mask = (rng.random(t.shape) < FRACTION) & eligible
    has = eligible.any(axis=1)
    first = eligible.argmax(axis=1)
    mask[np.nonzero(has)[0], first[has]] = True
    return mask


def _single(t, row):
    """one word per column: the one at `row` if eligible, else the nearest eligible one below it"""
    mask = np.zeros(t.shape, dtype=bool)
    n = t.shape[1]
    if not 0 <= row < n:                                     # a row is skipped for tables shorter than it
        return mask
    eligible = t[:, :row + 1] <= np.uint64(ELIGIBLE_MAX)
    has = eligible.any(axis=1)
    last = row - eligible[:, ::-1].argmax(axis=1)
    mask[np.nonzero(has)[0], last[has]] = True
    return mask


def shift_words(traces, pattern, rng):
    """-> (shifted_traces, masks): the words of `masks` re-represented as w + p.  `traces` are canonical 2-d uint64 arrays
    (columns x rows) and are left as they are.  Zeros are eligible and become the literal word p.
      all                        a seeded third of the eligible words of every column of every table, plus each column's first eligible word
      odd_columns, even_columns  the same third, only in columns of that parity: narrow and non-narrow columns alternate inside a chunk
      first_half, second_half    the same third, only in rows < n/2 / >= n/2
      single(row)                one word per column, at `row` (SINGLE_ROWS) or the nearest eligible row below; tables shorter than it: none
      zeros_to_p                 every zero of the memory table's DIFF_ADDR_COND and RC_VALUE columns, nothing else: the reference's case
    ("the same third": with generators of equal seed)"""
    traces = [np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
    assert all(int(t.max(initial=0)) < P for t in traces), "shift_words starts from canonical traces"
    masks = []
    for i, t in enumerate(traces):
        ncols, n = t.shape
        if pattern in ("all", "odd_columns", "even_columns", "first_half", "second_half"):
            m = _third(t, rng)                               # the same draw for the five patterns, given equal seeds
            if pattern == "odd_columns":
                m[0::2] = False
            elif pattern == "even_columns":
                m[1::2] = False
            elif pattern == "first_half":
                m[:, n // 2:] = False
            elif pattern == "second_half":
                m[:, :n // 2] = False
        elif pattern.startswith("single(") and pattern.endswith(")"):
            m = _single(t, SINGLE_ROWS[pattern[len("single("):-1]](n))
        elif pattern == "zeros_to_p":
            m = np.zeros(t.shape, dtype=bool)
            if i == MEMORY_TABLE:
                for c in (COL_MEM_DIFF_ADDR_COND, COL_MEM_RC_VALUE):
                    m[c] = t[c] == 0
        else:
            raise ValueError("unknown pattern " + repr(pattern))
        masks.append(m)
    shifted = [np.where(m, t + np.uint64(P), t) for t, m in zip(traces, masks)]
    assert sum(int(m.sum()) for m in masks) > 0, pattern
    for t, s, m in zip(traces, shifted, masks):
        assert np.array_equal(s % np.uint64(P), t) and np.array_equal(s != t, m) and (s[m] >= np.uint64(P)).all(), pattern
    return shifted, masks


def shift_parameters(params, compress):
    """-> (params, compress) with p added to every word (constraint parameters and compress challenges are small test values or
    zero: all eligible); at least one word of each changes"""
    out = []
    for words in (params, compress):
        words = [int(w) for w in words]
        assert all(w < P for w in words)
        shifted = [w + P if w <= ELIGIBLE_MAX else w for w in words]
        assert shifted != words and all(s % P == w and s < 1 << 64 for s, w in zip(shifted, words))
        out.append(shifted)
    return out[0], out[1]


def link_bytes_model(traces, piece_mb=16, solo_kb=512, pack=True, pack8=True):
    """-> (bytes that cross the link, per table a bool array: which columns are narrow in the sense of TraceUploader::column_is_narrow)
    for host tables on one rank under the staged upload: TraceUploader::plan() and copier() of olavm_amd/csrc/upload.h restated.
      a column of `piece` bytes or more is cut into row ranges of piece / 8 words, each a piece of its own;
      a column of at least `solo` bytes and at least 4096 rows is a piece of its own (only when packing is on and solo is not 0);
      smaller columns share pieces, piece / column bytes of them at a time, and travel whole;
      a piece of ONE column of 4096 rows or more costs 1 byte per word if all its words are < 2^8 (and pack8), else 4 bytes per word if
      all are < 2^32, else 8; every other piece costs 8 bytes per word;
      a column is narrow if every piece of it was packed."""
    piece, solo = piece_mb << 20, solo_kb << 10
    total, narrow = 0, []
    for t in traces:
        if isinstance(t, (list, tuple)):
            t = np.stack([np.asarray(c, dtype=np.uint64).reshape(-1) for c in t])
        t = np.asarray(t, dtype=np.uint64)
        ncols, n = t.shape
        col_bytes = n * 8
        if col_bytes >= piece:
            rows_per = piece // 8
            pieces = [(c, c + 1, r, min(rows_per, n - r)) for c in range(ncols) for r in range(0, n, rows_per)]
        else:
            is_solo = pack and solo != 0 and col_bytes >= solo and n >= 4096
            per = 1 if is_solo else max(1, piece // col_bytes)
            pieces = [(c, min(ncols, c + per), 0, n) for c in range(0, ncols, per)]
        nar = np.ones(ncols, dtype=bool)
        for c0, c1, r0, rows in pieces:
            wire = 8
            if pack and c1 - c0 == 1 and rows >= 4096:
                top = int(t[c0, r0:r0 + rows].max())
                wire = 1 if (pack8 and top < 1 << 8) else 4 if top < 1 << 32 else 8
            total += (c1 - c0) * rows * wire
            if wire == 8:
                nar[c0:c1] = False
        narrow.append(nar & pack)
    return total, narrow
