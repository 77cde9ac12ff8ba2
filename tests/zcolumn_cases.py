"""Inputs of the Z-column tests (tests/test_zcolumn_reference.py, tests/test_gpu_zcolumns.py): constraint-free AIR sets whose lookups
and permutation pairs have the shapes the factor kernels branch on, trace fillers that no executed table produces, and challenges
that no transcript would draw."""
import numpy as np

from olavm_amd.air.dsl import AirSet, AirTable, Col, CrossTableLookup, TableWithColumns
from tests.zcolumn_reference import P, ctl_sides, zero_factor_gamma

PSCAN_B = 2048                                   # rows per block of the product scan (kScanTile, scan.cuh)
MAXW = 0xFFFFFFFFFFFFFFFF


# ---- AIR sets: one table that is looking and looked side of its own lookups ------------------------------------------------
def narrow(big=False):
    """4 columns: two value columns, two filter columns.  Lookup A has a one-column tuple, a filtered looking side and an unfiltered
    looked side; lookup B two filtered looking sides and a filtered looked side; one permutation pair.  4 + 6 CTL Z columns and one
    permutation batch of two instances.  big (the 2^19- and 2^20-row cases): the pair and lookup A only, whose looked side then is a
    second table's, so that table 0 carries one pair of Z columns and one permutation batch."""
    t = AirTable("narrow", 4, 3)
    t.permutation_pair([(0, 1)])
    if big:
        return AirSet([t, AirTable("looked", 1, 3)], [CrossTableLookup([TableWithColumns(0, [Col.single(0)], Col.single(2))],
                                                                      TableWithColumns(1, [Col.single(0)]))])
    a = CrossTableLookup([TableWithColumns(0, [Col.single(0)], Col.single(2))], TableWithColumns(0, [Col.single(1)]))
    b = CrossTableLookup([TableWithColumns(0, [Col.single(1)], Col.single(3)), TableWithColumns(0, [Col.single(0)], Col.single(2))],
                         TableWithColumns(0, [Col.single(0)], Col.single(3)))
    return AirSet([t], [a, b])


WIDE_WORDS = 24


def wide():
    """32 columns: 24 value columns, filter columns 24..27.  Three lookups of 24-word tuples in which the table is looking and looked
    side: plain columns, linear combinations with coefficients other than 1 and non-zero constants, filters `col` and `1 - col`, an
    unfiltered looked side.  14 CTL Z columns.  Three permutation pairs of 1, 2 and 3 column pairs: with quotient_degree_factor 2
    and two challenges that is three batches of two instances."""
    t = AirTable("wide", 32, 3)
    t.permutation_pair([(0, 1)])
    t.permutation_pair([(2, 3), (4, 5)])
    t.permutation_pair([(6, 7), (8, 9), (10, 11)])
    w = WIDE_WORDS
    plain = Col.singles(range(w))
    comb = [Col.linear_combination([(k, 3 + k), ((k + 5) % w, P - 2)], 5 + k) if k % 3 else Col.single((k + 1) % w) for k in range(w)]
    bits = [Col.le_bits([(k + j) % w for j in range(3)]) if k % 2 else Col.linear_combination([(k, P - 1)], P - 1) for k in range(w)]
    one_minus = lambda c: Col.linear_combination([(c, P - 1)], 1)
    l0 = CrossTableLookup([TableWithColumns(0, plain, Col.single(24))], TableWithColumns(0, comb, one_minus(25)))
    l1 = CrossTableLookup([TableWithColumns(0, comb, one_minus(26)), TableWithColumns(0, bits, Col.single(25))], TableWithColumns(0, plain))
    l2 = CrossTableLookup([TableWithColumns(0, bits, Col.single(27))], TableWithColumns(0, comb, Col.single(24)))
    return AirSet([t], [l0, l1, l2])


def filter_columns(airset, table):
    """the trace columns the table's CTL filters read"""
    return sorted({c for t, _ in ctl_sides(airset, table, 1) if t.filter_column is not None for c, _ in t.filter_column.terms})


# ---- trace fillers -----------------------------------------------------------------------------------------------------
VALUES = ("random", "p-1", "non_canonical")
FILTERS = ("random", "ones", "zeros", "row0", "row_n-1", "row2047", "row2048")


def filter_rows(kind, n, rng):
    """one filter column; None where the kind's row does not exist at this size"""
    if kind == "random":
        return rng.integers(0, 2, size=n, dtype=np.uint64)
    if kind in ("ones", "zeros"):
        return np.full(n, int(kind == "ones"), dtype=np.uint64)
    r = {"row0": 0, "row_n-1": n - 1, "row2047": PSCAN_B - 1, "row2048": PSCAN_B}[kind]
    if r >= n:
        return None
    f = np.zeros(n, dtype=np.uint64)
    f[r] = 1
    return f


def fill(airset, table, log_n, values, filters, seed=0):
    """-> trace [ncols][2^log_n] of uint64, or None where the filter kind has no row at this size.  The columns the filters read are
    binary after reduction (so `col` and `1 - col` both are); under "non_canonical" every word is >= p: value cells cycle through
    2^64 - 1, p, p + 1 and p + random, filter cells are p and p + 1."""
    n = 1 << log_n
    rng = np.random.default_rng(9300 + 97 * log_n + seed)
    ncols = airset.tables[table].ncols
    if values == "p-1":
        tr = np.full((ncols, n), P - 1, dtype=np.uint64)
    else:
        tr = rng.integers(0, P, size=(ncols, n), dtype=np.uint64)
    if values == "non_canonical":
        small = rng.integers(0, (1 << 32) - 1, size=(ncols, n), dtype=np.uint64)        # p + small < 2^64
        kinds = (np.arange(ncols * n).reshape(ncols, n) + np.arange(ncols)[:, None]) % 4
        tr = np.choose(kinds, [np.uint64(MAXW), np.uint64(P), np.uint64(P + 1), np.uint64(P) + small]).astype(np.uint64)
    for c in filter_columns(airset, table):
        f = filter_rows(filters, n, rng)
        if f is None:
            return None
        tr[c] = f + np.uint64(P) if values == "non_canonical" else f
    return tr


# ---- challenges ----------------------------------------------------------------------------------------------------------
CHALLENGE_SETS = ("random", "first_word_only", "beta_one", "minus_ones", "non_canonical")


def challenges(name, count, seed):
    """`count` pairs (beta, gamma).  non_canonical: words >= p.  Only values below 2^32 - 1 have such a word, so these are p + the
    low halves of the random set's words, with 2^64 - 1 as the first gamma; reduce() gives the canonical words of the same values."""
    rng = np.random.default_rng(9400 + seed)
    rand = [tuple(int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)) for _ in range(count)]
    if name == "random":
        return rand
    if name == "non_canonical":
        out = [(P + b % ((1 << 32) - 1), P + g % ((1 << 32) - 1)) for b, g in rand]
        return [(out[0][0], MAXW)] + out[1:]
    return [{"first_word_only": (0, 1), "beta_one": (1, 0), "minus_ones": (P - 1, P - 1)}[name]] * count


def reduce(chs):
    return [(b % P, g % P) for b, g in chs]


def selected_rows(airset, table, tr_rows, side):
    """rows that the filter of CTL side `side` (index into ctl_sides(..., 1)) selects"""
    from tests.zcolumn_reference import Evaluated
    twc = ctl_sides(airset, table, 1)[side][0]
    return [i for i, f in enumerate(Evaluated(twc, tr_rows).filter) if f == 1]


def zero_factor_challenges(airset, table, tr_rows, side, row, seed):
    """two CTL challenges whose second makes combine() of side `side` vanish at `row`: from that row on the side's Z column under
    challenge 1 is zero, provided its filter selects the row"""
    ch = challenges("random", 2, seed)
    twc = ctl_sides(airset, table, 1)[side][0]
    return [ch[0], (ch[1][0], zero_factor_gamma(twc, tr_rows, ch[1][0], row))]
