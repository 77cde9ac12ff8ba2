"""Shared cases of the transform matrix (tests/test_gpu_transform_matrix.py, tests/alt_path_child.py): the pass plans of the
large transforms restated, input columns that sit on the limits of the T-form passes, and one runner that compares an operation of
`ola_ntt_batch` with the CPU oracle word for word.  No GPU is needed to import this module and pytest does not collect it."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests.oracle_lib import EDGE, P, rand_field

# the operations of include/ola_gpu.h (restated: this module does not import the backend)
OLA_NTT_EVALUATE, OLA_NTT_INTERPOLATE, OLA_NTT_COSET_LDE, OLA_NTT_COSET_INTERPOLATE, OLA_NTT_COSET_LDE_LEAF_ORDER = 0, 1, 2, 3, 4

SIZES = (14, 15, 16, 17, 18)
SHIFTS = (7, 49)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
# strided / bit-reversed closing / natural-order closing pass: the MODE template argument of the pass kernels
STRIDED, BITREV_LAST, NATURAL_LAST = 0, 1, 2


def pass_plan(L):
    """Pass widths of a 2^L transform, the first pass taking the top index bits: ntt2_run_group's P = ceil(L / 8) passes of
    split_even(L, P) reversed, so that the closing pass is the widest."""
    parts = (L + 7) // 8
    widths, total = [], L
    for i in range(parts):
        k = (total + (parts - i) - 1) // (parts - i)
        widths.append(k)
        total -= k
    return widths[::-1]


def pass_bits(L):
    """[(lo, R)] per pass of pass_plan(L): the pass transforms index bits [lo, lo + R)."""
    out, lo = [], L
    for R in pass_plan(L):
        lo -= R
        out.append((lo, R))
    return out


def operations(L):
    """The matrix' operations at size 2^L (the blow-ups other than 8 are run at the smallest size only)."""
    ops = ["evaluate", "interpolate", "coset_evaluate", "coset_interpolate", "lde8"]
    return ops + ["lde_rates"] if L == 14 else ops


def predicted_kernels(L, op):
    """The <R, MODE, INV, CB, LM> instantiations of ntt2t_pass_kernel that ntt2_run_group launches for `op` at 2^L, under the
    names ola_gpu_ntt_pass_times reports.  A strided pass multiplies what it loads (LM = 1) when it is not the first pass or
    when the transform has a coset pre-scale; coset interpolation is a plain inverse transform followed by scale_powers_kernel,
    so an inverse first pass never does.  The closing pass (LM = 2) writes natural order except for the leaf-order LDE, which
    the natural-order LDE of a blow-up above 1 runs too (followed by a row permutation).  run_case also inverts the forward
    transform in the two inverse cases, so these include the forward transform's kernels."""
    if op == "interpolate":
        return _kernels(L, op) | _kernels(L, "evaluate")
    if op == "coset_interpolate":
        return _kernels(L, op) | _kernels(L, "coset_evaluate")
    return _kernels(L, op)


def _kernels(L, op):
    inverse = op in ("interpolate", "coset_interpolate")
    prescale = op in ("coset_evaluate", "lde8", "lde_rates")
    closing = BITREV_LAST if op in ("lde8", "lde_rates") else NATURAL_LAST
    plan, out = pass_plan(L), set()
    for i, R in enumerate(plan):
        if i == len(plan) - 1:
            mode, lm = closing, 2
        else:
            mode, lm = STRIDED, (1 if (i > 0 or prescale) else 0)
        out.add("ntt2t_pass_kernel<%d,%d,%s,8,%d>" % (R, mode, "true" if inverse else "false", lm))
    return out


def canon(a):
    """Canonical representative of every word."""
    a = np.asarray(a, dtype=np.uint64)
    return np.where(a >= np.uint64(P), a - np.uint64(P), a)


@functools.lru_cache(maxsize=None)
def bitrev_perm(bits):
    r = np.zeros(1 << bits, dtype=np.int64)
    for b in range(bits):
        r |= ((np.arange(1 << bits, dtype=np.int64) >> b) & 1) << (bits - 1 - b)
    return r


def stress_columns(L, rng):
    """11 columns of 2^L words (one full column block of 8 and a block of 3):
      (a) every word 2^64 - 1;  (b) every word p - 1;
      (c) for every pass of pass_plan(L), for the lowest and the highest index bit b the pass transforms: word j is 2^64 - 1 where
          bit b of j is set and 0 elsewhere, so that every butterfly of that level takes the largest difference (4 or 6 columns);
      (d) EDGE tiled;  (e) random words in [p, 2^64);  (f) random canonical columns up to 11."""
    n = 1 << L
    j = np.arange(n, dtype=np.uint64)
    cols = [np.full(n, ALL_ONES, dtype=np.uint64), np.full(n, P - 1, dtype=np.uint64)]
    for lo, R in pass_bits(L):
        for b in (lo, lo + R - 1):
            cols.append(np.where((j >> np.uint64(b)) & np.uint64(1), ALL_ONES, np.uint64(0)).astype(np.uint64))
    cols.append(np.resize(EDGE, n))
    cols.append(rng.integers(P, 1 << 64, size=n, dtype=np.uint64, endpoint=False))
    while len(cols) < 11:
        cols.append(rand_field(rng, n))
    return np.stack(cols)


def stress_rng(L):
    return np.random.default_rng(7100 + L)


# ------------------------------------------------------------------------------------------------ the oracle side
def reference(oracle, op, L, cols, shifts=SHIFTS, blowups=None):
    """What the oracle computes for `op` on every column: {(key): array of the shape of the device's output}.  Keys are
    (operation name, parameter) of the device calls run_case makes."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    want = {}

    def per_column(f):      # the oracle's transforms keep no state and ctypes releases the interpreter lock: columns in parallel
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            return np.stack(list(ex.map(f, cols)))
    if op == "evaluate":
        want[("evaluate", None)] = per_column(lambda c: oracle.evaluate_poly(c))
    elif op == "interpolate":
        want[("interpolate", None)] = per_column(lambda c: oracle.interpolate_poly(c))
    elif op == "coset_evaluate":
        for s in shifts:
            want[("coset_lde", s)] = per_column(lambda c: oracle.evaluate_poly_with_offset(c, s, 1))
    elif op == "coset_interpolate":
        for s in shifts:
            want[("coset_interpolate", s)] = per_column(lambda c: oracle.interpolate_poly_with_offset(c, s))
    elif op in ("lde8", "lde_rates"):
        for r in (blowups if blowups is not None else ((3,) if op == "lde8" else (1, 2, 4))):
            want[("coset_lde", r)] = per_column(lambda c: oracle.evaluate_poly_with_offset(c, 7, 1 << r))
    else:
        raise ValueError("unknown operation %r" % (op,))
    return want


def _diff(found, name, L, got, want):
    """Append (operation, L, column, first differing index) for every column of `got` that differs from `want`, and
    (operation + ' word >= p', ...) for every column that holds a non-canonical word."""
    assert got.shape == want.shape, (name, got.shape, want.shape)
    for c in range(got.shape[0]):
        bad = np.flatnonzero(got[c] != want[c])
        if bad.size:
            found.append((name, L, c, int(bad[0])))
        big = np.flatnonzero(got[c] >= np.uint64(P))
        if big.size:
            found.append((name + " word >= p", L, c, int(big[0])))


def run_case(be, oracle, op, L, cols, want=None, shifts=SHIFTS, blowups=None):
    """Run `op` of the matrix on `cols` (shape (columns, 2^L)) through ola_ntt_batch and compare every word of every column with
    the oracle.  -> the mismatches as (operation, L, column, first differing index); every output word must also be < p."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    assert cols.shape[1] == 1 << L
    if want is None:
        want = reference(oracle, op, L, cols, shifts, blowups)
    found = []
    if op == "evaluate":
        _diff(found, "evaluate", L, be.ntt(OLA_NTT_EVALUATE, cols), want[("evaluate", None)])
    elif op == "interpolate":
        _diff(found, "interpolate", L, be.ntt(OLA_NTT_INTERPOLATE, cols), want[("interpolate", None)])
        # ... and it inverts evaluate (whose own words the "evaluate" case compares)
        back = be.ntt(OLA_NTT_INTERPOLATE, be.ntt(OLA_NTT_EVALUATE, cols))
        _diff(found, "interpolate(evaluate)", L, back, canon(cols))
    elif op == "coset_evaluate":
        for s in shifts:
            _diff(found, "coset_lde shift %d blowup_log 0" % s, L, be.ntt(OLA_NTT_COSET_LDE, cols, shift=s, blowup_log=0), want[("coset_lde", s)])
    elif op == "coset_interpolate":
        for s in shifts:
            _diff(found, "coset_interpolate shift %d" % s, L, be.ntt(OLA_NTT_COSET_INTERPOLATE, cols, shift=s), want[("coset_interpolate", s)])
            back = be.ntt(OLA_NTT_COSET_INTERPOLATE, be.ntt(OLA_NTT_COSET_LDE, cols, shift=s, blowup_log=0), shift=s)
            _diff(found, "coset_interpolate(coset_lde) shift %d" % s, L, back, canon(cols))
    else:
        for (_, r), w in sorted(want.items()):
            _diff(found, "coset_lde blowup_log %d" % r, L, be.ntt(OLA_NTT_COSET_LDE, cols, shift=7, blowup_log=r), w)
            leaf = be.ntt(OLA_NTT_COSET_LDE_LEAF_ORDER, cols, shift=7, blowup_log=r)
            _diff(found, "coset_lde_leaf_order blowup_log %d" % r, L, leaf, w[:, bitrev_perm(L + r)])
    return found
