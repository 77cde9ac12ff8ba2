"""The Z-column kernels of olavm_amd/csrc/stark.hip -- perm_factor_kernel, ctl_factor_kernel, the three-phase product scan
(scan.cuh: field_scan_tile_kernel, field_scan_totals_kernel, field_scan_apply_kernel over gl_mul) and shift_right_kernel --
through ola_perm_z / ola_ctl_z at challenges the CALLER chooses, on tables no execution produces: every word of every Z column equals Python integers
(tests/zcolumn_reference.py, pinned to the oracle prover by tests/test_zcolumn_reference.py).  No transcript is involved.

Sizes, each the smallest at which a path exists (PSCAN_B = 2048 rows per scan block, 256 threads of eight rows):
  2^1   fewer rows than one thread's eight elements
  2^8   part of one scan block; one workgroup of the factor kernels
  2^11  exactly one full block; no totals pass
  2^12  two blocks: totals and apply, two live threads of field_scan_totals_kernel
  2^19  256 block totals, one per thread
  2^20  512 block totals, two per thread: the only size at which field_scan_totals_kernel loops
`narrow` (tests/zcolumn_cases.py) runs at every size -- at 2^19 and 2^20 with one lookup, of which it is the filtered looking side
(one pair of Z columns), and its one permutation batch --, `wide` at 2^8, 2^11 and 2^12, the twelve tables of an executed program at the sizes they have.  Up to 2^12
every trace filler meets every challenge set; at 2^19 and 2^20 a random trace meets `random` and `zero_factor` with the zero in
the last scan block.  `zero_factor` is a lookup gamma that makes one selected row's factor 0, once at a row of the first scan block
and once at a row of a later one: from that row on the column is zero, in the reference and on the device.

A combination in which a permutation denominator vanishes (cells of p - 1 under (beta, gamma) = (0, 1), cells = 0 mod p under
(1, 0)) is one the reference prover panics on, "Tried to invert zero" (permutation.rs:143); the reference here raises
ZeroDivisionError and the device must refuse with those words.

The Python reference of the 2^20-row case (one pair of lookup columns under two challenge sets, one permutation batch of two
instances) takes 6.4 s on one core of the build machine's CPU (rows() 0.5 s, the lookup's linear combinations 0.3 s, 2 x 0.9 s for
the lookup columns, 3.6 s for the permutation batch); with four lookup columns it took 10 s, hence the one pair.  The whole case,
reference included, takes 2.6 s on the MI355X machine's host."""
import struct

import numpy as np
import pytest

from tests import zcolumn_cases as ZC, zcolumn_reference as R

pytestmark = pytest.mark.gpu
P = R.P
OLA_E_INVALID_ARG = -1


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0)
    yield b
    b.close()


def perm_shape(flat, tab):
    """[permutation_batch_size][num_challenges] out of a flat list of pairs"""
    return [flat[2 * i:2 * i + 2] for i in range(tab.quotient_degree_factor)]


def assert_columns_equal(got, want, what):
    want = np.array(want, dtype=np.uint64).reshape(len(want), got.shape[1])
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        cols, rows = np.nonzero(got != want)
        first = [(int(c), int(r), int(got[c, r]), int(want[c, r])) for c, r in list(zip(cols, rows))[:4]]
        raise AssertionError("%s: %d words differ, (column, row, got, want): %s" % (what, len(cols), first))
    assert int(got.max(initial=0)) < P, what


def check_ctl(be, s, table, tr, rows, ev, ctl, what):
    got = be.ctl_z(s.blob(), table, tr, ctl)
    assert_columns_equal(got, R.ctl_z(s, table, rows, ctl, ev), what + ": lookup columns")
    return got


def check_perm(be, s, table, tr, rows, perm, what):
    """the permutation columns, or the refusal where the reference has a zero denominator"""
    from olavm_amd.backend import OlaGpuError
    tab = s.tables[table]
    try:
        want = R.perm_z(tab, rows, perm)
    except ZeroDivisionError as e:
        with pytest.raises(OlaGpuError, match="Tried to invert zero: table %d, permutation batch %s " % (table, str(e).split("batch ")[1].split(",")[0])) as err:
            be.perm_z(s.blob(), table, tr, perm)
        assert err.value.code == OLA_E_INVALID_ARG, what
        return None
    got = be.perm_z(s.blob(), table, tr, perm)
    assert_columns_equal(got, want, what + ": permutation columns")
    assert all(int(x) == 1 for x in got[:, 0])
    return got


def zero_factor_targets(s, table, rows, n, blocks):
    """[(side, row)]: for an unfiltered and a filtered side, a selected row in each of the wanted scan blocks (where the table has
    such a side and the filter selects a row there)"""
    sides = R.ctl_sides(s, table, 1)
    pick = [next((k for k, (t, _) in enumerate(sides) if (t.filter_column is None) == plain), None) for plain in (True, False)]
    out = []
    for side in [k for k in pick if k is not None]:
        sel = ZC.selected_rows(s, table, rows, side)
        for lo, hi in blocks:
            inside = [r for r in sel if lo <= r < hi]
            if inside:
                out.append((side, inside[len(inside) // 2]))
    return out


def check_zero_factor(be, s, table, tr, rows, ev, blocks, what, seed):
    n, done = len(rows[0]), 0
    sides2 = R.ctl_sides(s, table, 2)
    sides1 = R.ctl_sides(s, table, 1)
    for side, row in zero_factor_targets(s, table, rows, n, blocks):
        ctl = ZC.zero_factor_challenges(s, table, rows, side, row, seed)
        got = check_ctl(be, s, table, tr, rows, ev, ctl, "%s, zero factor of side %d at row %d" % (what, side, row))
        col = next(k for k, (t, c) in enumerate(sides2) if t is sides1[side][0] and c == 1)
        assert not got[col, row:].any(), (what, side, row)  # (rows before it may hold the same tuple: no claim about them here)
        done += 1
    return done


def run_all_sets(be, s, table, tr, what, seed):
    """every challenge set of tests/zcolumn_cases.py on one trace"""
    rows = R.rows(tr)
    ev = R.evaluate_sides(s, table, rows)
    tab, n = s.tables[table], len(rows[0])
    for name in ZC.CHALLENGE_SETS:
        ctl = ZC.challenges(name, 2, seed)
        got = check_ctl(be, s, table, tr, rows, ev, ctl, "%s, %s" % (what, name))
        perm = perm_shape(ZC.challenges(name, 2 * tab.quotient_degree_factor, seed + 1), tab) if tab.permutation_pairs else None
        gotp = check_perm(be, s, table, tr, rows, perm, "%s, %s" % (what, name)) if perm else None
        if name == "non_canonical":                       # words >= p mean their reduced values
            assert max(max(c) for c in ctl) >= P
            assert np.array_equal(got, be.ctl_z(s.blob(), table, tr, ZC.reduce(ctl)))
            if gotp is not None:
                assert np.array_equal(gotp, be.perm_z(s.blob(), table, tr, [ZC.reduce(p) for p in perm]))
    blocks = [(0, min(n, ZC.PSCAN_B))] + ([(n - ZC.PSCAN_B, n)] if n > ZC.PSCAN_B else [])
    return check_zero_factor(be, s, table, tr, rows, ev, blocks, what, seed)


FILLERS = [(v, "random") for v in ZC.VALUES] + [("random", f) for f in ZC.FILTERS[1:]] + [("non_canonical", "ones"), ("p-1", "zeros")]
SMALL = [(shape, log_n, v, f) for shape, sizes in (("narrow", (1, 8, 11, 12)), ("wide", (8, 11, 12))) for log_n in sizes for v, f in FILLERS
         if ZC.filter_rows(f, 1 << log_n, np.random.default_rng(0)) is not None]


@pytest.mark.parametrize("shape,log_n,values,filters", SMALL, ids=lambda x: str(x))
def test_every_word_equals_the_integer_reference(be, shape, log_n, values, filters):
    s = ZC.narrow() if shape == "narrow" else ZC.wide()
    tr = ZC.fill(s, 0, log_n, values, filters)
    zeros = run_all_sets(be, s, 0, tr, "%s 2^%d %s/%s" % (shape, log_n, values, filters), log_n)
    # the unfiltered side always has its rows; a filtered side too unless the filters select nothing in the block
    assert zeros >= (2 if log_n > 11 else 1)
    if filters == "ones":
        assert zeros == (4 if log_n > 11 else 2)


@pytest.mark.parametrize("log_n", [19, 20])
def test_block_totals_one_and_two_per_thread(be, log_n):
    s = ZC.narrow(big=True)
    tr = ZC.fill(s, 0, log_n, "random", "random")
    rows, n = R.rows(tr), 1 << log_n
    ev = R.evaluate_sides(s, 0, rows)
    what = "narrow (one Z pair, one batch) 2^%d" % log_n
    assert len(R.ctl_sides(s, 0)) == 2 and s.tables[0].num_permutation_batches() == 1
    check_ctl(be, s, 0, tr, rows, ev, ZC.challenges("random", 2, log_n), what)
    check_perm(be, s, 0, tr, rows, perm_shape(ZC.challenges("random", 4, log_n + 1), s.tables[0]), what)
    # the zero at a selected row in the middle of the last scan block: every block total before it is non-zero, the last one is zero
    row = min((r for r in ZC.selected_rows(s, 0, rows, 0) if r >= n - ZC.PSCAN_B), key=lambda r: abs(r - (n - ZC.PSCAN_B // 2)))
    ctl = ZC.zero_factor_challenges(s, 0, rows, 0, row, log_n)
    got = check_ctl(be, s, 0, tr, rows, ev, ctl, what + ", zero factor at row %d" % row)
    assert got[0].all() and not got[1, row:].any() and got[1, :row].all()


def executed():
    from olavm_amd.air import miniexec as M, ola_tables as T
    s = T.ola_stark(range_bits=4, limb_bits=2)
    return s, M.instance(M.mixed_program())[0]


@pytest.mark.parametrize("table", range(12))
def test_tables_of_an_executed_program(be, table):
    s, traces = executed()
    tab, tr = s.tables[table], traces[table]
    rows = R.rows(tr)
    ev = R.evaluate_sides(s, table, rows)
    shape = be.table_shape(s.blob(), table)
    assert shape["perm_zs"] == tab.num_permutation_batches() and shape["ctl_zs"] == s.num_ctl_zs(table) == len(R.ctl_sides(s, table))
    for name in ZC.CHALLENGE_SETS:
        what = "%s, %s" % (tab.name, name)
        check_ctl(be, s, table, tr, rows, ev, ZC.challenges(name, 2, table), what)
        if tab.permutation_pairs:
            check_perm(be, s, table, tr, rows, perm_shape(ZC.challenges(name, 2 * tab.quotient_degree_factor, table + 50), tab), what)
        else:                                               # no permutation argument: zero columns, whatever the challenges
            assert be.perm_z(s.blob(), table, tr, [[(1, 1), (1, 1)]] * shape["permutation_batch_size"]).shape == (0, tr.shape[1])
    check_zero_factor(be, s, table, tr, rows, ev, [(0, tr.shape[1])], tab.name, table)


def test_non_binary_filter_is_refused_and_the_context_goes_on(be):
    from olavm_amd.backend import OlaGpuError
    s = ZC.narrow()
    ctl = ZC.challenges("random", 2, 3)
    for log_n, row, word in ((8, 0, 2), (12, 2048, P - 1), (12, 4095, P + 2)):
        tr = ZC.fill(s, 0, log_n, "random", "random")
        bad = tr.copy()
        bad[2, row] = word
        with pytest.raises(OlaGpuError, match="Non-binary filter\\?") as e:
            be.ctl_z(s.blob(), 0, bad, ctl)
        assert e.value.code == OLA_E_INVALID_ARG
        rows = R.rows(tr)
        check_ctl(be, s, 0, tr, rows, None, ctl, "after a refused filter")
        check_perm(be, s, 0, tr, rows, perm_shape(ZC.challenges("random", 4, 4), s.tables[0]), "after a refused filter")


def test_perm_z_leaves_the_filters_to_ctl_z(be):
    """ola_perm_z launches no lookup kernel (the reference's compute_permutation_z_polys never looks at a filter): on a trace with a
    non-binary filter cell it returns the permutation columns of that trace, word for word; ola_ctl_z on it is still refused"""
    from olavm_amd.backend import OlaGpuError
    s = ZC.narrow()
    ctl = ZC.challenges("random", 2, 3)
    perm = perm_shape(ZC.challenges("random", 4, 4), s.tables[0])
    for log_n, row, word in ((8, 0, 2), (12, 2048, P - 1), (12, 4095, P + 2)):
        bad = ZC.fill(s, 0, log_n, "random", "random")
        bad[2, row] = word
        assert check_perm(be, s, 0, bad, R.rows(bad), perm, "non-binary filter cell at row %d of 2^%d" % (row, log_n)) is not None
        with pytest.raises(OlaGpuError, match="Non-binary filter\\?") as e:
            be.ctl_z(s.blob(), 0, bad, ctl)
        assert e.value.code == OLA_E_INVALID_ARG


def test_ctl_z_launches_no_permutation_kernel(be):
    """ola_ctl_z runs the lookup step alone: cells of p - 1, which make every permutation denominator zero under (beta, gamma) =
    (1, 1), are nothing it could meet -- it has no permutation challenges, stand-ins included"""
    from olavm_amd.backend import OlaGpuError
    s = ZC.narrow()
    tr = ZC.fill(s, 0, 8, "p-1", "random")
    rows, ctl = R.rows(tr), ZC.challenges("random", 2, 5)
    with pytest.raises(ZeroDivisionError):
        R.perm_z(s.tables[0], rows, [[(1, 1), (1, 1)]] * 2)
    check_ctl(be, s, 0, tr, rows, None, ctl, "cells of p - 1")
    with pytest.raises(OlaGpuError, match="Tried to invert zero"):            # the same challenges from the caller are refused
        be.perm_z(s.blob(), 0, tr, [[(1, 1), (1, 1)]] * 2)
    check_ctl(be, s, 0, tr, rows, None, ctl, "cells of p - 1, after the refusal")


@pytest.mark.parametrize("shape,log_n,batch,row,instance", [("narrow", 8, 0, 0, 0), ("narrow", 12, 0, 3000, 0), ("wide", 12, 1, 2047, 1),
                                                           ("wide", 8, 2, 255, 1)])
def test_zero_permutation_denominator_is_refused_and_the_context_goes_on(be, shape, log_n, batch, row, instance):
    """gamma = -(sum beta^k rhs_k(row)) for one instance of one batch: row 0, a row of the second scan block, the second instance of
    a batch.  The reference panics (permutation.rs:143); a Z column with gl_inv(0) = 0 in it must not come back as a result."""
    from olavm_amd.backend import OlaGpuError
    s = ZC.narrow() if shape == "narrow" else ZC.wide()
    tab = s.tables[0]
    tr = ZC.fill(s, 0, log_n, "random", "random")
    rows = R.rows(tr)
    good = perm_shape(ZC.challenges("random", 4, 60 + log_n), tab)
    bad = [list(x) for x in good]
    beta = bad[instance][instance][0]                      # instance i of a batch uses sets[i][i] here (two challenges, batches of two)
    bad[instance][instance] = (beta, R.zero_denominator_gamma(tab.permutation_pairs[batch], rows, beta, row))
    with pytest.raises(ZeroDivisionError, match="batch %d, row %d" % (batch, row)):
        R.perm_z(tab, rows, bad)
    with pytest.raises(OlaGpuError, match="Tried to invert zero: table 0, permutation batch %d " % batch) as e:
        be.perm_z(s.blob(), 0, tr, bad)
    assert e.value.code == OLA_E_INVALID_ARG
    check_perm(be, s, 0, tr, rows, good, "after the refusal")
    check_ctl(be, s, 0, tr, rows, None, ZC.challenges("random", 2, 61), "after the refusal")


def test_prove_single_table_takes_lookup_challenges_as_their_reduced_values(be, oracle):
    """ola_prove_single_table with ctl_challenges >= p returns the bytes of the run with the reduced words.  The trace has a selected
    row whose tuple value is p - 1, and gamma is 2^64 - 1: unreduced, gl_add(p - 1, 2^64 - 1) leaves the word p + 2^32 - 3 = 2^64 - 2
    in the factor column, outside gl_add's contract.  (Before the words were reduced on entry the bytes came out the same all the
    same: the word has the right residue and the scan's first gl_mul reduces any 64-bit word.  This pins the behaviour, not that
    accident.)  The Z cap inside the bytes is the commitment of the reference's columns."""
    from olavm_amd.backend import Challenger
    s = ZC.narrow()
    blob, tab = s.blob(), s.tables[0]
    tr = ZC.fill(s, 0, 5, "random", "random")
    tr[0, 9], tr[2, 9] = P - 1, 1                          # lookup A's looking side selects row 9, tuple value p - 1
    tr[1, 11] = P - 1                                      # and its unfiltered looked side has one too
    raw = [(P + 3, ZC.MAXW), (ZC.MAXW - 5, P)]
    batch = be.commit(tr)
    ch0 = Challenger()
    ch0.observe(batch.cap())
    ch_raw, ch_red, ch_ref = ch0.clone(), ch0.clone(), ch0.clone()
    got_raw = be.prove_single_table(blob, 0, tr, batch, raw, [], ch_raw)
    got_red = be.prove_single_table(blob, 0, tr, batch, ZC.reduce(raw), [], ch_red)
    batch.free()
    # the reference's Z columns at the reduced words, committed by the oracle
    ch_ref.compact()
    perm = [[(ch_ref.get(), ch_ref.get()) for _ in range(2)] for _ in range(tab.quotient_degree_factor)]
    rows = R.rows(tr)
    z = R.perm_z(tab, rows, perm) + R.ctl_z(s, 0, rows, raw)
    want_cap = oracle.batch(np.array(z, dtype=np.uint64)).cap()
    (k,) = struct.unpack_from("<I", got_red, 0)
    at = 4 + 32 * k
    (kz,) = struct.unpack_from("<I", got_red, at)
    assert np.array_equal(np.frombuffer(got_red, dtype="<u8", count=4 * kz, offset=at + 4).reshape(kz, 4), want_cap)
    assert got_raw == got_red
    assert np.array_equal(ch_raw.state(), ch_red.state())
