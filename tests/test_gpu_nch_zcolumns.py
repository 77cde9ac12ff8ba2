"""The Z-column kernels at StarkConfig::num_challenges other than two: ctl_factor_kernel<G> (a lookup side's G = num_challenges
columns as one group), perm_factor_kernel over batches that num_challenges fills differently, and the product scan, through
ola_perm_z / ola_ctl_z at challenges the caller chooses.  Every word equals Python integers (tests/zcolumn_reference.py, which takes
the challenge count).  1 is the smallest group, 3 the first count that is no multiple of the permutation batch size, 8 the widest.

Sizes as in tests/test_gpu_zcolumns.py: 2^1 (fewer rows than a thread's eight), 2^8 (one scan block), 2^12 (two blocks: totals and
apply).  At three challenges the permutation cases must contain a batch that is only partly filled and a pair whose challenges fall
into two batches; both are asserted from the reference's batch list."""
import functools

import numpy as np
import pytest

from tests import zcolumn_cases as ZC, zcolumn_reference as R
from tests.test_gpu_zcolumns import assert_columns_equal

pytestmark = pytest.mark.gpu
P = R.P


@pytest.fixture(scope="module", params=[1, 3, 8])
def be(request):
    from olavm_amd.backend import Backend
    b = Backend(device=0, num_challenges=request.param)
    yield b
    b.close()


@pytest.fixture(scope="module")
def be3():
    from olavm_amd.backend import Backend
    b = Backend(device=0, num_challenges=3)
    yield b
    b.close()


def perm_sets(name, tab, nch, seed):
    """[permutation_batch_size][num_challenges] pairs"""
    flat = ZC.challenges(name, nch * tab.quotient_degree_factor, seed)
    return [flat[nch * i:nch * (i + 1)] for i in range(tab.quotient_degree_factor)]


def check_table(be, s, table, tr, sets, what, seed):
    from olavm_amd.backend import OlaGpuError
    nch = be.num_challenges
    tab, rows = s.tables[table], R.rows(tr)
    ev = R.evaluate_sides(s, table, rows)
    shape = be.table_shape(s.blob(), table)
    assert shape["perm_zs"] == tab.num_permutation_batches(nch) == len(R.permutation_batches(tab, nch)) * bool(tab.permutation_pairs)
    assert shape["ctl_zs"] == s.num_ctl_zs(table, nch) == len(R.ctl_sides(s, table, nch))
    for name in sets:
        ctl = ZC.challenges(name, nch, seed)
        got = be.ctl_z(s.blob(), table, tr, ctl)
        assert_columns_equal(got, R.ctl_z(s, table, rows, ctl, ev), "%s, %s, %d challenges: lookup columns" % (what, name, nch))
        if name == "non_canonical":
            assert max(max(c) for c in ctl) >= P and np.array_equal(got, be.ctl_z(s.blob(), table, tr, ZC.reduce(ctl)))
        if not tab.permutation_pairs:
            continue
        perm = perm_sets(name, tab, nch, seed + 1)
        try:
            want = R.perm_z(tab, rows, perm, nch)
        except ZeroDivisionError:                           # the reference prover panics there (permutation.rs:143)
            with pytest.raises(OlaGpuError, match="Tried to invert zero"):
                be.perm_z(s.blob(), table, tr, perm)
            continue
        assert_columns_equal(be.perm_z(s.blob(), table, tr, perm), want, "%s, %s, %d challenges: permutation columns" % (what, name, nch))


@pytest.mark.parametrize("shape,log_n", [(sh, k) for sh in ("narrow", "wide") for k in (1, 8, 12)], ids=str)
def test_every_word_equals_the_integer_reference(be, shape, log_n):
    s = ZC.narrow() if shape == "narrow" else ZC.wide()
    nch, tab = be.num_challenges, s.tables[0]
    batches = R.permutation_batches(tab, nch)
    if nch == 3:
        assert any(len(b) < tab.quotient_degree_factor for b in batches), "no partly filled batch"
        where = {}
        for k, b in enumerate(batches):
            for pair, _, _ in b:
                where.setdefault(id(pair), set()).add(k)
        assert any(len(v) == 2 for v in where.values()), "no pair whose challenges fall into two batches"
    # the 24-word tuples of `wide` under eight challenges are 112 reference columns: one challenge set at the largest size
    sets = ZC.CHALLENGE_SETS if log_n < 12 else ("random", "non_canonical") if shape == "narrow" else ("random",)
    for values, filters in (("random", "random"), ("non_canonical", "ones")) if log_n < 12 else (("random", "random"),):
        tr = ZC.fill(s, 0, log_n, values, filters)
        check_table(be, s, 0, tr, sets, "%s 2^%d %s/%s" % (shape, log_n, values, filters), log_n)


@functools.lru_cache(maxsize=None)
def executed():
    from olavm_amd.air import miniexec as M, ola_tables as T
    return T.ola_stark(range_bits=4, limb_bits=2), M.instance(M.mixed_program())[0]


@pytest.mark.parametrize("table", range(12))
def test_tables_of_an_executed_program_at_three_challenges(be3, table):
    s, traces = executed()
    tr = traces[table]
    check_table(be3, s, table, tr, ("random", "non_canonical", "minus_ones"), s.tables[table].name, table)
