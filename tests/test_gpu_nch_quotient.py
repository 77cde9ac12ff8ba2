"""The quotient phase at StarkConfig::num_challenges other than two, through ola_quotient at challenges, alphas and parameters the
caller chooses: every word of every chunk equals Python integers (tests/quotient_reference_nch.py, held to tests/quotient_reference.py
at two challenges by tests/test_quotient_reference_nch.py) and is canonical.

Three challenges have generated kernels (the n-ary interface of airq.cuh, printed by codegen.py): every comparison runs with the
generated kernel -- ola_air_kernels_available_cfg says it is there -- and under OLA_AIR_KERNELS=interpreter (quotient_kernel<3>):
  all twelve tables of an executed miniature program at 8 .. 256 rows, and the generators' 2-row padding tables (one workgroup of n
  threads per coset); the CPU table at 256 rows (exactly AIRQ_THREADS) and 512, the program table at 256 and 512 (two workgroups per
  coset); rows and Z columns of edge words; alphas (0, 0, 0), (1, p - 1, 0) and challenge words >= p.
The 512-row CPU table costs 2 s of integers per challenge set at three challenges (117 lookup columns): one set there.
One, four and eight challenges have no generated kernel and run quotient_kernel<1>, <4>, <8> -- eight the widest accumulator set."""
import numpy as np
import pytest

from tests import quotient_cases as QC, quotient_reference_nch as QN
from tests.test_gpu_quotient import assert_columns_equal, use_form

pytestmark = pytest.mark.gpu
P = QN.P
FORMS = ("generated", "interpreter")


@pytest.fixture(scope="module")
def backends():
    from olavm_amd.backend import Backend
    made = {}

    def get(nch):
        if nch not in made:
            made[nch] = Backend(device=0, num_challenges=nch)
            assert made[nch].air_kernels_available(QC.airset().blob(), 12) == [nch in (2, 3)] * 12
        return made[nch]
    yield get
    for b in made.values():
        b.close()


@pytest.fixture(scope="module")
def references(oracle):
    cache = {}

    def get(source, name):
        if (source, name) not in cache:
            cache[source, name] = QN.Quotient(oracle, QC.airset(), QC.NAMES.index(name), QC.valid(source)[name], QC.table_params(name))
        return cache[source, name]
    return get


def device_chunks(be, monkeypatch, table, trace_batch, zs, cs, params, n, form):
    use_form(monkeypatch, form)
    zb = be.commit(np.array(zs, dtype=np.uint64))
    try:
        pr = [int(v) + (P if cs["raw_params"] else 0) for v in params]
        return be.quotient(QC.airset().blob(), table, trace_batch, zb, cs["perm"], cs["ctl"], cs["alphas"], pr, n)
    finally:
        zb.free()


def compare(be, monkeypatch, references, source, name, sets, forms):
    s, t, nch = QC.airset(), QC.NAMES.index(name), be.num_challenges
    tab, trace = s.tables[t], QC.valid(source)[name]
    n, ref = trace.shape[1], references(source, name)
    tb = be.commit(trace)
    wrong = []
    for k, set_name in enumerate(sets):
        cs = QN.challenge_set(set_name, tab, nch, 100 * t + k)
        what = "%s of %s, %d rows, %s, %d challenges" % (name, source, n, set_name, nch)
        zs = QN.z_columns(s, t, trace, cs["perm"], cs["ctl"])
        want = ref.chunks(zs, cs["perm"], cs["ctl"], cs["alphas"])
        assert len(want) == nch * tab.quotient_degree_factor
        if set_name == "non_canonical":
            assert min([w for pair in cs["ctl"] for w in pair] + cs["alphas"]) >= P
        for form in forms:
            try:
                assert_columns_equal(device_chunks(be, monkeypatch, t, tb, zs, cs, QC.table_params(name), n, form), want, what + ", " + form)
            except AssertionError as e:
                wrong.append(str(e))
    tb.free()
    assert not wrong, "%d comparisons failed:\n" % len(wrong) + "\n".join(wrong)


SMALL = [("padding2", n) for n in QC.NAMES] + [("hash", n) for n in QC.NAMES]
LARGE = [("fib28", "cpu", ("random", "non_canonical")), ("rows512", "cpu", ("random",)), ("rows512", "program", QN.SETS)]


@pytest.mark.parametrize("source,name", SMALL, ids=str)
def test_three_challenges_every_table_both_kernel_forms(backends, monkeypatch, references, source, name):
    compare(backends(3), monkeypatch, references, source, name, QN.SETS, FORMS)


@pytest.mark.parametrize("source,name,sets", LARGE, ids=lambda x: x if isinstance(x, str) else str(len(x)))
def test_three_challenges_one_and_two_workgroups_per_coset(backends, monkeypatch, references, source, name, sets):
    assert QC.valid(source)[name].shape[1] in (256, 512) and QC.valid("hash")["program"].shape[1] == 256
    compare(backends(3), monkeypatch, references, source, name, sets, FORMS)


@pytest.mark.parametrize("values", ["random", "edge"])
@pytest.mark.parametrize("name", QC.POWER_OF_TWO_Q)
def test_three_challenges_generic_and_edge_words(backends, monkeypatch, oracle, name, values):
    """q a power of two: nothing needs to divide; rows and Z columns of p - 1, 0xFFFFFFFEFFFFFFFF and 0x00000000FFFFFFFF, 8 rows"""
    be, s, t, n = backends(3), QC.airset(), QC.NAMES.index(name), 8
    tab = s.tables[t]
    trace = QC.generic_trace(t, n, values, 3)
    zs = QC.generic_zs(tab.num_permutation_batches(3) + s.num_ctl_zs(t, 3), n, values, 50 * t + 3)
    cs = QN.challenge_set("random", tab, 3, 300 + 10 * t)
    params = [int(x) for x in np.random.default_rng(t).integers(0, P, size=tab.n_params, dtype=np.uint64)]
    want = QN.Quotient(oracle, s, t, trace, params).chunks(zs, cs["perm"], cs["ctl"], cs["alphas"])
    assert any(any(c) for c in want)
    tb = be.commit(trace)
    for form in FORMS:
        assert_columns_equal(device_chunks(be, monkeypatch, t, tb, zs, cs, params, n, form), want, "%s, %s values, %s" % (name, values, form))
    tb.free()


@pytest.mark.parametrize("nch", [1, 4, 8])
@pytest.mark.parametrize("name", QC.NAMES)
def test_counts_without_generated_kernels_run_the_interpreter(backends, monkeypatch, references, nch, name):
    compare(backends(nch), monkeypatch, references, "hash", name, ("random", "non_canonical"), ("default",))
