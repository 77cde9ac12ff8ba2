"""tests/quotient_reference_nch.py against tests/quotient_reference.py where both apply: at two challenges it returns that module's
chunks, word for word, on all twelve tables of an executed miniature program (quotient_reference itself is pinned to the oracle
prover's quotient caps by tests/test_quotient_reference.py).  At 1, 3 and 8 challenges the Z columns of tests/zcolumn_reference.py
leave a quotient of the right degree on valid traces, and one changed Z cell does not: the batches and the lookup order the module
assumes at those counts are the ones the Z columns were built with."""
import pytest

from tests import quotient_cases as QC, quotient_reference as QR, quotient_reference_nch as QN


@pytest.mark.parametrize("name", QC.NAMES)
def test_two_challenges_give_the_chunks_of_quotient_reference(oracle, name):
    s, t = QC.airset(), QC.NAMES.index(name)
    tab, trace = s.tables[t], QC.valid("hash")[name]
    for k, set_name in enumerate(("random", "non_canonical")):
        cs = QC.challenge_set(set_name, tab, 100 * t + k)
        mine = QN.challenge_set(set_name, tab, 2, 100 * t + k)
        assert mine == cs                                   # the same words: the comparison below is of the modules, not of the inputs
        zs = QR.z_columns(s, t, trace, cs["perm"], cs["ctl"])
        assert QN.z_columns(s, t, trace, cs["perm"], cs["ctl"]) == zs
        want = QR.Quotient(oracle, s, t, trace, QC.table_params(name)).chunks(zs, cs["perm"], cs["ctl"], cs["alphas"])
        got = QN.Quotient(oracle, s, t, trace, QC.table_params(name)).chunks(zs, cs["perm"], cs["ctl"], cs["alphas"])
        assert got == want and len(got) == 2 * tab.quotient_degree_factor


@pytest.mark.parametrize("nch", [1, 3, 8])
def test_valid_traces_divide_at_every_count(oracle, nch):
    """the permutation table of the set (rangecheck) and a lookup-only one (cmp): valid Z columns at nch challenges leave a quotient
    of the right degree, num_challenges * q chunks; one changed Z cell does not"""
    s = QC.airset()
    for name in ("rangecheck", "cmp"):
        t = QC.NAMES.index(name)
        tab, trace = s.tables[t], QC.valid("hash")[name]
        cs = QN.challenge_set("random", tab, nch, 7 * t + nch)
        zs = QN.z_columns(s, t, trace, cs["perm"], cs["ctl"])
        assert len(zs) == tab.num_permutation_batches(nch) + s.num_ctl_zs(t, nch)
        ref = QN.Quotient(oracle, s, t, trace, QC.table_params(name))
        chunks = ref.chunks(zs, cs["perm"], cs["ctl"], cs["alphas"])
        assert len(chunks) == nch * tab.quotient_degree_factor
    # q = 3 (storage_access): a degree check exists
    t = QC.NAMES.index("storage_access")
    tab, trace = s.tables[t], QC.valid("hash")["storage_access"]
    cs = QN.challenge_set("random", tab, nch, 99)
    zs = QN.z_columns(s, t, trace, cs["perm"], cs["ctl"])
    ref = QN.Quotient(oracle, s, t, trace)
    assert len(ref.chunks(zs, cs["perm"], cs["ctl"], cs["alphas"])) == 3 * nch
    bad = [list(c) for c in zs]
    bad[-1][3] = (bad[-1][3] + 1) % QN.P
    with pytest.raises(QN.QuotientDegreeError):
        ref.chunks(bad, cs["perm"], cs["ctl"], cs["alphas"])
