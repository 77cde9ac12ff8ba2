"""tests/zcolumn_reference.py against the CPU oracle's prover.  Z columns leave the prover only as the cap of their commitment, so the
transcript is replayed -- trace caps, lookup challenges, compact, permutation challenges -- the reference computes the columns at
those challenges, oracle.batch commits them, and the cap must be the Z cap inside the bytes of oracle.prove_with_traces: for every
table of an executed program that has no permutation argument, and for the synthetic sets of tests/zcolumn_cases.py, whose one
table is table 0, so that its permutation challenges follow the lookup challenges directly.  The permutation columns are also
compared word for word with the oracle's compute_permutation_z_polys at challenges of the caller's (oracle_permutation_z), where
the oracle refuses a zero denominator with the reference's words.  Mutations of the reference are noticed by both pins."""
import importlib.util
import os

import numpy as np
import pytest

from tests import zcolumn_cases as ZC, zcolumn_reference as R

P = R.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spans(proof):
    spec = importlib.util.spec_from_file_location("compare_with_dump", os.path.join(ROOT, "integration", "pin", "compare_with_dump.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.parse_all_proof(proof)


def z_caps(proof):
    """{table: Z cap [16][4]} out of AllProof bytes"""
    out = {}
    for name, a, b in _spans(proof):
        if "permutation_ctl_zs_cap" in name:
            out[int(name.split(":")[0].split()[1])] = np.frombuffer(proof[a:b], dtype="<u8").reshape(-1, 4)
    return out


def replay(oracle, traces):
    """the transcript up to the first prove_single_table: -> (challenger, lookup challenges)"""
    ch = oracle.challenger()
    for t in traces:
        ch.observe_cap(oracle.batch(t).cap())
    return ch, [(ch.get(), ch.get()) for _ in range(2)]


def draw_perm_challenges(ch, tab):
    ch.compact()
    return [[(ch.get(), ch.get()) for _ in range(2)] for _ in range(tab.quotient_degree_factor)]


def test_tables_without_permutation_arguments_of_an_executed_program(oracle):
    from olavm_amd.air import miniexec as M, ola_tables as T
    s = T.ola_stark(range_bits=4, limb_bits=2)
    traces, params, compress = M.instance(M.mixed_program())
    caps = z_caps(oracle.prove_with_traces(s.blob(), traces, params, compress))
    _, ctl = replay(oracle, traces)
    seen = 0
    for t, tab in enumerate(s.tables):
        if tab.permutation_pairs:
            continue
        z = R.ctl_z(s, t, R.rows(traces[t]), ctl)
        assert len(z) == s.num_ctl_zs(t) > 0
        assert np.array_equal(oracle.batch(np.array(z, dtype=np.uint64)).cap(), caps[t]), tab.name
        seen += 1
    assert seen >= 4


SYNTHETIC = [("narrow", 5, "random"), ("narrow", 5, "p-1"), ("narrow", 12, "random"), ("wide", 5, "random"), ("wide", 8, "non_canonical")]


def synthetic(name, log_n, values):
    s = ZC.narrow() if name == "narrow" else ZC.wide()
    return s, ZC.fill(s, 0, log_n, values, "random")


@pytest.fixture(scope="module")
def pinned(oracle):
    """per synthetic case: the set, the reduced trace, the transcript's challenges and the oracle prover's Z cap, computed once"""
    cache = {}

    def get(case):
        if case not in cache:
            s, tr = synthetic(*case)
            proof = oracle.prove_with_traces(s.blob(), [tr])
            ch, ctl = replay(oracle, [tr])
            cache[case] = (s, R.rows(tr), ctl, draw_perm_challenges(ch, s.tables[0]), z_caps(proof)[0])
        return cache[case]
    return get


def reference_cap(oracle, s, rows, ctl, perm, **mutation):
    z = R.perm_z(s.tables[0], rows, perm, **mutation) + R.ctl_z(s, 0, rows, ctl)
    assert len(z) == s.tables[0].num_permutation_batches() + s.num_ctl_zs(0)
    return oracle.batch(np.array(z, dtype=np.uint64)).cap()


@pytest.mark.parametrize("case", SYNTHETIC, ids=lambda c: "%s-2p%d-%s" % c)
def test_synthetic_sets_with_the_permutation_table_first(oracle, pinned, case):
    s, rows, ctl, perm, cap = pinned(case)
    assert np.array_equal(reference_cap(oracle, s, rows, ctl, perm), cap)


@pytest.mark.parametrize("name,log_n", [("narrow", 1), ("narrow", 8), ("wide", 8)])
@pytest.mark.parametrize("chal", ZC.CHALLENGE_SETS)
def test_permutation_columns_equal_the_oracles_at_caller_chosen_challenges(oracle, name, log_n, chal):
    s, tr = synthetic(name, log_n, "non_canonical" if chal == "non_canonical" else "random")
    tab = s.tables[0]
    flat = ZC.challenges(chal, 2 * tab.quotient_degree_factor, log_n)
    perm = [flat[0:2], flat[2:4]]
    want = oracle.permutation_z(s.blob(), 0, tr, perm, tab.num_permutation_batches())
    assert R.perm_z(tab, R.rows(tr), perm) == want.tolist()
    assert all(col[0] == 1 for col in want.tolist())


def test_a_changed_instance_to_challenge_mapping_is_noticed(oracle, pinned):
    """instance i of a batch takes sets[i].challenges[chal]: taking sets[0], or challenge 0, or the transposed sets[chal][i] one
    instance later, changes the cap and the words"""
    s, rows, ctl, perm, cap = pinned(("wide", 5, "random"))
    for wrong in (lambda i, c: (0, c), lambda i, c: (i, 0), lambda i, c: (c, 1 - i)):
        assert not np.array_equal(reference_cap(oracle, s, rows, ctl, perm, challenge_of=wrong), cap)
    assert np.array_equal(reference_cap(oracle, s, rows, ctl, perm, challenge_of=lambda i, c: (i, c)), cap)
    # three pairs, two challenges, batches of two: (pair 0, 0) (pair 0, 1) | (pair 1, 0) (pair 1, 1) | (pair 2, 0) (pair 2, 1)
    assert [[(len(p), i, c) for p, i, c in b] for b in R.permutation_batches(s.tables[0])] == [[(k, 0, 0), (k, 1, 1)] for k in (1, 2, 3)]


def test_an_inclusive_permutation_product_is_noticed(oracle, pinned):
    s, rows, ctl, perm, cap = pinned(("narrow", 5, "random"))
    assert not np.array_equal(reference_cap(oracle, s, rows, ctl, perm, exclusive=False), cap)
    want = oracle.permutation_z(s.blob(), 0, np.array(rows, dtype=np.uint64), perm, 1).tolist()
    assert R.perm_z(s.tables[0], rows, perm) == want and R.perm_z(s.tables[0], rows, perm, exclusive=False) != want
    # and the lookup columns are inclusive: row 0 of a side that selects row 0 already holds its factor
    tr = ZC.fill(s, 0, 5, "random", "ones")
    z = R.ctl_z(s, 0, R.rows(tr), [(1, 5), (0, 7)])
    assert z[0][0] == (int(tr[0, 0]) + 5) % P and z[1][0] == (int(tr[1, 0]) + 5) % P


@pytest.mark.parametrize("row,instance", [(0, 0), (19, 0), (31, 1)])
def test_a_zero_denominator_raises_in_the_reference_and_in_the_oracle(oracle, row, instance):
    """gamma = -(sum beta^k rhs_k(row)) for one instance of a batch: permutation.rs:143 inverts that row's denominator"""
    s, tr = synthetic("wide", 5, "random")
    tab, rows = s.tables[0], R.rows(tr)
    flat = ZC.challenges("random", 4, 77)
    perm = [flat[0:2], flat[2:4]]
    batch = 1                                                       # the pair of two column pairs; instance i uses sets[i][i]
    assert R.perm_z(tab, rows, perm) == oracle.permutation_z(s.blob(), 0, tr, perm, 3).tolist()
    beta = perm[instance][instance][0]
    perm[instance][instance] = (beta, R.zero_denominator_gamma(tab.permutation_pairs[batch], rows, beta, row))
    with pytest.raises(ZeroDivisionError, match="Tried to invert zero: permutation batch 1, row %d" % row):
        R.perm_z(tab, rows, perm)
    with pytest.raises(RuntimeError, match="Tried to invert zero: permutation batch 1, row %d" % row):
        oracle.permutation_z(s.blob(), 0, tr, perm, 3)


def test_a_non_binary_filter_raises_and_filters_select(oracle):
    s = ZC.narrow()
    tr = ZC.fill(s, 0, 4, "random", "row_n-1")
    rows = R.rows(tr)
    z = R.ctl_z(s, 0, rows, [(3, 4), (5, 6)])
    assert z[0] == [1] * 15 + [(rows[0][15] + 4) % P]            # lookup A's looking side selects the last row only
    want = 1
    for i in range(4):
        want = want * (rows[1][i] + 4) % P
    assert z[1][3] == want                                         # its looked side has no filter: every row counts
    tr[2, 7] = 2
    with pytest.raises(ValueError, match="Non-binary filter"):
        R.ctl_z(s, 0, R.rows(tr), [(3, 4), (5, 6)])
    with pytest.raises(RuntimeError, match="Non-binary filter"):
        oracle.prove_with_traces(s.blob(), [tr])
