"""Every pass plan of the large transforms against the oracle, at the smallest size that has it.

Transforms of 2^14 points and more run `ceil(L / 8)` passes whose widths depend on L (tests/transform_cases.py: pass_plan), and
each (width, position, direction, coset or not) is its own instantiation of ntt2t_pass_kernel.  The matrix below runs every
operation of ola_ntt_batch at every L of 14..18 -- 7+7, 7+8, 8+8, 5+6+6, 6+6+6: every width and every plan shape there is -- on
eleven columns (one full column block of a strided pass and a block of three) that sit on the limits of the T-form limb
arithmetic, and compares every word with the oracle.  The last test of the module checks, from the launches
ola_gpu_ntt_pass_times recorded, that the matrix reached exactly the instantiations the planner's rules predict."""
import numpy as np
import pytest

from tests import transform_cases as TC
from tests.oracle_lib import rand_field

pytestmark = pytest.mark.gpu

F, T = "false", "true"
# <R, MODE, INV, CB, LM> per (L, kind of transform), written out from ntt2_run_group's rules (MODE 0 strided, 1 bit-reversed
# closing, 2 natural-order closing; LM 0 no load multiplier, 1 table in LDS, 2 registers):
#   L   plan    plain forward              coset forward, natural out   coset forward, leaf order    inverse
#   14  7,7     <7,0,F,0> <7,2,F,2>        <7,0,F,1> <7,2,F,2>          <7,0,F,1> <7,1,F,2>          <7,0,T,0> <7,2,T,2>
#   15  7,8     <7,0,F,0> <8,2,F,2>        <7,0,F,1> <8,2,F,2>          <7,0,F,1> <8,1,F,2>          <7,0,T,0> <8,2,T,2>
#   16  8,8     <8,0,F,0> <8,2,F,2>        <8,0,F,1> <8,2,F,2>          <8,0,F,1> <8,1,F,2>          <8,0,T,0> <8,2,T,2>
#   17  5,6,6   <5,0,F,0> <6,0,F,1> <6,2,F,2>   <5,0,F,1> <6,0,F,1> <6,2,F,2>   <5,0,F,1> <6,0,F,1> <6,1,F,2>   <5,0,T,0> <6,0,T,1> <6,2,T,2>
#   18  6,6,6   <6,0,F,0> <6,0,F,1> <6,2,F,2>   <6,0,F,1> <6,2,F,2>             <6,0,F,1> <6,1,F,2>             <6,0,T,0> <6,0,T,1> <6,2,T,2>
EXPECTED_KERNELS = {"ntt2t_pass_kernel<%d,%d,%s,8,%d>" % k for k in [
    # strided first passes without a load multiplier (evaluate; interpolate and coset interpolate)
    (5, 0, F, 0), (6, 0, F, 0), (7, 0, F, 0), (8, 0, F, 0),
    (5, 0, T, 0), (6, 0, T, 0), (7, 0, T, 0), (8, 0, T, 0),
    # strided passes with the load multipliers in LDS: first passes of the coset transforms, middle passes of the three-pass sizes
    (5, 0, F, 1), (6, 0, F, 1), (7, 0, F, 1), (8, 0, F, 1),
    (6, 0, T, 1),
    # closing passes, natural order (evaluate, single-shift coset evaluate; interpolate) and leaf order (LDE)
    (6, 2, F, 2), (7, 2, F, 2), (8, 2, F, 2),
    (6, 2, T, 2), (7, 2, T, 2), (8, 2, T, 2),
    (6, 1, F, 2), (7, 1, F, 2), (8, 1, F, 2),
]}

_ledger = {}        # (L, op) -> the kernels ola_gpu_ntt_pass_times reported for that case
_shared_want = {}   # the oracle's answers that the blocking tests use again


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0)
    b.ntt_pass_times(True)
    yield b
    b.close()


def stress(L):
    return TC.stress_columns(L, TC.stress_rng(L))


def want_for(oracle, op, L):
    """The oracle's side of a matrix case on the stress columns; kept for the L = 18 cases that the blocking tests repeat."""
    if (op, L) in _shared_want:
        return _shared_want[(op, L)]
    want = TC.reference(oracle, op, L, stress(L))
    if L == 18 and op in ("evaluate", "lde8"):
        _shared_want[(op, L)] = want
    return want


def run_matrix_case(be, oracle, L, op, cols=None):
    be.ntt_pass_times()                      # forget launches of other tests
    found = TC.run_case(be, oracle, op, L, stress(L), want=want_for(oracle, op, L)) if cols is None else TC.run_case(be, oracle, op, L, cols)
    _ledger.setdefault((L, op), set()).update(be.ntt_pass_times())
    return found


CASES = [(L, op) for L in TC.SIZES for op in TC.operations(L)]


@pytest.mark.parametrize("L,op", CASES, ids=["2p%d-%s" % c for c in CASES])
def test_transform_matrix_matches_oracle(be, oracle, L, op):
    found = run_matrix_case(be, oracle, L, op)
    assert not found, "(operation, L, column, first differing index): %s" % found[:12]


@pytest.mark.parametrize("ncols", [8, 9, 16, 17])
def test_column_blocks_every_column(be, oracle, ncols):
    """A strided pass handles eight columns per workgroup and stops at the batch's last column: exactly one block, one block
    and one column, two blocks, two blocks and one column; evaluate (natural order) and the x8 LDE (leaf order, and the
    natural order made from it)."""
    cols = rand_field(np.random.default_rng(8000 + ncols), (ncols, 1 << 14))
    found = TC.run_case(be, oracle, "evaluate", 14, cols) + TC.run_case(be, oracle, "lde8", 14, cols)
    assert not found, "(operation, L, column, first differing index): %s" % found[:12]


# ------------------------------------------------------------------------------------------------ column-group blocking
def _launches(be):
    return sum(k["launches"] for k in be.ntt_pass_times().values())


def test_blocked_evaluate_two_column_groups(be, oracle, monkeypatch):
    """OLA_NTT2_GROUP_MB=1 at 2^18 (4 MiB per column with its scratch): 11 columns run as groups of 8 and 3, each group all
    three passes: 6 launches instead of 3, the same words."""
    monkeypatch.setenv("OLA_NTT2_GROUP_MB", "1")
    be.ntt_pass_times()
    found = TC.run_case(be, oracle, "evaluate", 18, stress(18), want=want_for(oracle, "evaluate", 18))
    assert _launches(be) == 3 * 2
    assert not found, found[:12]


def test_blocked_lde_column_groups_and_single_cosets(be, oracle, monkeypatch):
    """OLA_NTT2_GROUP_MB=1, leaf-order x8 LDE of 11 columns at 2^18: column groups 8 + 3, cosets one at a time: 16 groups of
    three passes."""
    from olavm_amd.backend import OLA_NTT_COSET_LDE_LEAF_ORDER
    monkeypatch.setenv("OLA_NTT2_GROUP_MB", "1")
    cols = stress(18)
    want = want_for(oracle, "lde8", 18)[("coset_lde", 3)][:, TC.bitrev_perm(21)]
    be.ntt_pass_times()
    leaf = be.ntt(OLA_NTT_COSET_LDE_LEAF_ORDER, cols, shift=7, blowup_log=3)
    assert _launches(be) == 3 * 16
    found = []
    TC._diff(found, "blocked coset_lde_leaf_order", 18, leaf, want)
    assert not found, found[:12]


def test_blocked_lde_coset_pairs(be, oracle, monkeypatch):
    """OLA_NTT2_GROUP_MB=16, leaf-order x8 LDE of 3 columns at 2^18 (6 MiB per coset): one column group, cosets in pairs:
    4 groups of three passes, each starting two cosets further into the per-coset tables."""
    from olavm_amd.backend import OLA_NTT_COSET_LDE_LEAF_ORDER
    monkeypatch.setenv("OLA_NTT2_GROUP_MB", "16")
    cols = stress(18)[:3]
    want = want_for(oracle, "lde8", 18)[("coset_lde", 3)][:3][:, TC.bitrev_perm(21)]
    be.ntt_pass_times()
    leaf = be.ntt(OLA_NTT_COSET_LDE_LEAF_ORDER, cols, shift=7, blowup_log=3)
    assert _launches(be) == 3 * 4
    found = []
    TC._diff(found, "blocked coset_lde_leaf_order", 18, leaf, want)
    assert not found, found[:12]


# ------------------------------------------------------------------------------------------------ the coverage ledger
def test_matrix_reaches_every_planned_instantiation(be, oracle):
    """The union of the pass kernels launched by the matrix is EXPECTED_KERNELS, and EXPECTED_KERNELS is what pass_plan and the
    planner's rules (transform_cases.predicted_kernels) give for 14..18 over the operations.  If this fails after a change of
    the planner (another split, another closing pass, a new template argument), the matrix above no longer runs every kernel
    the planner can choose at these sizes: extend it, then write the new set out here.

    Reachable instantiations that need L >= 20 and stay with test_gpu_parity.py::test_ntt_three_pass_sizes_match_oracle
    (2^20, 2^21), ::test_ntt_large_roundtrip_and_spot_values and test_gpu_fullsize.py: the inverse middle passes of width 7 and 8,
    <7,0,true,8,1> (6+7+7 at 2^20) and <8,0,true,8,1> (7+8+8 at 2^23).  Their forward twins run here as the first passes of the
    coset transforms at 2^14 .. 2^16.  Inverse transforms are always natural-order and never pre-scaled, width 4 is never
    planned, and a width-5 pass is never a closing pass, so nothing else is reachable."""
    predicted = set()
    for L, op in CASES:
        predicted |= TC.predicted_kernels(L, op)
    assert predicted == EXPECTED_KERNELS, "the planner's rules changed: extend the matrix and write the new set out"
    for L, op in CASES:                                  # cases deselected from this run: one random column each, still compared
        if (L, op) not in _ledger:
            assert not run_matrix_case(be, oracle, L, op, cols=rand_field(np.random.default_rng(L), (1, 1 << L)))
    for (L, op), seen in sorted(_ledger.items()):
        assert seen == TC.predicted_kernels(L, op), ("the passes of %s at 2^%d are not the planned ones" % (op, L), sorted(seen))
    reached = set().union(*_ledger.values())
    assert reached == EXPECTED_KERNELS, ("the transform matrix must be extended: not launched %s, not expected %s"
                                         % (sorted(EXPECTED_KERNELS - reached), sorted(reached - EXPECTED_KERNELS)))
