"""tests/quotient_reference.py at any StarkConfig::num_challenges.  That module's argument_values and z_columns take the permutation
batches of two challenges (get_permutation_batches, permutation.rs:265-280, chunks the (pair, challenge) product, so the batches
themselves depend on the count); everything else in it -- the points, the selectors, the program's values, the alpha folding, the
interpolation and the split -- goes by the lengths of what it is handed and is used from there unchanged.  The challenge count is
len(alphas) = len(ctl_challenges) = len(perm_challenges[i]).

tests/test_quotient_reference_nch.py holds this module to quotient_reference's chunks at two challenges on all twelve tables."""
import numpy as np

from olavm_amd.air.dsl import KIND_ALL, KIND_FIRST, KIND_TRANSITION
from tests import quotient_reference as Q, zcolumn_reference as Z

P = Q.P
QuotientDegreeError, DEGREE_MESSAGE = Q.QuotientDegreeError, Q.DEGREE_MESSAGE


def argument_values(airset, table, Tl, Tn, Zl, Zn, perm_challenges, ctl_challenges, npoints):
    """[(kind, values)] after the program's, in eval_vanishing_poly's order (vanishing_poly.rs:20-45): Z(1) = 1 per permutation
    batch, the batches' products (permutation.rs:302-360), then two checks per lookup column (cross_table_lookup.rs:380-421)"""
    tab, nch = airset.tables[table], len(ctl_challenges)
    const = lambda v: Q.obj([v % P] * npoints)
    emits = []
    batches = Z.permutation_batches(tab, nch) if tab.permutation_pairs else []
    for b in range(len(batches)):
        emits.append((KIND_FIRST, (Zl[b] - 1) % P))
    for b, instances in enumerate(batches):
        pl, pr = const(1), const(1)
        for pair, s, c in instances:
            beta, gamma = Z.gp(perm_challenges[s][c])
            lhs, rhs, w = const(gamma), const(gamma), 1
            for l, r in pair:
                lhs, rhs = (lhs + w * Tl[l]) % P, (rhs + w * Tl[r]) % P
                w = w * beta % P
            pl, pr = pl * lhs % P, pr * rhs % P
        emits.append((KIND_ALL, (Zn[b] * pr - Zl[b] * pl) % P))
    lins = {}                                                        # a side's linear combinations serve every challenge

    def side(twc):
        if id(twc) not in lins:
            lins[id(twc)] = [([Q.lin(col, T) for col in twc.columns], None if twc.filter_column is None else Q.lin(twc.filter_column, T))
                             for T in (Tl, Tn)]
        return lins[id(twc)]
    for i, (twc, c) in enumerate(Z.ctl_sides(airset, table, nch)):
        beta, gamma = Z.gp(ctl_challenges[c])
        sel = []
        for cols, f in side(twc):
            combo, w = const(gamma), 1
            for v in cols:
                combo = (combo + w * v) % P
                w = w * beta % P
            sel.append(combo if f is None else (f * combo + 1 - f) % P)
        zl, zn = Zl[len(batches) + i], Zn[len(batches) + i]
        emits.append((KIND_FIRST, (zl - sel[0]) % P))
        emits.append((KIND_TRANSITION, (zn - zl * sel[1]) % P))
    return emits


class Quotient(Q.Quotient):
    """quotient_reference.Quotient (no mutations) whose chunks() takes any number of challenges"""

    def __init__(self, oracle, airset, table, trace, params=None):
        super().__init__(oracle, airset, table, trace, params)

    def values(self, zs, perm_challenges, ctl_challenges, alphas):
        nch = len(alphas)
        assert len(ctl_challenges) == nch and all(len(s) == nch for s in perm_challenges or [])
        zc = Z.rows(zs)
        assert all(len(c) == self.n for c in zc)
        Zl = Q.lde(self.oracle, zc, self.step)
        Zn = [np.roll(c, -self.nxt) for c in Zl]
        emits = self.program + self.weighted(argument_values(self.airset, self.table, self.Tl, self.Tn, Zl, Zn, perm_challenges, ctl_challenges, self.size))
        out = []
        for alpha in (int(a) % P for a in alphas):
            acc = Q.obj([0] * self.size)
            for v in emits:                                          # ConstraintConsumer::constraint: acc = acc * alpha + c
                acc = (acc * alpha + v) % P
            out.append(acc * self.zh_inv % P)
        return out


def z_columns(airset, table, trace, perm_challenges, ctl_challenges):
    """the table's Z columns in the prover's order, permutation batches then lookups (tests/zcolumn_reference.py)"""
    rows, tab, nch = Z.rows(trace), airset.tables[table], len(ctl_challenges)
    perm = Z.perm_z(tab, rows, perm_challenges, nch) if tab.permutation_pairs else []
    return perm + Z.ctl_z(airset, table, rows, ctl_challenges)


# ---- challenge sets of tests/quotient_cases.py at a given count ------------------------------------------------------------------
SETS = ("random", "alphas_zero", "alphas_one_minus_one", "non_canonical")


def challenge_set(name, tab, nch, seed):
    """-> dict(ctl = [nch] pairs, perm = [q][nch] pairs or None, alphas = [nch], raw_params: the parameters go in as word + p).
    alphas_zero: (0, ..., 0); alphas_one_minus_one: (1, p - 1, 0, ...) cut to nch; non_canonical: every word >= p."""
    from tests import zcolumn_cases as ZC
    q = tab.quotient_degree_factor
    kind = "non_canonical" if name == "non_canonical" else "random"
    ctl = ZC.challenges(kind, nch, seed)
    flat = ZC.challenges(kind, nch * q, seed + 1000)
    perm = [flat[nch * i:nch * (i + 1)] for i in range(q)] if tab.permutation_pairs else None
    rand = [a for pair in ZC.challenges("random", (nch + 1) // 2, seed + 2000) for a in pair][:nch]
    alphas = {"alphas_zero": [0] * nch, "alphas_one_minus_one": ([1, P - 1] + [0] * nch)[:nch]}.get(name, rand)
    if name == "non_canonical":
        alphas = [P + a % ((1 << 32) - 1) for a in rand[:-1]] + [ZC.MAXW]
    return dict(ctl=ctl, perm=perm, alphas=list(alphas), raw_params=name == "non_canonical")
