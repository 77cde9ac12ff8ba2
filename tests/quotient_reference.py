"""compute_quotient_polys and the split into chunks (prover.rs:441-480, 571-705) over an olavm_amd.air.dsl.AirSet, on Python
integers: what tests/test_gpu_quotient.py compares ola_quotient with word for word, and tests/test_quotient_reference.py pins to the
quotient caps inside the oracle prover's bytes.

For every point x = 7 * w^i of the coset 7 * <w>, w of order n * 2^qdb, in natural order: the table's constraint program on the
local and the next row (the LDE value 2^qdb places on, wrapping round), the permutation checks and the cross-table lookup checks in
eval_vanishing_poly's order, each weighted by its kind -- L_first(x) = (x^n - 1) / (n (x - 1)), L_last(x) = (x^n - 1) / (n (g x - 1)),
x - g^-1 -- and folded with alpha, acc = acc * alpha + c, per challenge; times 1 / (x^n - 1); interpolated on the coset; cut into
chunks of n coefficients, column challenge * q + k.  x, x^n, the selectors and the alpha folding come from these definitions, one
Python integer per point (numpy object arrays carry them, nothing else); the only things taken from elsewhere are the low-degree
extension of the input columns and the final coset interpolation, which go through the oracle's transforms (pinned to naive
evaluation by tests/test_oracle.py).

`mutate` names one deliberate mistake (MUTATIONS); tests/test_quotient_reference.py shows that the pin notices each."""
import numpy as np

from olavm_amd.air.dsl import (KIND_ALL, KIND_FIRST, KIND_LAST, KIND_TRANSITION, OP_ADD, OP_CONST, OP_ISZERO, OP_LOCAL, OP_MUL, OP_NEXT,
                               OP_PARAM, OP_SUB)
from tests import zcolumn_reference as Z

P = Z.P
GENERATOR = 7                                   # the coset shift, and the generator of the whole multiplicative group
TWO_ADICITY = 32
MUTATIONS = ("swapped_alphas", "zh_natural_coset_order", "selectors_exchanged", "x_minus_g", "next_row_one_domain_step")
DEGREE_MESSAGE = "Quotient has failed, the vanishing polynomial is not divisible by Z_H"


class QuotientDegreeError(ValueError):
    pass


def root_of_unity(bits):
    """the generator of the subgroup of order 2^bits that the reference's transforms use: g_32 = 7^((p - 1) / 2^32), squared down"""
    return pow(pow(GENERATOR, (P - 1) >> TWO_ADICITY, P), 1 << (TWO_ADICITY - bits), P)


def obj(xs):
    a = np.empty(len(xs), dtype=object)
    a[:] = [int(x) for x in xs]
    return a


def inverses(a):
    return obj(Z.batch_inverse([int(x) for x in a]))


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def quotient_degree_bits(tab):
    return (tab.quotient_degree_factor - 1).bit_length()


def lde(oracle, cols, blowup):
    """[column] of object arrays: the columns' values on 7 * <w>, natural order"""
    out = []
    for col in cols:
        coeffs = oracle.interpolate_poly(np.array(col, dtype=np.uint64))
        out.append(obj(oracle.evaluate_poly_with_offset(coeffs, GENERATOR, blowup).tolist()))
    return out


def lin(col, T):
    """Column::eval (cross_table_lookup.rs:87-98) at every point"""
    acc = col.constant
    for c, f in col.terms:
        acc = (acc + f * T[c]) % P
    return acc


def program_values(tab, Tl, Tn, params, npoints):
    """[(kind, values)]: the emits of the table's constraint program, in program order"""
    const = lambda v: obj([v % P] * npoints)
    val, emits = {}, []
    for it in tab.schedule():
        if it[0] == "emit":
            emits.append((it[1], val[it[2]]))
            continue
        j = it[1]
        op, a, b = tab.nodes[j]
        if op == OP_LOCAL:
            v = Tl[a]
        elif op == OP_NEXT:
            v = Tn[a]
        elif op == OP_CONST:
            v = const(int(a))
        elif op == OP_PARAM:
            v = const(int(params[a]))
        elif op == OP_ADD:
            v = (val[a] + val[b]) % P
        elif op == OP_SUB:
            v = (val[a] - val[b]) % P
        elif op == OP_MUL:
            v = val[a] * val[b] % P
        elif op == OP_ISZERO:
            v = obj([1 if x == 0 else 0 for x in val[a]])
        else:
            raise ValueError(op)
        val[j] = v
    return emits


def argument_values(airset, table, Tl, Tn, Zl, Zn, perm_challenges, ctl_challenges, npoints):
    """[(kind, values)] after the program's, in eval_vanishing_poly's order: Z(1) = 1 per permutation batch, the batches' products
    (permutation.rs:302-360), then two checks per lookup column (cross_table_lookup.rs:380-421)"""
    tab = airset.tables[table]
    const = lambda v: obj([v % P] * npoints)
    emits = []
    batches = Z.permutation_batches(tab) if tab.permutation_pairs else []
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
    lins = {}                                                        # a side's linear combinations serve both challenges

    def side(twc):
        if id(twc) not in lins:
            lins[id(twc)] = [([lin(col, T) for col in twc.columns], None if twc.filter_column is None else lin(twc.filter_column, T)) for T in (Tl, Tn)]
        return lins[id(twc)]
    for i, (twc, c) in enumerate(Z.ctl_sides(airset, table, len(ctl_challenges))):
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


class Quotient:
    """One table's trace and parameters: the points, the selectors, the trace's extension and the program's values are computed once
    and serve every set of Z columns, challenges and alphas (chunks())."""

    def __init__(self, oracle, airset, table, trace, params=None, mutate=None):
        assert mutate is None or mutate in MUTATIONS
        self.oracle, self.airset, self.table, self.mutate = oracle, airset, table, mutate
        tab = self.tab = airset.tables[table]
        tr = Z.rows(trace)
        n = self.n = len(tr[0])
        degree_bits, qdb = n.bit_length() - 1, quotient_degree_bits(tab)
        assert 1 << degree_bits == n and all(len(c) == n for c in tr)
        size, step = n << qdb, 1 << qdb
        self.size, self.step = size, step
        w, g = root_of_unity(degree_bits + qdb), root_of_unity(degree_bits)
        xs = [GENERATOR]
        for _ in range(size - 1):
            xs.append(xs[-1] * w % P)
        x = obj(xs)
        zh = obj([pow(v, n, P) - 1 for v in xs])                   # Z_H(x) = x^n - 1, non-zero off the trace domain
        lag_first = zh * inverses(n * (x - 1) % P) % P              # L_0(x)     = (x^n - 1) / (n (x - 1))
        lag_last = zh * inverses(n * (g * x - 1) % P) % P           # L_{n-1}(x) = (x^n - 1) g^(n-1) / (n (x - g^(n-1))), g^(n-1) = g^-1
        z_last = (x - pow(g, -1, P)) % P
        if mutate == "selectors_exchanged":
            lag_first, lag_last = lag_last, lag_first
        if mutate == "x_minus_g":
            z_last = (x - g) % P
        if mutate == "zh_natural_coset_order":                      # point i takes the Z_H of the coset whose index is i's, bit-reversed
            zh = obj([zh[bitrev(i % step, qdb)] for i in range(size)])
        self.zh_inv = inverses(zh)
        self.weight = {KIND_ALL: None, KIND_TRANSITION: z_last, KIND_FIRST: lag_first, KIND_LAST: lag_last}
        self.nxt = 1 if mutate == "next_row_one_domain_step" else step
        self.Tl = lde(oracle, tr, step)
        self.Tn = [np.roll(c, -self.nxt) for c in self.Tl]
        self.program = self.weighted(program_values(tab, self.Tl, self.Tn, [int(v) % P for v in (params if params is not None else [])], size))

    def weighted(self, emits):
        return [v if self.weight[k] is None else v * self.weight[k] % P for k, v in emits]

    def values(self, zs, perm_challenges, ctl_challenges, alphas):
        """-> [challenge] of object arrays: the quotient's values on 7 * <w>, natural order"""
        zc = Z.rows(zs)
        assert all(len(c) == self.n for c in zc)
        Zl = lde(self.oracle, zc, self.step)
        Zn = [np.roll(c, -self.nxt) for c in Zl]
        emits = self.program + self.weighted(argument_values(self.airset, self.table, self.Tl, self.Tn, Zl, Zn, perm_challenges, ctl_challenges, self.size))
        al = [int(a) % P for a in alphas]
        if self.mutate == "swapped_alphas":
            al = al[::-1]
        out = []
        for alpha in al:
            acc = obj([0] * self.size)
            for v in emits:                                          # ConstraintConsumer::constraint: acc = acc * alpha + c
                acc = (acc * alpha + v) % P
            out.append(acc * self.zh_inv % P)
        return out

    def chunks(self, zs, perm_challenges, ctl_challenges, alphas):
        """-> [num_challenges * q][n] coefficients, as ola_quotient lays them out; QuotientDegreeError where the reference panics
        (prover.rs:469-473)"""
        q, n = self.tab.quotient_degree_factor, self.n
        out = []
        for vals in self.values(zs, perm_challenges, ctl_challenges, alphas):
            coeffs = self.oracle.interpolate_poly_with_offset(np.array(vals.tolist(), dtype=np.uint64), GENERATOR).tolist()
            if any(coeffs[n * q:]):
                raise QuotientDegreeError(DEGREE_MESSAGE)
            out += [coeffs[k * n:(k + 1) * n] for k in range(q)]
        return out


def compute_quotient_polys(oracle, airset, table, trace, zs, perm_challenges, ctl_challenges, alphas, params=None, mutate=None):
    """trace and zs are indexable as [column][row]; words >= p mean their residues"""
    return Quotient(oracle, airset, table, trace, params, mutate).chunks(zs, perm_challenges, ctl_challenges, alphas)


def z_columns(airset, table, trace, perm_challenges, ctl_challenges):
    """the table's Z columns in the prover's order, permutation batches then lookups (tests/zcolumn_reference.py)"""
    rows = Z.rows(trace)
    perm = Z.perm_z(airset.tables[table], rows, perm_challenges) if airset.tables[table].permutation_pairs else []
    return perm + Z.ctl_z(airset, table, rows, ctl_challenges)
