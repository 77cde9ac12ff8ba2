"""The generated quotient kernels for THREE challenges (olavm_amd/air/codegen.py, the n-ary interface of olavm_amd/csrc/airq.cuh:
AIRQ_PROLOGUE_N, AIRQ_EMIT_N / AIRQ_TO, AIRQ_REFOLD_N, AIRQ_EPILOGUE_N), executed on the HOST the way tests/test_codegen_host.py
executes the two-challenge print: the text of each of the twelve tables is compiled with g++ against host definitions of the macros
and evaluated at random points and at points of 0 / 1 cells; every output word equals an evaluation, in Python integers, of what the
AIR data say at three challenges -- the permutation batches of get_permutation_batches at that count (a pair's challenges in two
batches; a batch partly filled in the synthetic `wide` table of tests/zcolumn_cases.py, which runs too), three Z columns per lookup
side, three alpha weights per emit.

The two-challenge print must not have moved: it is printed without any of the n-ary macros."""
import os
import subprocess

import numpy as np
import pytest

from olavm_amd.air import codegen
from olavm_amd.air import ola_tables as T
from olavm_amd.air.dsl import KIND_ALL, KIND_FIRST, KIND_LAST, KIND_TRANSITION, OP_ADD, OP_CONST, OP_ISZERO, OP_LOCAL, OP_MUL, OP_NEXT, OP_PARAM, OP_SUB, P
from tests.test_codegen_host import col_value

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "olavm_amd", "csrc")
NCH = 3

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gl.cuh"
using namespace ola;
struct Acc160 { u64 lo, hi; u32 top; };
static inline void acc_mad(Acc160& a, u64 x, u64 w) {
    u64 plo, phi;
    mul_wide(x, w, plo, phi);
    a.lo += plo;
    phi += (a.lo < plo) ? 1ull : 0ull;
    a.hi += phi;
    a.top += (a.hi < phi) ? 1u : 0u;
}
static inline u64 acc_reduce(const Acc160& a) { return gl_sub(gl_reduce128_cc(a.lo, a.hi), (u64)a.top << 32); }
struct QuotParams { const u64 *Tl, *Tn, *Zl, *Zn, *D; u64 lag_first, lag_last, z_last; u64* out; };
#define AIRQ_PROLOGUE_N(K_, C_) constexpr int AIRQ_K = (K_); constexpr int AIRQ_NCH = (C_); const u64* D = P.D; \
    const u64 lag_first = P.lag_first, lag_last = P.lag_last, z_last = P.z_last; (void)lag_first; (void)lag_last; \
    Acc160 accA_[AIRQ_NCH] = {}, accT_[AIRQ_NCH] = {};
#define LC(c) P.Tl[c]
#define NC(c) P.Tn[c]
#define ZL(c) P.Zl[c]
#define ZN(c) P.Zn[c]
#define AIRQ_CACHE_DECL(S_) u64 cache_[S_]; for (int i_ = 0; i_ < (S_); i_++) cache_[i_] = 0xDEADBEEFDEADBEEFull
#define AIRQ_CACHE_PUT(s, v) (cache_[s] = (v))
#define CL(s) cache_[s]
#define AIRQ_SEGMENT_BARRIER_N
#define AIRQ_SEGMENT_BARRIER_CN
// the accumulator interface of airq.cuh, on the u64 forms of the multipliers (the limb forms are the device's)
#define AIRQ_LIMBS_AT(o) constexpr int AIRQ_L0 = (o); (void)AIRQ_L0
#define AIRQ_ACC Acc160
#define AIRQ_ACC_INIT(v) {(v), 0, 0}
#define AIRQ_W(s)
#define AIRQ_MAD(a, x, wi, s) acc_mad(a, x, D[wi])
#define AIRQ_ACC_REDUCE(a) acc_reduce(a)
#define AIRQ_REFOLD_N(S)
#define AIRQ_TO(S, c, i, s) acc_mad(acc##S##_[c], v_, D[8 + (c) * AIRQ_K + (i)]);
#define AIRQ_EMIT_N(mads, ...) { const u64 v_ = (__VA_ARGS__); mads }
#define AIRQ_EPILOGUE_N { const u64 zh_inv = D[0]; for (int c = 0; c < AIRQ_NCH; c++) \
    P.out[c] = gl_mul(gl_add(acc_reduce(accA_[c]), gl_mul(z_last, acc_reduce(accT_[c]))), zh_inv); }
#define AIRQ_THREADS 256
#define __global__
#define __launch_bounds__(...)
%(kernels)s
typedef void (*kern_t)(QuotParams);
static kern_t KERNELS[] = {%(names)s};
// stdin: per case "k ncols nz nd" then the words Tl, Tn, Zl, Zn, D, lag_first, lag_last, z_last; stdout: one word per challenge
int main() {
    unsigned k, ncols, nz, nd;
    while (scanf("%%u %%u %%u %%u", &k, &ncols, &nz, &nd) == 4) {
        std::vector<u64> w(2 * (size_t)ncols + 2 * (size_t)nz + nd + 3);
        for (u64& x : w) if (scanf("%%llu", &x) != 1) return 2;
        u64 out[%(nch)d] = {};
        const u64* p = w.data();
        QuotParams q;
        q.Tl = p; q.Tn = p + ncols; q.Zl = p + 2 * ncols; q.Zn = q.Zl + nz; q.D = q.Zn + nz;
        q.lag_first = q.D[nd]; q.lag_last = q.D[nd + 1]; q.z_last = q.D[nd + 2]; q.out = out;
        KERNELS[k](q);
        for (int c = 0; c < %(nch)d; c++) printf("%%llu ", out[c]);
        printf("\n");
    }
    return 0;
}
"""


def reference_point(airset, t, Tl, Tn, Zl, Zn, D, lag_first, lag_last, z_last, nch):
    """What the kernel of table t must return for one point at nch challenges, from the AIR data alone (Python integers mod p)."""
    tab = airset.tables[t]
    jobs = airset.ctl_jobs(t, nch)
    nperm = tab.num_permutation_batches(nch)
    bs = tab.quotient_degree_factor
    K = codegen.num_emits(airset, t, nch)
    d_params = 8 + nch * K
    d_perm = d_params + tab.n_params
    d_ctl = d_perm + 2 * nperm * bs
    val, emits = {}, []                                   # emits: (kind, value) in emit order
    for it in tab.schedule():
        if it[0] == "emit":
            emits.append((it[1], val[it[2]]))
            continue
        j = it[1]
        op, a, b = tab.nodes[j]
        val[j] = {OP_LOCAL: lambda: int(Tl[a]), OP_NEXT: lambda: int(Tn[a]), OP_CONST: lambda: int(a) % P, OP_PARAM: lambda: int(D[d_params + a]),
                  OP_ADD: lambda: (val[a] + val[b]) % P, OP_SUB: lambda: (val[a] - val[b]) % P, OP_MUL: lambda: val[a] * val[b] % P,
                  OP_ISZERO: lambda: 1 if val[a] == 0 else 0}[op]()
    # permutation checks: Z(1) = 1; Z(gx) * prod(rhs) = Z(x) * prod(lhs) per batch of `bs` (pair, challenge) instances
    for b in range(nperm):
        emits.append((KIND_FIRST, (int(Zl[b]) - 1) % P))
    total, inst = len(tab.permutation_pairs) * nch, 0
    for b in range(nperm):
        pl = pr = 1
        for i in range(bs):
            if inst >= total:
                break
            pair = tab.permutation_pairs[inst // nch]
            beta, gamma = int(D[d_perm + 2 * (b * bs + i)]), int(D[d_perm + 2 * (b * bs + i) + 1])
            lhs = sum(int(Tl[lc]) * pow(beta, k, P) for k, (lc, _) in enumerate(pair)) % P
            rhs = sum(int(Tl[rc]) * pow(beta, k, P) for k, (_, rc) in enumerate(pair)) % P
            pl, pr = pl * (lhs + gamma) % P, pr * (rhs + gamma) % P
            inst += 1
        emits.append((KIND_ALL, (int(Zn[b]) * pr - int(Zl[b]) * pl) % P))
    # cross-table lookups: Z(1) = select(f, combo)(1); Z(gx) = Z(x) * select(f, combo)(gx)
    off = d_ctl
    for i, twc in enumerate(jobs):
        gamma = int(D[off])
        weights = [1] + [int(D[off + 1 + k]) for k in range(1, len(twc.columns))]      # beta^0: the kernel does not read that slot
        off += 1 + len(twc.columns)
        sel = []
        for row in (Tl, Tn):
            combo = (sum(col_value(c, row) * w for c, w in zip(twc.columns, weights)) + gamma) % P
            if twc.filter_column is not None:
                f = col_value(twc.filter_column, row)
                combo = (f * combo + 1 - f) % P
            sel.append(combo)
        zl, zn = int(Zl[nperm + i]), int(Zn[nperm + i])
        emits.append((KIND_FIRST, (zl - sel[0]) % P))
        emits.append((KIND_TRANSITION, (zn - zl * sel[1]) % P))
    assert len(emits) == K
    out = []
    for c in range(nch):
        a = tr = 0
        for i, (kind, v) in enumerate(emits):
            w = int(D[8 + c * K + i])
            if kind == KIND_TRANSITION:
                tr += v * w
            else:
                a += v * {KIND_FIRST: lag_first, KIND_LAST: lag_last, KIND_ALL: 1}[kind] % P * w
        out.append((a + z_last * (tr % P)) % P * int(D[0]) % P)
    return out


@pytest.mark.parametrize("variant", ["full", "miniature", "wide"])
def test_three_challenge_kernels_on_the_host_equal_the_air_data(tmp_path, variant):
    if variant == "wide":                   # tests/zcolumn_cases.py: three permutation pairs in batches of two, 24-word lookups, no constraints
        from tests import zcolumn_cases as ZC
        airset = ZC.wide()
    else:
        airset = T.ola_stark() if variant == "full" else T.ola_stark(range_bits=4, limb_bits=2)
    nt = len(airset.tables)
    bodies, names = [], []
    for t in range(nt):
        name = "airq_host3_%d" % t
        src, K = codegen.table_kernel(airset, t, name, NCH)
        assert K == codegen.num_emits(airset, t, NCH)
        assert "AIRQ_PROLOGUE_N(%d, 3)" % K in src and "AIRQ_EPILOGUE_N" in src and "accA0" not in src and "AIRQ_EMIT_ALL(" not in src
        two, _ = codegen.table_kernel(airset, t, name, 2)
        assert not any(m in two for m in ("AIRQ_PROLOGUE_N", "AIRQ_EMIT_N", "AIRQ_TO(", "AIRQ_EPILOGUE_N"))      # the two-challenge print has not moved
        bodies.append(src)
        names.append(name)
    odd = [t for t in range(nt) if len(airset.tables[t].permutation_pairs) * NCH % airset.tables[t].quotient_degree_factor]
    assert bool(odd) == (variant == "wide"), "the synthetic table has a partly filled permutation batch at three challenges, the twelve have none"
    assert variant == "wide" or any(tab.permutation_pairs and tab.quotient_degree_factor == 2 for tab in airset.tables)      # a pair's challenges in two batches
    cpp = tmp_path / "airq_host3.cpp"
    cpp.write_text(HARNESS % {"kernels": "\n".join(bodies), "names": ", ".join(names), "nch": NCH})
    exe = str(tmp_path / "airq_host3")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wno-unknown-pragmas", "-I" + CSRC, str(cpp), "-o", exe])
    rng = np.random.default_rng(20261021)
    cases, lines = [], []
    for t in range(nt):
        tab = airset.tables[t]
        nz = tab.num_permutation_batches(NCH) + len(airset.ctl_jobs(t, NCH))
        K = codegen.num_emits(airset, t, NCH)
        nd = 8 + NCH * K + tab.n_params + 2 * tab.num_permutation_batches(NCH) * tab.quotient_degree_factor + \
            sum(1 + len(j.columns) for j in airset.ctl_jobs(t, NCH))
        for rep in range(3):
            w = rng.integers(0, P, size=2 * tab.ncols + 2 * nz + nd + 3, dtype=np.uint64)
            if rep == 2:                                   # small values: is_zero sees zeros, filters see 0 / 1
                w[:2 * tab.ncols] = rng.integers(0, 2, size=2 * tab.ncols, dtype=np.uint64)
            cases.append((t, tab.ncols, nz, nd, w))
            lines.append("%d %d %d %d\n%s" % (t, tab.ncols, nz, nd, " ".join(str(int(x)) for x in w)))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = [[int(x) for x in ln.split()] for ln in r.stdout.strip().split("\n")]
    assert len(got) == len(cases)
    for (t, ncols, nz, nd, w), g in zip(cases, got):
        Tl, Tn = w[:ncols], w[ncols:2 * ncols]
        Zl, Zn = w[2 * ncols:2 * ncols + nz], w[2 * ncols + nz:2 * ncols + 2 * nz]
        D = w[2 * ncols + 2 * nz:2 * ncols + 2 * nz + nd]
        lag_first, lag_last, z_last = (int(x) for x in w[2 * ncols + 2 * nz + nd:])
        want = reference_point(airset, t, Tl, Tn, Zl, Zn, D, lag_first, lag_last, z_last, NCH)
        assert len(g) == NCH and g == want, "table %d (%s)" % (t, airset.tables[t].name)
