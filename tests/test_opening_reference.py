"""tests/opening_reference.py against the CPU oracle's prover: at 2^12 and 2^15 rows the reference's opening set is the oracle's
opening bytes and its final polynomial is the oracle's, with zeta, alpha and the betas replayed from the oracle's transcript; its
field arithmetic and its impulse evaluations against closed forms."""
import struct

import numpy as np
import pytest

from tests import opening_reference as R
from tests.oracle_lib import rand_field

P = R.P


def test_extension_arithmetic_against_closed_forms():
    assert R.ext_mul((0, 1), (0, 1)) == (7, 0)
    assert R.ext_mul((P - 1, P - 1), (P - 1, P - 1)) == (8, 2)                     # (1 + X)^2 = 8 + 2X
    assert R.ext_pow((0, 1), 10) == (7 ** 5, 0)
    assert R.ext_pow((3, 5), P * P - 1) == (1, 0)                                   # the order of the multiplicative group
    assert R.ext((3 + P, P)) == (3, 0)
    for log_n in (3, 12, 18, 32):
        g = R.root_of_unity(log_n)
        assert pow(g, 1 << log_n, P) == 1 and pow(g, 1 << (log_n - 1), P) == P - 1
    A, B = R.powers((2, 3), 9)
    assert [(a, b) for a, b in zip(A, B)] == [R.ext_pow((2, 3), k) for k in range(9)]
    assert R.fri_arity_bits(3) == [] and R.fri_arity_bits(12) == [4, 4] and R.fri_arity_bits(15) == [4, 4, 4] and R.fri_arity_bits(18) == [4, 4, 4, 4]


def test_impulses_evaluate_to_powers_of_the_point():
    n = 1 << 9
    ks = [0, 31, 32, n - 32, n - 1]
    cols = [[int(i == k) for i in range(n)] for k in ks]
    zeta = (0x123456789ABCDEF, P - 5)
    s = R.open_set(cols[:3], cols[3:], cols[:1], 0, zeta)
    g = R.root_of_unity(9)
    zn = (zeta[0] * g % P, zeta[1] * g % P)
    assert s["local"] + s["zs_local"] == [R.ext_pow(zeta, k) for k in ks]
    assert s["next"] + s["zs_next"] == [R.ext_pow(zn, k) for k in ks]
    assert s["ctl_last"] == [pow(g, (-k) % n, P) for k in ks[3:]]
    assert s["q_local"] == [(1, 0)]
    assert R.decode_open_set(R.open_set_bytes(s)) == s


def test_division_and_fold_on_a_small_polynomial():
    # C = 1 + 2X + 3X^2 + 4X^3 at z = 2: C(z) = 49, quotient 4X^2 + 11X + 24
    qa, qb, at = R._divide_by_linear([1, 2, 3, 4], [0, 0, 0, 0], (2, 0))
    assert (qa, qb, at) == ([24, 11, 4], [0, 0, 0], (49, 0))
    c = [(k + 1, 0) for k in range(32)]
    out, length = R.fold(c, 256, (2, 0))
    assert length == 16 and out == [(sum((k + 1) << k for k in range(16)), 0), (sum((k + 17) << k for k in range(16)) % P, 0)]
    assert R.fold(c, 256, (0, 0))[0] == [(1, 0), (17, 0)] and R.fold(c, 256, (1, 0))[0] == [(136, 0), (392, 0)]


@pytest.mark.parametrize("log_n,cols,nperm", [(12, (9, 5, 4), 2), (15, (4, 2, 1), 1), (12, (1, 3, 2), 0)])
def test_reference_equals_the_oracle_prover(oracle, log_n, cols, nperm):
    rng = np.random.default_rng(4100 + log_n + cols[0])
    n = 1 << log_n
    tv, zv, qc = (rand_field(rng, (c, n)) for c in cols)
    bt, bz, bq = oracle.batch(tv), oracle.batch(zv), oracle.batch(qc, from_coeffs=True)
    ch = oracle.challenger()
    for b in (bt, bz, bq):
        ch.observe_cap(b.cap())
    mine = ch.clone()
    o_zeta, o_open, o_fri = oracle.open_and_prove(bt, bz, bq, nperm, ch)

    trace_c, zs_c, quot_c = bt.coeffs().tolist(), bz.coeffs().tolist(), qc.tolist()
    zeta = (mine.get(), mine.get())
    assert zeta == tuple(int(x) for x in o_zeta)
    s = R.open_set(trace_c, zs_c, quot_c, nperm, zeta)
    assert R.open_set_bytes(s) == o_open
    for name in ("local", "zs_local", "q_local", "next", "zs_next"):        # observe_openings in to_fri_openings order
        mine.observe(np.array(s[name], dtype=np.uint64))
    mine.observe(np.array([(x, 0) for x in s["ctl_last"]], dtype=np.uint64))
    alpha = (mine.get(), mine.get())
    # the layer caps from the head of the FRI bytes; each is observed before its beta is drawn
    (nlayers,) = struct.unpack_from("<I", o_fri, 0)
    assert nlayers == len(R.fri_arity_bits(log_n))
    at, betas, o_caps = 4, [], []
    for _ in range(nlayers):
        (k,) = struct.unpack_from("<I", o_fri, at)
        cap = np.frombuffer(o_fri, dtype="<u8", count=4 * k, offset=at + 4).reshape(k, 4)
        at += 4 + 32 * k
        mine.observe_cap(cap)
        o_caps.append(cap)
        betas.append((mine.get(), mine.get()))
    want_len = n >> (4 * nlayers)
    tail = o_fri[len(o_fri) - 8 - 4 - 16 * want_len:len(o_fri) - 8]
    assert struct.unpack_from("<I", tail, 0) == (want_len,)
    o_final = np.frombuffer(tail, dtype="<u8", offset=4).reshape(want_len, 2)
    layers = R.fri_layers(trace_c, zs_c, quot_c, nperm, zeta, alpha, betas)
    got = R.final_poly(trace_c, zs_c, quot_c, nperm, zeta, alpha, betas, layers=layers)
    assert got == [tuple(r) for r in o_final.tolist()]
    # the layers' caps: the oracle's transform and tree over the reference's folded polynomials are the prover's caps
    caps = R.layer_caps(oracle, layers)
    assert len(caps) == nlayers and all(np.array_equal(c, o) for c, o in zip(caps, o_caps))
    # the composition's values at the three points are the alpha-combinations of the openings (what the verifier recomputes)
    _, values = R.composed_quotients(trace_c, zs_c, quot_c, nperm, zeta, alpha)
    acc, a = (0, 0), (1, 0)
    for v in s["local"] + s["zs_local"] + s["q_local"]:
        t = R.ext_mul(a, v)
        acc, a = ((acc[0] + t[0]) % P, (acc[1] + t[1]) % P), R.ext_mul(a, alpha)
    assert values[0] == acc
