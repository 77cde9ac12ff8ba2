"""The opening phase on Python integers: what StarkOpeningSet::new opens and what prove_openings / fri_committed_trees leave as the
final polynomial, in F_p[X]/(X^2 - 7), p = 2^64 - 2^32 + 1.  No GPU, and no oracle call in the arithmetic (layer_caps alone borrows
the oracle's transform and Merkle tree, to turn this module's folded polynomials into caps): tests/test_opening_reference.py pins this
module to the CPU oracle at transcript challenges, tests/test_gpu_opening_edges.py and the `openeval` job of
tests/alt_path_child.py hold the HIP kernels to it at challenges the caller chooses.

An extension element is a pair (a, b) = a + b X of ints in [0, p).  Columns are sequences of ints (coefficients, low degree
first).  Formulas: the comments of compose_kernel, final_poly_coeffs and fold_kernel in olavm_amd/csrc/fri.hip."""
import struct
from operator import mul

import numpy as np

P = 0xFFFFFFFF00000001
W = 7                                            # X^2 = 7
POWER_OF_TWO_GENERATOR = 1753635133440165772     # of order 2^32
CFG = {"rate_bits": 3, "fri_arity_bits": 4, "fri_final_poly_bits": 5, "cap_height": 4}     # the library's defaults


# ------------------------------------------------------------------------------------------------ the field
def ext(z):
    """canonical pair of any two words"""
    return int(z[0]) % P, int(z[1]) % P


def ext_mul(x, y):
    return (x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P


def ext_pow(x, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = ext_mul(r, x)
        x = ext_mul(x, x)
        e >>= 1
    return r


def root_of_unity(log_n):
    return pow(POWER_OF_TWO_GENERATOR, 1 << (32 - log_n), P)


def powers(z, n):
    """(a-parts, b-parts) of z^0 .. z^(n-1)"""
    A, B = [0] * n, [0] * n
    a, b = 1, 0
    za, zb = z
    for k in range(n):
        A[k], B[k] = a, b
        a, b = (a * za + W * b * zb) % P, (a * zb + b * za) % P
    return A, B


def eval_columns(cols, z):
    """f(z) of every base-field column at the extension point z: a power table, then one dot product per component"""
    if not len(cols):
        return []
    A, B = powers(z, len(cols[0]))
    return [(sum(map(mul, f, A)) % P, sum(map(mul, f, B)) % P) for f in cols]


# ------------------------------------------------------------------------------------------------ StarkOpeningSet::new
def open_set(trace_c, zs_c, quot_c, nperm, zeta):
    """-> dict of the six spans: local, next, zs_local, zs_next, q_local (lists of pairs) and ctl_last (list of ints)"""
    n = len(trace_c[0])
    log_n = n.bit_length() - 1
    zeta = ext(zeta)
    g = root_of_unity(log_n)
    zeta_next = (zeta[0] * g % P, zeta[1] * g % P)
    g_inv = pow(g, P - 2, P)
    both = eval_columns(list(trace_c) + list(zs_c) + list(quot_c), zeta)
    nxt = eval_columns(list(trace_c) + list(zs_c), zeta_next)
    Wd, Z = len(trace_c), len(zs_c)
    last = eval_columns(list(zs_c)[nperm:], (g_inv, 0))
    assert all(v[1] == 0 for v in last)
    return {"local": both[:Wd], "next": nxt[:Wd], "zs_local": both[Wd:Wd + Z], "zs_next": nxt[Wd:], "ctl_last": [v[0] for v in last],
            "q_local": both[Wd + Z:]}


SPANS = ("local", "next", "zs_local", "zs_next", "ctl_last", "q_local")      # the order of OpeningSet::write


def open_set_bytes(s):
    """wire format: per span a 32-bit count, then the canonical little-endian words"""
    out = b""
    for name in SPANS:
        v = s[name]
        out += struct.pack("<I", len(v))
        for e in v:
            out += struct.pack("<Q", e) if name == "ctl_last" else struct.pack("<QQ", *e)
    return out


def decode_open_set(buf):
    """the inverse of open_set_bytes; refuses trailing bytes"""
    s, at = {}, 0
    for name in SPANS:
        (k,) = struct.unpack_from("<I", buf, at)
        at += 4
        if name == "ctl_last":
            s[name] = list(struct.unpack_from("<%dQ" % k, buf, at))
            at += 8 * k
        else:
            w = struct.unpack_from("<%dQ" % (2 * k), buf, at)
            s[name] = [(w[2 * i], w[2 * i + 1]) for i in range(k)]
            at += 16 * k
    assert at == len(buf), "trailing bytes after the opening set"
    return s


# ------------------------------------------------------------------------------------------------ prove_openings, fri_committed_trees
def fri_arity_bits(log_n, cfg=CFG):
    """ConstantArityBits(arity_bits, final_poly_bits)"""
    out, d = [], log_n
    while d > cfg["fri_final_poly_bits"] and d + cfg["rate_bits"] - cfg["fri_arity_bits"] >= cfg["cap_height"]:
        out.append(cfg["fri_arity_bits"])
        d -= cfg["fri_arity_bits"]
    return out


def _combine(cols, apow):
    """sum_i apow[i] * cols[i] as two lists of canonical ints (object arrays carry the multiply-adds; one reduction at the end)"""
    n = len(cols[0])
    ca, cb = np.zeros(n, dtype=object), np.zeros(n, dtype=object)
    for f, (a, b) in zip(cols, apow):
        f = np.asarray(f, dtype=object)
        if a:
            ca = ca + f * a
        if b:
            cb = cb + f * b
    return (ca % P).tolist(), (cb % P).tolist()


def _divide_by_linear(ca, cb, z):
    """(C - C(z)) / (X - z): synthetic division from the top coefficient, n - 1 coefficients; also returns C(z)"""
    n = len(ca)
    qa, qb = [0] * (n - 1), [0] * (n - 1)
    za, zb = z
    a = b = 0
    for k in range(n - 1, -1, -1):
        a, b = (a * za + W * b * zb + ca[k]) % P, (a * zb + b * za + cb[k]) % P
        if k:
            qa[k - 1], qb[k - 1] = a, b
    return qa, qb, (a, b)


def composed_quotients(trace_c, zs_c, quot_c, nperm, zeta, alpha):
    """the batches' (C_b - C_b(z_b)) / (X - z_b) joined by the powers of alpha, times X: n coefficients as pairs"""
    n = len(trace_c[0])
    log_n = n.bit_length() - 1
    zeta, alpha = ext(zeta), ext(alpha)
    g = root_of_unity(log_n)
    Wd, Z, Q = len(trace_c), len(zs_c), len(quot_c)
    apow = [(1, 0)]
    for _ in range(Wd + Z + Q):
        apow.append(ext_mul(apow[-1], alpha))
    first = list(trace_c) + list(zs_c)
    c1a, c1b = _combine(first, apow)                                    # C1 = sum_{i<W+Z} alpha^i f_i
    if Q:
        qa, qb = _combine(quot_c, apow[Wd + Z:])                        # C0 = C1 + sum_j alpha^(W+Z+j) q_j
        c0a, c0b = [(x + y) % P for x, y in zip(c1a, qa)], [(x + y) % P for x, y in zip(c1b, qb)]
    else:
        c0a, c0b = c1a, c1b
    batches = [(c0a, c0b, zeta, Wd + Z + Q), (c1a, c1b, (zeta[0] * g % P, zeta[1] * g % P), Wd + Z)]
    if Z > nperm:                                                       # C2 = sum_j alpha^j zs[nperm + j]
        c2a, c2b = _combine(list(zs_c)[nperm:], apow)
        batches.append((c2a, c2b, (pow(g, P - 2, P), 0), Z - nperm))
    fa, fb = [0] * (n - 1), [0] * (n - 1)
    values = []
    for ca, cb, z, count in batches:                                    # final = final * alpha^count + quotient
        qa, qb, at_z = _divide_by_linear(ca, cb, z)
        values.append(at_z)
        sa, sb = apow[count]
        fa, fb = ([(x * sa + W * y * sb + q) % P for x, y, q in zip(fa, fb, qa)],
                  [(x * sb + y * sa + q) % P for x, y, q in zip(fa, fb, qb)])
    return [(0, 0)] + list(zip(fa, fb)), values


def fold(c, length, beta, arity=16):
    """out[j] = sum_k beta^k c[arity j + k] on the coefficients c of a polynomial zero-padded to `length`"""
    ba, bb = beta
    out = []
    for j in range(0, len(c), arity):
        a = b = 0
        for x, y in reversed(c[j:j + arity]):
            a, b = (a * ba + W * b * bb + x) % P, (a * bb + b * ba + y) % P
        out.append((a, b))
    return out, length // arity


def fri_layers(trace_c, zs_c, quot_c, nperm, zeta, alpha, betas, cfg=CFG):
    """the commit phase's polynomials: [(non-zero prefix as pairs, length)] -- first what the first layer commits (the composed
    quotients, zero beyond n, length n << rate_bits), then what is left after each layer's fold by that layer's beta; the last entry
    is what the final polynomial is cut from"""
    n = len(trace_c[0])
    arities = fri_arity_bits(n.bit_length() - 1, cfg)
    assert len(betas) == len(arities), "one beta per layer of the reduction plan"
    c, _ = composed_quotients(trace_c, zs_c, quot_c, nperm, zeta, alpha)
    out = [(c, n << cfg["rate_bits"])]
    for ab, beta in zip(arities, betas):
        out.append(fold(out[-1][0], out[-1][1], ext(beta), 1 << ab))
    return out


def final_poly(trace_c, zs_c, quot_c, nperm, zeta, alpha, betas, cfg=CFG, layers=None):
    """the final polynomial of the FRI commit phase as a list of pairs: the composed quotients zero-padded to n << rate_bits, folded
    once per layer by that layer's beta, truncated to length >> rate_bits"""
    c, length = (layers or fri_layers(trace_c, zs_c, quot_c, nperm, zeta, alpha, betas, cfg))[-1]
    keep = length >> cfg["rate_bits"]
    return (c + [(0, 0)] * keep)[:keep]


def layer_caps(oracle, layers, cfg=CFG):
    """The Merkle caps of the layers that fri_committed_trees commits (all of `layers` but the last): the polynomial's values on the
    coset shift * H in bit-reversed order, `arity` extension elements to a leaf.  The transform and the hashing are the ORACLE's
    (an extension transform is two base-field ones: the twiddles are base-field), under the hasher it is set to; only the
    coefficients come from this module.  Every word of a layer's polynomial enters its cap, the zero words beyond the non-zero
    prefix included."""
    import numpy as np
    caps, shift = [], 7
    arity = 1 << cfg["fri_arity_bits"]
    for c, length in layers[:-1]:
        planes = np.zeros((2, length), dtype=np.uint64)
        planes[:, :len(c)] = np.array(c, dtype=np.uint64).T
        va, vb = (oracle.evaluate_poly_with_offset(pl, shift, 1) for pl in planes)
        bits = length.bit_length() - 1
        j = np.arange(length, dtype=np.uint64)
        rev = np.zeros(length, dtype=np.uint64)
        for b in range(bits):
            rev |= ((j >> np.uint64(b)) & np.uint64(1)) << np.uint64(bits - 1 - b)
        leaves = np.stack([va[rev], vb[rev]], axis=1).reshape(length // arity, 2 * arity)
        caps.append(oracle.merkle(leaves, cfg["cap_height"]))
        shift = pow(shift, arity, P)
    return caps
