"""Poseidon2 over Goldilocks (width 12, x^7, 4 + 22 + 4 rounds) as the reference's plonky2 fork computes it
(plonky2/plonky2/src/hash/poseidon2.rs:50 `Poseidon2::poseidon2`, constants in poseidon2_goldilocks.rs).

Three things live here:
  * `permute(state, params)`: a direct Python restatement of the reference's code (matmul_external :118, matmul_m4 :176,
    matmul_internal :155 -- which multiplies by MAT_DIAG12_M_1[i] - 1, as the code does), needing nothing but the parameters;
  * `install()`: the one method the interpreter of tools/rust_air_eval.py lacks to run poseidon2.rs from source,
    `Field::multiply_accumulate` (self + a * b), registered as a hook around `Interp.method` -- every other call goes to the
    interpreter unchanged;
  * `FastPoseidon2`: the restatement with the reference's constants, checked against the interpreted `poseidon2` (as
    tools/ref_verifier.py FastPoseidon is against `poseidon_naive`), for the many permutations of a verification.
"""
import os
import re

P = 0xFFFFFFFF00000001
W = 12
ROUND_F_BEGIN, ROUND_F_END, ROUND_P = 4, 8, 22
REL = "plonky2/plonky2/src/hash/poseidon2_goldilocks.rs"
REL_PERM = "plonky2/plonky2/src/hash/poseidon2.rs"


def strip_comments(text):
    """Rust source without // and /* */ comments (RC12 is followed by 22 commented-out rows)"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def read_params(reference):
    """(MAT_DIAG12_M_1 [12], RC12 [8][12], RC12_MID [22]) from the reference's poseidon2_goldilocks.rs"""
    text = strip_comments(open(os.path.join(reference, REL)).read())

    def grab(name):
        m = re.search(r"const\s+" + name + r"\s*:[^=]*=\s*\[(.*?)\];", text, re.S)
        return [int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", m.group(1))]

    diag, rc, mid = grab("MAT_DIAG12_M_1"), grab("RC12"), grab("RC12_MID")
    assert len(diag) == W and len(rc) == W * ROUND_F_END and len(mid) == ROUND_P, (len(diag), len(rc), len(mid))
    return {"diag_m_1": diag, "rc": [rc[W * r:W * (r + 1)] for r in range(ROUND_F_END)], "rc_mid": mid}


def params_from_header(path=None):
    """the same parameters out of include/ola_poseidon2_constants.h (what the product is built from; no reference needed)"""
    path = path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ola_poseidon2_constants.h")
    text = open(path).read()

    def grab(name):
        m = re.search(r"\b" + name + r"\[\d+\]\s*=\s*\{(.*?)\};", text, re.S)
        return [int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", m.group(1))]

    rc = grab("OLA_POSEIDON2_RC")
    return {"diag_m_1": grab("OLA_POSEIDON2_DIAG_M_1"), "rc": [rc[W * r:W * (r + 1)] for r in range(ROUND_F_END)],
            "rc_mid": grab("OLA_POSEIDON2_RC_MID")}


def _m4(x):
    for g in range(0, W, 4):
        a, b, c, d = x[g:g + 4]
        t0 = a + b
        t1 = c + d
        t2 = t1 + 2 * b
        t3 = t0 + 2 * d
        t4 = t3 + 4 * t1
        t5 = t2 + 4 * t0
        x[g:g + 4] = [(t3 + t5) % P, t5 % P, (t2 + t4) % P, t4 % P]


def matmul_external(x):
    _m4(x)
    stored = [sum(x[4 * j + l] for j in range(W // 4)) for l in range(4)]
    for i in range(W):
        x[i] = (x[i] + stored[i % 4]) % P


def matmul_internal(x, diag_m_1):
    s = sum(x)
    for i in range(W):
        x[i] = ((diag_m_1[i] - 1) * x[i] + s) % P


def _sbox(v):
    x2 = v * v % P
    return (x2 * v % P) * (x2 * x2 % P) % P


def permute_lanes(x, params):
    """the permutation on a list of 12 lanes, each an integer < p or a numpy object array of them (many states at once)"""
    x = list(x)
    matmul_external(x)
    for r in range(ROUND_F_BEGIN):
        x = [_sbox((x[i] + params["rc"][r][i]) % P) for i in range(W)]
        matmul_external(x)
    for r in range(ROUND_P):
        x[0] = _sbox((x[0] + params["rc_mid"][r]) % P)
        matmul_internal(x, params["diag_m_1"])
    for r in range(ROUND_F_BEGIN, ROUND_F_END):
        x = [_sbox((x[i] + params["rc"][r][i]) % P) for i in range(W)]
        matmul_external(x)
    return x


def permute(state, params):
    """Poseidon2::poseidon2 (poseidon2.rs:50) on 12 integers (any u64: taken mod p); returns 12 canonical integers"""
    return [int(v) for v in permute_lanes([int(v) % P for v in state], params)]


# ------------------------------------------------------------------------------------------------ the interpreted reference
_installed = False


def install():
    """registers Field::multiply_accumulate (field/types.rs: self + a * b) with the interpreter; idempotent"""
    global _installed
    import rust_air_eval as R
    if _installed:
        return R
    orig = R.Interp.method

    def method(self, r, name, args, src, line):
        if name == "multiply_accumulate" and isinstance(r, R.Fe) and len(args) == 2:
            return R.Fe(r.v + args[0].v * args[1].v)
        return orig(self, r, name, args, src, line)

    R.Interp.method = method
    _installed = True
    return R


def interp_poseidon2(it, state):
    """the reference's own `Poseidon2::poseidon2`, interpreted from poseidon2.rs"""
    R = install()
    out = it.call_assoc("Poseidon2", "poseidon2", [[R.Fe(int(v)) for v in state]], os.path.join(it.plonky2, "hash", "poseidon2.rs"))
    return [x.v for x in out]


class FastPoseidon2:
    """`permute` with the constants read through the interpreter's constant lookup; `check` compares it with the interpreted
    `poseidon2`.  Instances are callable the way tools/rust_air_eval.py's permutation hooks are (a list of Fe in, out)."""

    def __init__(self, it):
        R = install()
        src = R.X.Src.get(os.path.join(it.plonky2, "hash", "poseidon2_goldilocks.rs"))
        rc = [int(x) for row in it.const_value("RC12", src) for x in row]
        self.params = {"diag_m_1": [int(x) for x in it.const_value("MAT_DIAG12_M_1", src)],
                       "rc": [rc[W * r:W * (r + 1)] for r in range(ROUND_F_END)],
                       "rc_mid": [int(x) for x in it.const_value("RC12_MID", src)]}
        self.Fe = R.Fe

    def permute(self, state):
        return [self.Fe(x) for x in permute([x.v for x in state], self.params)]

    def __call__(self, state, segs=None):
        return self.permute(state)

    def check(self, it, count=6):
        R = install()
        for k in range(count):
            v = [P - 1] * W if k == 0 else [int(x) for x in R.stream_for(7900 + k, 9, W)]
            if interp_poseidon2(it, v) != permute(v, self.params):
                raise SystemExit("the direct Poseidon2 permutation disagrees with the interpreted poseidon2")


def splitmix_u64(seed, count):
    """`count` raw 64-bit words (splitmix64, NOT reduced mod p: about one in 2^32 is >= p, so some are forced to be)"""
    m = 2**64 - 1
    x = (seed * 0x9E3779B97F4A7C15 + 0x1234567) & m
    out = []
    for _ in range(count):
        x = (x + 0x9E3779B97F4A7C15) & m
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        out.append(z ^ (z >> 31))
    return out


def kat_inputs():
    """the known-answer inputs: all zero, 0..11, all p - 1, twelve stream states (the even ones with non-canonical words >= p)"""
    ins = [[0] * W, list(range(W)), [P - 1] * W]
    for k in range(12):
        s = splitmix_u64(100 + k, W)
        if k % 2 == 0:
            s = [P + (v % (2**64 - P)) if i % 3 == 0 else v for i, v in enumerate(s)]
        ins.append(s)
    return ins
