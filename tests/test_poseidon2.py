"""Poseidon2 over Goldilocks, the hash of the reference fork's Poseidon2GoldilocksConfig / Poseidon2GoldilocksConfig2 (plonk/config.rs:123-141),
without a GPU: the known answers (tests/golden/ref_poseidon2_vectors.json, the reference's own `Poseidon2::poseidon2` interpreted from
source), the Python restatement of tools/poseidon2_ref.py, the generated header, and the C library's host challenger under both Poseidon2
hashers (OLA_HASH_POSEIDON2 = 2, OLA_HASH_POSEIDON2_POW_POSEIDON = 3)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("OLA_REFERENCE", "/root/reference")
KATS = os.path.join(HERE, "golden", "ref_poseidon2_vectors.json")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import poseidon2_ref as Q  # noqa: E402

P = Q.P
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")


def _kats():
    return json.load(open(KATS))["vectors"]


def test_known_answers_cover_the_edge_inputs():
    ins = [v["input"] for v in _kats()]
    assert ins[0] == [0] * 12 and ins[1] == list(range(12)) and ins[2] == [P - 1] * 12 and len(ins) == 15
    assert sum(x >= P for s in ins for x in s) >= 12          # non-canonical words (>= p) are part of the inputs
    assert _kats()[0]["output"][:2] == [0x258f5d724d96657c, 0xe4705cb2bdf352a9]
    assert _kats()[1]["output"][:2] == [0xc928fbab20588837, 0x8f58371184fbe53f]


def test_restatement_equals_the_known_answers():
    p = Q.params_from_header()
    for v in _kats():
        assert Q.permute(v["input"], p) == v["output"]
    # the vectorised form (many states at once) is the same function
    a = np.array([v["input"] for v in _kats()], dtype=object) % P
    out = Q.permute_lanes([a[:, i] for i in range(12)], p)
    assert [[int(out[i][k]) for i in range(12)] for k in range(len(a))] == [v["output"] for v in _kats()]


def test_internal_layer_uses_the_diagonal_minus_one():
    """matmul_internal (poseidon2.rs:155) multiplies by MAT_DIAG12_M_1[i] - 1: the header's multipliers are that, and the function
    with the listed values themselves is a different one"""
    p = Q.params_from_header()
    text = open(os.path.join(ROOT, "include", "ola_poseidon2_constants.h")).read()
    import re
    d = [int(x, 16) for x in re.findall(r"0x[0-9a-f]+", re.search(r"OLA_POSEIDON2_DIAG\[12\] = \{(.*?)\};", text, re.S).group(1))]
    assert d == [x - 1 for x in p["diag_m_1"]]
    other = dict(p, diag_m_1=[x + 1 for x in p["diag_m_1"]])
    assert Q.permute([0] * 12, other) != _kats()[0]["output"]


@needs_ref
def test_known_answers_are_the_interpreted_reference():
    import rust_air_eval as R
    it = R.plonky2_interp(REF)
    for v in _kats()[:6]:
        assert Q.interp_poseidon2(it, v["input"]) == v["output"]
    fp = Q.FastPoseidon2(it)
    fp.check(it, count=3)
    assert fp.params == Q.params_from_header()


@needs_ref
def test_generated_header_and_fixture_are_current():
    """the header's parameters are the reference's (comments stripped: RC12 has 8 rows, not 30) and the generator would write the
    committed files as they are"""
    import gen_poseidon2_tables as G
    p = Q.read_params(REF)
    assert len(p["rc"]) == 8 and len(p["rc_mid"]) == 22
    assert p == Q.params_from_header()
    assert open(G.HEADER).read() == G.header_text(p)


# ------------------------------------------------------------------------------------------------ the reference's verdict on the proof
PROOF = os.path.join(HERE, "golden", "ref_verified", "wide_program_poseidon2.proof")


def _record():
    return json.load(open(PROOF[:-len(".proof")] + ".json"))


def test_record_belongs_to_the_committed_proof():
    """tests/make_ref_verdict_poseidon2.py's record of what the reference said of the GPU's Poseidon2 proof"""
    import hashlib
    raw, rec = open(PROOF, "rb").read(), _record()
    assert rec["config"] == "Poseidon2GoldilocksConfig" and rec["verify_proof"] == "Ok(())" and rec["write_all_proof_reproduces_the_bytes"]
    assert rec["proof_bytes"] == len(raw) and rec["proof_sha256"] == hashlib.sha256(raw).hexdigest()
    assert len(rec["tampered"]) == 19 and all(t["reference"].startswith("Err") for t in rec["tampered"])
    assert rec["config2"]["verify_proof"] == "Ok(())" and len(rec["config2"]["pow_witnesses"]) == 12
    assert rec["prove_single_table"] and all(r["equal"] and r["transcript_after_equal"] for r in rec["prove_single_table"])
    from tests.make_ref_verdict import instance
    assert [[int(x) for x in tr.shape] for tr in instance()[0]] == rec["trace_shapes"]


@needs_ref
def test_reference_verifier_replays_its_verdict():
    """the interpreted `write_all_proof` and `verify_proof` under Poseidon2GoldilocksConfig: the bytes back, Ok(()), and the recorded verdict on two
    corruptions"""
    sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
    import compare_with_dump as CD
    import ref_verifier as V
    from tests.make_ref_verdict import tamper
    raw, rec = open(PROOF, "rb").read(), _record()
    rv = V.RefVerifier(REF, hasher="poseidon2")
    proof = V.decode_all_proof(raw, "poseidon2")
    assert rv.encode(proof) == raw
    assert rv.verify(proof) == (True, None)
    spans = {n: (a, b) for n, a, b in CD.parse_all_proof(raw)}
    for t in [x for x in rec["tampered"] if x["span"] in ("table 0: trace_cap", "table 7: fri.pow_witness")]:
        bad, off = tamper(raw, spans, t["span"])
        assert off == t["byte"]
        ok, where = rv.verify(bad)
        assert not ok and "Err " + where == t["reference"], t["span"]


# ------------------------------------------------------------------------------------------------ the host challenger
class PyChallenger:
    """iop/challenger.rs:19-170 over Poseidon2Permutation: duplexing sponge, rate 8, overwrite mode; a HashOut is observed as its
    four elements"""

    def __init__(self, params):
        self.p, self.state, self.inp, self.out = params, [0] * 12, [], []

    def duplex(self):
        for i, x in enumerate(self.inp):
            self.state[i] = x
        self.inp = []
        self.state = Q.permute(self.state, self.p)
        self.out = self.state[:8]

    def observe(self, elems):
        for e in elems:
            self.out = []
            self.inp.append(int(e) % P)
            if len(self.inp) == 8:
                self.duplex()

    def get(self):
        if self.inp or not self.out:
            self.duplex()
        return self.out.pop()

    def compact(self):
        if self.inp:
            self.duplex()
        self.out = []


@pytest.mark.parametrize("hasher", ["poseidon2", "poseidon2_pow_poseidon"])
def test_host_challenger_is_the_poseidon2_transcript(hasher):
    """observe, observe_cap, get_challenge, get_hash (four challenges), compact: the C library's challenger against the restatement"""
    from olavm_amd.backend import Challenger, HASHERS, load_library
    L = load_library()
    ch, py = Challenger(L, hasher), PyChallenger(Q.params_from_header())
    assert ch.c.hasher == HASHERS[hasher] and ch.clone().c.hasher == HASHERS[hasher]
    rng = np.random.default_rng(5)
    for rnd in range(25):
        e = rng.integers(0, 2**64, int(rng.integers(0, 20)), dtype=np.uint64)
        ch.observe(e); py.observe([int(x) for x in e])
        d = rng.integers(0, 2**64, (int(rng.integers(0, 4)), 4), dtype=np.uint64)
        ch.observe_cap(d); py.observe([int(x) for x in d.ravel()])
        if rnd % 6 == 2:
            ch.compact(); py.compact()
        k = 4 if rnd % 3 == 0 else int(rng.integers(1, 12))    # get_hash draws four
        assert [ch.get() for _ in range(k)] == [py.get() for _ in range(k)], rnd
    assert [int(x) for x in ch.state()] == py.state


def test_unknown_hashers_are_still_refused():
    from olavm_amd.backend import OlaChallenger, load_library
    L = load_library()
    c = OlaChallenger()
    for h in (2, 3):
        assert L.ola_challenger_init_hasher(C.byref(c), C.c_uint32(h)) == 0 and c.hasher == h
    for h in (4, 5, 0xFFFFFFFF):
        assert L.ola_challenger_init_hasher(C.byref(c), C.c_uint32(h)) != 0
