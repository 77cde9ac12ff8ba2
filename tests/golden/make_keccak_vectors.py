"""Writes tests/golden/keccak_vectors.json from tests/keccak_ref.py, the restatement of KeccakGoldilocksConfig's hasher on Python integers
(pinned to hashlib.sha3_256 and the published Keccak-256 digests by tests/test_keccak.py).  Deterministic: tests/test_keccak.py checks that
a fresh derivation gives the committed file.

    python tests/golden/make_keccak_vectors.py

REJECTING_STATE_INDEX is the first i for which KeccakPermutation::permute of (i, 0, ..., 0) drops a word: found by tools/find_keccak_reject.cpp
(the library's host code) and only recorded here -- the twelve outputs below come from the restatement, which also checks that h1 does hold a
word >= p and that no smaller multiple of 2^24 does (a sample of the search; the whole search is 2^29 hashes)."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import keccak_ref as K  # noqa: E402

WIDTHS = [0, 1, 2, 15, 16, 17, 18, 33, 34, 35, 94, 134, 135, 136, 137]
REJECTING_STATE_INDEX = 494183523


def derive():
    rng = random.Random(0x6B65636B)
    P = K.P

    def elems(n):
        return [rng.randrange(P) for _ in range(n)]

    def digest(**fixed):
        d = bytearray(rng.randrange(256) for _ in range(K.DIGEST_BYTES))
        for k, v in fixed.items():
            d[int(k[1:])] = v
        return bytes(d)

    hashes = []
    for n in WIDTHS:
        xs = elems(n)
        if n > 2:
            xs[0], xs[-1] = P - 1, 0
        hashes.append({"input": xs, "digest": K.digest_words(K.hash_no_pad(xs))})
    nodes = []
    for l24, r0, r7 in ((0xFF, 0xFF, 0x00), (0x00, 0x00, 0xFF), (0xFF, 0x00, 0x00), (0x00, 0xFF, 0xFF)):
        l, r = digest(b24=l24), digest(b0=r0, b7=r7, b24=l24 ^ 0xFF)
        nodes.append({"left": K.digest_words(l), "right": K.digest_words(r), "digest": K.digest_words(K.two_to_one(l, r))})
    perms = []
    for k in range(8):
        s = [0] * 12 if k == 0 else [P - 1] * 12 if k == 1 else list(range(12)) if k == 2 else elems(12)
        perms.append({"input": s, "output": K.permute(s)})
    observed = [{"digest": K.digest_words(d), "elements": K.digest_elements(d)} for d in (digest(), digest(b24=0xFF, b6=0xFF, b7=0xFF, b20=0x80, b21=0x01), bytes(25), b"\xff" * 25)]

    def script(ops):
        ch, outs = K.Challenger(), []
        for op in ops:
            if op[0] == "observe":
                ch.observe(op[1])
            elif op[0] == "observe_cap":
                ch.observe_cap([op[1][i:i + 4] for i in range(0, len(op[1]), 4)])
            elif op[0] == "get":
                outs.append(ch.get_n(op[1]))
            else:
                ch.compact()
                outs.append(list(ch.state))
        return {"ops": ops, "outputs": outs, "state": list(ch.state)}

    def cap(n):
        return [w for _ in range(n) for w in K.digest_words(digest())]

    scripts = [script([["get", 1]]),
               script([["observe", elems(1)], ["get", 1]]),
               script([["observe", elems(8)], ["get", 3], ["get", 6], ["observe", elems(3)], ["get", 2]]),
               script([["observe", elems(7)], ["observe", elems(1)], ["observe", elems(1)], ["get", 9], ["compact"], ["get", 1]]),
               script([["observe_cap", cap(16)], ["get", 2], ["observe_cap", cap(1)], ["observe", elems(2)], ["get", 4]]),
               script([["observe", elems(21)], ["compact"], ["observe_cap", cap(3)], ["get", 12], ["compact"]])]

    s = [REJECTING_STATE_INDEX] + [0] * 11
    h1 = K.keccak256(K.words_bytes(s))
    words = [int.from_bytes(h1[8 * i:8 * i + 8], "little") for i in range(4)]
    assert any(w >= P for w in words), "the recorded state rejects no word"
    for i in range(0, REJECTING_STATE_INDEX, 1 << 24):
        h = K.keccak256(K.words_bytes([i] + [0] * 11))
        assert all(int.from_bytes(h[8 * k:8 * k + 8], "little") < P for k in range(4)), i
    stream = K.onion_stream(s)
    first16 = [next(stream) for _ in range(16)]
    rejecting = {"input": s, "h1_words": words, "rejected": [w for w in first16 if w >= P], "hashes_needed": 4, "output": K.permute(s)}
    assert rejecting["output"] == [w for w in first16 if w < P][:12] and rejecting["output"] != first16[:12]
    return {"generated_by": "tests/golden/make_keccak_vectors.py",
            "source": "tests/keccak_ref.py: Keccak-256 (original padding) restated on Python integers, pinned to hashlib.sha3_256 (domain byte 0x06) and "
                      "to the published digests of '' and 'abc'",
            "keccak256": {"": K.keccak256(b"").hex(), "abc": K.keccak256(b"abc").hex()},
            "hash_no_pad": hashes, "two_to_one": nodes, "permutation": perms, "digest_elements": observed, "challenger": scripts,
            "rejecting_state": rejecting}


def main():
    path = os.path.join(HERE, "keccak_vectors.json")
    open(path, "w").write(json.dumps(derive(), indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
