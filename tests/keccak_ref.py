"""KeccakGoldilocksConfig restated on Python integers (plonky2/plonky2/src/hash/keccak.rs, hash_types.rs:133-153, iop/challenger.rs:36-162,
hash/merkle_tree.rs, hash/merkle_proofs.rs): the independent side of every Keccak test.  It shares no code with olavm_amd/csrc/keccak.cuh.

The crate the reference calls (keccak_hash::keccak) is Keccak-256 with the original padding (0x01 .. 0x80).  Nothing in the Python
standard library computes that, so the permutation and the sponge here are pinned the other way round (tests/test_keccak.py): with
the domain byte 0x06 they must equal hashlib.sha3_256 on many lengths, with 0x01 they must give the two published Keccak-256 digests.

A digest is 25 bytes.  As words it is 4 little-endian u64, word 3 = byte 24 (the layout the library keeps in device memory)."""
import numpy as np

P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
RATE = 136
DIGEST_BYTES = 25

RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
      0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
      0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
      0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]


def _rho_offsets():
    """the rotation of lane (x, y): (t + 1)(t + 2) / 2 along the walk (x, y) -> (y, 2x + 3y) from (1, 0) (Keccak reference, 1.2)"""
    r = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        r[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


RHO = _rho_offsets()


def _rol(v, n):
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def keccak_f(a):
    """Keccak-f[1600] on a[x][y], Python integers"""
    for rc in RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rol(a[x][y], RHO[x][y])
        a = [[b[x][y] ^ ((~b[(x + 1) % 5][y] & M64) & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        a[0][0] ^= rc
    return a


def sponge256(data: bytes, domain: int) -> bytes:
    """32 bytes of the sponge with rate 136: `domain` after the message, 0x80 into the block's last byte"""
    pad = bytearray(data)
    pad.append(domain)
    while len(pad) % RATE:
        pad.append(0)
    pad[-1] |= 0x80
    a = [[0] * 5 for _ in range(5)]
    for off in range(0, len(pad), RATE):
        for i in range(RATE // 8):
            a[i % 5][i // 5] ^= int.from_bytes(pad[off + 8 * i:off + 8 * i + 8], "little")
        a = keccak_f(a)
    return b"".join(a[i % 5][i // 5].to_bytes(8, "little") for i in range(4))


def keccak256(data: bytes) -> bytes:
    return sponge256(data, 0x01)


def sha3_256(data: bytes) -> bytes:
    return sponge256(data, 0x06)


# ---- the same permutation and sponge on numpy arrays: one message per row, all of one length ----
def keccak_f_np(a):
    """a: list of 25 uint64 arrays, lane x + 5y"""
    a = list(a)
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x - 1) % 5] ^ ((c[(x + 1) % 5] << np.uint64(1)) | (c[(x + 1) % 5] >> np.uint64(63))) for x in range(5)]
        b = [None] * 25
        for x in range(5):
            for y in range(5):
                v, n = a[x + 5 * y] ^ d[x], RHO[x][y]
                b[y + 5 * ((2 * x + 3 * y) % 5)] = ((v << np.uint64(n)) | (v >> np.uint64(64 - n))) if n else v
        a = [b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]) for y in range(5) for x in range(5)]
        a[0] = a[0] ^ np.uint64(rc)
    return a


def sponge256_np(msgs: np.ndarray, domain: int = 0x01) -> np.ndarray:
    """msgs: (n, length) uint8; returns (n, 32) uint8"""
    n, length = msgs.shape
    padded = (length // RATE + 1) * RATE
    buf = np.zeros((n, padded), dtype=np.uint8)
    buf[:, :length] = msgs
    buf[:, length] = domain
    buf[:, padded - 1] |= 0x80
    words = buf.view("<u8").reshape(n, padded // 8)
    a = [np.zeros(n, dtype=np.uint64) for _ in range(25)]
    for off in range(0, padded // 8, RATE // 8):
        for i in range(RATE // 8):
            a[i] = a[i] ^ words[:, off + i]
        a = keccak_f_np(a)
    return np.ascontiguousarray(np.stack(a[:4], axis=1)).view(np.uint8).reshape(n, 32)


# ---- the hasher (hash/keccak.rs) ----
def digest_words(d25: bytes):
    """25 bytes -> the 4 words of the in-memory layout"""
    assert len(d25) == DIGEST_BYTES
    return [int.from_bytes(d25[0:8], "little"), int.from_bytes(d25[8:16], "little"), int.from_bytes(d25[16:24], "little"), d25[24]]


def digest_bytes(w4) -> bytes:
    assert int(w4[3]) < 256
    return b"".join(int(w4[i]).to_bytes(8, "little") for i in range(3)) + bytes([int(w4[3])])


def words_bytes(xs) -> bytes:
    return b"".join((int(x) % P).to_bytes(8, "little") for x in xs)


def hash_no_pad(xs) -> bytes:
    return keccak256(words_bytes(xs))[:DIGEST_BYTES]


def two_to_one(l: bytes, r: bytes) -> bytes:
    assert len(l) == DIGEST_BYTES and len(r) == DIGEST_BYTES
    return keccak256(l + r)[:DIGEST_BYTES]


def onion_select(stream):
    """KeccakPermutation's selection over the words of h1 || h2 || ...: words >= p are dropped, the first 12 survivors are the state"""
    out = []
    for w in stream:
        if w < P:
            out.append(w)
            if len(out) == 12:
                return out
    raise ValueError("the stream ended before twelve words survived")


def onion_stream(state):
    h = keccak256(words_bytes(state))
    while True:
        for i in range(4):
            yield int.from_bytes(h[8 * i:8 * i + 8], "little")
        h = keccak256(h)


def permute(state):
    assert len(state) == 12
    return onion_select(onion_stream(state))


def digest_elements(d25: bytes):
    """BytesHash<25>::to_vec: 7, 7, 7 and 4 bytes, little-endian"""
    return [int.from_bytes(d25[i:i + 7], "little") for i in range(0, DIGEST_BYTES, 7)]


class Challenger:
    """iop/challenger.rs:36-162 with H::Permutation = KeccakPermutation"""

    def __init__(self):
        self.state, self.inp, self.out = [0] * 12, [], []

    def clone(self):
        c = Challenger()
        c.state, c.inp, c.out = list(self.state), list(self.inp), list(self.out)
        return c

    def _duplex(self):
        for i, v in enumerate(self.inp):
            self.state[i] = v
        self.inp = []
        self.state = permute(self.state)
        self.out = list(self.state[:8])

    def observe(self, xs):
        for x in xs:
            self.out = []
            self.inp.append(int(x) % P)
            if len(self.inp) == 8:
                self._duplex()

    def observe_digest(self, d25: bytes):
        self.observe(digest_elements(d25))

    def observe_cap(self, cap):
        """cap: digests as 25 bytes each, or an (n, 4) array of words"""
        for d in cap:
            self.observe_digest(d if isinstance(d, (bytes, bytearray)) else digest_bytes(d))

    def get(self):
        if self.inp or not self.out:
            self._duplex()
        return self.out.pop()

    def get_n(self, n):
        return [self.get() for _ in range(n)]

    def compact(self):
        if self.inp:
            self._duplex()
        self.out = []


# ---- MerkleTree::new_v2 (every leaf hashed, whatever its width), heap-ordered ----
def _digest_rows(h32: np.ndarray) -> np.ndarray:
    """(n, 32) uint8 hashes -> (n, 4) uint64 digests in the in-memory layout"""
    d = np.ascontiguousarray(h32).view("<u8").reshape(-1, 4).copy()
    d[:, 3] &= np.uint64(0xFF)
    return d


def hash_rows(rows: np.ndarray) -> np.ndarray:
    """hash_no_pad of every row of a (n, width) uint64 array -> (n, 4) uint64"""
    rows = np.asarray(rows, dtype=np.uint64)
    canon = np.where(rows >= np.uint64(P), rows - np.uint64(P), rows).astype("<u8")
    return _digest_rows(sponge256_np(np.ascontiguousarray(canon).view(np.uint8).reshape(rows.shape[0], 8 * rows.shape[1])))


def nodes_of(children: np.ndarray) -> np.ndarray:
    """two_to_one of consecutive pairs: (2n, 4) -> (n, 4)"""
    b = np.ascontiguousarray(children.astype("<u8")).view(np.uint8).reshape(-1, 32)[:, :DIGEST_BYTES]
    return _digest_rows(sponge256_np(np.ascontiguousarray(b.reshape(-1, 2 * DIGEST_BYTES))))


class MerkleTree:
    def __init__(self, leaves: np.ndarray, cap_height: int):
        n = leaves.shape[0]
        assert n & (n - 1) == 0 and (1 << cap_height) <= n
        self.n, self.cap_height = n, cap_height
        self.heap = np.zeros((2 * n, 4), dtype=np.uint64)
        self.heap[n:] = hash_rows(leaves)
        level = n // 2
        while level >= (1 << cap_height) and level >= 1:
            self.heap[level:2 * level] = nodes_of(self.heap[2 * level:4 * level])
            level //= 2

    def cap(self) -> np.ndarray:
        c = 1 << self.cap_height
        return self.heap[c:2 * c].copy()

    def prove(self, j: int) -> np.ndarray:
        """siblings from the leaf up to below the cap, (depth, 4)"""
        i, out = self.n + j, []
        while i >= (2 << self.cap_height):
            out.append(self.heap[i ^ 1])
            i >>= 1
        return np.array(out, dtype=np.uint64).reshape(-1, 4)


def verify_to_cap(leaf, index: int, siblings, cap) -> bool:
    """verify_merkle_proof_to_cap (hash/merkle_proofs.rs:52-80) on 25-byte digests, Python integers"""
    cur = hash_no_pad(leaf)
    for s in siblings:
        s = s if isinstance(s, (bytes, bytearray)) else digest_bytes(s)
        cur = two_to_one(s, cur) if index & 1 else two_to_one(cur, s)
        index >>= 1
    c = cap[index]
    return cur == (c if isinstance(c, (bytes, bytearray)) else digest_bytes(c))
