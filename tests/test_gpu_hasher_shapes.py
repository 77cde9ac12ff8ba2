"""The kernel bodies of olavm_amd/csrc/merkle.hip that no other module reaches under some hasher, each at the smallest shape that
reaches it, against a checker that is not the library: the CPU oracle (Poseidon, Blake3), tools/poseidon2_ref.py (Poseidon2) and
tests/keccak_ref.py (Keccak).

  * leaf_hash_kernel<SpongeHash, RowMajorSrc>, one lane per leaf: from 8193 leaves (8192 and fewer take the quad form), at the
    sponge's absorb boundaries -- widths 1, 8 (one full block) and 9 (a second block of one word).
  * merkle_level_kernel<SpongeHash>, one lane per node: a level of more than 8192 nodes, so a tree of 2^15 leaves (width 2); the
    levels of 8192 .. 512 nodes of the same tree take merkle_level_quad_kernel, the rest merkle_top_kernel.
  * merkle_level_kernel<Blake3Hash / KeccakHash>: the byte hashes fuse their levels (merkle_levels_bytes_kernel) unless the cap lies
    above 256 nodes, so a tree of 2^11 leaves with a cap of 2^9: the levels of 1024 and 512 nodes, one launch each."""
import numpy as np
import pytest

from tests import keccak_ref as K
from tests.oracle_lib import rand_field
from tests.test_gpu_poseidon2 import hash_no_pad as poseidon2_hash_rows, merkle_cap as poseidon2_merkle_cap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    """backend(hasher): one context per hasher, closed when the module is done"""
    from olavm_amd.backend import Backend
    made = {}

    def get(hasher):
        if hasher not in made:
            made[hasher] = Backend(device=0, hasher=hasher)
        return made[hasher]
    yield get
    for b in made.values():
        b.close()


def reference_cap(oracle, hasher, leaves, cap_h):
    if hasher == "poseidon2":
        return poseidon2_merkle_cap(leaves, cap_h)
    if hasher == "keccak":
        return K.MerkleTree(leaves, cap_h).cap()
    with oracle.hasher(hasher):
        return oracle.merkle(leaves, cap_h)


@pytest.mark.parametrize("width", [1, 8, 9])
@pytest.mark.parametrize("hasher", ["poseidon", "poseidon2"])
def test_sponge_leaves_one_lane_per_leaf(backend, oracle, hasher, width):
    rng = np.random.default_rng(8193 + width)
    rows = rand_field(rng, (8193, width))
    got = backend(hasher).hash_rows(rows)
    idx = [0, 1, 63, 64, 4096, 8191, 8192]
    if hasher == "poseidon2":
        want = poseidon2_hash_rows(rows[idx])
    else:
        want = np.stack([oracle.hash_no_pad(rows[i]) for i in idx])
    assert np.array_equal(got[idx], want)


@pytest.mark.parametrize("hasher", ["poseidon", "poseidon2"])
def test_sponge_tree_with_a_level_above_the_quad_threshold(backend, oracle, hasher):
    rng = np.random.default_rng(15)
    leaves = rand_field(rng, (1 << 15, 2))
    assert np.array_equal(backend(hasher).merkle_cap(leaves, 4), reference_cap(oracle, hasher, leaves, 4))


@pytest.mark.parametrize("hasher", ["blake3", "keccak"])
def test_byte_hash_tree_with_a_cap_above_the_fused_levels(backend, oracle, hasher):
    rng = np.random.default_rng(11)
    leaves = rand_field(rng, (1 << 11, 3))
    assert np.array_equal(backend(hasher).merkle_cap(leaves, 9), reference_cap(oracle, hasher, leaves, 9))
