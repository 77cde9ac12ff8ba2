"""StarkConfig::num_challenges at the boundary, without a GPU: the range ola_gpu_init admits (1..8, the verifier's) and which
challenge counts have generated quotient kernels (ola_air_kernels_available_cfg, host only)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.backend import load_library
    return load_library()


def config(num_challenges):
    from olavm_amd.backend import OlaGpuConfig
    return OlaGpuConfig(-1, None, 3, 4, 16, 4, 5, 28, num_challenges, 0)


@pytest.mark.parametrize("nch", [0, 9])
def test_a_challenge_count_outside_1_to_8_is_an_invalid_argument(lib, nch):
    """with or without a device: the configuration is judged before the device is looked for"""
    ctx = C.c_void_p()
    assert lib.ola_gpu_init(C.byref(config(nch)), C.byref(ctx)) == -1
    assert b"num_challenges must be in 1..8" in lib.ola_gpu_last_error()
    assert not ctx.value


@pytest.mark.parametrize("nch", [1, 3, 8])
def test_a_challenge_count_in_range_gets_as_far_as_the_device(lib, nch):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_nch_*.py create such contexts")
    ctx = C.c_void_p()
    assert lib.ola_gpu_init(C.byref(config(nch)), C.byref(ctx)) == -2, lib.ola_gpu_last_error()


def test_generated_kernels_exist_for_two_and_three_challenges(lib):
    from olavm_amd.air import ola_tables as T
    from olavm_amd.backend import U64P, air_kernels_available
    for airset in (T.ola_stark(), T.ola_stark(range_bits=4, limb_bits=2)):
        blob = np.ascontiguousarray(airset.blob(), dtype=np.uint64)

        def available(cfg):
            flags = (C.c_uint8 * 12)()
            rc = lib.ola_air_kernels_available_cfg(cfg, blob.ctypes.data_as(U64P), blob.size, flags, 12)
            assert rc == 0, lib.ola_gpu_last_error()
            return [int(f) for f in flags]

        assert available(None) == [1] * 12                          # NULL: the defaults, two challenges
        assert available(C.byref(config(2))) == [1] * 12
        assert available(C.byref(config(3))) == [1] * 12
        assert available(C.byref(config(4))) == [0] * 12            # no kernel: the interpreter kernel proves these
        assert air_kernels_available(blob, 12, num_challenges=3) == [True] * 12
        flags = (C.c_uint8 * 12)()
        assert lib.ola_air_kernels_available_cfg(C.byref(config(9)), blob.ctypes.data_as(U64P), blob.size, flags, 12) == -1


def test_the_signature_of_two_challenges_is_unchanged_and_other_counts_differ():
    """a table without lookups and permutation pairs has the same description at every count: the count itself is hashed"""
    from olavm_amd.air import ola_tables as T
    from olavm_amd.air.dsl import AirSet
    s = T.ola_stark(range_bits=4, limb_bits=2)
    for t in range(12):
        assert s.signature(t) == s.signature(t, 2)
        assert len({s.signature(t, c) for c in range(1, 9)}) == 8
    lone = AirSet([t for t in s.tables if not t.permutation_pairs][:1], [])
    assert lone.signature_words(0, 3)[1:] == lone.signature_words(0, 2) and lone.signature(0, 3) != lone.signature(0, 2)
