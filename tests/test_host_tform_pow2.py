"""The multiplication-free 64-point closing block of the transform passes, on the host (no GPU)."""
import os
import subprocess


def test_tform_pow2_block_on_range_checked_limbs(tmp_path):
    """olavm_amd/csrc/tform.cuh's tf_mul_pow2 and tf_round6_pair -- the shift twiddles of the 6-bit closing pass -- compiled on a limb
    class that fails when a limb leaves the signed 32-bit bound: tests/host_tform_pow2_check.cpp checks every exponent 39 e mod 192
    (153 e for the inverse), e < 64, against canonical multiplication by the reference's w_64^e and the stated magnitudes, and whole
    64-point blocks (load multiplication, radix-16, shifts, radix-4, canonical fold) against a naive DFT, on random words and on
    tilings of {0, 1, p-1, p, 2^32-1, 2^32, 0xFFFFFFFF00000000, 2^64-1}."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(str(tmp_path), "host_tform_pow2_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(os.path.dirname(here), "olavm_amd", "csrc"),
                           os.path.join(here, "host_tform_pow2_check.cpp"), "-o", exe])
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "tform pow2 ok" in r.stdout, r.stdout + r.stderr
