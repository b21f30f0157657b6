"""include/troyn.hpp: the baby-step / giant-step linear transform with keys with grouped digits -- the *PlainSumBsgsGrouped
members and the Batch form against the bytes of the C ABI call, decryption, special_primes == 1 against the per-prime members, the refusals
(tests/cpp/test_troyn_grouped_bsgs.cpp), compiled with plain g++.  CPU: linked against the emulator build of the library;  GPU: against libtroyhip.so,
run on the device."""
import os
import subprocess

import pytest

from test_cpp_encrypt import ROOT, _build, _run

SRC = os.path.join(ROOT, "tests", "cpp", "test_troyn_grouped_bsgs.cpp")


def test_troyn_grouped_bsgs_on_emulator(tmp_path):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    exe = str(tmp_path / "test_troyn_grouped_bsgs_emul")
    _build(exe, os.path.join(ROOT, "tests", "emul"), "libtroyhip_emul.so", src=SRC)
    _run(exe, "128")


@pytest.mark.gpu
def test_troyn_grouped_bsgs_on_gpu(tmp_path):
    exe = str(tmp_path / "test_troyn_grouped_bsgs")
    _build(exe, os.path.join(ROOT, "troy_amd"), "libtroyhip.so", src=SRC)
    _run(exe, "4096")
