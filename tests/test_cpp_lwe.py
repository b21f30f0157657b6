"""include/troyn.hpp: LWEBatch, Evaluator::extractLWEs / packLWEs against extractLWE / packLWECiphertexts limb for limb (tests/cpp/test_troyn_lwe.cpp),
compiled with plain g++.  CPU: linked against the emulator build of the library;  GPU: against libtroyhip.so, run on the device."""
import os
import subprocess

import pytest

from test_cpp_encrypt import ROOT, _build, _run

SRC = os.path.join(ROOT, "tests", "cpp", "test_troyn_lwe.cpp")


def test_troyn_lwe_on_emulator(tmp_path):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    exe = str(tmp_path / "test_troyn_lwe_emul")
    _build(exe, os.path.join(ROOT, "tests", "emul"), "libtroyhip_emul.so", src=SRC)
    _run(exe, "256")


@pytest.mark.gpu
def test_troyn_lwe_on_gpu(tmp_path):
    exe = str(tmp_path / "test_troyn_lwe")
    _build(exe, os.path.join(ROOT, "troy_amd"), "libtroyhip.so", src=SRC)
    _run(exe, "4096")
