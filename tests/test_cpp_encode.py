"""include/troyn.hpp: the host C ABI of the CKKS slot encoder against the header's single-item CKKSEncoder, and the batched device encoders of
BatchEncoder / CKKSEncoder against loops of single calls (tests/cpp/test_troyn_encode.cpp), compiled with plain g++ -O2.  CPU: linked against the
emulator build of the library;  GPU: against libtroyhip.so, run on the device."""
import os
import subprocess

import pytest

from test_cpp_encrypt import ROOT, _build, _run

SRC = os.path.join(ROOT, "tests", "cpp", "test_troyn_encode.cpp")


def test_troyn_encode_on_emulator(tmp_path):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    exe = str(tmp_path / "test_troyn_encode_emul")
    _build(exe, os.path.join(ROOT, "tests", "emul"), "libtroyhip_emul.so", src=SRC)
    _run(exe, "256", "5")


@pytest.mark.gpu
def test_troyn_encode_on_gpu(tmp_path):
    exe = str(tmp_path / "test_troyn_encode")
    _build(exe, os.path.join(ROOT, "troy_amd"), "libtroyhip.so", src=SRC)
    _run(exe, "8192", "64")
