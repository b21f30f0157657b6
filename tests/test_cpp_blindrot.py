"""include/troyn.hpp: BlindRotationKey, KeyGenerator::createBlindRotationKey / secretCoefficients and Evaluator::blindRotate / blindRotateBatch /
lweModSwitch against the C ABI limb for limb (tests/cpp/test_troyn_blindrot.cpp), compiled with plain g++ and linked against the emulator build of the
library."""
import os
import subprocess

from test_cpp_encrypt import ROOT, _build, _run

SRC = os.path.join(ROOT, "tests", "cpp", "test_troyn_blindrot.cpp")


def test_troyn_blindrot_on_emulator(tmp_path):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    exe = str(tmp_path / "test_troyn_blindrot_emul")
    _build(exe, os.path.join(ROOT, "tests", "emul"), "libtroyhip_emul.so", src=SRC)
    _run(exe)
