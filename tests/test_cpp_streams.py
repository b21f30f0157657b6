"""include/troyn.hpp: no two calls of one troyn::KeyGenerator / troyn::Encryptor share stream words (tests/cpp/test_troyn_streams.cpp), compiled
with plain g++.  CPU: linked against the emulator build of the library;  GPU: against libtroyhip.so, run on the device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_troyn_streams.cpp")


def _build(out, libdir, libfile):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", out,
           os.path.join(libdir, libfile), "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout


def test_troyn_streams_on_emulator(tmp_path):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    exe = str(tmp_path / "test_troyn_streams_emul")
    _build(exe, os.path.join(ROOT, "tests", "emul"), "libtroyhip_emul.so")
    _run(exe, "128")


@pytest.mark.gpu
def test_troyn_streams_on_gpu(tmp_path):
    exe = str(tmp_path / "test_troyn_streams")
    _build(exe, os.path.join(ROOT, "troy_amd"), "libtroyhip.so")
    _run(exe, "4096")
