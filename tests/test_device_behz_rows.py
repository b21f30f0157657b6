"""The large-base matrix-core BEHZ kernels at every limb count that changes their shape (tests/behz_row_cases.py), on the emulator build of the
kernels, which has the MFMA instruction: the 32-bit m~ sum through LDS and the single evaluation of the m_sk row are checked bit for bit before any
run on a device.  tests/test_gpu_behz_rows.py runs the same cases on an MI355X.

Sensitivity, shown once on a scratch copy with this build (nothing of it is kept): behz2_floor_sk_kernel writing a negative alpha to LDS with its top digit
cleared (the sign extension lost) fails test_behz_rows[9] at "item 2", the item that carries the built quotients -1, -2, -3; items 0 and 1 pass."""
import os
import subprocess

import pytest

import behz_row_cases as BR
from conftest import ROOT

EMUL = os.path.join(ROOT, "tests", "emul", "libtroyhip_emul.so")

_setups = {}


@pytest.fixture(scope="module")
def emul_api():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    from troy_amd import api, capi
    lib = capi.load(EMUL)
    old = api.KernelProvider._lib
    api.KernelProvider.initialize(0, _lib=lib)
    yield api
    api.KernelProvider._lib = old


@pytest.mark.parametrize("L", BR.LIMBS)
def test_behz_rows(L, emul_api):
    BR.check(_setups, L)
