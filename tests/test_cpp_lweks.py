"""include/troyn.hpp: LWESwitchKey, KeyGenerator::createLWESwitchKey / extractionSecret and Evaluator::lweKeySwitch against the C ABI word for word, and
the pipeline extract -> lweKeySwitch -> blindRotateBatch returning f(message) (tests/cpp/test_troyn_lweks.cpp), compiled with plain g++ and linked against
the emulator build of the library.  The program writes the samples, the key and the results of one shape; the Python layer, given the same seeds and the
same samples, must produce the same bytes."""
import os
import subprocess

import numpy as np

import extprod_cases as XC
import lweks_cases as LC
from test_cpp_encrypt import ROOT, _build, _run
from troy_amd.capi import BFV

SRC = os.path.join(ROOT, "tests", "cpp", "test_troyn_lweks.cpp")


def _blocks(path):
    raw = np.fromfile(path, dtype=np.uint64)
    out, at = [], 0
    while at < raw.size:
        n = int(raw[at])
        out.append(raw[at + 1:at + 1 + n])
        at += 1 + n
    return out


def test_troyn_lweks_on_emulator(tmp_path):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    exe = str(tmp_path / "test_troyn_lweks_emul")
    libdir = os.path.join(ROOT, "tests", "emul")
    _build(exe, libdir, "libtroyhip_emul.so", src=SRC)
    dumped = str(tmp_path / "lweks.bin")
    _run(exe, dumped)
    c1, c0, key, switched, plain = _blocks(dumped)
    # the Python side on the same library: the same seeds give the same key, the same samples the same words
    from troy_amd import api, capi
    old = api.KernelProvider._lib
    api.KernelProvider.initialize(0, _lib=capi.load(os.path.join(libdir, "libtroyhip_emul.so")))
    try:
        N, n, w = 256, 16, 8
        ctx, _ = XC.real_context(BFV, N, (40, 40, 40, 40), 14)
        kg = api.KeyGenerator(ctx, seed=(61, 62))
        LK = kg.createLWESwitchKey(LC.Z16, base_bits=w)
        assert np.array_equal(LK.cpu().reshape(-1), key)
        R = c0.size
        assert c1.size == R * N and switched.size == plain.size == R * (n + 1)
        lwes = api.LWEBatch(ctx, R, 1, 1, c1=api.DeviceBuffer.from_numpy(c1.copy()), c0=api.DeviceBuffer.from_numpy(c0.copy()))
        ev = api.Evaluator(ctx)
        assert np.array_equal(ev.lweKeySwitch(lwes, LK, to_2n=True).to_numpy(), switched)
        assert np.array_equal(ev.lweKeySwitch(lwes, LK, to_2n=False).to_numpy(), plain)
        assert np.array_equal(plain.reshape(R, n + 1), LC.LM.key_switch_fast(c1.reshape(R, N), c0, LK.cpu(), int(ctx.coeff_modulus[0]), w, False))
    finally:
        api.KernelProvider._lib = old
