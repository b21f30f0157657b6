"""include/troyn.hpp: Decryptor::invariantNoiseBudget / invariantNoiseBudgetBatch (tests/cpp/test_troyn_noise.cpp) against the reference's recorded
budgets of one small BFV and one small BGV parameter set, compiled with plain g++.  CPU: linked against the emulator build of the library;  GPU:
against libtroyhip.so, run on the device."""
import os
import subprocess

import pytest

import noise_cases as NC
from test_cpp_encrypt import ROOT, _build, _run

SRC = os.path.join(ROOT, "tests", "cpp", "test_troyn_noise.cpp")
SETS = {"bfv_n128_k4": "bfv", "bgv_n128_k4": "bgv"}
STAGES = [["pk"], ["pk", "multiply"], ["pk", "multiply", "relinearize"], ["pk", "multiply", "relinearize", "modswitch_to_last"]]


def _args(name):
    cfg = NC.CONFIGS[name]
    records = {tuple(r["sequence"]): r["budget"] for r in NC.records_of(name)}
    return [SETS[name], str(cfg["N"]), str(cfg["tbits"]), ",".join(str(b) for b in cfg["bits"])] + [str(records[tuple(s)]) for s in STAGES]


@pytest.mark.parametrize("name", sorted(SETS))
def test_troyn_noise_on_emulator(name, tmp_path):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    exe = str(tmp_path / "test_troyn_noise_emul")
    _build(exe, os.path.join(ROOT, "tests", "emul"), "libtroyhip_emul.so", src=SRC)
    _run(exe, *_args(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_troyn_noise_on_gpu(name, tmp_path):
    exe = str(tmp_path / "test_troyn_noise")
    _build(exe, os.path.join(ROOT, "troy_amd"), "libtroyhip.so", src=SRC)
    _run(exe, *_args(name))
