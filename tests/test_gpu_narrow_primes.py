"""Coefficient primes below 2^33 at real ring sizes on the MI355X (run with `-m gpu`): the standalone transform by prime width and kernel form, the
whole op list of the named narrow parameter sets at both launch plans, and seeded random narrow sets -- exact integer equality against the CPU oracle
(tests/narrow_cases.py; the same helpers run on the host emulator from tests/test_emul_parity.py).  Every test that targets a kernel form reads the
path counters, so that a launch which lands on another kernel fails instead of passing there."""
import os
import subprocess
import sys

import pytest

import cases
import narrow_cases as NP
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from troy_amd import api, capi
    capi.load()  # the gfx950 library or a loud failure -- never a fallback
    api.KernelProvider.initialize(0)
    return api


@pytest.mark.parametrize("logn", [12, 13, 14, 15, 16, 17])
def test_ntt_widths_small_counts(logn, gpu, oracle_lib):
    """the smallest NTT prime, 20 .. 34-bit primes and a 60-bit one in ONE launch; uniform, zero, p - 1, alternating and delta rows.  A ragged row
    count takes the generic kernel, five whole groups the two-pass kernels (FP64 instances for everything below 2^50, integer for the 60-bit prime)"""
    NP.check_ntt_widths(gpu, oracle_lib, logn, "ragged", "generic")
    primes = NP.check_ntt_widths(gpu, oracle_lib, logn, "even", "ntt2")
    assert min(primes) == NP.smallest_ntt_prime(1 << logn) and max(primes) >> 59 == 1 and sum(p < (1 << 33) for p in primes) >= 6


@pytest.mark.parametrize("logn", [12, 13, 14, 15])
def test_ntt_widths_single_pass_by_itself(logn, gpu, oracle_lib):
    """the same rows at a count past the dispatcher's threshold: ntt1.hip by itself -- guarded integer butterflies for every prime below 2^33 (and the
    60-bit one), the FP64 instance for the 34-bit prime; every row against the oracle"""
    NP.check_ntt_widths(gpu, oracle_lib, logn, "large", "ntt1")


def test_ntt_widths_xcd_order(gpu, oracle_lib):
    """N = 2^15, the seven primes below 2^33 (one guarded class), 2049 rows each.  For 256 CUs the planner picks 19 rows of one prime per workgroup:
    7 x 108 = 756 workgroups -- more than two rounds of the chip, from where the XCD-aware order is taken, and not a multiple of 8, so the padded
    last eighth runs (fewer rows per prime make the planner pick more rows per workgroup and stay below two rounds).  The counter says the order ran.
    Every 5th row goes to the oracle: 5 is coprime to 7, so each prime has every 5th of its rows compared, and a workgroup -- 19 consecutive rows of
    one prime (16 on a part of 304 CUs) -- has at least three rows compared in each direction; the round trip covers every row"""
    from troy_amd import capi
    N = 32768
    primes = [p for p in NP.width_primes(gpu, N) if p < (1 << 33)]
    assert len(primes) == 7
    ctx = gpu.SEALContext(gpu.CKKS, N, primes, 0)
    rows = len(primes) * 2049
    buf = gpu.DeviceBuffer(rows * N)
    ctx.fill_uniform(buf, rows, primes, seed=79)
    x = NP.ntt_inputs(primes, rows, N, 0, x=buf.to_numpy().reshape(rows, N))
    del buf
    x0 = capi.stat("ntt1_xcd_launches")
    NP.check_ntt_rows(gpu, oracle_lib, ctx, primes, x, "ntt1", stride=5)
    assert capi.stat("ntt1_xcd_launches") == x0 + 4, "the XCD-aware workgroup order did not run"


@pytest.mark.parametrize("logn", [12, 15])
def test_ntt_negacyclic_product_vs_python_integers(logn, gpu):
    NP.check_ntt_convolution(gpu, logn)


def _child(code, env, timeout=900):
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    head = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from troy_amd import api\n"
            "from oracle import oracle\n"
            "import narrow_cases as NP\n"
            "api.KernelProvider.initialize(0)\n") % (tests_dir, ROOT)
    out = subprocess.run([sys.executable, "-c", head + code + "print('narrow ok')\n"], env={**os.environ, **env}, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and "narrow ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.parametrize("env,plan", [
    # integer kernels for every prime: below 2^33 the guarded asm butterfly on primes whose high word is zero, in both transforms
    ({"TROYHIP_FP64": "off"}, [(12, "large", "ntt1"), (15, "large", "ntt1"), (12, "even", "ntt2"), (16, "even", "ntt2")]),
    # the single-pass kernels forced at a small count, one size of each size class (whole limb in LDS / N = 2^15)
    ({"TROYHIP_NTT": "single"}, [(12, "even", "ntt1"), (14, "even", "ntt1"), (15, "even", "ntt1")]),
    ({"TROYHIP_NTT": "single", "TROYHIP_FP64": "off"}, [(13, "even", "ntt1"), (15, "even", "ntt1")]),
    # the two-pass kernels forced at a count the single pass would take
    ({"TROYHIP_NTT": "twopass"}, [(12, "large", "ntt2"), (15, "large", "ntt2")]),
])
def test_ntt_widths_under_library_switches(env, plan, gpu):
    """the oracle comparison repeated in child processes (the library reads its switches once), the counters asserting the forced form"""
    fp64 = env.get("TROYHIP_FP64") != "off"
    _child("".join("NP.check_ntt_widths(api, oracle, %d, %r, %r, fp64=%r)\n" % (logn, count, form, fp64) for logn, count, form in plan), env)


@pytest.mark.parametrize("name", cases.NARROW)
def test_named_sets_small_launch_plan(name, gpu, oracle_lib):
    """one ciphertext: the merged small-launch forms, every op of cases.scenario against the oracle"""
    assert NP.check_named_small_plan(name) >= 3


@pytest.mark.parametrize("name", cases.NARROW)
def test_named_sets_large_launch_plan(name, gpu, oracle_lib):
    """a batch past Context::small_launch and past the single-pass dispatcher's threshold: multiply, relinearize, (rescale,) rotate against the
    oracle on three items and against the one-ciphertext plan on every item"""
    cfg = cases.CONFIGS[name]
    B, d, primes = NP.check_named_large_plan(name)
    if cfg["N"] <= 32768:
        # the single-pass kernels took launches of this batch.  WHICH class a prime gets inside launch_ntt1 is a function of its width alone, and the
        # width-matrix tests above assert it exactly; here the counters can only be as sharp as the set: in a BGV / CKKS set every transformed prime is a
        # key prime, so without one in [2^50, 2^58) every integer launch is the guarded class, and the FP64 class runs iff a prime lies in [2^33, 2^50).
        # A BFV set also transforms its auxiliary base (50- or 58-bit primes of the library's own choice), which may take either class.
        assert d["ntt1_int_launches"] > 0, (name, B, d)
        if cfg["scheme"] != cases.BFV:
            assert not [p for p in primes if (1 << 50) <= p < (1 << 58)], "named BGV / CKKS sets: narrow and 60-bit primes only"
            assert (d["ntt1_fp_launches"] > 0) == bool([p for p in primes if (1 << 33) <= p < (1 << 50)]), (name, B, d)
    else:
        assert d["ntt1_int_launches"] == d["ntt1_fp_launches"] == 0 and d["ntt2_fp_launches"] > 0, (name, B, d)


# 24 seeds; the oracle alone says which sets are rejected (plain modulus equal to a 20-bit coefficient prime, not enough 18- or 20-bit primes at
# N = 2^15): 336 is the only one of these, 341 and 342 are two more and are left out
SEEDS = list(range(324, 341)) + list(range(343, 350))


def test_random_narrow_parameter_sets(gpu, oracle_lib):
    """24 seeded sets over widths of 18 .. 60 bits with the CKKS widths as drawn, N = 4096 / 8192 / 32768 (every level at 4096, the first above).  A
    set both sides reject is no pass: at most two of the seeds may be one"""
    rejected = []
    for seed in SEEDS:
        cfg, n = NP.check_narrow_random(seed, (4096, 8192, 32768))
        print(seed, cfg, n)
        if n is None:
            rejected.append((seed, cfg))
        else:
            assert n >= 3, cfg
    assert len(rejected) <= 2, rejected
