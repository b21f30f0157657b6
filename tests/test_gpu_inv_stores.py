"""The plain stores of the single-pass inverse transform at N = 2^15 (ntt1_inv_body): thread t of the workgroup holds coefficient t + 1024 r in register r
(the last stage pairs register r with r + 16) and writes 32 values per row, canonical.  A store that goes to the wrong register position, or leaves
before its canonicalisation, puts 1024 consecutive coefficients in the wrong place or leaves them lazy -- so every one of the 32 positions is compared
on its own.  The test pins what any re-ordering of those stores (per register group, behind the last-stage butterflies: docs/LAB_NOTEBOOK.md) has to keep.

Two ciphertexts of two polynomials are small launches, which take the two-pass kernels: TROYHIP_NTT=single in a child process forces the single-pass
kernel on them (asserted through the path counters and through the NAME of the instance the launches carry), TROYHIP_NTT=twopass in another gives
the same transform by the other route, and the oracle gives it a third time.  One prime set per instance: 58 bits (guard-free integer), 60 bits (guarded integer), 49 bits (FP64).  Rows: all zero, every residue at p - 1, uniform."""
import os

import numpy as np
import pytest

import cases
import hoist_cases as HC
import round_cases as RC
from troy_amd import synth
from troy_amd.capi import CKKS

pytestmark = pytest.mark.gpu

N = 32768
SETS = {"lean58": [58, 58, 58], "guarded60": [60, 60, 60], "fp49": [49, 49, 49]}  # the widths of the data limbs; the special prime has the same
INSTANCE = {"lean58": "ntt1_inv_kernel<true, false>", "guarded60": "ntt1_inv_kernel<false, false>", "fp49": "ntt1_inv_fp_kernel<false>"}  # plain stores

CHILD = """
import numpy as np
from troy_amd import capi
cfg = dict(scheme=%d, N=%d, bits=%r, tbits=0)
primes = api.CoeffModulus.Create(cfg["N"], cfg["bits"])
ctx = api.SEALContext(cfg["scheme"], cfg["N"], primes, 0)
ev = api.Evaluator(ctx)
data = np.load(%r)
class S: pass
S.ctx = ctx
kernels = RC.Kernels(S)
s0 = HC.route_stats()
with kernels:
    got = ev.transformFromNtt(api.Ciphertext.from_numpy(ctx, data, True, 1.0, 1)).cpu()
d = HC.delta(HC.route_stats(), s0)
assert (HC.single_pass(d) > 0, HC.two_pass(d) > 0) == %r, d
want = %r  # the instance the launches must name (a build that records no names, the emulator's, leaves `on` false)
if kernels.on and want:
    inv = {n: k for n, k in kernels.calls.items() if "ntt1" in n or "ntt2" in n}
    assert inv and all(want in n for n in inv), (want, kernels.calls)
print("kernels", kernels.calls)
np.save(%r, got)
"""


def inputs(primes, seed):
    """[2 ciphertexts][2 polynomials][K][N]: ciphertext 0 = (all zero, every residue p - 1), ciphertext 1 uniform"""
    a = synth.uniform_ct(seed, primes, 2, N, 2)
    a[0, 0] = 0
    a[0, 1] = np.asarray(primes, dtype=np.uint64)[:, None] - np.uint64(1)
    return a


@pytest.mark.parametrize("name", list(SETS))
def test_inverse_stores_every_register_position(name, tmp_path):
    bits = SETS[name] + SETS[name][:1]
    cfg = dict(scheme=CKKS, N=N, bits=bits, tbits=0)
    orc = cases.oracle_backend(cfg)
    primes = [int(p) for p in orc.primes][:-1]  # the data level
    assert [p.bit_length() for p in primes] == SETS[name]
    a = inputs(primes, 77)
    src = str(tmp_path / "in.npy")
    np.save(src, a)
    exp = np.stack([orc.export(orc.from_ntt(orc.ct(a[i], True))).data for i in range(2)])
    got = {}
    for form, routes in (("single", (True, False)), ("twopass", (False, True))):
        dst = str(tmp_path / (form + ".npy"))
        RC.run_in_child(CHILD % (CKKS, N, bits, src, routes, INSTANCE[name] if form == "single" else "", dst), {"TROYHIP_NTT": form})
        got[form] = np.load(dst)
        assert got[form].shape == a.shape
    for r in range(32):  # register position r of thread t: coefficients 1024 r .. 1024 r + 1023
        pos = slice(1024 * r, 1024 * (r + 1))
        for j, p in enumerate(primes):
            assert (got["single"][:, :, j, pos] < np.uint64(p)).all(), (name, "register", r, "limb", j, "not canonical")
        assert np.array_equal(got["single"][..., pos], exp[..., pos]), (name, "register", r, "against the oracle", np.argwhere(got["single"][..., pos] != exp[..., pos])[:4])
        assert np.array_equal(got["single"][..., pos], got["twopass"][..., pos]), (name, "register", r, "against the two-pass kernels")
    # what the rows are: the zero row stays zero, and the inverse transform of the constant p - 1 is p - 1 at coefficient 0 alone
    assert not got["single"][0, 0].any()
    assert np.array_equal(got["single"][0, 1, :, 0], np.asarray(primes, dtype=np.uint64) - np.uint64(1)) and not got["single"][0, 1, :, 1:].any()
