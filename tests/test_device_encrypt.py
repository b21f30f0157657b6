"""Device encryption (troyhip_encrypt / troyhip_encrypt_symmetric / troyhip_expand_seed) on the emulator build of the kernels: item i of a batch
is byte-identical to the host form called with item i's seed.  tests/test_gpu_encrypt.py runs the same checks on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import enc_cases as E
from conftest import ROOT
from troy_amd.capi import BFV, CKKS

EMUL = os.path.join(ROOT, "tests", "emul", "libtroyhip_emul.so")


@pytest.fixture(scope="module")
def emul_api():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    from troy_amd import api, capi
    lib = capi.load(EMUL)
    old = api.KernelProvider._lib
    api.KernelProvider.initialize(0, _lib=lib)
    yield api
    api.KernelProvider._lib = old


N_REJ = 256
REJ_CFGS = {  # 60-bit primes where about one word in 17 is rejected by uniform_below(p)
    "ckks_n256_rej60": dict(scheme=CKKS, N=N_REJ, tbits=0, primes=E.rejecting_primes(N_REJ, 3)),
    "bfv_n256_rej60": dict(scheme=BFV, N=N_REJ, tbits=20, primes=E.rejecting_primes(N_REJ, 3)),
}


def setup_for(name):
    if name in REJ_CFGS:
        cfg = REJ_CFGS[name]
        return E.Setup.from_cfg(cfg, primes=cfg["primes"])
    return E.Setup.from_cfg(cases.CONFIGS[name])


def levels_of(S, form):
    return S.data_levels() if (S.scheme == CKKS or form.endswith("0")) else [S.ctx.first_limbs]


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("name", cases.SMALL + sorted(REJ_CFGS))
def test_device_matches_host(name, form, emul_api):
    S = setup_for(name)
    for limbs in levels_of(S, form):
        for batch in (1, 3, 17):
            E.check_form(S, form, limbs, batch, per_item=True)
        E.check_form(S, form, limbs, 3, per_item=False, pad=S.N)  # one plaintext for every item, strided output


def test_rejections_happen(emul_api):
    """the draws of this case include hundreds of rejected words: the ranks of the scan, not the word positions, decide where a draw lands"""
    S = setup_for("ckks_n256_rej60")
    batch, limbs = 17, S.ctx.first_limbs
    expected = batch * N_REJ * sum(E.rejection_rate(p) for p in S.primes[:limbs])
    assert expected > 200, expected
    E.check_form(S, "sk0", limbs, batch)
    E.check_form(S, "sks", limbs, batch)
    a = E.a_seeds_for(batch, base=99)
    dev = S.expand_device(a, limbs)
    for b in range(batch):
        assert np.array_equal(dev[b], S.expand_host(a[b], limbs))


TAIL_SCRIPT = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
from troy_amd import api, capi
import enc_cases as E
lib = capi.load({emul!r})
api.KernelProvider.initialize(0, _lib=lib)
S = E.Setup(capi.CKKS, {N}, E.rejecting_primes({N}, 3), 0)
for form in ("sk", "sks", "sk0"):
    E.check_form(S, form, S.ctx.first_limbs, 5)
a = E.a_seeds_for(4)
dev = S.expand_device(a, 2)
assert all(np.array_equal(dev[b], S.expand_host(a[b], 2)) for b in range(4))
print("tail_items", capi.stat("enc_tail_items", lib))
"""


def test_short_window_tail(emul_api):
    """TROYHIP_ENC_MARGIN=0 (probe switch): every window that meets a rejection comes up short and the sequential tail finishes it; same bytes"""
    script = TAIL_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), emul=EMUL, N=N_REJ)
    env = dict(os.environ, TROYHIP_ENC_MARGIN="0")
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    n = int(out.stdout.split("tail_items")[1].split()[0])
    assert n > 0, out.stdout


@pytest.mark.parametrize("name", ["bfv_n128_k4", "ckks_n128_k6"])
def test_split_batches(name, emul_api):
    """a batch of 64 equals two calls of 32 with the corresponding seeds"""
    S = setup_for(name)
    limbs = S.ctx.first_limbs
    rng = np.random.default_rng(5)
    seeds, a_seeds = E.seeds_for(64, base=3), E.a_seeds_for(64, base=3)
    plains = S.plains(64, limbs, rng)
    for form in ("pk", "sks"):
        a = a_seeds if form == "sks" else None
        whole, _ = S.device(form, seeds, limbs, plains, a_seeds=a)
        h1, _ = S.device(form, seeds[:32], limbs, plains[:32], a_seeds=None if a is None else a[:32])
        h2, _ = S.device(form, seeds[32:], limbs, plains[32:], a_seeds=None if a is None else a[32:])
        assert np.array_equal(whole, np.concatenate([h1, h2]))
        again, _ = S.device(form, seeds, limbs, plains, a_seeds=a)
        assert np.array_equal(whole, again)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6", "bgv_n128_k4"])
def test_expand_seed(name, emul_api):
    S = setup_for(name)
    for limbs in S.data_levels():
        a = E.a_seeds_for(5, base=limbs)
        dev = S.expand_device(a, limbs, pad=7)
        for b in range(5):
            assert np.array_equal(dev[b], S.expand_host(a[b], limbs))
    # the c1 a seeded encryption stores is the expansion of its seed
    seeds, a = E.seeds_for(3), E.a_seeds_for(3, base=11)
    ct, _ = S.device("sks0", seeds, S.ctx.first_limbs, a_seeds=a)
    assert np.array_equal(ct[:, 1], S.expand_device(a, S.ctx.first_limbs))


@pytest.mark.parametrize("name", ["bfv_n128_k4", "ckks_n128_k6", "bgv_n128_k4"])
def test_python_batch_forms(name, emul_api):
    """Encryptor(seed).xBatch(..) == the same number of successive single calls, and the call after the batch matches too (the counter)"""
    api = emul_api
    S = setup_for(name)
    limbs = S.ctx.first_limbs
    P = S.plains(4, limbs, np.random.default_rng(8))
    scale = 2.0**20 if S.scheme == CKKS else 1.0

    def pair():
        a, b = api.Encryptor(S.ctx, S.pk, seed=(77, 5)), api.Encryptor(S.ctx, S.pk, seed=(77, 5))
        a.setSecretKey(S.sk)
        b.setSecretKey(S.sk)
        return a, b

    def as_host(ct):
        return ct.buf.to_numpy().reshape(ct.batch, 2, ct.limbs, S.N)

    for batch_fn, single_fn, arg in (("encryptBatch", "encrypt", P), ("encryptSymmetricBatch", "encryptSymmetric", P),
                                     ("encryptZeroBatch", "encryptZero", 4), ("encryptZeroSymmetricBatch", "encryptZeroSymmetric", 4)):
        dev, host = pair()
        ct = getattr(dev, batch_fn)(arg, scale) if not isinstance(arg, int) else getattr(dev, batch_fn)(arg)
        assert ct.batch == 4 and ct.size() == 2 and ct.limbs == limbs and ct.is_ntt_form == (S.scheme == CKKS)
        exp = np.stack([getattr(host, single_fn)(P[i]) if not isinstance(arg, int) else getattr(host, single_fn)() for i in range(4)])
        assert np.array_equal(as_host(ct), exp), batch_fn
        nxt = getattr(dev, single_fn)(P[0]) if not isinstance(arg, int) else getattr(dev, single_fn)()
        exp_next = getattr(host, single_fn)(P[0]) if not isinstance(arg, int) else getattr(host, single_fn)()
        assert np.array_equal(nxt, exp_next), batch_fn
    # the zero forms at a lower level
    if len(S.data_levels()) > 1:
        dev, host = pair()
        ct = dev.encryptZeroBatch(2, limbs=limbs - 1)
        assert np.array_equal(as_host(ct), np.stack([host.encryptZero(limbs - 1) for _ in range(2)]))


def test_argument_errors_match_host(emul_api):
    from troy_amd import capi
    S = setup_for("bfv_n128_k4")
    first = S.ctx.first_limbs
    seeds = E.seeds_for(2)
    P = S.plains(2, first, np.random.default_rng(1))
    K = S.ctx.key_limbs
    cases_ = [  # (device call, host call): same status and message
        (lambda: S.device_rc("pk", seeds, K, None), lambda: S.host("pk0", seeds[0], K)),                       # the key level is no data level
        (lambda: S.device_rc("sk", seeds, first - 1, P), None),                                                  # BFV plaintext below the first level
        (lambda: S.device_rc("sks0", seeds, first, a_seeds=np.array([5, 0], dtype=np.uint64)),
         lambda: S.host("sks0", seeds[0], first, a_seed=0)),                                                     # a zero a_seed
    ]
    for dev, host in cases_:
        rc, msg, _ = dev()
        assert rc == capi.INVALID_ARGUMENT, msg
        if host is not None:
            with pytest.raises(capi.InvalidArgument) as ei:
                host()
            assert str(ei.value) == msg
        else:
            assert msg == "plain is not valid for encryption parameters"
    # more than N coefficients
    big = np.zeros((2, S.N + 1), dtype=np.uint64)
    rc, msg, _ = S.device_rc("pk", seeds, first, big)
    assert rc == capi.INVALID_ARGUMENT and msg == "plain is not valid for encryption parameters"
    with pytest.raises(capi.InvalidArgument, match="plain is not valid"):
        S.host("pk", seeds[0], first, big[0])
    # batch 0 and null pointers
    rc, msg, _ = S.device_rc("pk0", seeds, first, batch=0)
    assert rc == capi.INVALID_ARGUMENT
    import ctypes as C
    st = capi.CtStruct(None, 2 * first * S.N, 0, first, 0, 0.0, 0)
    rc = S.lib.troyhip_encrypt(S.ctx.h, C.c_void_p(S.dpk.ptr), E._p(seeds), None, C.c_uint64(0), C.c_uint64(0), C.c_double(1.0), C.byref(st), C.c_uint64(2), None)
    assert rc == capi.INVALID_ARGUMENT
    rc = S.lib.troyhip_encrypt(S.ctx.h, None, E._p(seeds), None, C.c_uint64(0), C.c_uint64(0), C.c_double(1.0), None, C.c_uint64(2), None)
    assert rc == capi.INVALID_ARGUMENT
    rc = S.lib.troyhip_expand_seed(S.ctx.h, E._p(np.array([0], dtype=np.uint64)), first, C.c_void_p(S.dsk.ptr), C.c_uint64(0), C.c_uint64(1), None)
    assert rc == capi.INVALID_ARGUMENT and S.lib.troyhip_last_error().decode() == "the seed of a seeded ciphertext is not zero"
