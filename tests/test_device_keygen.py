"""Device key generation (troyhip_keygen / troyhip_create_relin_key / _galois_keys / _kswitch_key) on the emulator build of the kernels: every key
of a call is byte-identical to the host form called with the same seed, secret key and element.  tests/test_gpu_keygen.py runs the same checks on
an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import enc_cases as E
import keygen_cases as G
from conftest import ROOT
from troy_amd.capi import BFV, BGV, CKKS

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
NAMES = cases.SMALL + sorted(REJ_CFGS)


def setup_for(name):
    if name in REJ_CFGS:
        cfg = REJ_CFGS[name]
        return G.Setup.from_cfg(cfg, primes=cfg["primes"])
    return G.Setup.from_cfg(cases.CONFIGS[name])


@pytest.mark.parametrize("name", NAMES)
def test_keygen_matches_host(name, emul_api):
    S = setup_for(name)
    for batch in (1, 3, 17):
        G.check_keygen(S, batch, with_pk=True)
        G.check_keygen(S, batch, with_pk=False)
    G.check_keygen(S, 3, with_pk=True, pad=S.N + 5)  # strided outputs


@pytest.mark.parametrize("name", NAMES)
def test_relin_and_kswitch_keys_match_host(name, emul_api):
    S = setup_for(name)
    G.check_relin(S)
    G.check_kswitch(S)


@pytest.mark.parametrize("name", NAMES)
def test_galois_keys_match_host(name, emul_api):
    """the full default set, the automorphism set and a repeated element, all in one call"""
    S = setup_for(name)
    elts = S.kg.galoisEltsAll() + S.kg.automorphismElts() + [3]
    dev = G.check_galois(S, elts)
    assert np.array_equal(dev[elts.index(3)].to_numpy(), dev[-1].to_numpy())


def test_rejections_happen(emul_api):
    """a relin key of this case draws thousands of rejected words: the ranks, not the word positions, place the draws"""
    S = setup_for("ckks_n256_rej60")
    expected = (S.K - 1) * N_REJ * sum(E.rejection_rate(p) for p in S.primes)
    assert expected > 40, expected
    G.check_relin(S)


def test_bgv_error_is_a_multiple_of_t(emul_api):
    """c0 + c1 s - [l == j] (q_special mod p_j) src_j of a BGV key is t e with a small e, in every digit"""
    api = emul_api
    S = setup_for("bgv_n128_k4")
    rc, key = S.device_relin_rc()
    assert rc == 0, key
    K, N, t = S.K, S.N, S.t
    s2 = [[int(S.sk[l][n]) ** 2 % S.primes[l] for n in range(N)] for l in range(K)]
    for j in range(K - 1):
        rows = np.zeros((K, N), dtype=np.uint64)
        for l in range(K):
            p = S.primes[l]
            c0, c1, sk = key[j, 0, l].astype(object), key[j, 1, l].astype(object), S.sk[l].astype(object)
            v = (c0 + c1 * sk) % p
            if l == j:
                v = (v - (S.primes[K - 1] % p) * np.array(s2[l], dtype=object)) % p
            rows[l] = v.astype(np.uint64)
        buf = api.DeviceBuffer.from_numpy(rows)
        S.ctx.ntt(buf, K, S.primes[:K], inverse=True)
        coeff = buf.to_numpy().reshape(K, N)
        for l in range(K):
            p = S.primes[l]
            centred = [int(x) - p if int(x) > p // 2 else int(x) for x in coeff[l]]
            assert all(c % t == 0 and abs(c // t) <= 21 for c in centred), (j, l)
            assert any(c != 0 for c in centred)


def test_argument_errors_match_host(emul_api):
    api = emul_api
    from troy_amd import capi
    S = setup_for("bfv_n128_k4")
    N = S.N
    for bad in (4, 2 * N, 2 * N + 1):  # even, and >= 2N
        rc, msg = S.device_galois_rc([bad])
        assert rc == capi.INVALID_ARGUMENT and msg == "Galois element is not valid", (bad, msg)
        with pytest.raises(capi.InvalidArgument) as ei:
            S.host_galois(bad)
        assert str(ei.value) == msg
    # a bad element anywhere in the list: refused before anything is written
    elts = np.array([3, 5, 6], dtype=np.uint32)
    bufs = [api.DeviceBuffer(S.ksk_words()) for _ in elts]
    for b in bufs:
        b.zero()
    table = (C.c_void_p * 3)(*[b.ptr for b in bufs])
    rc = S.lib.troyhip_create_galois_keys(S.ctx.h, C.c_uint64(1), C.c_uint64(2), C.c_void_p(S.dsk.ptr), G._p(elts), table, C.c_uint64(3), None)
    assert rc == capi.INVALID_ARGUMENT and S.lib.troyhip_last_error().decode() == "Galois element is not valid"
    assert all(not b.to_numpy().any() for b in bufs)
    # count outside 1 .. 65535, null pointers
    rc, msg = S.device_galois_rc([])
    assert rc == capi.INVALID_ARGUMENT and msg == "batch must lie in 1 .. 65535"
    rc, msg = S.device_keygen_rc(G.seeds_for(1), batch=0)
    assert rc == capi.INVALID_ARGUMENT and msg == "batch must lie in 1 .. 65535"
    rc, msg = S.device_keygen_rc(G.seeds_for(1), batch=65536)
    assert rc == capi.INVALID_ARGUMENT
    out = api.DeviceBuffer(S.ksk_words())
    assert S.lib.troyhip_create_relin_key(S.ctx.h, C.c_uint64(1), C.c_uint64(2), None, C.c_void_p(out.ptr), None) == capi.INVALID_ARGUMENT
    assert S.lib.troyhip_create_relin_key(S.ctx.h, C.c_uint64(1), C.c_uint64(2), C.c_void_p(S.dsk.ptr), None, None) == capi.INVALID_ARGUMENT
    assert S.lib.troyhip_create_kswitch_key(S.ctx.h, C.c_uint64(1), C.c_uint64(2), C.c_void_p(S.dsk.ptr), None, C.c_void_p(out.ptr), None) == capi.INVALID_ARGUMENT
    assert S.lib.troyhip_create_galois_keys(S.ctx.h, C.c_uint64(1), C.c_uint64(2), C.c_void_p(S.dsk.ptr), None, table, C.c_uint64(1), None) == capi.INVALID_ARGUMENT
    null_table = (C.c_void_p * 1)(None)
    assert S.lib.troyhip_create_galois_keys(S.ctx.h, C.c_uint64(1), C.c_uint64(2), C.c_void_p(S.dsk.ptr), G._p(elts), null_table, C.c_uint64(1),
                                            None) == capi.INVALID_ARGUMENT
    assert S.lib.troyhip_keygen(S.ctx.h, None, C.c_void_p(out.ptr), C.c_uint64(0), None, C.c_uint64(0), C.c_uint64(1), None) == capi.INVALID_ARGUMENT
    assert S.lib.troyhip_keygen(S.ctx.h, G._p(G.seeds_for(1)), None, C.c_uint64(0), None, C.c_uint64(0), C.c_uint64(1), None) == capi.INVALID_ARGUMENT


def test_single_prime_context_refuses_like_host(emul_api):
    """K = 1: "keyswitching is not supported by the context", a logic error, from every key-switching form; an element check comes first"""
    from troy_amd import capi
    S = G.Setup(CKKS, 64, [E.rejecting_primes(64, 1)[0]], 0)
    assert S.K == 1
    with pytest.raises(capi.LogicError) as ei:
        S.host_relin()
    msg = str(ei.value)
    assert msg == "keyswitching is not supported by the context"
    for rc, m in (S.device_relin_rc(), S.device_galois_rc([3]), S.device_kswitch_rc(S.sk)):
        assert rc == capi.LOGIC_ERROR and m == msg
    rc, m = S.device_galois_rc([2])
    assert rc == capi.INVALID_ARGUMENT and m == "Galois element is not valid"
    G.check_keygen(S, 2)  # the secret and public keys need no key switching


def test_host_only_context_is_refused(emul_api):
    api = emul_api
    from troy_amd import capi
    ctx = api.SEALContext(BFV, 64, api.CoeffModulus.Create(64, [40, 40, 40]), api.PlainModulus.Batching(64, 10), host_only=True)
    msg = "this context was created host-only (troyhip_context_create_host)"
    sk = np.zeros(ctx.key_limbs * 64, dtype=np.uint64)
    out = np.zeros((ctx.key_limbs - 1) * 2 * ctx.key_limbs * 64, dtype=np.uint64)
    lib = ctx.lib
    assert lib.troyhip_create_relin_key(ctx.h, C.c_uint64(1), C.c_uint64(2), G._p(sk), G._p(out), None) == capi.LOGIC_ERROR
    assert lib.troyhip_last_error().decode() == msg
    assert lib.troyhip_keygen(ctx.h, G._p(G.seeds_for(1)), G._p(sk), C.c_uint64(0), None, C.c_uint64(0), C.c_uint64(1), None) == capi.LOGIC_ERROR
    assert lib.troyhip_last_error().decode() == msg


TAIL_SCRIPT = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
from troy_amd import api, capi
import enc_cases as E, keygen_cases as G
lib = capi.load({emul!r})
api.KernelProvider.initialize(0, _lib=lib)
S = G.Setup(capi.CKKS, {N}, E.rejecting_primes({N}, 3), 0)
G.check_keygen(S, 5)
G.check_relin(S)
G.check_galois(S, [3, 5, 2 * {N} - 1])
print("tail_items", capi.stat("enc_tail_items", lib))
"""


def test_short_window_tail(emul_api):
    """TROYHIP_ENC_MARGIN=0 (probe switch): every window that meets a rejection comes up short and the sequential tail finishes it; same bytes"""
    script = TAIL_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), emul=EMUL, N=N_REJ)
    env = dict(os.environ, TROYHIP_ENC_MARGIN="0")
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    n = int(out.stdout.split("tail_items")[1].split()[0])
    assert n > 0, out.stdout


SPLIT_SCRIPT = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
from troy_amd import api, capi
import keygen_cases as G
lib = capi.load({emul!r})
api.KernelProvider.initialize(0, _lib=lib)
S = G.Setup(capi.BGV, 128, api.CoeffModulus.Create(128, [40, 36, 36, 40]), api.PlainModulus.Batching(128, 10))
G.check_galois(S, S.kg.galoisEltsAll() + [3])
G.check_relin(S)
print("split ok")
"""


def test_split_runs_match_host(emul_api):
    """TROYHIP_KEYGEN_RUN=2 (probe switch): a call of 14 Galois keys runs as seven runs of two keys; every key still matches the host"""
    script = SPLIT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), emul=EMUL)
    env = dict(os.environ, TROYHIP_KEYGEN_RUN="2")
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "split ok" in out.stdout


@pytest.mark.parametrize("name", ["bfv_n128_k4", "bgv_n128_k4", "ckks_n128_k6"])
def test_python_device_forms(name, emul_api):
    """KeyGenerator.create*(device=True) hold the host keys; keygenBatch == KeyGenerator(seed) per row"""
    api = emul_api
    S = setup_for(name)
    kg = S.kg
    rk = kg.createRelinKeys(device=True)
    assert np.array_equal(rk.keys[0].to_numpy().reshape(S.ksk_shape()), kg.createRelinKeys())
    gk = kg.createGaloisKeys(device=True)
    host = kg.createGaloisKeys([3, 2 * S.N - 1])
    for e, h in host.items():
        assert np.array_equal(gk.keys[api.GaloisKeys.getIndex(e)].to_numpy().reshape(S.ksk_shape()), h)
    assert len(gk.keys) == len(set(kg.galoisEltsAll()))
    ak = kg.createAutomorphismKeys(device=True)
    assert sorted(ak.keys) == sorted(api.GaloisKeys.getIndex(e) for e in kg.automorphismElts())
    e = kg.automorphismElts()[-1]
    assert np.array_equal(ak.keys[api.GaloisKeys.getIndex(e)].to_numpy().reshape(S.ksk_shape()), kg.createAutomorphismKeys()[e])
    # every createKeySwitchingKeys call of a generator draws from a seed of its own: the forms are compared at equal call numbers of two generators
    other, third = api.KeyGenerator(S.ctx, seed=(3, 4)).secretKey(), api.KeyGenerator(S.ctx, seed=(4, 3)).secretKey()
    twin = api.KeyGenerator(S.ctx, seed=S.seed)
    for new_key in (other, third, other):
        ks = kg.createKeySwitchingKeys(new_key, device=True)
        assert np.array_equal(ks.keys[0].to_numpy().reshape(S.ksk_shape()), twin.createKeySwitchingKeys(new_key))
    with pytest.raises(ValueError):
        ks.set_device(1, api.DeviceBuffer(5))
    seeds = G.seeds_for(3)
    sk, pk = api.KeyGenerator.keygenBatch(S.ctx, seeds)
    assert sk.shape == (3, S.K, S.N) and pk.shape == (3, 2, S.K, S.N)
    for i in range(3):
        g = api.KeyGenerator(S.ctx, seed=tuple(int(x) for x in seeds[i]))
        assert np.array_equal(sk.to_numpy().reshape(sk.shape)[i], g.secretKey())
        assert np.array_equal(pk.to_numpy().reshape(pk.shape)[i], g.createPublicKey())


@pytest.mark.parametrize("name", ["bfv_n128_k4", "bgv_n128_k4"])
def test_end_to_end_rotate_and_relinearize(name, emul_api):
    """device keys -> encryptBatch -> rotateRows and multiply-relinearize -> decrypt: the expected slots"""
    api = emul_api
    S = setup_for(name)
    N, t, B = S.N, S.t, 3
    sk, pk = api.KeyGenerator.keygenBatch(S.ctx, [[11, 12]])
    kg = api.KeyGenerator(S.ctx, seed=(11, 12))
    assert np.array_equal(sk.to_numpy().reshape(S.K, N), kg.secretKey())
    rk, gk = kg.createRelinKeys(device=True), kg.createGaloisKeys(device=True)
    enc = api.BatchEncoder(S.ctx)
    rng = np.random.default_rng(7)
    x = rng.integers(0, t, (B, N), dtype=np.uint64)
    px = np.stack([enc.encode(v) for v in x])
    ct = api.Encryptor(S.ctx, pk.to_numpy().reshape(2, S.K, N), seed=(5, 5)).encryptBatch(px)
    ev = api.Evaluator(S.ctx)
    dsk = api.DeviceBuffer.from_numpy(kg.secretKey())
    half = N // 2
    for step in (1, -1, 5):
        rot = ev.rotateRows(ct, step, gk)
        plain = ev.decrypt(rot, dsk)
        for b in range(B):
            exp = np.concatenate([np.roll(x[b][:half], -step), np.roll(x[b][half:], -step)])
            assert np.array_equal(np.asarray(enc.decode(plain[b]), dtype=np.uint64), exp), (step, b)
    prod = ev.multiply(ct, ct)
    ev.relinearizeInplace(prod, rk)
    assert prod.size() == 2
    plain = ev.decrypt(prod, dsk)
    for b in range(B):
        exp = (x[b].astype(object) ** 2 % t).astype(np.uint64)
        assert np.array_equal(np.asarray(enc.decode(plain[b]), dtype=np.uint64), exp), b
