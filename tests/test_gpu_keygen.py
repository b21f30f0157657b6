"""Device key generation on the MI355X: every key of a call is byte-identical to the host form with the same seed, secret key and element (the
small shapes in full, rejecting 60-bit primes at N = 4096, and bench.py's three workload shapes on sampled keys of the whole default Galois set),
and a BGV N = 2^16 rotate chain under device-generated keys decrypts to the rotated slots.  At the bench shapes the keys are also compared
with the independent model of the streams (tests/sampler_model.py), and the noise of a device-drawn relin key with the exact CBD pmf."""
import ctypes as C

import numpy as np
import pytest

import cases
import enc_cases as E
import keygen_cases as G
import sampler_model as M
from troy_amd.capi import BFV, BGV, CKKS

pytestmark = pytest.mark.gpu

BENCH = {  # bench.py's workload parameters
    "bfv_n32768_l14": dict(scheme=BFV, N=32768, bits=[60] + [58] * 13 + [60], tbits=20),
    "ckks_n32768_chain": dict(scheme=CKKS, N=32768, bits=[60] + [40] * 13 + [60], tbits=0),
    "bgv_n65536_relin_rot": dict(scheme=BGV, N=65536, bits=[60] + [50] * 13 + [60], tbits=20),
}


NARROW = ["nar_bgv_n8192_k4", "nar_bfv_n4096_k3"]  # narrow data primes under 60-bit ends, and an all-narrow set (primes of 22 .. 32 bits)


@pytest.fixture(scope="module")
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


@pytest.mark.parametrize("name", cases.SMALL)
def test_small_shapes_match_host(name, gpu_api):
    S = G.Setup.from_cfg(cases.CONFIGS[name])
    for batch in (1, 3, 17):
        G.check_keygen(S, batch, with_pk=True)
        G.check_keygen(S, batch, with_pk=False)
    G.check_keygen(S, 3, pad=S.N + 5)
    G.check_relin(S)
    G.check_kswitch(S)
    G.check_galois(S, S.kg.galoisEltsAll() + S.kg.automorphismElts() + [3])


@pytest.mark.parametrize("name", NARROW)
def test_narrow_primes_match_host(name, gpu_api):
    """primes of 22 .. 32 bits: secret / public key, relin key, a key-switch key and Galois keys byte-identical to the host KeyGenerator"""
    S = G.Setup.from_cfg(cases.CONFIGS[name])
    G.check_keygen(S, 3, with_pk=True)
    G.check_keygen(S, 3, with_pk=False, pad=S.N + 5)
    G.check_relin(S)
    G.check_kswitch(S)
    elts = S.kg.galoisEltsAll()
    G.check_galois(S, elts, items=[0, len(elts) // 2, len(elts) - 1])


def test_rejecting_primes_n4096(gpu_api):
    S = G.Setup(CKKS, 4096, E.rejecting_primes(4096, 4), 0)
    G.check_keygen(S, 9)
    G.check_relin(S)
    G.check_kswitch(S)
    G.check_galois(S, S.kg.galoisEltsAll(), items=[0, 5, 21])


@pytest.mark.parametrize("name", sorted(BENCH))
def test_bench_shapes(name, gpu_api):
    """the relin key, and the first, middle and last keys of the default Galois set -- the whole set generated in one call"""
    S = G.Setup.from_cfg(BENCH[name])
    G.check_relin(S)
    elts = S.kg.galoisEltsAll()
    G.check_galois(S, elts, items=[0, len(elts) // 2, len(elts) - 1])
    G.check_keygen(S, 2)


def test_bgv_n65536_rotate_chain(gpu_api):
    api = gpu_api
    S = G.Setup.from_cfg(BENCH["bgv_n65536_relin_rot"])
    N, t = S.N, S.t
    sk, pk = api.KeyGenerator.keygenBatch(S.ctx, [[21, 22]])
    kg = api.KeyGenerator(S.ctx, seed=(21, 22))
    gk = kg.createGaloisKeys([S.ctx.galois_elt_from_step(1), S.ctx.galois_elt_from_step(-4)], device=True)
    rk = kg.createRelinKeys(device=True)
    enc = api.BatchEncoder(S.ctx)
    x = np.random.default_rng(3).integers(0, t, (2, N), dtype=np.uint64)
    ct = api.Encryptor(S.ctx, pk.to_numpy().reshape(2, S.K, N), seed=(8, 8)).encryptBatch(np.stack([enc.encode(v) for v in x]))
    ev = api.Evaluator(S.ctx)
    for step in (1, 1, -4, 1):
        ev.rotateRowsInplace(ct, step, gk)
    prod = ev.multiply(ct, ct)
    ev.relinearizeInplace(prod, rk)
    plain = ev.decrypt(prod, sk)
    half = N // 2
    for b in range(2):
        rot = np.concatenate([np.roll(x[b][:half], -(1 + 1 - 4 + 1)), np.roll(x[b][half:], -(1 + 1 - 4 + 1))])
        exp = (rot.astype(object) ** 2 % t).astype(np.uint64)
        assert np.array_equal(np.asarray(enc.decode(plain[b]), dtype=np.uint64), exp), b


# ---- the device against the independent model of the streams (tests/sampler_model.py) at the bench shapes, where the windows, the scan across
# workgroups and the LDS-staged scatter differ from anything the emulator-sized cases run.  The draws are recovered with Python integers and the
# oracle's NTT; nothing here goes through the host forms.
EDGE_SEEDS = {0: (0x5EED, 7), 63: (0x8000000000000123, 0), 127: (0xFFFFFFFFFFFFFFF0, 0x9000000000000001)}


def noise_at(S, c0, c1, l, src=None):
    """e of one limb of a key polynomial pair, from -(c0 + c1 s) + (q_special mod p_l) src; divided by t for BGV (None unless exact)"""
    p = S.primes[l]
    extra = None if src is None else M.mulmod(src, S.primes[-1] % p, p)
    return M.unscale(M.noise_of(c0, c1, S.sk[l], p, S.N, extra), S.t if S.scheme == BGV else 1)


@pytest.mark.parametrize("name", sorted(BENCH))
def test_keygen_b128_matches_model(name, gpu_api):
    """troyhip_keygen at B = 128: the secret key, c1 and the recovered noise of items 0, 63 and 127"""
    api = gpu_api
    S = G.Setup.from_cfg(BENCH[name])
    N, K, P, B = S.N, S.K, S.primes, 128
    seeds = G.seeds_for(B)
    for i, seed in EDGE_SEEDS.items():
        seeds[i] = seed
    sk, pk = api.KeyGenerator.keygenBatch(S.ctx, seeds)
    for i, seed in EDGE_SEEDS.items():
        s, a, e, _ = M.keygen(*seed, N, P)
        got_sk = sk.to_numpy(K * N, offset=i * K * N).reshape(K, N)
        got_pk = pk.to_numpy(2 * K * N, offset=i * 2 * K * N).reshape(2, K, N)
        assert np.array_equal(got_sk, M.lifted_ntt(s, N, P)), i
        assert np.array_equal(got_pk[1], a), i
        S.sk = got_sk
        for l in (0, K - 1):
            assert np.array_equal(noise_at(S, got_pk[0, l], got_pk[1, l], l), e), (i, l)


def check_key_digits(S, buf, stream_id, src0, what):
    """digits 0 and K - 2 of a device key: c1 in limbs 0 and K - 1 against the model at its stream position -- the position of digit K - 2 depends on
    every rejection before it -- and the noise recovered from the same limbs; src0: limb 0 of the key's source polynomial (NTT form)"""
    N, K, P = S.N, S.K, S.primes
    a, e, _ = M.kswitch_key(*S.seed, stream_id, N, P)
    for j in (0, K - 2):
        for l in (0, K - 1):
            c0 = buf.to_numpy(N, offset=((j * 2 + 0) * K + l) * N)
            c1 = buf.to_numpy(N, offset=((j * 2 + 1) * K + l) * N)
            assert np.array_equal(c1, a[j, l]), (what, j, l)
            assert np.array_equal(noise_at(S, c0, c1, l, src0 if l == j else None), e[j]), (what, j, l)
    return e


@pytest.mark.parametrize("name", sorted(BENCH))
def test_relin_and_galois_keys_match_model(name, gpu_api):
    """troyhip_create_relin_key, and the default Galois set in one call: its first, a middle and its last key"""
    S = G.Setup.from_cfg(BENCH[name])
    N, P = S.N, S.primes
    s = M.keygen(*S.seed, N, P)[0]
    assert np.array_equal(S.sk, M.lifted_ntt(s, N, P))
    out = gpu_api.DeviceBuffer(S.ksk_words())
    rc = S.lib.troyhip_create_relin_key(S.ctx.h, C.c_uint64(S.seed[0]), C.c_uint64(S.seed[1]), C.c_void_p(S.dsk.ptr), C.c_void_p(out.ptr), None)
    assert rc == 0, S.lib.troyhip_last_error().decode()
    check_key_digits(S, out, M.RELIN, M.mulmod(S.sk[0], S.sk[0], P[0]), "relin")
    elts = S.kg.galoisEltsAll()
    keys = S.device_galois(elts)
    for i in (0, len(elts) // 2, len(elts) - 1):
        src0 = M.ntt(N, P[0], M.lift(M.galois_coeffs(s, elts[i]), P[0]))
        check_key_digits(S, keys[i], M.galois_stream(elts[i]), src0, "galois %d" % elts[i])


@pytest.mark.parametrize("name", sorted(BENCH))
def test_kswitch_two_new_keys(name, gpu_api):
    """KeyGenerator.createKeySwitchingKeys(device=True) twice with two new_keys: no shared c1, and each is the host form of the same call number"""
    api = gpu_api
    S = G.Setup.from_cfg(BENCH[name])
    twin = api.KeyGenerator(S.ctx, seed=S.seed)
    k1, k2 = api.KeyGenerator(S.ctx, seed=(3, 4)).secretKey(), api.KeyGenerator(S.ctx, seed=(4, 3)).secretKey()
    dev = [S.kg.createKeySwitchingKeys(k, device=True).keys[0].to_numpy().reshape(S.ksk_shape()) for k in (k1, k2)]
    for j in range(S.K - 1):
        for l in range(S.K):
            assert not np.array_equal(dev[0][j, 1, l], dev[1][j, 1, l]), (j, l)
    for d, k in zip(dev, (k1, k2)):
        assert np.array_equal(d, twin.createKeySwitchingKeys(k))


def test_cbd_chisquare_of_a_device_relin_key(gpu_api):
    """The noise of the 14 digits of a device-drawn relin key at bfv_n32768_l14 (14 x 32768 coefficients), recovered in the limb of the special prime
    (no source term there), is the model's, and Binomial(42, 1/2) - 21 at a one-sided p >= 1e-6.  The model alone, seed (0x5EED, 7): p = 0.214 over 27 cells, variance 10.485"""
    from math import comb
    from scipy import stats
    S = G.Setup.from_cfg(BENCH["bfv_n32768_l14"])
    N, K, P = S.N, S.K, S.primes
    rc, key = S.device_relin_rc()
    assert rc == 0, key
    e = np.stack([noise_at(S, key[j, 0, K - 1], key[j, 1, K - 1], K - 1) for j in range(K - 1)])
    assert e.size == 14 * 32768 and np.abs(e).max() <= 21

    def pvalue(v):
        obs = np.array([(v == k).sum() for k in range(-21, 22)], dtype=float)
        exp = np.array([comb(42, k + 21) for k in range(-21, 22)], dtype=float) / 2.0**42 * v.size
        lo = 0
        while exp[:lo + 1].sum() < 5:  # pool the tails until every expected count is at least 5 (the pmf is symmetric)
            lo += 1
        hi = 42 - lo
        o = np.concatenate([[obs[:lo + 1].sum()], obs[lo + 1:hi], [obs[hi:].sum()]])
        x = np.concatenate([[exp[:lo + 1].sum()], exp[lo + 1:hi], [exp[hi:].sum()]])
        return len(o), stats.chisquare(o, x).pvalue

    model = M.kswitch_key(*S.seed, M.RELIN, N, P)[1]
    print("CBD chi-square, device: %d cells, p = %.4f; model: %d cells, p = %.4f; device variance %.4f" % (*pvalue(e), *pvalue(model), e.astype(float).var()))
    assert np.array_equal(e, model)
    assert pvalue(e)[1] >= 1e-6
