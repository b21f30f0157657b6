"""Device key generation on the MI355X: every key of a call is byte-identical to the host form with the same seed, secret key and element (the
small shapes in full, rejecting 60-bit primes at N = 4096, and bench.py's three workload shapes on sampled keys of the whole default Galois set),
and a BGV N = 2^16 rotate chain under device-generated keys decrypts to the rotated slots."""
import numpy as np
import pytest

import cases
import enc_cases as E
import keygen_cases as G
from troy_amd.capi import BFV, BGV, CKKS

pytestmark = pytest.mark.gpu

BENCH = {  # bench.py's workload parameters
    "bfv_n32768_l14": dict(scheme=BFV, N=32768, bits=[60] + [58] * 13 + [60], tbits=20),
    "ckks_n32768_chain": dict(scheme=CKKS, N=32768, bits=[60] + [40] * 13 + [60], tbits=0),
    "bgv_n65536_relin_rot": dict(scheme=BGV, N=65536, bits=[60] + [50] * 13 + [60], tbits=20),
}


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
