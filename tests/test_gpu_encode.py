"""Device encoding on the MI355X: item i of a batch is byte-identical to the host form with item i (the small configs in full, the bench shapes at
B = 128 on sample items), and an all-device pipeline encode -> encrypt -> multiply -> relinearize -> decrypt -> decode gives the slot products."""
import numpy as np
import pytest

import cases
import encode_cases as E
from troy_amd.capi import BGV, CKKS

pytestmark = pytest.mark.gpu

BENCH = {  # bench.py's workload parameters
    "bfv_n32768_l14": dict(scheme=1, N=32768, bits=[60] + [58] * 13 + [60], tbits=20),
    "ckks_n32768_chain": dict(scheme=CKKS, N=32768, bits=[60] + [40] * 13 + [60], tbits=0),
    "bgv_n65536_relin_rot": dict(scheme=BGV, N=65536, bits=[60] + [50] * 13 + [60], tbits=20),
}
SMALL = cases.SMALL + ["cfgA_bfv_n4096_k3", "ckks_n4096_k4", "bgv_n4096_k3"]


NARROW = ["nar_bgv_n8192_k4", "nar_bfv_n4096_k3"]  # narrow data primes under 60-bit ends, and an all-narrow set (primes of 22 .. 32 bits)


@pytest.fixture(scope="module")
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


@pytest.mark.parametrize("name", SMALL)
def test_small_configs_match_host(name, gpu_api):
    cfg = cases.CONFIGS[name]
    ctx = E.context(cfg)
    rng = np.random.default_rng(ctx.N)
    if cfg["scheme"] == CKKS:
        slots = ctx.N // 2
        for limbs in E.levels(ctx):
            for scale in (2.0**20, 2.0**40, 2.0**80):
                for batch in (1, 3, 17):
                    E.check_ckks(ctx, batch, slots if batch != 3 else slots // 3, limbs, scale, rng, complex_=batch != 1, pad=7 if batch == 3 else 0)
    else:
        for batch in (1, 3, 17):
            for count in (0, ctx.N // 3, ctx.N):
                E.check_bfv(ctx, batch, count, rng, pad=5 if batch == 3 else 0)


@pytest.mark.parametrize("name", NARROW)
def test_narrow_primes_match_host(name, gpu_api):
    """BFV / BGV batch encoding under primes of 22 .. 32 bits (the plaintext side is t alone; the context tables are the narrow set's)"""
    ctx = E.context(cases.CONFIGS[name])
    rng = np.random.default_rng(ctx.N + 1)
    for batch in (1, 3, 17):
        for count in (0, ctx.N // 3, ctx.N):
            E.check_bfv(ctx, batch, count, rng, pad=5 if batch == 3 else 0)


def test_narrow_ckks_primes_match_host(gpu_api):
    """CKKS encoding into residues of 25 .. 32-bit primes at every level: the Garner digits / base-2^64 composition over narrow moduli"""
    ctx = E.context(cases.CONFIGS["nar_ckks_n16384_k5"])
    rng = np.random.default_rng(ctx.N + 2)
    for limbs in E.levels(ctx):
        for scale in (2.0**20, 2.0**40, 2.0**80):
            E.check_ckks(ctx, 3, ctx.N // 2, limbs, scale, rng, complex_=True, pad=7)


@pytest.mark.parametrize("name", sorted(BENCH))
def test_bench_shapes_b128(name, gpu_api):
    cfg = BENCH[name]
    ctx = E.context(cfg)
    rng = np.random.default_rng(7)
    items = [0, 63, 127]
    if cfg["scheme"] == CKKS:
        for limbs in (ctx.first_limbs, ctx.last_limbs):
            E.check_ckks(ctx, 128, ctx.N // 2, limbs, 2.0**40, rng, items=items)
        E.check_ckks(ctx, 128, ctx.N // 2, ctx.key_limbs, 2.0**80, rng, items=[5])  # 15 limbs at the key level, the shift > 64 path
    else:
        E.check_bfv(ctx, 128, ctx.N, rng, items=items)


@pytest.mark.parametrize("name", ["bfv_n32768_l14", "ckks_n32768_chain"])
def test_all_device_pipeline(name, gpu_api):
    """encodeBatch(device) -> encryptBatch(DeviceBuffer) -> multiply -> relinearize -> decrypt -> decodeBatch over B = 128 items"""
    api = gpu_api
    cfg = BENCH[name]
    ctx = E.context(cfg)
    B, N = 128, ctx.N
    kg = api.KeyGenerator(ctx, seed=(0x5EED, 11))
    sk, pk = kg.secretKey(), kg.createPublicKey()
    rk = api.RelinKeys(ctx)
    rk.set(0, kg.createRelinKeys())
    ev = api.Evaluator(ctx)
    encr = api.Encryptor(ctx, pk, seed=(3, 4))
    encr.setSecretKey(sk)
    rng = np.random.default_rng(11)
    if cfg["scheme"] == CKKS:
        enc = api.CKKSEncoder(ctx)
        scale = 2.0**40
        x = rng.uniform(-2, 2, (B, N // 2)) + 1j * rng.uniform(-2, 2, (B, N // 2))
        y = rng.uniform(-2, 2, (B, N // 2))
        px, py = enc.encodeBatch(x, scale, device=True), enc.encodeBatch(y, scale, device=True)
        cx, cy = encr.encryptBatch(px, scale), encr.encryptSymmetricBatch(py, scale)
        prod = ev.multiply(cx, cy)
        ev.relinearizeInplace(prod, rk)
        plain = ev.decrypt(prod, api.DeviceBuffer.from_numpy(sk))
        got = enc.decodeBatch(plain, prod.scale)
        assert np.abs(got - x * y).max() < 1e-4, np.abs(got - x * y).max()
    else:
        enc = api.BatchEncoder(ctx)
        t = ctx.plain_modulus
        x = rng.integers(0, t, (B, N), dtype=np.uint64)
        y = rng.integers(0, t, (B, N), dtype=np.uint64)
        px, py = enc.encodeBatch(x, device=True), enc.encodeBatch(y, device=True)
        cx, cy = encr.encryptBatch(px), encr.encryptSymmetricBatch(py)
        prod = ev.multiply(cx, cy)
        ev.relinearizeInplace(prod, rk)
        plain = ev.decrypt(prod, api.DeviceBuffer.from_numpy(sk))
        got = enc.decodeBatch(plain)
        assert np.array_equal(got, (x.astype(object) * y.astype(object) % t).astype(np.uint64))
