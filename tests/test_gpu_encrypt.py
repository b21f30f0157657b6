"""Device encryption on the MI355X: item i of a batch is byte-identical to the host form with item i's seed (small shapes, every form and level;
the bench shapes on a few items), and a headline batch encrypted on the device multiplies, relinearizes and decrypts to the slot products."""
import numpy as np
import pytest

import cases
import enc_cases as E
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
    S = E.Setup.from_cfg(cases.CONFIGS[name])
    for form in E.FORMS:
        levels = S.data_levels() if (S.scheme == CKKS or form.endswith("0")) else [S.ctx.first_limbs]
        for limbs in levels:
            for batch in (1, 3, 17):
                E.check_form(S, form, limbs, batch)
            E.check_form(S, form, limbs, 3, per_item=False, pad=S.N)


def test_rejecting_primes_match_host(gpu_api):
    S = E.Setup(CKKS, 4096, E.rejecting_primes(4096, 4), 0)
    for form in ("sk", "sks0", "pk"):
        E.check_form(S, form, S.ctx.first_limbs, 33, items=[0, 13, 32])


def test_bfv_bench_shape(gpu_api):
    S = E.Setup.from_cfg(BENCH["bfv_n32768_l14"])
    for form in ("pk", "sks"):
        E.check_form(S, form, S.ctx.first_limbs, 4, items=[0, 3])


def test_ckks_bench_shape_every_level(gpu_api):
    S = E.Setup.from_cfg(BENCH["ckks_n32768_chain"])
    for limbs in S.data_levels():
        E.check_form(S, "pk0", limbs, 2, items=[1])
    E.check_form(S, "sk0", S.ctx.first_limbs, 2, items=[1])
    E.check_form(S, "sk0", S.ctx.last_limbs, 2, items=[0])


def test_bgv_bench_shape(gpu_api):
    S = E.Setup.from_cfg(BENCH["bgv_n65536_relin_rot"])
    E.check_form(S, "pk", S.ctx.first_limbs, 3, items=[2])
    E.check_form(S, "sks", S.ctx.first_limbs, 2, items=[0])


def test_headline_batch_multiply_relin_decrypt(gpu_api):
    """B = 128 ciphertexts of the headline shape encrypted on the device, squared, relinearized and decrypted on the device: the slot products"""
    api = gpu_api
    cfg = BENCH["bfv_n32768_l14"]
    S = E.Setup.from_cfg(cfg)
    N, t, B = S.N, S.t, 128
    rng = np.random.default_rng(2024)
    enc = api.BatchEncoder(S.ctx)
    x = rng.integers(0, t, (B, N), dtype=np.uint64)
    y = rng.integers(0, t, (B, N), dtype=np.uint64)
    px = np.stack([enc.encode(v) for v in x])
    py = np.stack([enc.encode(v) for v in y])
    dev = api.Encryptor(S.ctx, S.pk, seed=(9, 9))
    dev.setSecretKey(S.sk)
    cx = dev.encryptBatch(px)
    cy = dev.encryptSymmetricBatch(py)
    for i in (0, 41, 90, 127):  # sample items against the host path
        got = cx.buf.to_numpy(2 * cx.limbs * N, offset=i * cx.bstride).reshape(2, cx.limbs, N)
        exp = S.host("pk", [(9 + 1 + i) & E.MASK, 9], S.ctx.first_limbs, px[i])
        assert np.array_equal(got, exp), i
    kg = api.KeyGenerator(S.ctx, seed=(0x5EED, 7))
    rk = api.RelinKeys(S.ctx)
    rk.set(0, kg.createRelinKeys())
    ev = api.Evaluator(S.ctx)
    prod = ev.multiply(cx, cy)
    ev.relinearizeInplace(prod, rk)
    dsk = api.DeviceBuffer.from_numpy(S.sk)
    plain = ev.decrypt(prod, dsk)
    for b in range(B):
        got = enc.decode(plain[b])
        assert np.array_equal(np.asarray(got, dtype=np.uint64), (x[b].astype(object) * y[b].astype(object) % t).astype(np.uint64)), b
