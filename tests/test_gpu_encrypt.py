"""Device encryption on the MI355X: item i of a batch is byte-identical to the host form with item i's seed (small shapes, every form and level;
the bench shapes on a few items), and a headline batch encrypted on the device multiplies, relinearizes and decrypts to the slot products.  At the bench shapes the symmetric forms are also compared with the independent model of the
streams (tests/sampler_model.py)."""
import numpy as np
import pytest

import cases
import enc_cases as E
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
    S = E.Setup.from_cfg(cases.CONFIGS[name])
    for form in E.FORMS:
        levels = S.data_levels() if (S.scheme == CKKS or form.endswith("0")) else [S.ctx.first_limbs]
        for limbs in levels:
            for batch in (1, 3, 17):
                E.check_form(S, form, limbs, batch)
            E.check_form(S, form, limbs, 3, per_item=False, pad=S.N)


@pytest.mark.parametrize("name", NARROW)
def test_narrow_primes_match_host(name, gpu_api):
    """primes of 22 .. 32 bits: the uniform sampler rejects against tiny moduli; every form at the first level, encryptions of zero at every level"""
    S = E.Setup.from_cfg(cases.CONFIGS[name])
    for form in E.FORMS:
        for limbs in (S.data_levels() if form.endswith("0") else [S.ctx.first_limbs]):
            E.check_form(S, form, limbs, 5)
        E.check_form(S, form, S.ctx.first_limbs, 3, per_item=False, pad=S.N)


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


# ---- the device against the independent model of the streams (tests/sampler_model.py) at the bench shapes: c1 and the recovered noise, with
# Python integers and the oracle's NTT; nothing here goes through the host forms.
EDGE_SEEDS = {0: (0x5EED, 7), 63: (0x8000000000000123, 0), 127: (0xFFFFFFFFFFFFFFF0, 0x9000000000000001)}


def symmetric_b128(S, limbs, seeded, rng):
    """troyhip_encrypt_symmetric at B = 128, one plaintext for every item: items 0, 63 and 127 against the model, in the first and the last limb"""
    import ctypes as C
    from troy_amd import api, capi
    N, P, B = S.N, S.primes, 128
    seeds = E.seeds_for(B, base=limbs)
    for i, seed in EDGE_SEEDS.items():
        seeds[i] = seed
    a_seeds = E.a_seeds_for(B, base=limbs) if seeded else None
    plain = S.plains(1, limbs, rng)
    dplain = api.DeviceBuffer.from_numpy(np.ascontiguousarray(plain, dtype=np.uint64))
    stride = 2 * limbs * N
    out = api.DeviceBuffer(B * stride)
    st = capi.CtStruct(out.ptr, stride, 0, limbs, 0, 0.0, 0)
    rc = S.lib.troyhip_encrypt_symmetric(S.ctx.h, C.c_void_p(S.dsk.ptr), E._p(seeds), None if a_seeds is None else E._p(a_seeds), C.c_void_p(dplain.ptr),
                                         C.c_uint64(N if S.scheme == CKKS else plain.shape[1]), C.c_uint64(0), C.c_double(2.0**20 if S.scheme == CKKS else 1.0),
                                         C.byref(st), C.c_uint64(B), None)
    assert rc == capi.OK, S.lib.troyhip_last_error().decode()
    for i, seed in EDGE_SEEDS.items():
        ct = out.to_numpy(stride, offset=i * stride).reshape(2, limbs, N)
        if seeded:
            a, e = M.symmetric_seeded(*seed, int(a_seeds[i]), N, P[:limbs])
        else:
            a, e, _ = M.symmetric(*seed, N, P[:limbs])
        for l in (0, limbs - 1):
            c1 = ct[1, l] if S.scheme == CKKS else M.ntt(N, P[l], ct[1, l])
            assert np.array_equal(c1, a[l]), (seeded, limbs, i, l)
            assert np.array_equal(M.symmetric_noise(S.scheme, ct, S.sk, l, limbs, P, S.t, N, plain[0]), e), (seeded, limbs, i, l)


@pytest.mark.parametrize("name", sorted(BENCH))
def test_symmetric_b128_matches_model(name, gpu_api):
    """seeded and unseeded, at the first level, and for CKKS also at the last"""
    S = E.Setup.from_cfg(BENCH[name])
    rng = np.random.default_rng(12)
    for limbs in ([S.ctx.first_limbs, S.ctx.last_limbs] if S.scheme == CKKS else [S.ctx.first_limbs]):
        for seeded in (False, True):
            symmetric_b128(S, limbs, seeded, rng)
