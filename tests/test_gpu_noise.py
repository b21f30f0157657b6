"""invariantNoiseBudget on the MI355X: the device form against the reference's recorded budgets (ciphertexts made on the device), the crafted
boundary cases, item for item against the host form (the small parameter sets in full, B = 128 at the larger shapes on items 0, 63, 127), the
refusals, and an all-device pipeline in which a positive budget and a correct decryption go together."""
import numpy as np
import pytest

import cases
import noise_cases as NC
from troy_amd import capi

pytestmark = pytest.mark.gpu


NARROW = ["nar_bgv_n8192_k4", "nar_bfv_n4096_k3"]  # narrow data primes under 60-bit ends, and an all-narrow set (primes of 22 .. 32 bits)


@pytest.fixture(scope="module")
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


_setups = {}


def setup_of(name):
    if name not in _setups:
        _setups[name] = NC.Setup(NC.CONFIGS[name] if name in NC.CONFIGS else cases.CONFIGS[name], relin=name not in NC.BENCH)
    return _setups[name]


@pytest.mark.parametrize("name", sorted(NC.CONFIGS))
def test_golden_device(name, gpu_api):
    """the recipes of tests/golden/noise_budget.json with the ciphertexts encrypted and evaluated on the device: the reference's budgets"""
    S = setup_of(name)
    records = NC.records_of(name)
    assert len(records) == len(NC.SEQUENCES)
    for r in records:
        ct = S.run_sequence_device(r["sequence"])
        assert (ct.size(), ct.limbs) == (r["size"], r["limbs"])
        got = gpu_api.Evaluator(S.ctx).invariantNoiseBudget(ct, S.dsk)
        print(name, r["sequence"], "device", int(got[0]), "recorded", r["budget"])
        assert int(got[0]) == r["budget"], (name, r["sequence"])


@pytest.mark.parametrize("name", NC.SMALL)
def test_boundaries_small(name, gpu_api):
    S = setup_of(name)
    for limbs in (S.ctx.first_limbs, S.ctx.last_limbs):
        NC.check_boundaries_device(S, limbs)


@pytest.mark.parametrize("name", sorted(NC.BENCH))
def test_boundaries_bench_shapes(name, gpu_api):
    """every boundary target at the first and the last level, the coefficient at N - 1, index 0 and an interior position by turns; ONE batch per level"""
    S = setup_of(name)
    for limbs in (S.ctx.first_limbs, S.ctx.last_limbs):
        q = S.q(limbs)
        T = NC.boundary_targets(q)[::29 if limbs > 2 else 3]
        pos = [(0, S.N - 1, S.N // 3)[i % 3] for i in range(len(T))]
        cts = np.stack([NC.crafted(S, limbs, t, p) for t, p in zip(T, pos)])
        rc, got = S.device(cts)
        assert rc == capi.OK, got
        assert list(zip(*got)) == [NC.expected_of(q, t) for t in T]
        for i in (0, len(T) // 2, len(T) - 1):
            assert S.host(cts[i])[1] == NC.expected_of(q, T[i])


@pytest.mark.parametrize("name", NC.SMALL + ["cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_device_matches_host(name, gpu_api):
    S = setup_of(name)
    ref = NC.make_ref(S)
    small = S.N <= 128
    for limbs in S.levels():
        for size in (2, 3):
            for batch, pad in (((1, 0), (3, 5), (17, 0)) if small else ((3, 5),)):
                NC.check_device_matches_host(S, batch, size, limbs, pad, ref=ref)


@pytest.mark.parametrize("name", NARROW)
def test_narrow_primes_device_matches_host(name, gpu_api):
    """primes of 22 .. 32 bits: the Garner digits and the base-2^64 composition of the noise norm over narrow moduli -- budgets and norms of real
    ciphertexts of size 2 and 3 at every level equal the host form's, and every boundary target at the first and the last level"""
    S = setup_of(name)
    ref = NC.make_ref(S)
    for limbs in S.levels():
        for size in (2, 3):
            NC.check_device_matches_host(S, 3, size, limbs, 5, ref=ref)
    for limbs in (S.ctx.first_limbs, S.ctx.last_limbs):
        NC.check_boundaries_device(S, limbs)


@pytest.mark.parametrize("name", ["cfgB_bfv_n8192_k5"] + sorted(NC.BENCH))
def test_b128_matches_host(name, gpu_api):
    """B = 128 fresh ciphertexts made on the device; items 0, 63 and 127 against the host form and the model, item 0 against the reference live"""
    S = setup_of(name)
    enc = S.encryptor((9, 9))
    rng = np.random.default_rng(128)
    cts = enc.encryptBatch(rng.integers(0, S.t, (128, S.N), dtype=np.uint64))
    ev = gpu_api.Evaluator(S.ctx)
    budgets, norms = ev.invariantNoiseBudget(cts, S.dsk, with_norm=True)
    assert budgets.shape == (128,) and (budgets > 0).all()
    host = cts.cpu()
    for b in (0, 63, 127):
        rc, h = S.host(host[b])
        assert rc == capi.OK and (int(budgets[b]), NC.words_to_int(norms[b])) == h, (name, b)
        assert h == S.model(host[b])
    ref = NC.make_ref(S)
    if ref is not None:
        from oracle import ref as R
        assert ref.decrypt(R.Ct(host[0]))[1] == int(budgets[0])
    # the last level too: switched down on the device
    while cts.limbs > S.ctx.last_limbs:
        cts = ev.modSwitchToNext(cts)
    budgets, norms = ev.invariantNoiseBudget(cts, S.dsk, with_norm=True)
    host = cts.cpu()
    for b in (0, 63, 127):
        assert (int(budgets[b]), NC.words_to_int(norms[b])) == S.host(host[b])[1] == S.model(host[b]), (name, b)


def test_refusals(gpu_api):
    K = NC.Setup(cases.CONFIGS["ckks_n128_k6"])
    for name in ("bfv_n64_k3", "bgv_n128_k4"):
        NC.check_refusals(setup_of(name), K)


@pytest.mark.parametrize("name", ["bfv_n128_k4", "bgv_n128_k4"])
def test_python_layer(name, gpu_api):
    NC.check_python_layer(setup_of(name))


def test_budget_and_decryption_go_together(gpu_api):
    """encodeBatch -> encryptBatch -> multiply -> relinearize -> budget over B = 128 at bfv_n32768_l14: every budget is positive and every item
    decrypts and decodes to the slot products"""
    api = gpu_api
    S = setup_of("bfv_n32768_l14")
    ctx, B, N, t = S.ctx, 128, S.N, S.t
    rk = S.kg.createRelinKeys(device=True)
    ev = api.Evaluator(ctx)
    encr = S.encryptor((3, 4))
    enc = api.BatchEncoder(ctx)
    rng = np.random.default_rng(11)
    x = rng.integers(0, t, (B, N), dtype=np.uint64)
    y = rng.integers(0, t, (B, N), dtype=np.uint64)
    cx, cy = encr.encryptBatch(enc.encodeBatch(x, device=True)), encr.encryptSymmetricBatch(enc.encodeBatch(y, device=True))
    fresh = ev.invariantNoiseBudget(cx, S.dsk)
    prod = ev.multiply(cx, cy)
    ev.relinearizeInplace(prod, rk)
    budgets = ev.invariantNoiseBudget(prod, S.dsk)
    print("fresh", fresh.min(), fresh.max(), "after multiply + relinearize", budgets.min(), budgets.max())
    assert budgets.shape == (B,) and (budgets > 0).all() and (budgets < fresh).all()
    got = enc.decodeBatch(ev.decrypt(prod, S.dsk))
    assert np.array_equal(got, (x.astype(object) * y.astype(object) % t).astype(np.uint64))
