"""Device encoding (troyhip_batch_encode / _decode, troyhip_ckks_encode / _decode) on the emulator build of the kernels: item i of a batch is
byte-identical to the host form called with item i.  tests/test_gpu_encode.py runs the same checks on an MI355X."""
import os
import subprocess

import numpy as np
import pytest

import cases
import encode_cases as E
from conftest import ROOT
from troy_amd.capi import BFV, CKKS

EMUL = os.path.join(ROOT, "tests", "emul", "libtroyhip_emul.so")

N4096 = {"bfv_n4096": cases.CONFIGS["cfgA_bfv_n4096_k3"], "bgv_n4096": cases.CONFIGS["bgv_n4096_k3"], "ckks_n4096": cases.CONFIGS["ckks_n4096_k4"]}
ALL = {**{n: cases.CONFIGS[n] for n in cases.SMALL}, **N4096}
PLAIN = [n for n in ALL if ALL[n]["scheme"] != CKKS]
CKKS_CFGS = [n for n in ALL if ALL[n]["scheme"] == CKKS]


@pytest.fixture(scope="module")
def emul_api():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    from troy_amd import api, capi
    lib = capi.load(EMUL)
    old = api.KernelProvider._lib
    api.KernelProvider.initialize(0, _lib=lib)
    yield api
    api.KernelProvider._lib = old


@pytest.mark.parametrize("name", PLAIN)
def test_batch_encoder_matches_host(name, emul_api):
    ctx = E.context(ALL[name])
    N = ctx.N
    rng = np.random.default_rng(N + ALL[name]["scheme"])
    small = N <= 128
    for batch in ((1, 3, 17) if small else (1, 3)):
        for count in (0, N // 3, N):
            E.check_bfv(ctx, batch, count, rng, pad=5 if batch == 3 else 0)


@pytest.mark.parametrize("name", CKKS_CFGS)
def test_ckks_encoder_matches_host(name, emul_api):
    ctx = E.context(ALL[name])
    N, slots = ctx.N, ctx.N // 2
    rng = np.random.default_rng(N)
    small = N <= 128
    for limbs in E.levels(ctx):
        for scale in (2.0**20, 2.0**40, 2.0**80):  # 2^80: the shift > 64 path (or "too large" where the level is narrower)
            for batch in ((1, 3, 17) if small else (1, 3)):
                for count in (0, slots // 3, slots):
                    E.check_ckks(ctx, batch, count, limbs, scale, rng, complex_=bool(count % 2 == 0), pad=7 if batch == 3 else 0)


@pytest.mark.parametrize("name", CKKS_CFGS)
def test_ckks_roundtrip(name, emul_api):
    """decode(encode(x)) == x within 2^-(log2 scale) * N: the rounding to integers, scaled back, through a transform of norm <= N / 2 per slot"""
    ctx = E.context(ALL[name])
    rng = np.random.default_rng(3)
    scale = 2.0**40
    for limbs in E.levels(ctx):
        if limbs * 30 < 60:
            continue
        r = E.check_ckks(ctx, 3, ctx.N // 2, limbs, scale, rng, magnitude=100.0)
        V, _, dec = r
        assert np.abs(dec - V).max() < ctx.N / scale, np.abs(dec - V).max()


def test_ckks_negative_and_real_values(emul_api):
    ctx = E.context(ALL["ckks_n128_k6"])
    slots, limbs = ctx.N // 2, ctx.first_limbs
    V = np.zeros((2, slots, 2))
    V[0, :, 0] = -np.arange(1, slots + 1) * 1.5  # every value negative, real
    V[1, :, 0], V[1, :, 1] = -0.0, -2.25         # negative zeros and a negative imaginary part
    rc, enc = E.ckks_device_encode(ctx, V, limbs, 2.0**30)
    assert rc == 0, enc
    for b in range(2):
        assert np.array_equal(enc[b], E.ckks_host_encode(ctx, V[b], limbs, 2.0**30)[1])


def test_errors_match_host(emul_api):
    from troy_amd import api, capi
    ckks = E.context(ALL["ckks_n128_k6"])
    slots, first = ckks.N // 2, ckks.first_limbs
    V = E.ckks_values(np.random.default_rng(1), 4, slots)
    # too large: item 2 only; the message names it
    big = V.copy()
    big[2, 5, 0] = 2.0**200
    rc, msg = E.ckks_device_encode(ckks, big, first, 2.0**20)
    hrc, hmsg = E.ckks_host_encode(ckks, big[2], first, 2.0**20)
    assert rc == hrc == capi.INVALID_ARGUMENT and hmsg == "encoded values are too large" and msg == hmsg + " (item 2)"
    # non-finite, in either part
    for bad in (np.inf, -np.inf, np.nan):
        nf = V.copy()
        nf[1, 3, 1] = bad
        rc, msg = E.ckks_device_encode(ckks, nf, first, 2.0**20)
        hrc, hmsg = E.ckks_host_encode(ckks, nf[1], first, 2.0**20)
        assert rc == hrc == capi.INVALID_ARGUMENT and hmsg == "encoded values are not finite" and msg == hmsg + " (item 1)"
    # bad limbs, too many values, bad scale on decode
    for limbs in (0, ckks.key_limbs + 1, -1):
        rc, msg = E.ckks_device_encode(ckks, V, limbs, 2.0**20)
        assert (rc, msg) == E.ckks_host_encode(ckks, V[0], limbs, 2.0**20) == (capi.INVALID_ARGUMENT, "parms_id is not valid for encryption parameters")
        Z = np.zeros((1, max(limbs, 1), ckks.N), dtype=np.uint64)
        assert E.ckks_device_decode(ckks, Z, limbs, 2.0**20) == E.ckks_host_decode(ckks, Z[0], limbs, 2.0**20) == \
            (capi.INVALID_ARGUMENT, "plain is not valid for encryption parameters")
    rc, msg = E.ckks_device_encode(ckks, np.zeros((1, slots + 1, 2)), first, 2.0**20)
    assert (rc, msg) == E.ckks_host_encode(ckks, np.zeros((slots + 1, 2)), first, 2.0**20) == (capi.INVALID_ARGUMENT, "values_size is too large")
    P = np.zeros((1, first, ckks.N), dtype=np.uint64)
    for scale in (0.0, -1.0, 2.0**400):
        rc, msg = E.ckks_device_decode(ckks, P, first, scale)
        assert (rc, msg) == E.ckks_host_decode(ckks, P[0], first, scale) == (capi.INVALID_ARGUMENT, "scale out of bounds")
    # batch 0 and 65536
    for batch in (0, 65536):
        assert E.ckks_device_encode(ckks, V, first, 2.0**20, batch=batch) == (capi.INVALID_ARGUMENT, "batch must lie in 1 .. 65535")
        assert E.ckks_device_decode(ckks, P, first, 2.0**20, batch=batch) == (capi.INVALID_ARGUMENT, "batch must lie in 1 .. 65535")
    # wrong scheme both ways
    bfv = E.context(ALL["bfv_n64_k3"])
    X = np.zeros((1, 4), dtype=np.uint64)
    assert E.bfv_device(ckks, "enc", X, 4, ckks.N)[0] == capi.INVALID_ARGUMENT
    assert E.bfv_device(ckks, "enc", X, 4, ckks.N)[1] == "unsupported scheme"
    assert E.ckks_device_encode(bfv, V[:1], bfv.first_limbs, 2.0**20) == (capi.INVALID_ARGUMENT, "unsupported scheme")
    with pytest.raises(capi.InvalidArgument, match="unsupported scheme"):
        E.bfv_host_encode(ckks, X[0])
    # batching not enabled: the context is created, the encoders refuse it with the host's status and message
    nb = api.SEALContext(BFV, 64, api.CoeffModulus.Create(64, [40, 40, 40]), 65537 + 2)  # 65539 is prime but not 1 mod 128
    rc, msg = E.bfv_device(nb, "enc", X, 4, 64)
    assert rc == capi.LOGIC_ERROR and msg == "batching is not enabled for the encryption parameters"
    assert E.bfv_device(nb, "dec", X, 4, 64) == (rc, msg)
    with pytest.raises(capi.LogicError) as ei:
        E.bfv_host_encode(nb, X[0])
    assert str(ei.value) == msg
    # BFV: too many values, batch bounds
    rc, msg = E.bfv_device(bfv, "enc", np.zeros((1, 65), dtype=np.uint64), 65, 64)
    assert (rc, msg) == (capi.INVALID_ARGUMENT, "values_matrix size is too large")
    for batch in (0, 65536):
        assert E.bfv_device(bfv, "enc", X, 4, 64, batch=batch) == (capi.INVALID_ARGUMENT, "batch must lie in 1 .. 65535")


def test_host_ckks_on_host_only_context(emul_api):
    """the host forms need no device tables"""
    from troy_amd import api
    cfg = ALL["ckks_n128_k6"]
    dev = E.context(cfg)
    host = api.SEALContext(CKKS, 128, api.CoeffModulus.Create(128, cfg["bits"]), 0, host_only=True)
    V = E.ckks_values(np.random.default_rng(9), 1, 64)[0]
    a, b = E.ckks_host_encode(host, V, 5, 2.0**30), E.ckks_host_encode(dev, V, 5, 2.0**30)
    assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1])
    assert np.array_equal(E.ckks_host_decode(host, a[1], 5, 2.0**30)[1].view(np.uint64), E.ckks_host_decode(dev, a[1], 5, 2.0**30)[1].view(np.uint64))


@pytest.mark.parametrize("name", ["bfv_n128_k4", "bgv_n128_k4", "ckks_n128_k6"])
def test_python_batch_forms(name, emul_api):
    api = emul_api
    ctx = E.context(ALL[name])
    rng = np.random.default_rng(4)
    if ctx.scheme == CKKS:
        enc = api.CKKSEncoder(ctx)
        assert enc.slotCount() == ctx.N // 2
        vals = rng.uniform(-4, 4, (3, 40)) + 1j * rng.uniform(-4, 4, (3, 40))
        P = enc.encodeBatch(vals, 2.0**30)
        for b in range(3):
            assert np.array_equal(P[b], enc.encode(vals[b], 2.0**30))
        real = enc.encodeBatch(vals.real, 2.0**30, limbs=ctx.first_limbs - 1)
        assert np.array_equal(real[1], enc.encode(vals[1].real, 2.0**30, limbs=ctx.first_limbs - 1))
        D = enc.decodeBatch(P, 2.0**30)
        dbuf = enc.decodeBatch(enc.encodeBatch(vals, 2.0**30, device=True), 2.0**30, device=True)
        assert np.array_equal(dbuf.to_numpy().view(np.float64).reshape(3, -1, 2)[..., 0], D.real)
        for b in range(3):
            assert np.array_equal(D[b].view(np.uint64), enc.decode(P[b], 2.0**30).view(np.uint64))
        assert np.abs(D[:, :40] - vals).max() < 1e-6
    else:
        enc = api.BatchEncoder(ctx)
        t = ctx.plain_modulus
        signed = rng.integers(-(t // 2), t // 2, (3, ctx.N), dtype=np.int64)
        P = enc.encodeBatch(signed)
        for b in range(3):
            assert np.array_equal(P[b], enc.encode(signed[b]))
        assert np.array_equal(enc.decodeBatch(P, signed=True), signed)
        assert np.array_equal(enc.decodeBatch(enc.encodeBatch(signed, device=True)), np.stack([enc.decode(P[b]) for b in range(3)]))
        short = P[:, :ctx.N - 3]
        assert np.array_equal(enc.decodeBatch(short)[2], enc.decode(short[2]))
