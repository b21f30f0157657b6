"""Shared checks of the device encoders (troyhip_batch_encode / _decode, troyhip_ckks_encode / _decode): item i of a device call must be
byte-identical to the host form called with item i (troyhip_host_batch_* / troyhip_host_ckks_*), doubles compared as their bit patterns.
Used by tests/test_device_encode.py (emulator build) and tests/test_gpu_encode.py (MI355X)."""
import ctypes as C

import numpy as np

from troy_amd import api, capi
from troy_amd.capi import CKKS


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def context(cfg):
    N = cfg["N"]
    t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
    return api.SEALContext(cfg["scheme"], N, api.CoeffModulus.Create(N, cfg["bits"]), t)


def levels(ctx):
    return list(range(ctx.key_limbs, ctx.last_limbs - 1, -1))


# ---------------------------------------------------------------- BFV / BGV
def bfv_host_encode(ctx, v):
    out = np.zeros(ctx.N, dtype=np.uint64)
    v = np.ascontiguousarray(v, dtype=np.uint64)
    capi.check(ctx.lib, ctx.lib.troyhip_host_batch_encode(ctx.h, _p(v), C.c_uint64(v.size), _p(out)))
    return out


def bfv_host_decode(ctx, p):
    out = np.zeros(ctx.N, dtype=np.uint64)
    p = np.ascontiguousarray(p, dtype=np.uint64)
    capi.check(ctx.lib, ctx.lib.troyhip_host_batch_decode(ctx.h, _p(p), C.c_uint64(p.size), _p(out)))
    return out


def bfv_device(ctx, fn, X, n, out_words, pad=0, batch=None):
    """one troyhip_batch_encode (fn 'enc') / _decode ('dec') call over the rows of X (n words used per row, rows X.shape[1] + 3 words apart);
    output rows out_words + pad apart.  Returns (status, [B][out_words] or the message)"""
    B = X.shape[0] if batch is None else batch
    istride = X.shape[1] + 3
    src = np.zeros((max(1, X.shape[0]), istride), dtype=np.uint64)
    src[:X.shape[0], :X.shape[1]] = X
    dsrc = api.DeviceBuffer.from_numpy(src)
    ostride = out_words + pad
    out = api.DeviceBuffer(max(1, B) * ostride)
    f = ctx.lib.troyhip_batch_encode if fn == "enc" else ctx.lib.troyhip_batch_decode
    rc = f(ctx.h, C.c_void_p(dsrc.ptr), C.c_uint64(n), C.c_uint64(istride), C.c_void_p(out.ptr), C.c_uint64(ostride), C.c_uint64(B), None)
    if rc != capi.OK:
        return rc, ctx.lib.troyhip_last_error().decode()
    return rc, out.to_numpy().reshape(B, ostride)[:, :out_words]


def check_bfv(ctx, batch, count, rng, pad=0, items=None):
    N, t = ctx.N, ctx.plain_modulus
    V = rng.integers(0, 2**64, (batch, count), dtype=np.uint64, endpoint=False)
    V[:, ::2] %= np.uint64(t)  # half of the values below t, half anywhere (>= t)
    rc, enc = bfv_device(ctx, "enc", V, count, N, pad)
    assert rc == capi.OK, enc
    for b in (range(batch) if items is None else items):
        assert np.array_equal(enc[b], bfv_host_encode(ctx, V[b])), ("encode", batch, count, b)
    for n in (N, N - 5, 1):
        rc, dec = bfv_device(ctx, "dec", enc[:, :n], n, N, pad)
        assert rc == capi.OK, dec
        for b in (range(batch) if items is None else items):
            assert np.array_equal(dec[b], bfv_host_decode(ctx, enc[b, :n])), ("decode", batch, n, b)
    rc, dec = bfv_device(ctx, "dec", enc, N, N)
    assert np.array_equal(dec[:, :count], V % np.uint64(t))
    return enc


# ---------------------------------------------------------------- CKKS
def ckks_host_encode(ctx, vals, limbs, scale):
    """vals [count][2] doubles -> (status, [limbs][N] or message)"""
    vals = np.ascontiguousarray(vals, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((max(limbs, 1), ctx.N), dtype=np.uint64)
    rc = ctx.lib.troyhip_host_ckks_encode(ctx.h, _p(vals), C.c_uint64(vals.shape[0]), limbs, C.c_double(scale), _p(out))
    return (rc, out) if rc == capi.OK else (rc, ctx.lib.troyhip_last_error().decode())


def ckks_host_decode(ctx, plain, limbs, scale):
    out = np.zeros((ctx.N // 2, 2), dtype=np.float64)
    rc = ctx.lib.troyhip_host_ckks_decode(ctx.h, _p(np.ascontiguousarray(plain, dtype=np.uint64)), limbs, C.c_double(scale), _p(out))
    return (rc, out) if rc == capi.OK else (rc, ctx.lib.troyhip_last_error().decode())


def ckks_device_encode(ctx, V, limbs, scale, pad=0, batch=None):
    """V [B][count][2] doubles; values rows 2 count + 4 doubles apart, plaintexts limbs N + pad words apart"""
    B = V.shape[0] if batch is None else batch
    count = V.shape[1]
    vstride = 2 * count + 4
    src = np.zeros((max(1, V.shape[0]), vstride), dtype=np.float64)
    src[:V.shape[0], :2 * count] = V.reshape(V.shape[0], -1)
    dsrc = api.DeviceBuffer.from_numpy(src.view(np.uint64))
    item = max(limbs, 0) * ctx.N
    out = api.DeviceBuffer(max(1, B) * max(1, item + pad))
    rc = ctx.lib.troyhip_ckks_encode(ctx.h, C.c_void_p(dsrc.ptr), C.c_uint64(count), C.c_uint64(vstride), limbs, C.c_double(scale), C.c_void_p(out.ptr),
                                     C.c_uint64(item + pad), C.c_uint64(B), None)
    if rc != capi.OK:
        return rc, ctx.lib.troyhip_last_error().decode()
    return rc, out.to_numpy().reshape(B, item + pad)[:, :item].reshape(B, limbs, ctx.N)


def ckks_device_decode(ctx, P, limbs, scale, pad=0, batch=None):
    B = P.shape[0] if batch is None else batch
    item = P.shape[1] * ctx.N
    src = np.zeros((max(1, P.shape[0]), item + pad), dtype=np.uint64)
    src[:P.shape[0], :item] = P.reshape(P.shape[0], -1)
    dsrc = api.DeviceBuffer.from_numpy(src)
    vstride = ctx.N + 2
    out = api.DeviceBuffer(max(1, B) * vstride)
    rc = ctx.lib.troyhip_ckks_decode(ctx.h, C.c_void_p(dsrc.ptr), limbs, C.c_double(scale), C.c_uint64(item + pad), C.c_void_p(out.ptr), C.c_uint64(vstride),
                                     C.c_uint64(B), None)
    if rc != capi.OK:
        return rc, ctx.lib.troyhip_last_error().decode()
    return rc, out.to_numpy().view(np.float64).reshape(B, vstride)[:, :ctx.N].reshape(B, ctx.N // 2, 2)


def ckks_values(rng, batch, count, magnitude=8.0, complex_=True):
    V = rng.uniform(-magnitude, magnitude, (batch, count, 2))
    if not complex_:
        V[..., 1] = 0.0
    return V


def check_ckks(ctx, batch, count, limbs, scale, rng, complex_=True, pad=0, items=None, magnitude=8.0, V=None):
    """device encode == host encode per item (or both refuse with the same message), device decode == host decode; returns the device plaintexts.
    V [batch][count][2]: the values to use instead of random ones"""
    if V is None:
        V = ckks_values(rng, batch, count, magnitude, complex_)
    rc, enc = ckks_device_encode(ctx, V, limbs, scale, pad)
    hosts = [ckks_host_encode(ctx, V[b], limbs, scale) for b in range(batch)]
    bad = [b for b in range(batch) if hosts[b][0] != capi.OK]
    if bad:
        assert rc == hosts[bad[0]][0] and enc == "%s (item %d)" % (hosts[bad[0]][1], bad[0]), (enc, hosts[bad[0]])
        return None
    assert rc == capi.OK, enc
    for b in (range(batch) if items is None else items):
        assert np.array_equal(enc[b], hosts[b][1]), ("encode", batch, count, limbs, scale, b)
    rc, dec = ckks_device_decode(ctx, enc, limbs, scale, pad)
    hrc, hmsg = ckks_host_decode(ctx, enc[0], limbs, scale)
    if hrc != capi.OK:  # a scale the level cannot decode ("scale out of bounds"): refused alike
        assert (rc, dec) == (hrc, hmsg)
        return None
    assert rc == capi.OK, dec
    for b in (range(batch) if items is None else items):
        hrc, exp = ckks_host_decode(ctx, enc[b], limbs, scale)
        assert hrc == capi.OK, exp
        assert np.array_equal(dec[b].view(np.uint64), exp.view(np.uint64)), ("decode", batch, count, limbs, scale, b)
    return V, enc, dec
