"""Shared checks of the device key generation (troyhip_keygen / troyhip_create_relin_key / _galois_keys / _kswitch_key): every key of a device
call must be byte-identical to the host form called with the same seed, secret key and element (troyhip_host_keygen / _relin_key / _galois_key /
_kswitch_key; the tested host path is the oracle).  Used by tests/test_device_keygen.py (emulator build) and tests/test_gpu_keygen.py (MI355X)."""
import ctypes as C

import numpy as np

from troy_amd import api, capi

MASK = 2**64 - 1
SEED = (0x5EED, 7)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Setup:
    def __init__(self, scheme, N, primes, t, seed=SEED):
        self.ctx = api.SEALContext(scheme, N, primes, t)
        self.scheme, self.N, self.t, self.primes = scheme, N, t, list(primes)
        self.K = self.ctx.key_limbs
        self.lib = self.ctx.lib
        self.seed = seed
        self.kg = api.KeyGenerator(self.ctx, seed=seed)
        self.sk = self.kg.secretKey()
        self.dsk = api.DeviceBuffer.from_numpy(self.sk)

    @classmethod
    def from_cfg(cls, cfg, primes=None):
        N = cfg["N"]
        primes = primes or api.CoeffModulus.Create(N, cfg["bits"])
        t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
        return cls(cfg["scheme"], N, primes, t)

    def ksk_words(self):
        return (self.K - 1) * 2 * self.K * self.N

    def ksk_shape(self):
        return (self.K - 1, 2, self.K, self.N)

    # ---- host forms
    def host_keygen(self, seed, with_pk=True):
        sk = np.zeros((self.K, self.N), dtype=np.uint64)
        pk = np.zeros((2, self.K, self.N), dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_keygen(self.ctx.h, C.c_uint64(int(seed[0])), C.c_uint64(int(seed[1])), _p(sk), _p(pk) if with_pk else None))
        return sk, pk

    def host_relin(self):
        out = np.zeros(self.ksk_shape(), dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_relin_key(self.ctx.h, C.c_uint64(self.seed[0]), C.c_uint64(self.seed[1]), _p(self.sk), _p(out)))
        return out

    def host_galois(self, elt):
        out = np.zeros(self.ksk_shape(), dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_galois_key(self.ctx.h, C.c_uint64(self.seed[0]), C.c_uint64(self.seed[1]), _p(self.sk), C.c_uint32(int(elt)),
                                                              _p(out)))
        return out

    def host_kswitch(self, new_key):
        out = np.zeros(self.ksk_shape(), dtype=np.uint64)
        new_key = np.ascontiguousarray(new_key, dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_kswitch_key(self.ctx.h, C.c_uint64(self.seed[0]), C.c_uint64(self.seed[1]), _p(self.sk), _p(new_key), _p(out)))
        return out

    # ---- device forms: (status, message) on failure, else the keys as numpy
    def device_keygen_rc(self, seeds, with_pk=True, pad=0, batch=None):
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        batch = len(seeds) if batch is None else batch
        kw = self.K * self.N
        sks, pks = kw + pad, 2 * kw + pad
        sk = api.DeviceBuffer(max(1, batch) * sks)
        pk = api.DeviceBuffer(max(1, batch) * pks) if with_pk else None
        rc = self.lib.troyhip_keygen(self.ctx.h, _p(seeds), C.c_void_p(sk.ptr), C.c_uint64(sks), None if pk is None else C.c_void_p(pk.ptr), C.c_uint64(pks),
                                     C.c_uint64(batch), None)
        if rc != capi.OK:
            return rc, self.lib.troyhip_last_error().decode()
        s = sk.to_numpy().reshape(batch, sks)[:, :kw].reshape(batch, self.K, self.N)
        p = None if pk is None else pk.to_numpy().reshape(batch, pks)[:, :2 * kw].reshape(batch, 2, self.K, self.N)
        return rc, (s, p)

    def device_keygen(self, seeds, with_pk=True, pad=0):
        rc, out = self.device_keygen_rc(seeds, with_pk, pad)
        assert rc == capi.OK, out
        return out

    def device_galois_rc(self, elts, sk=None):
        elts = np.ascontiguousarray(elts, dtype=np.uint32)
        bufs = [api.DeviceBuffer(max(1, self.ksk_words())) for _ in range(max(1, len(elts)))]
        table = (C.c_void_p * len(bufs))(*[b.ptr for b in bufs])
        dsk = self.dsk if sk is None else sk
        rc = self.lib.troyhip_create_galois_keys(self.ctx.h, C.c_uint64(self.seed[0]), C.c_uint64(self.seed[1]), C.c_void_p(dsk.ptr), _p(elts), table,
                                                 C.c_uint64(len(elts)), None)
        if rc != capi.OK:
            return rc, self.lib.troyhip_last_error().decode()
        return rc, bufs[:len(elts)]

    def device_galois(self, elts):
        rc, out = self.device_galois_rc(elts)
        assert rc == capi.OK, out
        return out

    def device_relin_rc(self):
        out = api.DeviceBuffer(max(1, self.ksk_words()))
        rc = self.lib.troyhip_create_relin_key(self.ctx.h, C.c_uint64(self.seed[0]), C.c_uint64(self.seed[1]), C.c_void_p(self.dsk.ptr), C.c_void_p(out.ptr), None)
        if rc != capi.OK:
            return rc, self.lib.troyhip_last_error().decode()
        return rc, out.to_numpy().reshape(self.ksk_shape())

    def device_kswitch_rc(self, new_key):
        out = api.DeviceBuffer(max(1, self.ksk_words()))
        dnew = api.DeviceBuffer.from_numpy(new_key)
        rc = self.lib.troyhip_create_kswitch_key(self.ctx.h, C.c_uint64(self.seed[0]), C.c_uint64(self.seed[1]), C.c_void_p(self.dsk.ptr), C.c_void_p(dnew.ptr),
                                                 C.c_void_p(out.ptr), None)
        if rc != capi.OK:
            return rc, self.lib.troyhip_last_error().decode()
        return rc, out.to_numpy().reshape(self.ksk_shape())


def seeds_for(batch, base=1000):
    return np.array([[(base * 7919 + 31 * i) & MASK, 0xABCDEF ^ i] for i in range(batch)], dtype=np.uint64)


def check_keygen(S, batch, with_pk=True, pad=0):
    seeds = seeds_for(batch, base=batch + 3 * pad)
    sk, pk = S.device_keygen(seeds, with_pk, pad)
    for b in range(batch):
        hsk, hpk = S.host_keygen(seeds[b], with_pk)
        assert np.array_equal(sk[b], hsk), ("sk", batch, b)
        if with_pk:
            assert np.array_equal(pk[b], hpk), ("pk", batch, b)


def check_relin(S):
    rc, dev = S.device_relin_rc()
    assert rc == capi.OK, dev
    assert np.array_equal(dev, S.host_relin())


def check_kswitch(S, other_seed=(99, 1)):
    new_key = api.KeyGenerator(S.ctx, seed=other_seed).secretKey()
    rc, dev = S.device_kswitch_rc(new_key)
    assert rc == capi.OK, dev
    assert np.array_equal(dev, S.host_kswitch(new_key))


def check_galois(S, elts, items=None):
    """every element of `elts` in ONE device call; compares the listed items (default: all) with the host form.  Returns the keys (DeviceBuffers)"""
    dev = S.device_galois(elts)
    for i in (range(len(elts)) if items is None else items):
        assert np.array_equal(dev[i].to_numpy().reshape(S.ksk_shape()), S.host_galois(elts[i])), ("galois", elts[i], i)
    return dev
