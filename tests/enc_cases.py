"""Shared checks of the device encryption (troyhip_encrypt / troyhip_encrypt_symmetric / troyhip_expand_seed): item i of a device call must be
byte-identical to the host function of the same form called with item i's seed (troyhip_host_encrypt*, the tested host path is the oracle).
Used by tests/test_device_encrypt.py (emulator build) and tests/test_gpu_encrypt.py (MI355X)."""
import ctypes as C

import numpy as np

from troy_amd import api, capi
from troy_amd.capi import CKKS

MASK = 2**64 - 1
FORMS = ["pk", "pk0", "sk", "sk0", "sks", "sks0"]  # public / symmetric / seeded symmetric; "0": an encryption of zero


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _is_prime(n):
    if n < 2:
        return False
    for q in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def rejecting_primes(N, count):
    """60-bit NTT primes just above 2^64 / 17: a 64-bit word is rejected by uniform_below(p) with probability (2^64 mod p) / 2^64, about 1/17"""
    out, p = [], (2**64 // 17) // (2 * N) * (2 * N) + 1
    while len(out) < count:
        p += 2 * N
        if _is_prime(p):
            out.append(p)
    return out


def rejection_rate(p):
    return (2**64 % p) / 2.0**64


class Setup:
    def __init__(self, scheme, N, primes, t, key_seed=(0x5EED, 7)):
        self.ctx = api.SEALContext(scheme, N, primes, t)
        self.scheme, self.N, self.t, self.primes = scheme, N, t, list(primes)
        self.lib = self.ctx.lib
        kg = api.KeyGenerator(self.ctx, seed=key_seed)
        self.sk, self.pk = kg.secretKey(), kg.createPublicKey()
        self.dsk, self.dpk = api.DeviceBuffer.from_numpy(self.sk), api.DeviceBuffer.from_numpy(self.pk)

    @classmethod
    def from_cfg(cls, cfg, primes=None):
        N = cfg["N"]
        primes = primes or api.CoeffModulus.Create(N, cfg["bits"])
        t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
        return cls(cfg["scheme"], N, primes, t)

    def data_levels(self):
        return list(range(self.ctx.first_limbs, self.ctx.last_limbs - 1, -1))

    def plains(self, batch, limbs, rng):
        """BFV/BGV: [batch][n] coefficients mod t (n < N: the host and the device both zero-extend); CKKS [batch][limbs][N] residues"""
        if self.scheme == CKKS:
            return np.stack([np.stack([rng.integers(0, p, self.N, dtype=np.uint64) for p in self.primes[:limbs]]) for _ in range(batch)])
        n = self.N - 3 if self.N > 8 else self.N
        return rng.integers(0, self.t, (batch, n), dtype=np.uint64)

    def host(self, form, seed, limbs, plain=None, a_seed=0):
        """the host form of `form` with one seed -> [2][limbs][N]"""
        out = np.zeros((2, limbs, self.N), dtype=np.uint64)
        lo, hi = C.c_uint64(int(seed[0])), C.c_uint64(int(seed[1]))
        n = 0 if plain is None else (self.N if self.scheme == CKKS else plain.size)
        pl = None if plain is None else _p(np.ascontiguousarray(plain))
        L = self.lib
        if form == "pk":
            rc = L.troyhip_host_encrypt(self.ctx.h, lo, hi, _p(self.pk), pl, C.c_uint64(n), limbs, _p(out))
        elif form == "sk":
            rc = L.troyhip_host_encrypt_symmetric(self.ctx.h, lo, hi, _p(self.sk), pl, C.c_uint64(n), limbs, _p(out))
        elif form in ("pk0", "sk0"):
            rc = L.troyhip_host_encrypt_zero(self.ctx.h, lo, hi, _p(self.pk if form == "pk0" else self.sk), int(form == "sk0"), limbs, _p(out))
        else:
            rc = L.troyhip_host_encrypt_symmetric_seeded(self.ctx.h, lo, hi, C.c_uint64(int(a_seed)), _p(self.sk), pl, C.c_uint64(n), limbs, _p(out))
        capi.check(L, rc)
        return out

    def device_rc(self, form, seeds, limbs, plains=None, per_item=True, a_seeds=None, pad=0, scale=1.0, batch=None):
        """one device call; returns (status, [batch][2][limbs][N] or None, descriptor)"""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        batch = len(seeds) if batch is None else batch
        N = self.N
        stride = 2 * limbs * N + pad
        out = api.DeviceBuffer(max(1, batch) * stride)
        st = capi.CtStruct(out.ptr, stride, 0, limbs, 0, 0.0, 0)
        dplain, n, pstride = None, 0, 0
        if plains is not None:
            P = np.ascontiguousarray(plains if per_item else plains[:1], dtype=np.uint64)
            dplain = api.DeviceBuffer.from_numpy(P)
            n = N if self.scheme == CKKS else P.shape[1]
            pstride = (P[0].size if per_item else 0)
        pl = None if dplain is None else C.c_void_p(dplain.ptr)
        L = self.lib
        if form in ("pk", "pk0"):
            rc = L.troyhip_encrypt(self.ctx.h, C.c_void_p(self.dpk.ptr), _p(seeds), pl, C.c_uint64(n), C.c_uint64(pstride), C.c_double(scale), C.byref(st),
                                   C.c_uint64(batch), None)
        else:
            aseeds = None if a_seeds is None else _p(np.ascontiguousarray(a_seeds, dtype=np.uint64))
            rc = L.troyhip_encrypt_symmetric(self.ctx.h, C.c_void_p(self.dsk.ptr), _p(seeds), aseeds, pl, C.c_uint64(n), C.c_uint64(pstride), C.c_double(scale),
                                             C.byref(st), C.c_uint64(batch), None)
        if rc != capi.OK:
            return rc, L.troyhip_last_error().decode(), st
        data = out.to_numpy().reshape(batch, stride)[:, :2 * limbs * N].reshape(batch, 2, limbs, N)
        return rc, data, st

    def device(self, *args, **kw):
        rc, data, st = self.device_rc(*args, **kw)
        assert rc == capi.OK, data
        return data, st

    def expand_device(self, a_seeds, limbs, pad=0):
        a = np.ascontiguousarray(a_seeds, dtype=np.uint64)
        stride = limbs * self.N + pad
        out = api.DeviceBuffer(len(a) * stride)
        capi.check(self.lib, self.lib.troyhip_expand_seed(self.ctx.h, _p(a), limbs, C.c_void_p(out.ptr), C.c_uint64(stride), C.c_uint64(len(a)), None))
        return out.to_numpy().reshape(len(a), stride)[:, :limbs * self.N].reshape(len(a), limbs, self.N)

    def expand_host(self, a_seed, limbs):
        out = np.zeros((limbs, self.N), dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_expand_seed(self.ctx.h, C.c_uint64(int(a_seed)), limbs, _p(out)))
        return out


def seeds_for(batch, base=1000):
    return np.array([[(base * 7919 + 31 * i) & MASK, 0xABCDEF ^ i] for i in range(batch)], dtype=np.uint64)


def a_seeds_for(batch, base=1000):
    return np.array([(base * 104729 + 17 * i + 1) & MASK for i in range(batch)], dtype=np.uint64)


def check_form(S, form, limbs, batch, per_item=True, pad=0, rng=None, items=None):
    """device call of `batch` items vs the host form per item (every item, or the listed `items`)"""
    rng = rng or np.random.default_rng(batch * 131 + limbs)
    seeds = seeds_for(batch, base=limbs * 10 + len(form))
    a_seeds = a_seeds_for(batch, base=limbs) if form.startswith("sks") else None
    plains = None if form.endswith("0") else S.plains(batch, limbs, rng)
    scale = 2.0**20 if S.scheme == CKKS and plains is not None else 1.0
    dev, st = S.device(form, seeds, limbs, plains, per_item, a_seeds, pad=pad, scale=scale)
    assert st.size == 2 and st.limbs == limbs and bool(st.is_ntt_form) == (S.scheme == CKKS) and st.correction_factor == 1
    assert st.scale == scale
    for b in (range(batch) if items is None else items):
        plain = None if plains is None else plains[b if per_item else 0]
        exp = S.host(form, seeds[b], limbs, plain, 0 if a_seeds is None else a_seeds[b])
        assert np.array_equal(dev[b], exp), (form, limbs, batch, b)
    return dev
