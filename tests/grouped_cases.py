"""Shared checks of key switching with grouped digits (troyhip_switch_key_grouped and the calls on it): an exact host model of
the definition in Python integers, the equality with the per-prime library at one special prime, the keys, decryption and noise under real keys, the
independence of the result from batch and scratch limit, the refusals and the Python layer.
Used by tests/test_device_grouped.py (emulator build) and tests/test_gpu_grouped.py (MI355X).

The model shares no table with the library: every constant (Q_j / p_i, P / p_m, their inverses, floor(P / 2)) is a Python integer computed where it is
used, the mod-down sums are formed over the integers (r = sum_m z_m (P / p_m) itself, not its residues), and the transforms are the oracle's."""
import ctypes as C
import math

import numpy as np

import hoist_cases as HC
from oracle import oracle
from troy_amd import api, capi, synth
from troy_amd.capi import BFV, BGV, CKKS

SCHEMES = {"bfv": BFV, "bgv": BGV, "ckks": CKKS}
# (bits, alpha): every digit group is at most as long as the special modulus (checked on the primes CoeffModulus.Create returns: test_sets_are_admissible)
SETS = {
    "R2": ([58, 58, 58, 58, 58, 60, 60], 2),      # Lmax = 5, groups {0,1} {2,3} {4}: a ragged last group
    "R3": ([58, 58, 58, 58, 58, 60, 60, 60], 3),  # groups {0,1,2} {3,4}
    "M2": ([60, 58, 50, 49, 40, 60, 60], 2),      # guarded, guard-free and FP64-class primes in one digit
    "S2": ([30, 30, 30, 30, 32, 32], 2),          # primes below 2^33
}
ALPHA1 = ["bfv_n64_k3", "bgv_n128_k4", "ckks_n128_k6"]
ALPHA1_GPU = ["cfgA_bfv_n4096_k3", "bgv_n4096_k3", "ckks_n4096_k4"]
KEY_SEED = 8100


def obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


_setups = {}


def setup(scheme, N, tag):
    key = (scheme, N, tag, api.KernelProvider.lib()._name)  # the emulator build and the device library each get contexts of their own
    if key not in _setups:
        S = HC.Setup(*HC.adhoc(scheme, N, SETS[tag][0])) if tag in SETS else HC.Setup(tag)
        S.alpha = SETS[tag][1] if tag in SETS else 1
        _setups[key] = S
    return _setups[key]


def groups(K, alpha, dl):
    return [list(range(i0, min(i0 + alpha, dl))) for i0 in range(0, dl, alpha)]


def synth_key(S, alpha, seed):
    """a synthetic uniform grouped key [digits][2][K][N] (the arithmetic is oblivious to key validity)"""
    K, N = S.K, S.N
    d = -(-(K - alpha) // alpha)
    return synth.uniform_rows(KEY_SEED + seed, S.primes, d * 2 * K, N).reshape(d, 2, K, N)


# ---------------------------------------------------------------- the definition, in exact integers
def model_switch(S, alpha, target, key, base, seen=None):
    """grouped key switch of `target` [dl][N] (the scheme's form) under `key` [digits][2][K][N], added onto `base` [2][dl][N] -> [2][dl][N].
    seen: a dict that collects the overshoots u = floor(r / P) and the BGV k_t values the mod-down met"""
    N, K, primes = S.N, S.K, S.primes
    dl = target.shape[0]
    sp = list(range(K - alpha, K))
    out_ids = list(range(dl)) + sp
    P = math.prod(primes[m] for m in sp)
    h = P // 2
    x = [obj(oracle.ntt_standalone(N, primes[i], target[i], 3) if S.ntt else target[i]) for i in range(dl)]
    # 1. + 2.
    acc = {(c, o): np.zeros(N, dtype=object) for c in range(2) for o in out_ids}
    for j, G in enumerate(groups(K, alpha, dl)):
        Q = math.prod(primes[i] for i in G)
        y = {i: x[i] * pow(Q // primes[i], -1, primes[i]) % primes[i] for i in G}
        for o in out_ids:
            p = primes[o]
            ext = x[o] if o in G else sum(y[i] * (Q // primes[i] % p) for i in G) % p
            e = obj(oracle.ntt_standalone(N, p, ext.astype(np.uint64), 1))
            for c in range(2):
                acc[c, o] = (acc[c, o] + e * obj(key[j, c, o])) % p
    # 3.
    out = np.zeros((2, dl, N), dtype=np.uint64)
    for c in range(2):
        a = {m: obj(oracle.ntt_standalone(N, primes[m], acc[c, m].astype(np.uint64), 3)) for m in sp}
        if S.scheme == BGV:
            z = {m: a[m] * pow(P // primes[m], -1, primes[m]) % primes[m] for m in sp}
        else:
            z = {m: (a[m] + h % primes[m]) * pow(P // primes[m], -1, primes[m]) % primes[m] for m in sp}
        r = sum(z[m] * (P // primes[m]) for m in sp)  # the integer itself
        if seen is not None:
            seen.setdefault("u", set()).update(int(v) for v in r // P)
        for i in range(dl):
            q = primes[i]
            inv = pow(P, -1, q)
            if S.scheme == BFV:
                coeff = obj(oracle.ntt_standalone(N, q, acc[c, i].astype(np.uint64), 3))
                v = (coeff - r % q + h % q) * inv
            elif S.scheme == BGV:
                coeff = obj(oracle.ntt_standalone(N, q, acc[c, i].astype(np.uint64), 3))
                kt = (-(r % S.t)) * pow(P, -1, S.t) % S.t
                if seen is not None:
                    seen.setdefault("kt", set()).update(int(v) for v in kt)
                v = (coeff - r % q - kt % q * (P % q)) * inv
            else:
                corr = (r % q - h % q) % q
                v = (acc[c, i] - obj(oracle.ntt_standalone(N, q, corr.astype(np.uint64), 1))) * inv
            out[c, i] = ((obj(base[c, i]) + v) % q).astype(np.uint64)
    return out


def model_galois(S, alpha, ct, elt, key):
    N, primes = S.N, S.primes
    dl = ct.shape[1]
    g = lambda row, j: oracle.apply_galois_ntt(N, elt, row) if S.ntt else oracle.apply_galois(N, elt, primes[j], row)
    base = np.zeros((2, dl, N), dtype=np.uint64)
    target = np.zeros((dl, N), dtype=np.uint64)
    for j in range(dl):
        base[0, j], target[j] = g(ct[0, j], j), g(ct[1, j], j)
    return model_switch(S, alpha, target, key, base)


# ---------------------------------------------------------------- the library, through the C ABI and the Python layer
def slabs():
    return capi.stat("grouped_ks_slabs", api.KernelProvider.lib())


def raw_switch(S, alpha, ctdata, target, base, key_buf, limit=0, batch=None, st=None):
    """troyhip_switch_key_grouped -> (rc, message, result [B][size][dl][N]); base: None or [B][polys][dl][N]"""
    B, dl, N = ctdata.shape[0], ctdata.shape[2], S.N
    ct = api.Ciphertext.from_numpy(S.ctx, ctdata, S.ntt)
    tb = api.DeviceBuffer.from_numpy(np.ascontiguousarray(target))
    bb = api.DeviceBuffer.from_numpy(np.ascontiguousarray(base)) if base is not None else None
    polys = base.shape[1] if base is not None else 0
    st = st or ct.struct()
    rc = S.lib.troyhip_switch_key_grouped(S.ctx.h, C.byref(st), C.c_void_p(tb.ptr), C.c_uint64(dl * N), C.c_void_p(bb.ptr) if bb else None, C.c_uint64(polys * dl * N), polys,
                                          C.c_void_p(key_buf.ptr) if key_buf is not None else None, alpha, C.c_uint64(limit), C.c_uint64(B if batch is None else batch), None)
    return rc, (S.lib.troyhip_last_error().decode() if rc else ""), ct.cpu()


def key_sets(S, alpha, key, elt=None):
    """the one synthetic key as RelinKeys, GaloisKeys (of `elt`) and KSwitchKeys with the grouped tag"""
    rk, gk, kk = api.RelinKeys(S.ctx, special_primes=alpha), api.GaloisKeys(S.ctx, special_primes=alpha), api.KSwitchKeys(S.ctx, special_primes=alpha)
    rk.set(0, key)
    kk.set(0, key)
    if elt is not None:
        gk.set_elt(elt, key)
    return rk, gk, kk


def check_model(S, alpha, dl, batch, seed, pattern="uniform", items=None):
    """all four calls at `dl` limbs over `batch` items, every limb of every item (or of `items`) against the model"""
    N, primes = S.N, S.primes[:dl]
    key = synth_key(S, alpha, seed)
    kb = api.DeviceBuffer.from_numpy(key)
    elt = S.ctx.galois_elt_from_step(1)
    rk, gk, kk = key_sets(S, alpha, key, elt)
    ct3 = synth.edge_ct(pattern, seed, primes, 3, N, batch, ntt_form=S.ntt)
    other = synth.uniform_ct(seed + 1, primes, 2, N, batch)
    where = (S.name, alpha, dl, pattern)
    # switch_key onto what ct holds, onto a base of one and of two polynomials
    for base in (None, other[:, :1], other):
        rc, msg, got = raw_switch(S, alpha, ct3[:, :2].copy(), ct3[:, 2], base, kb)
        assert rc == capi.OK, msg
        for b in (range(batch) if items is None else items):
            start = ct3[b, :2] if base is None else np.concatenate([base[b], np.zeros((2 - base.shape[1], dl, N), dtype=np.uint64)])
            assert np.array_equal(got[b], model_switch(S, alpha, ct3[b, 2], key, start)), where + ("switch_key", None if base is None else base.shape[1], b)
    # relinearize of a size-3 operand, out of place and in place
    a3 = api.Ciphertext.from_numpy(S.ctx, ct3, S.ntt)
    r = S.ev.relinearize(a3, rk)
    assert (r.size(), r.limbs, r.is_ntt_form, r.batch) == (2, dl, S.ntt, batch) and np.array_equal(a3.cpu(), ct3)
    got = r.cpu()
    for b in (range(batch) if items is None else items):
        exp = model_switch(S, alpha, ct3[b, 2], key, ct3[b, :2])
        assert np.array_equal(got[b], exp), where + ("relinearize", b)
        assert all((got[b, :, j] < np.uint64(primes[j])).all() for j in range(dl))
    S.ev.relinearizeInplace(a3, rk)
    assert a3.size() == 2 and np.array_equal(a3.cpu()[:, :2], got), where + ("relinearizeInplace",)
    # a size-2 operand: a copy out of place, untouched in place, no key needed -- as with per-prime keys
    empty = api.RelinKeys(S.ctx, special_primes=alpha)
    r2 = S.ev.relinearize(a3, empty)
    assert r2 is not a3 and r2.size() == 2 and np.array_equal(r2.cpu(), a3.cpu()[:, :2]), where + ("relinearize of size 2",)
    S.ev.relinearizeInplace(a3, empty)
    assert a3.size() == 2 and np.array_equal(a3.cpu()[:, :2], got), where + ("relinearizeInplace of size 2",)
    # applyGalois, applyKeySwitching
    a2 = api.Ciphertext.from_numpy(S.ctx, ct3[:, :2].copy(), S.ntt, capacity=3 if batch % 2 else None)
    gg = S.ev.applyGalois(a2, elt, gk).cpu()
    kg = S.ev.applyKeySwitching(a2, kk).cpu()
    for b in (range(batch) if items is None else items):
        assert np.array_equal(gg[b], model_galois(S, alpha, ct3[b, :2], elt, key)), where + ("applyGalois", b)
        base = np.stack([ct3[b, 0], np.zeros((dl, N), dtype=np.uint64)])
        assert np.array_equal(kg[b], model_switch(S, alpha, ct3[b, 1], key, base)), where + ("applyKeySwitching", b)


def check_boundaries(S, alpha, dl):
    """mod-down boundaries built from the model.  dl = 1 mod alpha: the last digit is one limb, its extension is the limb itself; with the constant
    polynomial 1 in that limb and zero elsewhere the accumulators ARE the last key row, so the special limbs in coefficient form are chosen freely:
    BFV / CKKS: a + h = P - 1, P, P + 1 (the wrap), and z vectors whose integer sums give every overshoot 0 .. alpha - 1; BGV: k_t = 0 and k_t = t - 1"""
    assert dl % alpha == 1 % alpha
    N, K, primes = S.N, S.K, S.primes
    sp = list(range(K - alpha, K))
    P = math.prod(primes[m] for m in sp)
    h = P // 2
    key = synth_key(S, alpha, 77)
    jl = (dl - 1) // alpha
    rows = {m: synth.uniform_rows(5 + m, [primes[m]], 2, N).astype(object) for m in sp}  # coefficient form, [c][N]
    n = 0
    if S.scheme == BGV:
        for z0 in (0, primes[sp[0]] % S.t):  # r = z0 (P / p_0): k_t = 0, and r = P mod t: k_t = t - 1
            for m in sp:
                rows[m][:, n] = z0 * (P // primes[m]) % primes[m] if m == sp[0] else 0
            n += 1
    else:
        for a in (P - h - 1, P - h, P - h + 1, 0, P - 1):
            for m in sp:
                rows[m][:, n] = a % primes[m]
            n += 1
        for k in range(0, alpha + 1):  # k entries p_m - 1, the rest 0: overshoot max(k - 1, 0)
            for idx, m in enumerate(sp):
                z = primes[m] - 1 if idx < k else 0
                rows[m][:, n] = (z * (P // primes[m]) - h) % primes[m]
            n += 1
    for m in sp:
        for c in range(2):
            key[jl, c, m] = oracle.ntt_standalone(N, primes[m], rows[m][c].astype(np.uint64), 1)
    target = np.zeros((1, dl, N), dtype=np.uint64)
    if S.ntt:
        target[0, dl - 1, :] = 1
    else:
        target[0, dl - 1, 0] = 1
    base = synth.uniform_ct(9, primes[:dl], 2, N, 1)
    seen = {}
    exp = model_switch(S, alpha, target[0], key, base[0], seen)
    assert set(range(alpha)) <= seen["u"], seen  # the model met every overshoot
    if S.scheme == BGV:
        assert {0, S.t - 1} <= seen["kt"], sorted(seen["kt"])[:4]
    rc, msg, got = raw_switch(S, alpha, base.copy(), target[:, :], None, api.DeviceBuffer.from_numpy(key))
    assert rc == capi.OK, msg
    assert np.array_equal(got[0], exp), (S.name, alpha, dl, "boundaries")


# ---------------------------------------------------------------- alpha = 1 is the existing library
def check_alpha1_results(S, seed=5):
    """every level: the four calls with the tag special_primes = 1 against the per-prime calls under the same key, byte for byte"""
    N, K = S.N, S.K
    key = synth.uniform_kswitch_key(KEY_SEED + seed, S.primes, N)
    elt = S.ctx.galois_elt_from_step(1)
    rk1, gk1, kk1 = key_sets(S, 1, key, elt)
    rk0, gk0, kk0 = api.RelinKeys(S.ctx), api.GaloisKeys(S.ctx), api.KSwitchKeys(S.ctx)
    rk0.set(0, key); gk0.set_elt(elt, key); kk0.set(0, key)
    kb = api.DeviceBuffer.from_numpy(key)
    for dl in S.all_levels():
        for batch in (1, 5):
            ct3 = synth.uniform_ct(seed + dl, S.primes[:dl], 3, N, batch)
            mk3 = lambda: api.Ciphertext.from_numpy(S.ctx, ct3, S.ntt)
            mk2 = lambda: api.Ciphertext.from_numpy(S.ctx, ct3[:, :2].copy(), S.ntt, capacity=3 if batch % 2 else None)
            where = (S.name, dl, batch)
            assert np.array_equal(S.ev.relinearize(mk3(), rk1).cpu(), S.ev.relinearize(mk3(), rk0).cpu()), where + ("relinearize",)
            a, b = mk3(), mk3()
            S.ev.relinearizeInplace(a, rk1); S.ev.relinearizeInplace(b, rk0)
            assert np.array_equal(a.cpu()[:, :2], b.cpu()[:, :2]), where + ("relinearizeInplace",)
            assert np.array_equal(S.ev.applyGalois(mk2(), elt, gk1).cpu(), S.ev.applyGalois(mk2(), elt, gk0).cpu()), where + ("applyGalois",)
            assert np.array_equal(S.ev.applyKeySwitching(mk2(), kk1).cpu(), S.ev.applyKeySwitching(mk2(), kk0).cpu()), where + ("applyKeySwitching",)
            # switch_key itself, accumulating onto what ct holds
            rc, msg, got = raw_switch(S, 1, ct3[:, :2].copy(), ct3[:, 2], None, kb)
            assert rc == capi.OK, msg
            ct = api.Ciphertext.from_numpy(S.ctx, ct3[:, :2].copy(), S.ntt)
            st = ct.struct()
            tb = api.DeviceBuffer.from_numpy(np.ascontiguousarray(ct3[:, 2]))
            capi.check(S.lib, S.lib.troyhip_switch_key(S.ctx.h, C.byref(st), C.c_void_p(tb.ptr), C.c_uint64(dl * N), C.c_void_p(kb.ptr), C.c_uint64(batch), None))
            assert np.array_equal(got, ct.cpu()), where + ("switch_key",)


def key_generators(S, seed=(0x6A0, 9)):
    return api.KeyGenerator(S.ctx, seed=seed), api.KeyGenerator(S.ctx, seed=seed)


def dev_key(keys, index=0):
    K, N = keys.context.key_limbs, keys.context.N
    return keys.keys[index].to_numpy().reshape(keys.digits, 2, K, N)


def check_alpha1_keys(S):
    """special_primes = 1: host and device keys of all three sources equal today's keys byte for byte"""
    kg, kg2 = key_generators(S)
    other = api.KeyGenerator(S.ctx, seed=(77, 1)).secretKey()
    elts = [S.ctx.galois_elt_from_step(1), 2 * S.N - 1]
    assert np.array_equal(kg.createRelinKeys(special_primes=1), kg2.createRelinKeys())
    assert np.array_equal(dev_key(kg.createRelinKeys(special_primes=1, device=True)), kg2.createRelinKeys())
    g0 = kg2.createGaloisKeys(elts)
    g1, g1d = kg.createGaloisKeys(elts, special_primes=1), kg.createGaloisKeys(elts, special_primes=1, device=True)
    for e in elts:
        assert np.array_equal(g1[e], g0[e]) and np.array_equal(dev_key(g1d, api.GaloisKeys.getIndex(e)), g0[e])
    for dev in (False, True):  # call k of a generator draws from (lo + k, hi): the two generators stay in step
        a, b = kg.createKeySwitchingKeys(other, special_primes=1, device=dev), kg2.createKeySwitchingKeys(other)
        assert np.array_equal(dev_key(a) if dev else a, b)


def check_keys(S, alphas=(2, 3)):
    """device == host for every source; a Galois set in one call == element by element; createKeySwitchingKeys call k draws from stream (lo + k, hi);
    the layout: the grouped key differs from an encryption of zero by (P mod p_i) s' on the limbs of G_j only (checked through decryption of the rows)"""
    N, K, primes = S.N, S.K, S.primes
    other = api.KeyGenerator(S.ctx, seed=(77, 1)).secretKey()
    elts = [S.ctx.galois_elt_from_step(1), 2 * N - 1, S.ctx.galois_elt_from_step(-1)]
    for alpha in alphas:
        if alpha > min(8, K - 1):
            continue
        kg, kg2 = key_generators(S)
        digits, lmax, words = S.ev.groupedKeyShape(alpha)
        assert (digits, lmax, words) == (-(-(K - alpha) // alpha), K - alpha, digits * 2 * K * N)
        hr = kg.createRelinKeys(special_primes=alpha)
        assert hr.shape == (digits, 2, K, N)
        assert np.array_equal(dev_key(kg.createRelinKeys(special_primes=alpha, device=True)), hr)
        hg = kg.createGaloisKeys(elts, special_primes=alpha)
        dg = kg.createGaloisKeys(elts, special_primes=alpha, device=True)
        for e in elts:
            assert np.array_equal(dev_key(dg, api.GaloisKeys.getIndex(e)), hg[e]), (alpha, e)
            assert np.array_equal(kg.createGaloisKeys([e], special_primes=alpha, device=True).keys[api.GaloisKeys.getIndex(e)].to_numpy().reshape(hg[e].shape), hg[e])
        # the stream counting: call 0 and call 1 of one generator; a second generator seeded (lo + 1, hi) reproduces call 1 as its call 0
        k0 = kg.createKeySwitchingKeys(other, special_primes=alpha)
        k1 = kg.createKeySwitchingKeys(other, special_primes=alpha, device=True)
        assert kg.kswitch_calls == 2
        shifted = api.KeyGenerator(S.ctx, seed=(kg.seed[0] + 1, kg.seed[1]))
        shifted._sk, shifted._dsk = kg._sk, None
        assert np.array_equal(dev_key(k1), shifted.createKeySwitchingKeys(other, special_primes=alpha))
        assert not np.array_equal(dev_key(k1), k0)
        assert np.array_equal(kg2.createKeySwitchingKeys(other, special_primes=alpha, device=True).keys[0].to_numpy().reshape(k0.shape), k0)
        # the rows: c0 + c1 s = -e (small, times t for BGV) off the group, -e + (P mod p_i) s^2 on it
        sk = kg.secretKey()
        Pm = math.prod(primes[K - alpha:])
        for j in range(digits):
            for i in range(K):
                p = primes[i]
                v = (obj(hr[j, 0, i]) + obj(hr[j, 1, i]) * obj(sk[i])) % p
                if j * alpha <= i < min((j + 1) * alpha, lmax):
                    v = (v - (Pm % p) * obj(sk[i]) * obj(sk[i])) % p
                e = obj(oracle.ntt_standalone(N, p, v.astype(np.uint64), 3))
                e = np.where(e > p // 2, e - p, e)
                if S.scheme == BGV:
                    assert not (e % S.t).any()
                    e = e // S.t
                assert np.abs(e).max() <= 21, (alpha, j, i)


# ---------------------------------------------------------------- decryption and noise under real keys
def noise_margin_bits(primes, alpha, dl, N, err=21):
    """the difference of the two derived bounds in bits, ceil(log2(B_grouped / B_per_prime)) where positive, else 0"""
    K = len(primes)
    P = math.prod(primes[K - alpha:])
    d = -(-dl // alpha)
    qmax = max(math.prod(primes[i] for i in G) for G in groups(K, alpha, dl))
    grouped = d * alpha * qmax * N * err / P + (alpha - 0.5) * (1 + N)
    per_prime = dl * max(primes[:dl]) * N * err / primes[K - 1] + 0.5 * (1 + N)
    return max(0, math.ceil(math.log2(grouped / per_prime)))


class Real:
    def __init__(self, S, alpha):
        self.S, self.alpha = S, alpha
        ctx = S.ctx
        self.kg = api.KeyGenerator(ctx, seed=(0x40157, 3))
        self.enc = api.Encryptor(ctx, self.kg.createPublicKey(), seed=(12, 34))
        self.dec = api.Decryptor(ctx, self.kg.secretKey())
        self.steps = [-1, 4]  # the NAF terms of 3: the rotation by 3 walks two key switches
        elts = [ctx.galois_elt_from_step(s) for s in self.steps] + [2 * S.N - 1]
        self.rk, self.gk = api.RelinKeys(ctx), api.GaloisKeys(ctx)
        self.rk.set(0, self.kg.createRelinKeys())
        for e, k in self.kg.createGaloisKeys(elts).items():
            self.gk.set_elt(e, k)
        self.rk_g = self.kg.createRelinKeys(special_primes=alpha, device=True)
        self.gk_g = self.kg.createGaloisKeys(elts, special_primes=alpha, device=True)


def check_decrypt_bfv_bgv(S, alpha, batch=2):
    """multiply + grouped relinearize and grouped rotations of a fresh ciphertext at K - alpha limbs: exact decryption, equal to the per-prime calls' at the
    same level; the noise budget at least the per-prime one minus the derived margin.  -> [(call, grouped budget, per-prime budget, margin)]"""
    R = Real(S, alpha)
    ev, N, dl = S.ev, S.N, S.K - alpha
    rng = np.random.default_rng(3)
    benc = api.BatchEncoder(S.ctx)
    vals = rng.integers(0, S.t, (batch, N), dtype=np.uint64)
    plains = [benc.encode(v) for v in vals]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([R.enc.encrypt(p) for p in plains]))
    a = ev.modSwitchTo(a, dl) if a.limbs > dl else a
    assert a.limbs == dl
    margin = noise_margin_bits(S.primes, alpha, dl, N)
    prod = ev.multiply(a, a)
    pairs = [("relinearize", ev.relinearize(prod, R.rk_g), ev.relinearize(prod, R.rk), (vals * vals) % np.uint64(S.t) if S.t < 2**32 else None, 0),
             ("rotateRows 3", ev.rotateRows(a, 3, R.gk_g), ev.rotateRows(a, 3, R.gk), vals, 3),   # NAF: 3 = -1 + 4, the keys hold -1 and 4: two terms
             ("rotateColumns", ev.rotateColumns(a, R.gk_g), ev.rotateColumns(a, R.gk), vals, None)]
    out = []
    for name, g, p, want, step in pairs:
        assert g.size() == 2 and g.limbs == dl
        gc, pc = g.cpu(), p.cpu()
        for b in range(batch):
            mg = benc.decode(R.dec.decrypt(gc[b], correction_factor=g.correction_factor))
            mp = benc.decode(R.dec.decrypt(pc[b], correction_factor=p.correction_factor))
            assert np.array_equal(mg, mp), (S.name, name, b)
            w = want[b].reshape(2, -1)
            w = np.roll(w, -step, axis=1) if step else (w[::-1] if step is None else w)
            assert np.array_equal(mg.reshape(2, -1), w), (S.name, name, b, "decryption")
            bg, bp = R.dec.invariantNoiseBudget(gc[b]), R.dec.invariantNoiseBudget(pc[b])
            print(S.name, "alpha", alpha, name, "item", b, "budget grouped", bg, "per-prime", bp, "margin", margin)
            assert bp > 0 and bg >= bp - margin, (S.name, name, b, bg, bp, margin)
            out.append((name, bg, bp, margin))
    return out


def check_decrypt_ckks(S, alpha, batch=2, scale=2.0 ** 40):
    """grouped relinearize, rotateVector (NAF) and complexConjugate: the median slot error is the per-prime call's, within the factor 1.5 of the sequential checks"""
    R = Real(S, alpha)
    ev, N, dl = S.ev, S.N, S.K - alpha
    rng = np.random.default_rng(4)
    cenc = api.CKKSEncoder(S.ctx)
    vals = np.stack([rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2) for _ in range(batch)])
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([R.enc.encrypt(cenc.encode(v, scale)) for v in vals]), True, scale)
    a = ev.modSwitchTo(a, dl) if a.limbs > dl else a
    prod = ev.multiply(a, a)
    pairs = [("relinearize", ev.relinearize(prod, R.rk_g), ev.relinearize(prod, R.rk), vals * vals, scale * scale),
             ("rotateVector 3", ev.rotateVector(a, 3, R.gk_g), ev.rotateVector(a, 3, R.gk), np.roll(vals, -3, axis=1), scale),
             ("complexConjugate", ev.complexConjugate(a, R.gk_g), ev.complexConjugate(a, R.gk), np.conj(vals), scale)]
    out = []
    for name, g, p, want, sc in pairs:
        assert g.size() == 2 and g.limbs == dl and g.scale == p.scale == sc
        gc, pc = g.cpu(), p.cpu()
        eg = np.concatenate([np.abs(cenc.decode(R.dec.decrypt(gc[b]), sc) - want[b]) for b in range(batch)])
        ep = np.concatenate([np.abs(cenc.decode(R.dec.decrypt(pc[b]), sc) - want[b]) for b in range(batch)])
        print(S.name, "alpha", alpha, name, "median slot error grouped", np.median(eg), "per-prime", np.median(ep), "maxima", eg.max(), ep.max())
        assert ep.max() < 1e-3, "the per-prime call itself is expected to be right"
        assert np.median(eg) <= 1.5 * np.median(ep), (S.name, name, np.median(eg), np.median(ep))
        out.append((name, float(np.median(eg)), float(np.median(ep))))
    return out


# ---------------------------------------------------------------- independence, refusals, launch geometry
def scratch_words(S, dl, alpha, batch):
    w = C.c_uint64(0)
    capi.check(S.lib, S.lib.troyhip_switch_key_grouped_scratch_words(S.ctx.h, dl, alpha, C.c_uint64(batch), C.byref(w)))
    return w.value


def check_independence(S, alpha, dl, seed=31):
    """the same bytes for batch 1 / 3 / 5 and under a scratch limit of one item per slab; below one item the call is refused"""
    N = S.N
    key = synth_key(S, alpha, seed)
    kb = api.DeviceBuffer.from_numpy(key)
    elt = S.ctx.galois_elt_from_step(1)
    _, gk, _ = key_sets(S, alpha, key, elt)
    ct3 = synth.uniform_ct(seed, S.primes[:dl], 3, N, 5)
    s0 = slabs()
    rc, msg, ref = raw_switch(S, alpha, ct3[:, :2].copy(), ct3[:, 2], None, kb)
    assert rc == capi.OK and slabs() - s0 == 1, msg
    for nb in (1, 3):
        for b0 in range(0, 5, nb):
            part = ct3[b0:b0 + nb]
            assert np.array_equal(raw_switch(S, alpha, part[:, :2].copy(), part[:, 2], None, kb)[2], ref[b0:b0 + nb]), ("batch", nb, b0)
    one = scratch_words(S, dl, alpha, 1)
    assert one < scratch_words(S, dl, alpha, 2)
    s0 = slabs()
    rc, msg, got = raw_switch(S, alpha, ct3[:, :2].copy(), ct3[:, 2], None, kb, limit=one)
    assert rc == capi.OK and slabs() - s0 == 5 and np.array_equal(got, ref), msg
    s0 = slabs()
    rc, msg, got = raw_switch(S, alpha, ct3[:, :2].copy(), ct3[:, 2], None, kb, limit=2 * one)
    assert rc == capi.OK and slabs() - s0 >= 3 and np.array_equal(got, ref), msg
    rc, msg, _ = raw_switch(S, alpha, ct3[:, :2].copy(), ct3[:, 2], None, kb, limit=one - 1)
    assert (rc, msg) == (capi.INVALID_ARGUMENT, "scratch_limit_words is too small for one ciphertext")
    # applyGalois: its own runs of items
    a2 = lambda d: api.Ciphertext.from_numpy(S.ctx, d[:, :2].copy(), S.ntt)
    whole = S.ev.applyGalois(a2(ct3), elt, gk).cpu()
    for b in range(5):
        assert np.array_equal(S.ev.applyGalois(a2(ct3[b:b + 1]), elt, gk).cpu()[0], whole[b])
    st = a2(ct3)
    s = st.struct()
    limit = one + 2 * dl * N + 32 * 10 + 128
    capi.check(S.lib, S.lib.troyhip_apply_galois_grouped(S.ctx.h, C.byref(s), C.c_uint32(elt), C.c_void_p(kb.ptr), alpha, C.c_uint64(limit), C.c_uint64(5), None))
    assert np.array_equal(st.cpu(), whole)


def check_refusals(S, alpha):
    inv, logic = capi.INVALID_ARGUMENT, capi.LOGIC_ERROR
    N, K, lmax = S.N, S.K, S.K - alpha
    key = synth_key(S, alpha, 3)
    kb = api.DeviceBuffer.from_numpy(key)
    ct = lambda dl, size=2: synth.uniform_ct(4, S.primes[:dl], size, N, 1)
    d = ct(lmax, 3)
    call = lambda data, k=kb, al=alpha, st=None: raw_switch(S, al, data[:, :2].copy(), data[:, -1], None, k, st=st)[:2]
    assert call(d)[0] == capi.OK
    if lmax + 1 < K and S.ctx.first_limbs >= lmax + 1:
        assert call(ct(lmax + 1, 3)) == (inv, "operand has more limbs than the grouped key serves")
    assert call(d, k=None) == (inv, "kswitch_keys is not valid for encryption parameters")
    for bad in (0, -1, 9, K):
        assert call(d, al=bad) == (inv, "special_primes must lie in 1 .. min(8, key limbs - 1)"), bad
    wrong = api.Ciphertext.from_numpy(S.ctx, d[:, :2].copy(), S.ntt).struct()
    wrong.is_ntt_form = 0 if S.ntt else 1
    msg = {BFV: "BFV encrypted cannot be in NTT form", BGV: "BGV encrypted cannot be in NTT form", CKKS: "CKKS encrypted must be in NTT form"}[S.scheme]
    assert call(d, st=wrong) == (inv, msg)
    small = api.Ciphertext.from_numpy(S.ctx, d[:, :2].copy(), S.ntt).struct()
    small.size = 1
    assert call(d, st=small) == (inv, "encrypted size must be at least 2")
    # the shape query and the generators refuse the same alphas; a host-only context refuses the device form
    for bad in (0, 9, K):
        HC.with_raises(capi.InvalidArgument, "special_primes must lie in", lambda: S.ev.groupedKeyShape(bad))
        HC.with_raises(capi.InvalidArgument, "special_primes must lie in", lambda: api.KeyGenerator(S.ctx, seed=(1, 2)).createRelinKeys(special_primes=bad))
    # a key made with another alpha does not fit the key set
    if alpha + 1 <= min(8, K - 1) and -(-(K - alpha - 1) // (alpha + 1)) != key.shape[0]:
        HC.with_raises(capi.InvalidArgument, "kswitch_keys is not valid", lambda: api.RelinKeys(S.ctx, special_primes=alpha + 1).set(0, key))
    HC.with_raises(capi.InvalidArgument, "kswitch_keys is not valid", lambda: api.RelinKeys(S.ctx).set(0, key))
    # the calls that take per-prime keys only
    elt = S.ctx.galois_elt_from_step(1)
    rk, gk, _ = key_sets(S, alpha, key, elt)
    a = api.Ciphertext.from_numpy(S.ctx, d[:, :2].copy(), S.ntt)
    pt = api.DeviceBuffer(K * N)
    text = "grouped keys are not supported by this call"
    HC.with_raises(capi.InvalidArgument, text, lambda: S.ev.applyGaloisHoisted(a, [elt], gk))
    HC.with_raises(capi.InvalidArgument, text, lambda: S.ev.applyGaloisPlainSumHoisted(a, [elt], [pt], gk))
    HC.with_raises(capi.InvalidArgument, text, lambda: S.ev.applyGaloisPlainSumBsgs(a, [elt], [elt], [[pt]], gk))
    HC.with_raises(capi.InvalidArgument, text, lambda: S.ev.packLWEs([], gk))
    HC.with_raises(capi.InvalidArgument, text, lambda: S.ev.evaluatePolynomial(a, [1, 1], rk))
    # a missing key, as today
    HC.with_raises(capi.InvalidArgument, "Galois key not present", lambda: S.ev.applyGalois(a, 2 * N - 1, gk))
    HC.with_raises(capi.InvalidArgument, "Galois key not present", lambda: (S.ev.rotateVector if S.ntt else S.ev.rotateRows)(a, 2, gk))
    HC.with_raises(capi.InvalidArgument, "not enough relinearization keys", lambda: S.ev.relinearize(api.Ciphertext.from_numpy(S.ctx, d, S.ntt), api.RelinKeys(S.ctx, special_primes=alpha)))


def check_refusals_context():
    """K < 2, a special modulus shorter than a digit, a host-only context"""
    N = 64
    one = api.SEALContext(BFV, N, api.CoeffModulus.Create(N, [40]), int(api.PlainModulus.Batching(N, 10)))
    HC.with_raises(capi.LogicError, "keyswitching is not supported by the context", lambda: one.grouped_key_shape(1))
    short = api.SEALContext(BFV, N, api.CoeffModulus.Create(N, [50, 50, 50, 50, 40, 40]), int(api.PlainModulus.Batching(N, 10)))
    HC.with_raises(capi.InvalidArgument, "special modulus is smaller than a digit", lambda: short.grouped_key_shape(2))
    HC.with_raises(capi.InvalidArgument, "special modulus is smaller than a digit", lambda: api.KeyGenerator(short, seed=(1, 2)).createRelinKeys(special_primes=2))
    # ... but one special prime is the existing key switch, which takes a special prime shorter than a data prime
    assert short.grouped_key_shape(1)[:2] == (5, 5)
    assert np.array_equal(api.KeyGenerator(short, seed=(1, 2)).createRelinKeys(special_primes=1), api.KeyGenerator(short, seed=(1, 2)).createRelinKeys())
    primes = api.CoeffModulus.Create(N, [40, 40, 40, 40])
    host = api.SEALContext(BFV, N, primes, int(api.PlainModulus.Batching(N, 10)), host_only=True)
    kg = api.KeyGenerator(host, seed=(1, 2))
    assert kg.createRelinKeys(special_primes=2).shape == (1, 2, 4, N)
    w = api.DeviceBuffer(8)
    table = (C.c_void_p * 1)(w.ptr)
    rc = host.lib.troyhip_create_kswitch_keys_grouped(host.h, C.c_uint64(1), C.c_uint64(2), C.c_void_p(w.ptr), 1, None, None, C.c_uint64(1), 2, table, None)
    assert rc == capi.LOGIC_ERROR and "host-only" in host.lib.troyhip_last_error().decode()


def check_large_grid(S, alpha, dl, batch, seed=41):
    """every launch of the call is one-dimensional; a batch whose launches pass 65535 blocks in x (the only dimension they have): items 0, the middle one
    and the last against the model, and every item against the call at batch 1 on a sample"""
    N = S.N
    key = synth_key(S, alpha, seed)
    kb = api.DeviceBuffer.from_numpy(key)
    block = synth.uniform_ct(seed, S.primes[:dl], 3, N, 64)
    ct3 = np.tile(block, (-(-batch // 64), 1, 1, 1))[:batch].copy()
    ct3[batch // 2], ct3[batch - 1] = block[5][::-1], block[7][::-1]  # the sampled items are no copies of their neighbours in the tiling
    # the smallest launches: the mod-down (batch * 2 * N threads, 256 per block) and the inner product (four items per thread)
    assert -(-batch * 2 * N // 256) > 65535 and -(-(dl + alpha) * N // 256) * -(-batch // 4) > 65535
    rc, msg, got = raw_switch(S, alpha, ct3[:, :2].copy(), ct3[:, 2], None, kb)
    assert rc == capi.OK, msg
    for b in (0, batch // 2, batch - 1):
        assert np.array_equal(got[b], model_switch(S, alpha, ct3[b, 2], key, ct3[b, :2])), (S.name, "item", b)
    for b in (1, batch // 3, batch - 2):
        assert np.array_equal(raw_switch(S, alpha, ct3[b:b + 1, :2].copy(), ct3[b:b + 1, 2], None, kb)[2][0], got[b]), (S.name, "item alone", b)
