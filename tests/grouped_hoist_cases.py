"""Shared checks of the hoisted calls with grouped keys (troyhip_apply_galois_hoisted_grouped, troyhip_galois_plain_sum_hoisted_grouped; DESIGN.md section
4.17): an exact host model of the definition in Python integers, the equality with the per-prime hoisted calls at one special prime, the independence of
the result from batch, order and scratch limit, decryption and noise under real keys, the refusals and the launch geometry.
Used by tests/test_device_grouped_hoist.py (emulator build) and tests/test_gpu_grouped_hoist.py (MI355X).

The model is grouped_cases.model_switch's arithmetic with the automorphism applied to every extended digit in the coefficient domain (the negation modulo
the output prime); the device permutes transforms, the model permutes coefficients, as in hoist_cases.model_item."""
import ctypes as C
import math

import numpy as np

import grouped_cases as GC
import hoist_cases as HC
import hoist_lt_cases as LC
from oracle import oracle
from troy_amd import api, app, capi, synth
from troy_amd.capi import BFV, BGV, CKKS

obj = GC.obj
LAUNCH = 16  # HOIST_MAX_ROT
SYMBOLS = ("troyhip_apply_galois_hoisted_grouped", "troyhip_galois_plain_sum_hoisted_grouped", "troyhip_apply_galois_hoisted_grouped_scratch_words",
           "troyhip_galois_plain_sum_hoisted_grouped_scratch_words")


class Keys:
    """synthetic uniform grouped keys of a setup, one per Galois element and seeded by it, on the host and in a tagged GaloisKeys"""

    def __init__(self, S, alpha):
        self.S, self.alpha = S, alpha
        self.gk = api.GaloisKeys(S.ctx, special_primes=alpha)
        self.host = {}

    def key(self, elt):
        if elt not in self.host:
            self.host[elt] = GC.synth_key(self.S, self.alpha, elt)
            self.gk.set_elt(elt, self.host[elt])
        return self.host[elt]

    def of(self, elts):
        return [self.key(g) if g != 1 else None for g in elts]


_keys = {}


def keys_of(S, alpha=None):
    alpha = S.alpha if alpha is None else alpha
    k = (id(S), alpha)
    if k not in _keys:
        _keys[k] = Keys(S, alpha)
    return _keys[k]


# ---------------------------------------------------------------- the definition, in exact integers
def model_ext(S, alpha, c1):
    """step 1 before the transform: {(j, o): ext_j[p_o]} of c1 [dl][N] (the scheme's form), coefficient form, o over the output primes"""
    N, K, primes = S.N, S.K, S.primes
    dl = c1.shape[0]
    out_ids = list(range(dl)) + list(range(K - alpha, K))
    x = [obj(oracle.ntt_standalone(N, primes[i], c1[i], 3) if S.ntt else c1[i]) for i in range(dl)]
    ext = {}
    for j, G in enumerate(GC.groups(K, alpha, dl)):
        Q = math.prod(primes[i] for i in G)
        y = {i: x[i] * pow(Q // primes[i], -1, primes[i]) % primes[i] for i in G}
        for o in out_ids:
            p = primes[o]
            ext[j, o] = (x[o] if o in G else sum(y[i] * (Q // primes[i] % p) for i in G) % p).astype(np.uint64)
    return ext, out_ids


def model_inner(S, ext, out_ids, elt, key):
    """step 2: {(c, o): sum_j NTT(sigma_g(ext_j[p_o])) * key[j][c][o] mod p_o}"""
    N, primes = S.N, S.primes
    d = 1 + max(j for j, _ in ext)
    acc = {}
    for o in out_ids:
        p = primes[o]
        e = [obj(oracle.ntt_standalone(N, p, oracle.apply_galois(N, elt, p, ext[j, o]), 1)) for j in range(d)]
        for c in range(2):
            acc[c, o] = sum(e[j] * obj(key[j, c, o]) for j in range(d)) % p
    return acc


def model_moddown(S, alpha, acc, base):
    """step 3 of grouped_cases.model_switch, term for term: base [2][dl][N] + the mod-down by P of acc"""
    N, K, primes = S.N, S.K, S.primes
    dl = base.shape[1]
    sp = list(range(K - alpha, K))
    P = math.prod(primes[m] for m in sp)
    h = P // 2
    out = np.zeros((2, dl, N), dtype=np.uint64)
    for c in range(2):
        a = {m: obj(oracle.ntt_standalone(N, primes[m], acc[c, m].astype(np.uint64), 3)) for m in sp}
        if S.scheme == BGV:
            z = {m: a[m] * pow(P // primes[m], -1, primes[m]) % primes[m] for m in sp}
        else:
            z = {m: (a[m] + h % primes[m]) * pow(P // primes[m], -1, primes[m]) % primes[m] for m in sp}
        r = sum(z[m] * (P // primes[m]) for m in sp)  # the integer itself
        for i in range(dl):
            q = primes[i]
            inv = pow(P, -1, q)
            if S.scheme == BFV:
                coeff = obj(oracle.ntt_standalone(N, q, acc[c, i].astype(np.uint64), 3))
                v = (coeff - r % q + h % q) * inv
            elif S.scheme == BGV:
                coeff = obj(oracle.ntt_standalone(N, q, acc[c, i].astype(np.uint64), 3))
                kt = (-(r % S.t)) * pow(P, -1, S.t) % S.t
                v = (coeff - r % q - kt % q * (P % q)) * inv
            else:
                corr = (r % q - h % q) % q
                v = (acc[c, i] - obj(oracle.ntt_standalone(N, q, corr.astype(np.uint64), 1))) * inv
            out[c, i] = ((obj(base[c, i]) + v) % q).astype(np.uint64)
    return out


def sigma(S, elt, row, j):
    return oracle.apply_galois_ntt(S.N, elt, row) if S.ntt else oracle.apply_galois(S.N, elt, S.primes[j], row)


def model_rotation(S, alpha, ct, elt, key, ext=None):
    """rotation `elt` of one ciphertext ct [2][dl][N] under the grouped key -> [2][dl][N]; ext: model_ext(ct[1]) made before"""
    if elt == 1:
        return ct.copy()
    dl = ct.shape[1]
    ext, out_ids = ext or model_ext(S, alpha, ct[1])
    base = np.zeros((2, dl, S.N), dtype=np.uint64)
    for j in range(dl):
        base[0, j] = sigma(S, elt, ct[0, j], j)
    return model_moddown(S, alpha, model_inner(S, ext, out_ids, elt, key), base)


def model_sum(S, alpha, ct, elts, keys, pts):
    """sum_r pts[r] * (element elts[r] of ct): the plaintext-weighted sum of the inner products before one mod-down, onto the base of section 4.11"""
    N, primes = S.N, S.primes
    dl = ct.shape[1]
    ext, out_ids = model_ext(S, alpha, ct[1])
    acc = {(c, o): np.zeros(N, dtype=object) for c in range(2) for o in out_ids}
    for g, key, pt in zip(elts, keys, pts):
        if g == 1:
            continue
        inner = model_inner(S, ext, out_ids, g, key)
        for c in range(2):
            for o in out_ids:
                acc[c, o] = (acc[c, o] + obj(pt[o]) * inner[c, o]) % primes[o]
    # the base in NTT form over the data limbs, back in the ciphertext's own form
    coeff = [[oracle.ntt_standalone(N, primes[j], ct[k, j], 3) if S.ntt else ct[k, j] for j in range(dl)] for k in range(2)]
    base = np.zeros((2, dl, N), dtype=np.uint64)
    for j in range(dl):
        q = primes[j]
        b = np.zeros((2, N), dtype=object)
        for g, pt in zip(elts, pts):
            rot = oracle.ntt_standalone(N, q, oracle.apply_galois(N, g, q, coeff[0][j]) if g != 1 else coeff[0][j], 1)
            b[0] += obj(pt[j]) * obj(rot)
            if g == 1:
                b[1] += obj(pt[j]) * obj(oracle.ntt_standalone(N, q, coeff[1][j], 1))
        for k in range(2):
            row = (b[k] % q).astype(np.uint64)
            base[k, j] = row if S.ntt else oracle.ntt_standalone(N, q, row, 3)
    if all(g == 1 for g in elts):
        return base
    return model_moddown(S, alpha, acc, base)


# ---------------------------------------------------------------- the library, through the Python layer
def rotations(S, alpha, data, elts, limit=0, gk=None):
    """-> [R][batch][2][limbs][N]"""
    K = keys_of(S, alpha)
    K.of(elts)
    out = S.ev.applyGaloisHoistedGrouped(S.ct(data), elts, K.gk if gk is None else gk, scratch_limit_words=limit)
    assert len(out) == len(elts)
    for o in out:
        assert (o.size(), o.limbs, o.is_ntt_form, o.batch) == (2, data.shape[2], S.ntt, data.shape[0])
    return np.stack([o.cpu() for o in out])


def transform(S, alpha, data, elts, pts, limit=0, gk=None):
    """-> [batch][2][limbs][N]"""
    K = keys_of(S, alpha)
    K.of(elts)
    bufs = [api.DeviceBuffer.from_numpy(p) for p in pts]
    out = S.ev.applyGaloisPlainSumHoistedGrouped(S.ct(data), elts, bufs, K.gk if gk is None else gk, scratch_limit_words=limit)
    assert (out.size(), out.limbs, out.is_ntt_form, out.batch) == (2, data.shape[2], S.ntt, data.shape[0])
    return out.cpu()


def canonical(S, got):
    return all((got[..., j, :] < np.uint64(S.primes[j])).all() for j in range(got.shape[-2]))


def check_rotations(S, alpha, dl, batch, elts, seed, items=None, limit=0):
    data = S.inputs(dl, batch, seed)
    got = rotations(S, alpha, data, elts, limit=limit)
    assert got.shape == (len(elts), batch, 2, dl, S.N) and canonical(S, got)
    keys = keys_of(S, alpha).of(elts)
    for b in (range(batch) if items is None else items):
        ext = model_ext(S, alpha, data[b, 1])
        for r, g in enumerate(elts):
            assert np.array_equal(got[r, b], model_rotation(S, alpha, data[b], g, keys[r], ext)), (S.name, alpha, dl, "rotation", r, "element", g, "item", b)
    return got, data


def check_transform(S, alpha, dl, batch, elts, seed, items=None, limit=0):
    data = S.inputs(dl, batch, seed)
    pts = LC.plains_of(S, len(elts), LC.PLAIN_SEED + seed)
    got = transform(S, alpha, data, elts, pts, limit=limit)
    assert got.shape == (batch, 2, dl, S.N) and canonical(S, got)
    keys = keys_of(S, alpha).of(elts)
    for b in (range(batch) if items is None else items):
        assert np.array_equal(got[b], model_sum(S, alpha, data[b], elts, keys, pts)), (S.name, alpha, dl, "item", b, elts)
    return got, data, pts


def small_levels(S, tag):
    """every level Lmax .. 1 for R2 and R3 (ragged and truncated groups, fewer limbs than special primes); the first level and a ragged one otherwise"""
    lmax = S.K - S.alpha
    return list(range(lmax, 0, -1)) if tag in ("R2", "R3") else [lmax, lmax - 1 if (lmax - 1) % S.alpha else lmax - 2]


def check_model_small(S, tag):
    """batch 5 (a group of four and a remainder) and batch 2 (four rotations per thread), R = 5 with element 1 and a repeated element (a ragged group of
    four rotations); both calls, and the linear transform whose elements are all 1 (no key read)"""
    elts = S.elts(5)
    assert 1 in elts and len(set(elts)) < 5
    for dl in small_levels(S, tag):
        for batch in (5, 2):
            check_rotations(S, S.alpha, dl, batch, elts, seed=100 + dl)
            check_transform(S, S.alpha, dl, batch, elts, seed=100 + dl)
    lmax = S.K - S.alpha
    lt0 = lt_slabs()
    data = S.inputs(lmax, 2, 77)
    pts = LC.plains_of(S, 2, 78)
    got = S.ev.applyGaloisPlainSumHoistedGrouped(S.ct(data), [1, 1], [api.DeviceBuffer.from_numpy(p) for p in pts], api.GaloisKeys(S.ctx, special_primes=S.alpha)).cpu()
    assert lt_slabs() - lt0 == 1
    for b in range(2):
        assert np.array_equal(got[b], model_sum(S, S.alpha, data[b], [1, 1], [None, None], pts))


def check_model_large(S, ragged):
    """N = 4096, the two-pass transforms: batch 5, R = 3, items 0 and 4, the first level and a ragged one"""
    e = S.elts(3)
    for dl in (S.K - S.alpha, ragged):
        check_rotations(S, S.alpha, dl, 5, e, seed=300 + dl, items=[0, 4])
        check_transform(S, S.alpha, dl, 5, [e[0], 1, e[1]], seed=300 + dl, items=[0, 4])


def check_many(S, batch, seed=61):
    """R = 17 distinct elements: the rotations run two chunks (16 and 1), the linear transform its accumulating launch"""
    elts = HC.many_elts(S, 17)
    assert len(set(elts)) == 17 and 1 not in elts
    dl = S.K - S.alpha
    s0, l0 = rot_slabs(), lt_slabs()
    check_rotations(S, S.alpha, dl, batch, elts, seed)
    assert rot_slabs() - s0 == 2
    check_transform(S, S.alpha, dl, batch, elts, seed)
    assert lt_slabs() - l0 == 1


# ---------------------------------------------------------------- alpha = 1 is the existing library
def check_alpha1(S, batch=3, seed=9):
    """special_primes = 1 with the per-prime keys: the bytes of troyhip_apply_galois_hoisted / troyhip_galois_plain_sum_hoisted, at every level"""
    elts = S.elts(3)
    lt_elts = [elts[0], 1, elts[1]]
    gk1 = api.GaloisKeys(S.ctx, special_primes=1)
    for g in set(elts):
        gk1.set_elt(g, S.key(g))  # the per-prime key [K-1][2][K][N]: its shape is the grouped shape at alpha = 1
    for dl in S.all_levels():
        data = S.inputs(dl, batch, seed + dl)
        want = S.hoisted(data, elts)
        got = S.ev.applyGaloisHoistedGrouped(S.ct(data), elts, gk1)
        assert np.array_equal(np.stack([o.cpu() for o in got]), want), (S.name, dl, "rotations")
        pts = LC.plains_of(S, 3, seed)
        want = LC.fused(S, data, lt_elts, pts)
        got = S.ev.applyGaloisPlainSumHoistedGrouped(S.ct(data), lt_elts, [api.DeviceBuffer.from_numpy(p) for p in pts], gk1)
        assert np.array_equal(got.cpu(), want), (S.name, dl, "linear transform")


# ---------------------------------------------------------------- independence
def rot_slabs():
    return capi.stat("grouped_hoist_slabs", api.KernelProvider.lib())


def lt_slabs():
    return capi.stat("grouped_hoist_lt_slabs", api.KernelProvider.lib())


def rot_words(S, dl, alpha, batch, rots):
    w = C.c_uint64(0)
    capi.check(S.lib, S.lib.troyhip_apply_galois_hoisted_grouped_scratch_words(S.ctx.h, dl, alpha, C.c_uint64(batch), rots, C.byref(w)))
    return w.value


def lt_words(S, dl, alpha, batch):
    w = C.c_uint64(0)
    capi.check(S.lib, S.lib.troyhip_galois_plain_sum_hoisted_grouped_scratch_words(S.ctx.h, dl, alpha, C.c_uint64(batch), C.byref(w)))
    return w.value


def check_scratch_formula(S, alpha, dl):
    """the queries return the figures of DESIGN.md section 4.17"""
    N, rl, d, ckks = S.N, dl + alpha, -(-dl // alpha), int(S.ntt)
    slack = 32 * 8 + 128
    for batch, rots in ((1, 1), (5, 3), (2, 40)):
        want = batch * N * (ckks * dl + d * rl) + min(rots, LAUNCH) * batch * N * (2 * rl + dl + ckks * (2 * alpha + 2 * dl)) + slack
        assert rot_words(S, dl, alpha, batch, rots) == want
        want = batch * N * (ckks * dl + d * rl + 2 * rl + 2 * dl + (1 - ckks) * 2 * dl + ckks * (2 * alpha + 2 * dl)) + slack
        assert lt_words(S, dl, alpha, batch) == want


def check_independence(S, alpha, dl, seed=31):
    """the same bytes at batch 1 and batch 5, with the elements reordered, and under the scratch limit of (one item, one rotation): one item per slab and
    one rotation per chunk; one word less is refused"""
    check_scratch_formula(S, alpha, dl)
    data = S.inputs(dl, 5, seed)
    elts = S.elts(5)
    real = sum(1 for g in elts if g != 1)
    pts = LC.plains_of(S, 5, seed)
    perm = [3, 0, 4, 2, 1]
    # rotations
    s0 = rot_slabs()
    ref = rotations(S, alpha, data, elts)
    assert rot_slabs() - s0 == 2  # two runs of consecutive elements other than 1
    for b in range(5):
        assert np.array_equal(rotations(S, alpha, data[b:b + 1], elts)[:, 0], ref[:, b]), ("item alone", b)
    got = rotations(S, alpha, data, [elts[i] for i in perm])
    for pos, i in enumerate(perm):
        assert np.array_equal(got[pos], ref[i]), ("reordered", i)
    for r, g in enumerate(elts):
        assert np.array_equal(rotations(S, alpha, data, [g])[0], ref[r]), ("element alone", g)
    one = rot_words(S, dl, alpha, 1, 1)
    s0 = rot_slabs()
    assert np.array_equal(rotations(S, alpha, data, elts, limit=one), ref)
    assert rot_slabs() - s0 == real * 5
    HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small for one rotation of one ciphertext", lambda: rotations(S, alpha, data, elts, limit=one - 1))
    # linear transform
    s0 = lt_slabs()
    ref = transform(S, alpha, data, elts, pts)
    assert lt_slabs() - s0 == 1
    for b in range(5):
        assert np.array_equal(transform(S, alpha, data[b:b + 1], elts, pts)[0], ref[b]), ("item alone", b)
    assert np.array_equal(transform(S, alpha, data, [elts[i] for i in perm], pts[perm]), ref), "reordered"
    one = lt_words(S, dl, alpha, 1)
    s0 = lt_slabs()
    assert np.array_equal(transform(S, alpha, data, elts, pts, limit=one), ref)
    assert lt_slabs() - s0 == 5
    HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small for one ciphertext", lambda: transform(S, alpha, data, elts, pts, limit=one - 1))


# ---------------------------------------------------------------- real keys
STEPS = (1, -2, 0, 5)


class Real:
    def __init__(self, S, alpha, steps=STEPS):
        ctx = S.ctx
        self.S, self.alpha, self.steps = S, alpha, steps
        self.kg = api.KeyGenerator(ctx, seed=(0x40157, 3))
        self.enc = api.Encryptor(ctx, self.kg.createPublicKey(), seed=(12, 34))
        self.dec = api.Decryptor(ctx, self.kg.secretKey())
        elts = [ctx.galois_elt_from_step(s) for s in steps if s]
        self.gk = api.GaloisKeys(ctx)
        for e, k in self.kg.createGaloisKeys(elts).items():
            self.gk.set_elt(e, k)
        self.gk_g = self.kg.createGaloisKeys(elts, special_primes=alpha, device=True)


def check_real_bfv_bgv(S, alpha, batch=2):
    """hoisted rotations with real grouped keys: decryption equal to rotateRows with the same keys; the budget at least the per-prime sequential one minus
    the derived margin of section 4.16 minus the 2 bits of floor jitter hoist_cases asserts.  The linear transform decrypts to what hoisted rotations,
    multiplyPlain and add decrypt to.  -> [(step, item, hoisted budget, sequential grouped budget, sequential per-prime budget, margin)]"""
    R = Real(S, alpha)
    ev, N, dl = S.ev, S.N, S.K - alpha
    rng = np.random.default_rng(3)
    benc = api.BatchEncoder(S.ctx)
    vals = rng.integers(0, S.t, (batch, N), dtype=np.uint64)
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([R.enc.encrypt(benc.encode(v)) for v in vals]))
    a = ev.modSwitchTo(a, dl) if a.limbs > dl else a
    assert a.limbs == dl
    margin = GC.noise_margin_bits(S.primes, alpha, dl, N)
    hoisted = ev.rotateRowsHoistedGrouped(a, R.steps, R.gk_g)
    out = []
    for r, s in enumerate(R.steps):
        h = hoisted[r].cpu()
        seq_g = ev.rotateRows(a, s, R.gk_g).cpu() if s else a.cpu()
        seq_p = ev.rotateRows(a, s, R.gk).cpu() if s else a.cpu()
        if s == 0:
            assert np.array_equal(h, a.cpu())
        for b in range(batch):
            m = benc.decode(R.dec.decrypt(h[b], correction_factor=hoisted[r].correction_factor))
            assert np.array_equal(m, benc.decode(R.dec.decrypt(seq_g[b], correction_factor=a.correction_factor))), (S.name, s, b)
            assert np.array_equal(m.reshape(2, -1), np.roll(vals[b].reshape(2, -1), -s, axis=1)), (S.name, s, b, "decryption")
            bh, bg, bp = (R.dec.invariantNoiseBudget(x[b]) for x in (h, seq_g, seq_p))
            print(S.name, "alpha", alpha, "step", s, "item", b, "budget hoisted grouped", bh, "sequential grouped", bg, "sequential per-prime", bp, "margin", margin)
            assert bp > 0 and bh >= bp - margin - 2, (S.name, s, b, bh, bp, margin)
            out.append((s, b, bh, bg, bp, margin))
    # the linear transform against hoisted rotations + multiplyPlain + add
    K = S.ctx.key_limbs
    diags = [rng.integers(0, S.t, N, dtype=np.uint64) for _ in R.steps]
    d_coeff = [api.DeviceBuffer.from_numpy(benc.encode(d)) for d in diags]
    d_ntt = [ev.transformPlainToNtt(p, K) for p in d_coeff]
    got = ev.rotateRowsPlainSumHoistedGrouped(a, R.steps, d_ntt, R.gk_g)
    assert (got.size(), got.limbs, got.is_ntt_form, got.batch) == (2, dl, False, batch)
    seq = None
    for term, p in zip(ev.rotateRowsHoistedGrouped(a, R.steps, R.gk_g), d_coeff):
        ev.multiplyPlainNormalInplace(term, p)
        if seq is None:
            seq = term
        else:
            ev.addInplace(seq, term)
    f, q = got.cpu(), seq.cpu()
    for b in range(batch):
        df = R.dec.decrypt(f[b], correction_factor=got.correction_factor)
        assert np.array_equal(df, R.dec.decrypt(q[b], correction_factor=seq.correction_factor)), (S.name, "linear transform", b)
        m = vals[b].reshape(2, -1).astype(object)
        exp = sum(d.reshape(2, -1).astype(object) * np.roll(m, -s, axis=1) for s, d in zip(R.steps, diags)) % S.t
        assert np.array_equal(benc.decode(df).reshape(2, -1), exp.astype(np.uint64)), (S.name, "linear transform", b, "decryption")
        print(S.name, "alpha", alpha, "linear transform item", b, "budget fused", R.dec.invariantNoiseBudget(f[b]), "composition", R.dec.invariantNoiseBudget(q[b]))
    return out


def check_real_ckks(S, alpha, batch=2, scale=2.0 ** 40):
    """median slot error of the hoisted form <= 1.5 x the sequential grouped median (the statistic of section 4.10), both maxima below 0.1, no ratio of
    maxima; the same statistic for the linear transform against its composition of existing calls"""
    R = Real(S, alpha)
    ev, N, dl = S.ev, S.N, S.K - alpha
    n = N // 2
    rng = np.random.default_rng(4)
    cenc = api.CKKSEncoder(S.ctx)
    vals = [rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in range(batch)]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([R.enc.encrypt(cenc.encode(v, scale)) for v in vals]), True, scale)
    a = ev.modSwitchTo(a, dl) if a.limbs > dl else a
    assert a.limbs == dl
    hoisted = ev.rotateVectorHoistedGrouped(a, R.steps, R.gk_g)
    out = []
    err = lambda ct, want, sc: np.concatenate([np.abs(cenc.decode(R.dec.decrypt(ct[b]), sc) - want[b]) for b in range(batch)])
    for r, s in enumerate(R.steps):
        assert hoisted[r].scale == a.scale and hoisted[r].is_ntt_form and hoisted[r].limbs == dl
        want = [np.roll(v, -s) for v in vals]
        d_h = err(hoisted[r].cpu(), want, scale)
        d_s = err(ev.rotateVector(a, s, R.gk_g).cpu() if s else a.cpu(), want, scale)
        print(S.name, "alpha", alpha, "step", s, "median slot error hoisted", np.median(d_h), "sequential grouped", np.median(d_s), "maxima", d_h.max(), d_s.max())
        assert d_h.max() < 0.1 and d_s.max() < 0.1
        assert np.median(d_h) <= 1.5 * np.median(d_s), (S.name, s, np.median(d_h), np.median(d_s))
        out.append((s, float(np.median(d_h)), float(np.median(d_s))))
    # the linear transform: the plaintexts at scale 2^20 so that the product's scale stays inside the modulus at this level
    ps = 2.0 ** 20
    K = S.ctx.key_limbs
    diags = [rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in R.steps]
    plains_np = [cenc.encode(d, ps, limbs=K) for d in diags]
    got = ev.rotateVectorPlainSumHoistedGrouped(a, R.steps, [api.DeviceBuffer.from_numpy(p) for p in plains_np], R.gk_g, plain_scale=ps)
    assert got.scale == a.scale * ps and got.is_ntt_form and (got.size(), got.limbs, got.batch) == (2, dl, batch)
    seq = None
    for s, p in zip(R.steps, plains_np):
        term = ev.rotateVector(a, s, R.gk_g) if s else a.copy()
        ev.multiplyPlainInplace(term, api.DeviceBuffer.from_numpy(p[:dl]), ps)
        if seq is None:
            seq = term
        else:
            ev.addInplace(seq, term)
    exact = [sum(d * np.roll(v, -s) for s, d in zip(R.steps, diags)) for v in vals]
    d_f, d_s = err(got.cpu(), exact, scale * ps), err(seq.cpu(), exact, scale * ps)
    print(S.name, "alpha", alpha, "linear transform median slot error fused", np.median(d_f), "composition", np.median(d_s), "maxima", d_f.max(), d_s.max())
    assert d_f.max() < 0.1 and d_s.max() < 0.1
    assert np.median(d_f) <= 1.5 * np.median(d_s), (S.name, "linear transform", np.median(d_f), np.median(d_s))
    return out


def check_matvec(S, alpha, d=8, batch=2):
    """app.DiagonalMatvec.apply picks the grouped member for a key set with the grouped tag (BFV / BGV)"""
    rng = np.random.default_rng(5)
    M = LC.matvec_matrix(rng, d, lambda n: rng.integers(1, 1 << 9, n, dtype=np.uint64))
    mv = app.DiagonalMatvec(S.ctx, M)
    R = Real(S, alpha, steps=tuple(mv.requiredSteps()))
    benc = api.BatchEncoder(S.ctx)
    mv.encodeDiagonals(benc)
    xs = [rng.integers(0, S.t, d, dtype=np.uint64) for _ in range(batch)]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([R.enc.encrypt(benc.encode(np.tile(x, S.N // d))) for x in xs]))
    a = S.ev.modSwitchTo(a, S.K - alpha) if a.limbs > S.K - alpha else a
    l0 = lt_slabs()
    y = mv.apply(S.ev, a, R.gk_g)
    assert lt_slabs() - l0 == 1
    yc = y.cpu()
    for b in range(batch):
        exp = (M.astype(object).dot(xs[b].astype(object)) % S.t).astype(np.uint64)
        assert np.array_equal(benc.decode(R.dec.decrypt(yc[b], correction_factor=y.correction_factor)), np.tile(exp, S.N // d)), (S.name, b)


# ---------------------------------------------------------------- refusals
def raw_rot(S, st_in, out_ptr, out_stride, elts, keys, alpha, n=None, batch=1, limit=0, ctx=None):
    so = capi.CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    R = len(elts)
    rc = S.lib.troyhip_apply_galois_hoisted_grouped((ctx or S.ctx).h, C.byref(st_in), C.byref(so), (C.c_uint32 * max(R, 1))(*elts), (C.c_void_p * max(R, 1))(*keys),
                                                    R if n is None else n, alpha, C.c_uint64(limit), C.c_uint64(batch), None)
    return rc, (S.lib.troyhip_last_error().decode() if rc else "")


def raw_lt(S, st_in, out_ptr, out_stride, elts, keys, pls, alpha, n=None, batch=1, limit=0, ctx=None):
    so = capi.CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    R = len(elts)
    rc = S.lib.troyhip_galois_plain_sum_hoisted_grouped((ctx or S.ctx).h, C.byref(st_in), C.byref(so), (C.c_uint32 * max(R, 1))(*elts), (C.c_void_p * max(R, 1))(*keys),
                                                        (C.c_void_p * max(R, 1))(*pls), R if n is None else n, C.c_double(1.0), alpha, C.c_uint64(limit), C.c_uint64(batch), None)
    return rc, (S.lib.troyhip_last_error().decode() if rc else "")


def check_refusals(S, alpha):
    inv = capi.INVALID_ARGUMENT
    N, K, lmax = S.N, S.K, S.K - alpha
    item = 2 * lmax * N
    g = S.ctx.galois_elt_from_step(1)
    G = keys_of(S, alpha)
    G.key(g)
    kp = G.gk.keys[api.GaloisKeys.getIndex(g)].ptr
    pl = [api.DeviceBuffer.from_numpy(p) for p in LC.plains_of(S, 2)]
    pp = pl[0].ptr
    a = S.ct(S.inputs(lmax, 1, 5))
    st = a.struct()
    out = api.DeviceBuffer(3 * 2 * (lmax + 1) * N)
    both = lambda st_in, o, stride, elts, keys, al=alpha, **kw: (raw_rot(S, st_in, o, stride, elts, keys, al, **kw), raw_lt(S, st_in, o, stride, elts, keys, [pp] * len(elts), al, **kw))
    same = lambda pair, want: pair[0] == want and pair[1] == want
    assert both(st, out.ptr, item, [g], [kp]) == ((capi.OK, ""), (capi.OK, ""))
    # a missing key, an even element, an element >= 2N
    assert same(both(st, out.ptr, item, [g], [None]), (inv, "Galois key not present"))
    assert same(both(st, out.ptr, item, [1, g], [None, None]), (inv, "Galois key not present"))
    assert same(both(st, out.ptr, item, [2], [kp]), (inv, "Galois element is not valid"))
    assert same(both(st, out.ptr, item, [2 * N + 1], [kp]), (inv, "Galois element is not valid"))
    assert raw_rot(S, st, out.ptr, item, [g], [kp], alpha, n=0) == (inv, "hoisted rotations take at least one Galois element")
    assert raw_lt(S, st, out.ptr, item, [g], [kp], [pp], alpha, n=0) == (inv, "hoisted linear transform takes at least one Galois element")
    assert raw_lt(S, st, out.ptr, item, [g], [kp], [None], alpha) == (inv, "plain_ntt is not valid for encryption parameters")
    # an operand above K - alpha limbs; alpha out of range
    if S.ctx.first_limbs >= lmax + 1:
        big = S.ct(S.inputs(lmax + 1, 1, 6))
        assert same(both(big.struct(), out.ptr, 2 * (lmax + 1) * N, [g], [kp]), (inv, "operand has more limbs than the grouped key serves"))
    for bad in (0, -1, 9, K):
        assert same(both(st, out.ptr, item, [g], [kp], al=bad), (inv, "special_primes must lie in 1 .. min(8, key limbs - 1)")), bad
    # size 3, the wrong form
    a3 = api.Ciphertext.from_numpy(S.ctx, synth.uniform_ct(6, S.primes[:lmax], 3, N, 1), S.ntt)
    assert same(both(a3.struct(), out.ptr, item, [g], [kp]), (inv, "encrypted size must be 2"))
    wrong = a.struct()
    wrong.is_ntt_form = 0 if S.ntt else 1
    msg = {BFV: "BFV encrypted cannot be in NTT form", BGV: "BGV encrypted cannot be in NTT form", CKKS: "CKKS encrypted must be in NTT form"}[S.scheme]
    assert same(both(wrong, out.ptr, item, [g], [kp]), (inv, msg))
    # the destination: overlapping the operand, missing, too narrow
    assert raw_rot(S, st, a.buf.ptr, item, [g], [kp], alpha) == (inv, "hoisted rotations: destination must be a distinct buffer")
    assert raw_lt(S, st, a.buf.ptr, item, [g], [kp], [pp], alpha) == (inv, "hoisted linear transform: destination must be a distinct buffer")
    assert both(st, None, item, [g], [kp])[0][0] == inv and both(st, None, item, [g], [kp])[1][0] == inv
    assert same(both(st, out.ptr, item - 1, [g], [kp]), (inv, "destination batch stride too small for the result size"))
    # the scratch limit and its queries
    assert raw_rot(S, st, out.ptr, item, [g], [kp], alpha, limit=rot_words(S, lmax, alpha, 1, 1) - 1)[0] == inv
    assert raw_lt(S, st, out.ptr, item, [g], [kp], [pp], alpha, limit=lt_words(S, lmax, alpha, 1) - 1)[0] == inv
    w = C.c_uint64(0)
    assert S.lib.troyhip_apply_galois_hoisted_grouped_scratch_words(S.ctx.h, lmax + 1, alpha, C.c_uint64(1), 1, C.byref(w)) == inv
    assert S.lib.troyhip_galois_plain_sum_hoisted_grouped_scratch_words(S.ctx.h, lmax, K, C.c_uint64(1), C.byref(w)) == inv
    # a host-only context: the queries answer, the calls refuse
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    assert S.lib.troyhip_apply_galois_hoisted_grouped_scratch_words(host.h, lmax, alpha, C.c_uint64(1), 1, C.byref(w)) == capi.OK and w.value == rot_words(S, lmax, alpha, 1, 1)
    for rc, text in both(st, out.ptr, item, [g], [kp], ctx=host):
        assert rc == capi.LOGIC_ERROR and "host-only" in text
    # element 1 alone needs no key and is a copy
    assert raw_rot(S, st, out.ptr, item, [1], [None], alpha) == (capi.OK, "")
    assert np.array_equal(out.to_numpy(item), a.cpu().reshape(-1))
    # the Python layer: a per-prime key set is refused by the *Grouped members, a grouped one by the existing members (grouped_cases pins the latter)
    per_prime = api.GaloisKeys(S.ctx)
    text = "this call takes keys with grouped digits"
    HC.with_raises(capi.InvalidArgument, text, lambda: S.ev.applyGaloisHoistedGrouped(a, [g], per_prime))
    HC.with_raises(capi.InvalidArgument, text, lambda: S.ev.applyGaloisPlainSumHoistedGrouped(a, [g], pl[:1], per_prime))
    HC.with_raises(capi.InvalidArgument, text, lambda: (S.ev.rotateVectorHoistedGrouped if S.ntt else S.ev.rotateRowsHoistedGrouped)(a, [1], per_prime))
    HC.with_raises(capi.InvalidArgument, text, lambda: (S.ev.rotateVectorPlainSumHoistedGrouped if S.ntt else S.ev.rotateRowsPlainSumHoistedGrouped)(a, [1], pl[:1], per_prime))
    HC.with_raises(capi.InvalidArgument, "grouped keys are not supported by this call", lambda: S.ev.applyGaloisHoisted(a, [g], G.gk))
    HC.with_raises(capi.InvalidArgument, "Galois key not present", lambda: S.ev.applyGaloisHoistedGrouped(a, [1, g], api.GaloisKeys(S.ctx, special_primes=alpha)))
    HC.with_raises(capi.InvalidArgument, "at least one", lambda: S.ev.applyGaloisHoistedGrouped(a, [], G.gk))
    HC.with_raises(capi.InvalidArgument, "one plaintext per element", lambda: S.ev.applyGaloisPlainSumHoistedGrouped(a, [g, 1], pl[:1], G.gk))
    HC.with_raises(capi.LogicError, "unsupported scheme", lambda: (S.ev.rotateRowsHoistedGrouped if S.ntt else S.ev.rotateVectorHoistedGrouped)(a, [1], G.gk))
    # the step members equal the element members
    steps = [1, 0]
    fn = S.ev.rotateVectorHoistedGrouped if S.ntt else S.ev.rotateRowsHoistedGrouped
    got = fn(a, steps, G.gk)
    want = S.ev.applyGaloisHoistedGrouped(a, [g, 1], G.gk)
    assert all(np.array_equal(x.cpu(), y.cpu()) for x, y in zip(got, want))


# ---------------------------------------------------------------- launch geometry
def check_large_grid(S, alpha, dl, batch, seed=41):
    """R = 1 and a batch whose launches all pass 65535 blocks in x: the first, the last and one middle item of both calls against the call at batch 1"""
    N = S.N
    g = S.ctx.galois_elt_from_step(1)
    block = S.inputs(dl, 64, seed)
    data = np.tile(block, (-(-batch // 64), 1, 1, 1))[:batch].copy()
    data[batch // 2], data[batch - 1] = block[5][::-1], block[7][::-1]  # the sampled items are no copies of their neighbours in the tiling
    # the smallest launches: the inner products (four items per thread over rl * N coefficients) and the mod-down (batch * 2 * N threads)
    assert -(-(dl + alpha) * N // 256) * -(-batch // 4) > 65535 and -(-batch * 2 * N // 256) > 65535
    pts = LC.plains_of(S, 1, seed)
    rot = rotations(S, alpha, data, [g])[0]
    lt = transform(S, alpha, data, [g], pts)
    for b in (0, batch // 2, batch - 1):
        assert np.array_equal(rotations(S, alpha, data[b:b + 1], [g])[0, 0], rot[b]), (S.name, "rotation, item", b)
        assert np.array_equal(transform(S, alpha, data[b:b + 1], [g], pts)[0], lt[b]), (S.name, "linear transform, item", b)
    assert np.array_equal(rot[0], model_rotation(S, alpha, data[0], g, keys_of(S, alpha).key(g)))
