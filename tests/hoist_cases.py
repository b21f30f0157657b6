"""Shared checks of hoisted rotations (troyhip_apply_galois_hoisted): an exact host model of the definition, the independence
of the result from how it was asked for, the comparison with the sequential rotation under real keys, the refusals and the Python layer.
Used by tests/test_device_hoist.py (emulator build) and tests/test_gpu_hoist.py (MI355X).

The model restates the definition independently of the device code: the automorphism is applied in the COEFFICIENT domain (oracle.apply_galois modulo
the output prime) and transformed (oracle.ntt_standalone), where the device permutes the transformed digits; the inner product and the mod-down are
Python integers."""
import ctypes as C

import numpy as np

import cases
from oracle import oracle
from troy_amd import api, capi, synth
from troy_amd.capi import BFV, BGV, CKKS

BENCH = {  # bench.py's workload parameters (tools/encrypt_bench.py SHAPES)
    "bfv_n32768_l14": dict(scheme=BFV, N=32768, bits=[60] + [58] * 13 + [60], tbits=20),
    "bgv_n65536_relin_rot": dict(scheme=BGV, N=65536, bits=[60] + [50] * 13 + [60], tbits=20),
}
SMALL = ["bfv_n64_k3", "bgv_n128_k4", "ckks_n128_k6"]          # batch 5 (a blocked group of four and a remainder), R = 3
MEDIUM = ["cfgA_bfv_n4096_k3", "bgv_n4096_k3", "ckks_n4096_k4"]  # batch 2, R = 5 with element 1: the single-pass and fused mod-down routes
NARROW = ["nar_bfv_n4096_k3"]                                    # primes below 2^33: the element-wise epilogue
KEY_SEED = 7100


def config(name):
    return BENCH[name] if name in BENCH else cases.CONFIGS[name]


def obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


class Setup:
    """one parameter set; synthetic uniform keys (the arithmetic is oblivious to key validity), one per Galois element, seeded by the element"""

    def __init__(self, name):
        cfg = self.cfg = config(name)
        self.name, self.scheme, self.N = name, cfg["scheme"], cfg["N"]
        N = self.N
        self.primes = [int(p) for p in api.CoeffModulus.Create(N, cfg["bits"])]
        self.t = int(api.PlainModulus.Batching(N, cfg["tbits"])) if cfg["tbits"] else 0
        self.ctx = api.SEALContext(self.scheme, N, self.primes, self.t)
        self.lib = self.ctx.lib
        self.K = len(self.primes)
        self.ev = api.Evaluator(self.ctx)
        self.ntt = self.scheme == CKKS
        self.gk = api.GaloisKeys(self.ctx)
        self.host_keys = {}

    def levels(self):
        return sorted({self.ctx.first_limbs, self.ctx.last_limbs}, reverse=True)

    def key(self, elt, rows_only=None):
        """the key of element `elt`: on the device in self.gk, on the host [K-1][2][K][N]; the synthetic generator and its device twin agree, so a large
        key is filled on the device and only the rows the model reads (digits below `rows_only`) come back"""
        idx = api.GaloisKeys.getIndex(elt)
        K, N = self.K, self.N
        if elt not in self.host_keys:
            if rows_only is None:
                k = synth.uniform_kswitch_key(KEY_SEED + elt, self.primes, N)
                self.gk.set(idx, k)
            else:
                buf = api.DeviceBuffer((K - 1) * 2 * K * N)
                self.ctx.fill_uniform(buf, (K - 1) * 2 * K, self.primes, KEY_SEED + elt)
                self.gk.set_device(idx, buf)
                k = np.zeros((K - 1, 2, K, N), dtype=np.uint64)
                k[:rows_only] = buf.to_numpy(rows_only * 2 * K * N).reshape(rows_only, 2, K, N)
            self.host_keys[elt] = k
        return self.host_keys[elt]

    def inputs(self, limbs, batch, seed):
        return synth.uniform_ct(seed, self.primes[:limbs], 2, self.N, batch)

    def ct(self, data):
        """an odd batch leaves room for a third polynomial per item: the operand is then a strided batch"""
        return api.Ciphertext.from_numpy(self.ctx, data, self.ntt, capacity=3 if data.shape[0] % 2 else None)

    def elts(self, R):
        """R elements: the conjugation 2N - 1, rotation steps, a repeated element; from R = 5 on element 1 as well"""
        N = self.N
        e = [self.ctx.galois_elt_from_step(1), 2 * N - 1, self.ctx.galois_elt_from_step(1), 1, self.ctx.galois_elt_from_step(-3 if N > 64 else 2)]
        if R == 2:
            return [e[1], e[0]]
        return e[:R]

    def hoisted(self, data, elts, limit=0, rows_only=None):
        """-> [R][batch][2][limbs][N] through the Python layer"""
        for g in elts:
            if g != 1:
                self.key(g, rows_only)
        out = self.ev.applyGaloisHoisted(self.ct(data), elts, self.gk, scratch_limit_words=limit)
        assert len(out) == len(elts)
        for o in out:
            assert (o.size(), o.limbs, o.is_ntt_form, o.batch) == (2, data.shape[2], self.ntt, data.shape[0])
        return np.stack([o.cpu() for o in out])


# ---------------------------------------------------------------- the definition, in exact integers
def model_item(S, ct, elt, key):
    """rotation `elt` of one ciphertext ct [2][dl][N] under `key` [K-1][2][K][N] -> [2][dl][N]"""
    N, K, primes = S.N, S.K, S.primes
    dl = ct.shape[1]
    if elt == 1:
        return ct.copy()
    qk = primes[K - 1]
    out_primes = primes[:dl] + [qk]
    key_limb = list(range(dl)) + [K - 1]
    # d_j: limb j of c1 in coefficient form, canonical
    d = [oracle.ntt_standalone(N, primes[j], ct[1, j], 3) if S.ntt else ct[1, j] for j in range(dl)]
    # 1. + 2.  e[i][j] = NTT_{p_i}(d_j mod p_i) read through pi_g  ==  NTT_{p_i}(sigma_g(d_j mod p_i)), and the inner product with the unpermuted key
    acc = np.zeros((2, dl + 1, N), dtype=object)
    for i, p in enumerate(out_primes):
        for j in range(dl):
            e = oracle.ntt_standalone(N, p, oracle.apply_galois(N, elt, p, d[j] % np.uint64(p)), 1)
            for k in range(2):
                acc[k, i] += obj(e) * obj(key[j, k, key_limb[i]])
        acc[:, i] %= p
    # sigma_g(c0)
    base = np.zeros((2, dl, N), dtype=object)
    for j in range(dl):
        base[0, j] = obj(oracle.apply_galois_ntt(N, elt, ct[0, j]) if S.ntt else oracle.apply_galois(N, elt, primes[j], ct[0, j]))
    # 3. the scheme's mod-down by the special prime, added to (sigma_g(c0), 0)
    half = qk >> 1
    out = np.zeros((2, dl, N), dtype=np.uint64)
    for k in range(2):
        if S.ntt:
            last = obj(oracle.ntt_standalone(N, qk, acc[k, dl].astype(np.uint64), 3))
        else:
            coeff = [obj(oracle.ntt_standalone(N, p, acc[k, i].astype(np.uint64), 3)) for i, p in enumerate(out_primes)]
            last = coeff[dl]
        for j in range(dl):
            q = primes[j]
            inv = pow(qk, -1, q)
            if S.scheme == BFV:
                tl = (last + half) % qk
                v = (coeff[j] - tl % q + half % q) * inv
            elif S.scheme == BGV:
                kt = (-last) % S.t * pow(qk, -1, S.t) % S.t
                v = (coeff[j] - kt % q * (qk % q) - last % q) * inv
            else:
                tl = (last + half) % qk
                corr = ((tl % q) + (q - half % q)) % q
                v = (acc[k, j] - obj(oracle.ntt_standalone(N, q, corr.astype(np.uint64), 1))) * inv
            out[k, j] = ((base[k, j] + v) % q).astype(np.uint64)
    return out


def check_model(S, limbs, batch, R, seed, items=None, rows_only=None):
    """every limb of every output item (or of `items`) equals the model"""
    data = S.inputs(limbs, batch, seed)
    elts = S.elts(R)
    got = S.hoisted(data, elts, rows_only=rows_only)
    assert got.shape == (R, batch, 2, limbs, S.N)
    for r, g in enumerate(elts):
        for b in (range(batch) if items is None else items):
            exp = model_item(S, data[b], g, S.host_keys.get(g))
            assert np.array_equal(got[r, b], exp), (S.name, limbs, "rotation", r, "element", g, "item", b)
            assert all((got[r, b, :, j] < np.uint64(S.primes[j])).all() for j in range(limbs))
    return got, data, elts


# ---------------------------------------------------------------- independence
def scratch_words(S, limbs, items, rots):
    """what Evaluator::apply_galois_hoisted asks of the arena for a slab of `items` x `rots` (evaluator.cpp)"""
    N, dl, rl = S.N, limbs, limbs + 1
    return items * N * (rl * dl + (dl if S.ntt else 0)) + rots * items * N * (2 * rl + 3 * dl + 4) + 32 * 8 + 128


def slabs():
    return capi.stat("hoist_slabs", api.KernelProvider.lib())


def check_independence(S, limbs, batch, seed):
    data = S.inputs(limbs, batch, seed)
    elts = S.elts(5)
    real = sum(1 for g in elts if g != 1)
    runs = sum(1 for i, g in enumerate(elts) if g != 1 and (i == 0 or elts[i - 1] == 1))
    s0 = slabs()
    ref = S.hoisted(data, elts)
    assert slabs() - s0 == runs == 2  # under the default limit a slab is a run of consecutive elements other than 1 (which is a copy)
    # R = 1 calls per element
    for r, g in enumerate(elts):
        assert np.array_equal(S.hoisted(data, [g])[0], ref[r]), ("alone", g)
    # a permuted element list
    perm = [3, 0, 4, 2, 1]
    got = S.hoisted(data, [elts[i] for i in perm])
    for pos, i in enumerate(perm):
        assert np.array_equal(got[pos], ref[i]), ("permuted", i)
    # batch 1 per item
    for b in range(batch):
        assert np.array_equal(S.hoisted(data[b:b + 1], elts)[:, 0], ref[:, b]), ("item alone", b)
    # a scratch limit of one rotation of the whole batch: one slab per element that needs a key
    s0 = slabs()
    assert np.array_equal(S.hoisted(data, elts, limit=scratch_words(S, limbs, batch, 1)), ref)
    assert slabs() - s0 == real >= 2
    # ... and of one rotation of one item: the digits of each item are made once, one slab per (item, element)
    s0 = slabs()
    assert np.array_equal(S.hoisted(data, elts, limit=scratch_words(S, limbs, 1, 1)), ref)
    assert slabs() - s0 == real * batch
    # below that: refused
    with_raises(capi.InvalidArgument, "scratch_limit_words is too small", lambda: S.hoisted(data, elts, limit=scratch_words(S, limbs, 1, 1) - 1))


def with_raises(exc, match, fn):
    import pytest
    with pytest.raises(exc, match=match):
        fn()


# ---------------------------------------------------------------- against the sequential path, with real keys
class RealSetup:
    def __init__(self, name, steps):
        cfg = self.cfg = config(name)
        self.scheme, self.N, self.steps = cfg["scheme"], cfg["N"], steps
        N = self.N
        self.primes = api.CoeffModulus.Create(N, cfg["bits"])
        self.t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
        self.ctx = api.SEALContext(self.scheme, N, self.primes, self.t)
        self.kg = api.KeyGenerator(self.ctx, seed=(0x40157, 3))
        self.sk = self.kg.secretKey()
        self.enc = api.Encryptor(self.ctx, self.kg.createPublicKey(), seed=(12, 34))
        self.dec = api.Decryptor(self.ctx, self.sk)
        self.ev = api.Evaluator(self.ctx)
        self.gk = api.GaloisKeys(self.ctx)
        for e, k in self.kg.createGaloisKeys([self.ctx.galois_elt_from_step(s) for s in steps if s]).items():
            self.gk.set_elt(e, k)


def check_sequential_bfv_bgv(name, steps=(1, -2, 0, 5), batch=2):
    """decryption equality, differing limbs, and the noise budget within 2 bits of the sequential rotation's; -> the observed budget gaps"""
    S = RealSetup(name, steps)
    rng = np.random.default_rng(3)
    benc = api.BatchEncoder(S.ctx)
    plains = [benc.encode(rng.integers(0, S.t, S.N, dtype=np.uint64)) for _ in range(batch)]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(p) for p in plains]))
    hoisted = S.ev.rotateRowsHoisted(a, steps, S.gk)
    differs, gaps = False, []
    for r, s in enumerate(steps):
        seq = S.ev.rotateRows(a, s, S.gk).cpu()
        h = hoisted[r].cpu()
        if s == 0:
            assert np.array_equal(h, a.cpu())
        differs = differs or not np.array_equal(h, seq)
        for b in range(batch):
            assert np.array_equal(S.dec.decrypt(h[b]), S.dec.decrypt(seq[b])), (name, s, b)
            if s:  # the rotation moved the slots: rows rotate left by s
                m = benc.decode(S.dec.decrypt(h[b])).reshape(2, -1)
                assert np.array_equal(m, np.roll(benc.decode(plains[b]).reshape(2, -1), -s, axis=1)), (name, s, b)
            bh, bs = S.dec.invariantNoiseBudget(h[b]), S.dec.invariantNoiseBudget(seq[b])
            print(name, "step", s, "item", b, "budget hoisted", bh, "sequential", bs)
            assert bs > 0 and bh >= bs - 2, (name, s, b, bh, bs)
            gaps.append(bs - bh)
    assert differs, "the hoisted limbs are not expected to equal the sequential ones (q_j mod p_i where a coefficient is negated)"
    return gaps


def check_sequential_ckks(name, steps=(1, -2, 0, 5), batch=2, scale=2.0 ** 25):
    """hoisted slot error <= 4 x the sequential path's, both against the exactly rotated input; -> [(hoisted, sequential)]"""
    S = RealSetup(name, steps)
    rng = np.random.default_rng(4)
    cenc = api.CKKSEncoder(S.ctx)
    vals = [rng.uniform(-1, 1, S.N // 2) + 1j * rng.uniform(-1, 1, S.N // 2) for _ in range(batch)]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(cenc.encode(v, scale)) for v in vals]), True, scale)
    hoisted = S.ev.rotateVectorHoisted(a, steps, S.gk)
    errs = []
    for r, s in enumerate(steps):
        seq = S.ev.rotateVector(a, s, S.gk).cpu() if s else a.cpu()
        h = hoisted[r].cpu()
        assert hoisted[r].scale == a.scale and hoisted[r].is_ntt_form
        d_h = np.concatenate([np.abs(cenc.decode(S.dec.decrypt(h[b]), scale) - np.roll(vals[b], -s)) for b in range(batch)])
        d_s = np.concatenate([np.abs(cenc.decode(S.dec.decrypt(seq[b]), scale) - np.roll(vals[b], -s)) for b in range(batch)])
        e_h, e_s = d_h.max(), d_s.max()
        print(name, "step", s, "max slot error hoisted", e_h, "sequential", e_s, "medians", np.median(d_h), np.median(d_s))
        assert e_s < 0.1, "the sequential rotation itself is expected to be right"
        assert e_h <= 4 * e_s, (name, s, e_h, e_s)
        # the maxima are single-slot draws; the medians over batch x N/2 slots are the tight comparison of the two noise levels
        assert np.median(d_h) <= 1.5 * np.median(d_s), (name, s, np.median(d_h), np.median(d_s))
        errs.append((e_h, e_s))
    return errs


# ---------------------------------------------------------------- refusals and the Python layer
def raw_call(S, st_in, out_ptr, out_stride, elts, keys, n=None, batch=1, limit=0):
    so = capi.CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    R = len(elts)
    e = (C.c_uint32 * max(R, 1))(*elts)
    k = (C.c_void_p * max(R, 1))(*keys)
    rc = S.lib.troyhip_apply_galois_hoisted(S.ctx.h, C.byref(st_in), C.byref(so), e, k, R if n is None else n, C.c_uint64(limit), C.c_uint64(batch), None)
    return (rc, S.lib.troyhip_last_error().decode() if rc else "", so)


def check_refusals(S):
    inv = capi.INVALID_ARGUMENT
    limbs, N = S.ctx.first_limbs, S.N
    item = 2 * limbs * N
    g = S.ctx.galois_elt_from_step(1)
    S.key(g)
    kp = S.gk.keys[api.GaloisKeys.getIndex(g)].ptr
    a = S.ct(S.inputs(limbs, 1, 5))
    a3 = api.Ciphertext.from_numpy(S.ctx, synth.uniform_ct(6, S.primes[:limbs], 3, N, 1), S.ntt)
    out = api.DeviceBuffer(3 * item)
    st = a.struct()
    assert raw_call(S, st, out.ptr, item, [g], [None])[:2] == (inv, "Galois key not present")
    assert raw_call(S, st, out.ptr, item, [1, g], [None, None])[:2] == (inv, "Galois key not present")
    assert raw_call(S, st, out.ptr, item, [2], [kp])[:2] == (inv, "Galois element is not valid")
    assert raw_call(S, st, out.ptr, item, [2 * N + 1], [kp])[:2] == (inv, "Galois element is not valid")
    assert raw_call(S, a3.struct(), out.ptr, item, [g], [kp])[:2] == (inv, "encrypted size must be 2")
    wrong = a.struct()
    wrong.is_ntt_form = 0 if S.ntt else 1
    msg = {BFV: "BFV encrypted cannot be in NTT form", BGV: "BGV encrypted cannot be in NTT form", CKKS: "CKKS encrypted must be in NTT form"}[S.scheme]
    assert raw_call(S, wrong, out.ptr, item, [g], [kp])[:2] == (inv, msg)
    assert raw_call(S, st, out.ptr, item, [g], [kp], n=0)[0] == inv
    assert raw_call(S, st, out.ptr, item, [g], [kp], n=-1)[0] == inv
    assert raw_call(S, st, a.buf.ptr, item, [g], [kp])[0] == inv            # out aliases in
    assert raw_call(S, st, None, item, [g], [kp])[0] == inv
    assert raw_call(S, st, out.ptr, item - 1, [g], [kp])[0] == inv
    # element 1 alone needs no key and is a copy; the call fills in the descriptor
    rc, _, so = raw_call(S, st, out.ptr, item, [1], [None])
    assert rc == capi.OK and (so.size, so.limbs, bool(so.is_ntt_form), so.scale, so.correction_factor) == (2, limbs, S.ntt, a.scale, a.correction_factor)
    assert np.array_equal(out.to_numpy(item), a.cpu().reshape(-1))
    # the Python layer: the same messages as exceptions
    with_raises(capi.InvalidArgument, "Galois key not present", lambda: S.ev.applyGaloisHoisted(a, [1, g], api.GaloisKeys(S.ctx)))
    with_raises(capi.InvalidArgument, "at least one", lambda: S.ev.applyGaloisHoisted(a, [], S.gk))
    with_raises(capi.InvalidArgument, "encrypted size must be 2", lambda: S.ev.applyGaloisHoisted(a3, [g], S.gk))
    with_raises(capi.LogicError, "unsupported scheme", lambda: (S.ev.rotateRowsHoisted if S.ntt else S.ev.rotateVectorHoisted)(a, [1], S.gk))


def check_python_layer(S):
    """rotate*Hoisted map steps through galois_elt_from_step, step 0 is a copy, and the results equal applyGaloisHoisted's"""
    limbs = S.ctx.first_limbs
    data = S.inputs(limbs, 3, 21)
    steps = [1, 0, -1]
    elts = [S.ctx.galois_elt_from_step(s) if s else 1 for s in steps]
    ref = S.hoisted(data, elts)
    fn = S.ev.rotateVectorHoisted if S.ntt else S.ev.rotateRowsHoisted
    got = fn(S.ct(data), steps, S.gk)
    assert isinstance(got, list) and len(got) == 3
    for r in range(3):
        assert np.array_equal(got[r].cpu(), ref[r])
    assert np.array_equal(got[1].cpu(), data)
    first = got[0]
    del got  # a result outlives its siblings
    assert np.array_equal(first.cpu(), ref[0])
