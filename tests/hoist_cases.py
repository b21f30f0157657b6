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
    "ckks_n32768_chain": dict(scheme=CKKS, N=32768, bits=[60] + [40] * 13 + [60], tbits=0),
}
SMALL = ["bfv_n64_k3", "bgv_n128_k4", "ckks_n128_k6"]          # batch 5 (a blocked group of four and a remainder), R = 3
# batch 2, R = 5 with element 1: 60 rows per launch of the second half, far below the single-pass threshold (four rows per workgroup slot of the chip:
# 4096 rows at N = 4096 on 256 CUs) -- the merged two-pass mod-down (BFV, BGV) and the element-wise CKKS correction; the large-launch routes are
# check_large_route's
MEDIUM = ["cfgA_bfv_n4096_k3", "bgv_n4096_k3", "ckks_n4096_k4"]
NARROW = ["nar_bfv_n4096_k3"]                                    # primes below 2^33: the element-wise epilogue
KEY_SEED = 7100


def config(name):
    return BENCH[name] if name in BENCH else cases.CONFIGS[name]


def adhoc(scheme, N, bits, tbits=None):
    """(name, parameters) of a set no table names: Setup(*adhoc(...))"""
    tbits = 0 if scheme == CKKS else (tbits or (20 if N >= 4096 else 10))
    return "%s_n%d_%s" % ({BFV: "bfv", BGV: "bgv", CKKS: "ckks"}[scheme], N, "_".join(map(str, bits))), dict(scheme=scheme, N=N, bits=list(bits), tbits=tbits)


def obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


class Setup:
    """one parameter set; synthetic uniform keys (the arithmetic is oblivious to key validity), one per Galois element, seeded by the element"""

    def __init__(self, name, cfg=None, patterns=("uniform", "uniform", "uniform")):
        """patterns: synth.edge_rows patterns of (ciphertext, keys, plaintexts)"""
        cfg = self.cfg = cfg or config(name)
        self.name, self.scheme, self.N = name, cfg["scheme"], cfg["N"]
        self.ct_pattern, self.key_pattern, self.pt_pattern = patterns
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

    def all_levels(self):
        return list(range(self.ctx.first_limbs, self.ctx.last_limbs - 1, -1))

    def three_levels(self):
        """the first, one middle and the last level"""
        f, l = self.ctx.first_limbs, self.ctx.last_limbs
        return sorted({f, (f + l) // 2, l}, reverse=True)

    def key(self, elt, rows_only=None):
        """the key of element `elt`: on the device in self.gk, on the host [K-1][2][K][N]; the synthetic generator and its device twin agree, so a large
        key is filled on the device and only the rows the model reads (digits below `rows_only`) come back"""
        idx = api.GaloisKeys.getIndex(elt)
        K, N = self.K, self.N
        if elt not in self.host_keys:
            if rows_only is None:
                k = synth.edge_rows(self.key_pattern, KEY_SEED + elt, self.primes, (K - 1) * 2 * K, N).reshape(K - 1, 2, K, N)
                self.gk.set(idx, k)
            else:
                assert self.key_pattern == "uniform"
                buf = api.DeviceBuffer((K - 1) * 2 * K * N)
                self.ctx.fill_uniform(buf, (K - 1) * 2 * K, self.primes, KEY_SEED + elt)
                self.gk.set_device(idx, buf)
                k = np.zeros((K - 1, 2, K, N), dtype=np.uint64)
                k[:rows_only] = buf.to_numpy(rows_only * 2 * K * N).reshape(rows_only, 2, K, N)
            self.host_keys[elt] = k
        return self.host_keys[elt]

    def inputs(self, limbs, batch, seed):
        return synth.edge_ct(self.ct_pattern, seed, self.primes[:limbs], 2, self.N, batch, ntt_form=self.ntt)

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


def check_model(S, limbs, batch, R, seed, items=None, rows_only=None, elts=None, rots=None, limit=0):
    """every limb of every output item (or of `items`) of every rotation (or of the positions `rots`) equals the model"""
    data = S.inputs(limbs, batch, seed)
    elts = S.elts(R) if elts is None else list(elts)
    R = len(elts)
    got = S.hoisted(data, elts, limit=limit, rows_only=rows_only)
    assert got.shape == (R, batch, 2, limbs, S.N)
    for r, g in enumerate(elts):
        if rots is not None and r not in rots:
            continue
        for b in (range(batch) if items is None else items):
            exp = model_item(S, data[b], g, S.host_keys.get(g))
            assert np.array_equal(got[r, b], exp), (S.name, limbs, "rotation", r, "element", g, "item", b)
            assert all((got[r, b, :, j] < np.uint64(S.primes[j])).all() for j in range(limbs))
    return got, data, elts


def many_elts(S, R, one_at=None):
    """R distinct Galois elements other than 1: 3, 2N - 1, 2N - 3, N + 1, then a seeded spread over the odd numbers below 2N (all of them from R = N - 1 on);
    `one_at`: element 1 put at that position on top of them"""
    N = S.N
    rest = [int(g) for g in 2 * np.random.default_rng(N).permutation(np.arange(1, N)) + 1]
    e = list(dict.fromkeys([3, 2 * N - 1, 2 * N - 3, N + 1] + rest))[:R]
    assert len(e) == R and all(g & 1 and 1 < g < 2 * N for g in e)
    return e if one_at is None else e[:one_at] + [1] + e[one_at:]


# ---------------------------------------------------------------- the routes only large launches take
ROUTE_STATS = ("ntt1_int_launches", "ntt1_fp_launches", "ntt2_int_launches", "ntt2_fp_launches")


def route_stats():
    lib = api.KernelProvider.lib()
    return {n: capi.stat(n, lib) for n in ROUTE_STATS}


def delta(after, before):
    return {n: after[n] - before[n] for n in after}


_cus = []


def device_cus():
    """compute units of device 0 as the library counts them (ntt1.hip device_cus): both thresholds below scale with it.  torch is asked in a child
    process, once: it brings a HIP runtime of its own, which finds no device in a process where the library's runtime has opened it"""
    import subprocess
    import sys
    if not _cus:
        out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        _cus.append(int(out.stdout.split()[-1]))
    return _cus[0]


def single_pass_rows(N, cus):
    """ntt1_supported (ntt1.hip): four rows per workgroup slot of the chip -- one workgroup per CU at N >= 2^14, two at 2^13, four at 2^12"""
    logn = N.bit_length() - 1
    assert 12 <= logn <= 15
    return 4 * cus * {12: 4, 13: 2}.get(logn, 1)


def unmerged_rows(N, cus):
    """the smallest row count at which Context::small_launch (context.cpp: (rows * N >> 11) < 64 CUs) is false"""
    return -(-((64 * cus) << 11) // N)


def items_for(rows, rows_per_item, extra=1):
    """the smallest item count whose launch has `rows` rows, and `extra` more so that a ragged group occurs"""
    return -(-rows // rows_per_item) + extra


def check_large_route(S, limbs, batch, elts, seed, rows_only=None, limit=0, model_rots=None, alone=True):
    """ONE hoisted call of `batch` items: items 0, the middle one and the last of the first and the last rotation (or of the positions `model_rots`)
    against the model; with `alone`, EVERY item of every rotation bit-for-bit against the same call at batch 1 (the small-launch routes, which the model
    pins at the small shapes).  -> the path-counter deltas (the large call, one call at batch 1)"""
    data = S.inputs(limbs, batch, seed)
    R = len(elts)
    for g in elts:
        if g != 1:
            S.key(g, rows_only)
    s0 = route_stats()
    got = S.hoisted(data, elts, limit=limit, rows_only=rows_only)
    big = delta(route_stats(), s0)
    one = None
    for b in range(batch if alone else 1):
        s0 = route_stats()
        got1 = S.hoisted(data[b:b + 1], elts, rows_only=rows_only)[:, 0]
        one = one or delta(route_stats(), s0)
        assert np.array_equal(got1, got[:, b]), (S.name, "item", b, "differs from the same call at batch 1")
    for r in sorted({0, R - 1} if model_rots is None else model_rots):
        for b in sorted({0, batch // 2, batch - 1}):
            exp = model_item(S, data[b], elts[r], S.host_keys.get(elts[r]))
            assert np.array_equal(got[r, b], exp), (S.name, limbs, "rotation", r, "element", elts[r], "item", b)
    print(S.name, "batch", batch, "R", R, "counters of the large call", big, "of the call at batch 1", one)
    return big, one


def single_pass(d):
    return d["ntt1_int_launches"] + d["ntt1_fp_launches"]


def two_pass(d):
    return d["ntt2_int_launches"] + d["ntt2_fp_launches"]


# ---------------------------------------------------------------- prime classes, limb counts and levels
INT_SETS = [[60, 60, 60, 60, 60], [58, 58, 58, 58], [60, 58, 50, 49, 60]]  # the integer instances (guarded at 60 bits, guard-free at 58) with more than one digit
FP_WIDTHS = [34, 40, 41, 47, 48, 49, 50]                                    # the FP64 instances' range, edge to edge (50 bits: the first integer width)
MIXED_SETS = [[50, 30, 50, 30, 45, 60], [60, 22, 24, 60]]                   # wide and narrow primes in one modulus
LIMB_COUNTS = list(range(2, 19))                                            # K = 2: one digit; K above 15 leaves the fused shapes
EVERY_LEVEL = [(K, limbs) for K in (8, 18) for limbs in range(K - 2, 0, -1)]     # below the first level, which LIMB_COUNTS runs
SCHEMES = {"bfv": BFV, "bgv": BGV, "ckks": CKKS}


def int_setup(scheme, N, bits):
    return Setup(*adhoc(SCHEMES[scheme], N, bits, 40 if scheme == "bfv" and bits == INT_SETS[0] and N == 128 else None))


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


# ---------------------------------------------------------------- more than HOIST_MAX_ROT = 16 elements
def slab_plan(S, limbs, batch, R, limit=0):
    """(items, rotations) per slab as Evaluator::apply_galois_hoisted plans them (evaluator.cpp), restated"""
    N, dl, rl = S.N, limbs, limbs + 1
    limit = limit or 1 << 28
    slack = 32 * 8 + 128
    per_item, per_rot_item = N * (rl * dl + (dl if S.ntt else 0)), N * (2 * rl + 3 * dl + 4)
    if batch * (per_item + per_rot_item) + slack <= limit:
        return batch, min(R, 16, (limit - slack - batch * per_item) // (batch * per_rot_item))
    return (limit - slack) // (per_item + per_rot_item), 1


def expected_slabs(S, limbs, batch, elts, limit=0):
    """a slab is up to `rs` consecutive elements other than 1, of a run of `bs` items"""
    bs, rs = slab_plan(S, limbs, batch, len(elts), limit)
    runs, n = [], 0
    for g in list(elts) + [1]:
        if g == 1:
            runs += [n] if n else []
            n = 0
        else:
            n += 1
    return -(-batch // bs) * sum(-(-n // rs) for n in runs)


def check_many_elements(S, limbs, batch, R, seed):
    """R elements, element 1 in their middle: every output against the model under the default scratch limit (slabs of 16 rotations and a remainder), and
    bit-for-bit the same under a limit that allows 7 rotations per slab and one that allows a single one; the slab counter follows the slab arithmetic"""
    elts = many_elts(S, R - 1, one_at=(R - 1) // 2)
    s0 = slabs()
    ref, data, _ = check_model(S, limbs, batch, R, seed, elts=elts)
    want = expected_slabs(S, limbs, batch, elts)
    assert slabs() - s0 == want == -(-((R - 1) // 2) // 16) + -(-(R - 1 - (R - 1) // 2) // 16), (S.name, R, batch)
    for rs in (7, 1):
        limit = scratch_words(S, limbs, batch, rs)
        assert slab_plan(S, limbs, batch, R, limit) == (batch, rs)
        s0 = slabs()
        assert np.array_equal(S.hoisted(data, elts, limit=limit), ref), (S.name, R, batch, "rotations per slab", rs)
        assert slabs() - s0 == expected_slabs(S, limbs, batch, elts, limit) > want, (S.name, R, batch, rs)


def check_every_element(S, limbs, batch, count, seed):
    """`count` distinct elements other than 1 (all of them at count = N - 1) and element 1, a key per element: every output against the model --
    galois_ntt_index over the elements of a ring"""
    elts = many_elts(S, count, one_at=count // 2)
    check_model(S, limbs, batch, len(elts), seed, elts=elts, items=[0])
    return elts
