"""Shared checks of the external product with RGSW ciphertexts (troyhip_external_product_sum, troyhip_external_product_sum_scratch_words, troyhip_host_rgsw,
troyhip_create_rgsw).  Every step is exact arithmetic modulo p_i on canonical residues, so every comparison here is
np.array_equal: against the exact model in Python integers (extprod_model, anchor A2), against troyhip_switch_key through the C ABI (anchor A1), of the call
against itself under another order of the terms, batch size or scratch limit, and of decryptions under real keys against the product in R_t.
Used by tests/test_device_extprod.py (emulator build) and tests/test_gpu_extprod.py (MI355X)."""
import ctypes as C

import numpy as np

import extprod_model as XM
import hoist_cases as HC
from troy_amd import api, capi, synth
from troy_amd.capi import BFV, BGV, CKKS

SYMBOLS = ("troyhip_external_product_sum", "troyhip_external_product_sum_scratch_words", "troyhip_host_rgsw", "troyhip_create_rgsw")
COUNTERS = ("extprod_slabs", "extprod_chunks")
SETS = ["bfv_n64_k3", "bgv_n128_k4"]
NARROW = "nar_bfv_n4096_k3"                      # primes below 2^33: the element-wise epilogue
MEDIUM = ["cfgA_bfv_n4096_k3", "bgv_n4096_k3"]
TERMS = [1, 3, 16, 17]                           # 17 crosses the per-launch cap of 16 terms: the second launch accumulates
BATCHES = [1, 2, 5]                              # 1, 2: the small-batch instance; 5: a group of four and a ragged remainder, and a strided operand
RGSW_SEED = 8200


def stat(name):
    return capi.stat(name, api.KernelProvider.lib())


def check_symbols(lib, header_text):
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in capi.SYMBOLS and "int %s(" % sym in header_text, sym
    for name in COUNTERS:
        assert capi.stat(name, lib) >= 0


# ---------------------------------------------------------------- synthetic operands
def rgsw_of(S, seed):
    """a synthetic RGSW (the arithmetic is oblivious to its validity) in the setup's key pattern -> (host [2][K-1][2][K][N], RGSWCiphertext), made once"""
    cache = S.__dict__.setdefault("_rgsws", {})
    if seed not in cache:
        K, N = S.K, S.N
        g = synth.edge_rows(S.key_pattern, RGSW_SEED + seed, S.primes, 2 * (K - 1) * 2 * K, N).reshape(2, K - 1, 2, K, N)
        cache[seed] = (g, api.RGSWCiphertext.from_numpy(S.ctx, g))
    return cache[seed]


def run(S, datas, seeds, base=None, limit=0):
    """externalProductSum over the terms (datas[r] [batch][2][limbs][N], RGSW of seeds[r]) -> [batch][2][limbs][N]; the metadata is the operands'"""
    cts = [S.ct(d) for d in datas]
    out = S.ev.externalProductSum(cts, [rgsw_of(S, s)[1] for s in seeds], base=None if base is None else S.ct(base), scratch_limit_words=limit)
    a = cts[0]
    assert (out.size(), out.limbs, out.batch, out.is_ntt_form, out.scale, out.correction_factor) == (2, a.limbs, a.batch, False, a.scale, a.correction_factor)
    return out.cpu()


_refs = {}


def reference(S, limbs, batch, R, seed=9100):
    """the operands, the base and what the model makes of them with and without the base, computed once per shape and left unchanged ->
    (datas [R][batch][2][limbs][N], seeds, base [batch][2][limbs][N], expected without base, expected with base)"""
    key = (S.name, S.ct_pattern, S.key_pattern, limbs, batch, R, seed)
    if key not in _refs:
        datas = [S.inputs(limbs, batch, seed + 31 * r + batch) for r in range(R)]
        seeds = [r % 5 for r in range(R)]  # RGSWs repeat, as a selector does in a fold
        base = synth.uniform_ct(seed + 7, S.primes[:limbs], 2, S.N, batch)
        plain, based = [], []
        for b in range(batch):
            acc = XM.inner_products(S, [d[b] for d in datas], [rgsw_of(S, s)[0] for s in seeds])
            plain.append(XM.mod_down(S, acc))
            based.append(XM.mod_down(S, acc, base[b]))
        ref = (datas, seeds, base, np.stack(plain), np.stack(based))
        for a in ref[2:]:
            a.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def canonical(S, got):
    return all((got[:, :, j] < np.uint64(S.primes[j])).all() for j in range(got.shape[2]))


# ---------------------------------------------------------------- anchor A2: the model
def check_model(S, limbs, batch, R):
    """every limb equals the model and is canonical, with and without a base; ceil(R / 16) launches of the inner product, one slab"""
    datas, seeds, base, plain, based = reference(S, limbs, batch, R)
    for b, exp in ((None, plain), (base, based)):
        s0, c0 = stat("extprod_slabs"), stat("extprod_chunks")
        got = run(S, datas, seeds, base=b)
        assert (stat("extprod_slabs") - s0, stat("extprod_chunks") - c0) == (1, -(-R // 16)), (S.name, R, batch)
        assert np.array_equal(got, exp), (S.name, limbs, "terms", R, "batch", batch, "base" if b is not None else "no base")
        assert canonical(S, got)


# ---------------------------------------------------------------- anchor A1: troyhip_switch_key
def raw_switch_key(S, out_buf, limbs, target_ptr, target_stride, key_ptr, batch):
    """troyhip_switch_key through the C ABI onto the dense batch in out_buf"""
    st = capi.CtStruct(out_buf.ptr, 2 * limbs * S.N, 2, limbs, 0, 1.0, 1)
    rc = S.lib.troyhip_switch_key(S.ctx.h, C.byref(st), C.c_void_p(target_ptr), C.c_uint64(target_stride), C.c_void_p(key_ptr), C.c_uint64(batch), None)
    assert rc == capi.OK, S.lib.troyhip_last_error().decode()


def check_anchor(S, limbs, batch):
    """R = 1, no base, the operand (0, c1): the bytes of troyhip_switch_key onto a zeroed ciphertext with target c1 and key G[1]; (c0, 0) with G[0] likewise"""
    N, K = S.N, S.K
    pw = limbs * N
    g, G = rgsw_of(S, 2)
    half_words = (K - 1) * 2 * K * N
    for h in range(2):
        data = S.inputs(limbs, batch, 40 + h + batch)
        data[:, 1 - h] = 0
        got = run(S, [data], [2])
        a = S.ct(data)
        out = api.DeviceBuffer(batch * 2 * pw)
        out.zero()
        raw_switch_key(S, out, limbs, a.buf.ptr + 8 * h * pw, a.bstride, G.buf.ptr + 8 * h * half_words, batch)
        exp = out.to_numpy().reshape(batch, 2, limbs, N)
        assert np.array_equal(got, exp), (S.name, limbs, batch, "half", h)
        assert got.any()


# ---------------------------------------------------------------- independence
def scratch_words(S, limbs, items, terms):
    """what Evaluator::external_product_sum asks of the arena for a slab of `items` items and chunks of `terms` terms (evaluator.cpp), restated"""
    N, dl, rl = S.N, limbs, limbs + 1
    return items * N * (2 * rl + 2 * dl + 4) + terms * items * N * 2 * rl * dl + 32 * 8 + 128


def check_independence(S, limbs, batch=5, R=4):
    """the same bytes for permuted terms, for every item alone, and under the least limit the call accepts, where every (item, term) is a chunk of its own"""
    datas, seeds, base, _, based = reference(S, limbs, batch, R)
    perm = [2, 0, 3, 1]
    assert np.array_equal(run(S, [datas[i] for i in perm], [seeds[i] for i in perm], base=base), based), (S.name, "permuted terms")
    for b in range(batch):
        alone = run(S, [d[b:b + 1] for d in datas], seeds, base=base[b:b + 1])
        assert np.array_equal(alone[0], based[b]), (S.name, limbs, "item alone", b)
    one = S.ev.externalProductSumScratchWords(limbs, 1, 1)
    assert one == scratch_words(S, limbs, 1, 1)
    assert S.ev.externalProductSumScratchWords(limbs, R, batch) == scratch_words(S, limbs, batch, R)
    assert S.ev.externalProductSumScratchWords(limbs, 40, batch) == scratch_words(S, limbs, batch, 16)
    s0, c0 = stat("extprod_slabs"), stat("extprod_chunks")
    assert np.array_equal(run(S, datas, seeds, base=base, limit=one), based), (S.name, limbs, "one term of one item per chunk")
    assert (stat("extprod_slabs") - s0, stat("extprod_chunks") - c0) == (batch, batch * R)
    two = scratch_words(S, limbs, batch, 2)  # the whole batch, two terms per chunk
    s0, c0 = stat("extprod_slabs"), stat("extprod_chunks")
    assert np.array_equal(run(S, datas, seeds, base=base, limit=two), based), (S.name, limbs, "two terms per chunk")
    assert (stat("extprod_slabs") - s0, stat("extprod_chunks") - c0) == (1, -(-R // 2))
    HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small for one term of one ciphertext", lambda: run(S, datas, seeds, base=base, limit=one - 1))


# ---------------------------------------------------------------- the lazy sums at their bound
def check_lazy_bound(name="bgv_n128_k4", R=16, batch=2):
    """keys of p - 1 throughout with ciphertexts of p - 1 throughout and with the delta pattern: 2 R dl products of the largest operands per output, in
    runs of at most 63.  An accumulator that overflows cannot pass."""
    for ct_pattern in ("max", "delta"):
        S = HC.Setup(name, patterns=(ct_pattern, "max", "uniform"))
        limbs = S.ctx.first_limbs
        assert 2 * R * limbs > 63  # more than one run of the multiply-accumulate sums
        datas, seeds, base, plain, based = reference(S, limbs, batch, R)
        assert np.array_equal(run(S, datas, seeds), plain), (name, ct_pattern)
        assert np.array_equal(run(S, datas, seeds, base=base), based), (name, ct_pattern, "base")


# ---------------------------------------------------------------- RGSW generation
def real_context(scheme, N, bits, tbits):
    primes = api.CoeffModulus.Create(N, list(bits))
    t = int(api.PlainModulus.Batching(N, tbits))
    return api.SEALContext(scheme, N, primes, t), t


def plain_ntt(ctx, coeffs):
    """[K][N]: what troyhip_plain_to_ntt(limbs = K) writes for the coefficients mod t"""
    ev = api.Evaluator(ctx)
    p = api.DeviceBuffer.from_numpy(np.ascontiguousarray(coeffs, dtype=np.uint64))
    return ev.transformPlainToNtt(p, ctx.key_limbs, n_coeffs=len(coeffs)).to_numpy().reshape(ctx.key_limbs, ctx.N)


def check_rgsw_generation(scheme, N=256, bits=(40, 40, 40, 40), tbits=14):
    """the host form equals the two troyhip_host_kswitch_key calls on m and m (.) sk with the seeds lo and lo + 1; the device form equals the host form;
    the second RGSW of a generator uses the seeds lo + 2 and lo + 3, a batch of two the same four"""
    ctx, t = real_context(scheme, N, bits, tbits)
    K = ctx.key_limbs
    lo, hi = 77, 5
    rng = np.random.default_rng(11)
    ms = [np.array([0, 1, 0, t - 1, 1], dtype=np.uint64), rng.integers(0, 3, N).astype(np.uint64)]
    ms[1][ms[1] == 2] = t - 1
    kg = api.KeyGenerator(ctx, seed=(lo, hi))
    sk = kg.secretKey()
    primes = [int(p) for p in ctx.coeff_modulus]
    expect = []
    for i, m in enumerate(ms):
        mn = plain_ntt(ctx, m)
        msk = np.stack([np.array([int(a) * int(b) % primes[l] for a, b in zip(mn[l], sk[l])], dtype=np.uint64) for l in range(K)])
        halves = []
        for h, src in enumerate((mn, msk)):
            k = np.zeros((K - 1, 2, K, N), dtype=np.uint64)
            capi.check(ctx.lib, ctx.lib.troyhip_host_kswitch_key(ctx.h, C.c_uint64(lo + 2 * i + h), C.c_uint64(hi), api._u64p(sk), api._u64p(np.ascontiguousarray(src)),
                                                                 api._u64p(k)))
            halves.append(k)
        assert not np.array_equal(halves[0][:, 1], halves[1][:, 1])  # the two halves draw from two seeds
        expect.append(np.stack(halves))
    host = [kg.createRGSW(m) for m in ms]
    assert kg.kswitch_calls == 4
    for i in range(2):
        assert np.array_equal(host[i], expect[i]), ("host form", i)
    kg2 = api.KeyGenerator(ctx, seed=(lo, hi))
    dev = [kg2.createRGSW(m, device=True) for m in ms]
    assert kg2.kswitch_calls == 4 and all(isinstance(g, api.RGSWCiphertext) for g in dev)
    for i in range(2):
        assert np.array_equal(dev[i].cpu(), expect[i]), ("device form", i)
    kg3 = api.KeyGenerator(ctx, seed=(lo, hi))
    both = kg3.createRGSWBatch(ms)
    assert kg3.kswitch_calls == 4
    for i in range(2):
        assert np.array_equal(both[i].cpu(), expect[i]), ("device batch", i)
    # a plaintext handed over in NTT form at the key level is taken as it is
    kg4 = api.KeyGenerator(ctx, seed=(lo, hi))
    assert np.array_equal(kg4.createRGSW(plain_ntt(ctx, ms[0])), expect[0])


# ---------------------------------------------------------------- real keys
class Real:
    def __init__(self, scheme, N, bits, tbits):
        self.scheme, self.N = scheme, N
        self.ctx, self.t = real_context(scheme, N, bits, tbits)
        self.kg = kg = api.KeyGenerator(self.ctx, seed=(61, 62))
        self.enc = api.Encryptor(self.ctx, kg.createPublicKey(), seed=(12, 34))
        self.dec = api.Decryptor(self.ctx, kg.secretKey())
        self.ev = api.Evaluator(self.ctx)

    def encrypt(self, msgs):
        return api.Ciphertext.from_numpy(self.ctx, np.stack([self.enc.encrypt(m) for m in msgs]))

    def centred(self, m):
        m = np.asarray(m).astype(np.int64)
        return np.where(m > self.t // 2, m - self.t, m)


def composition_b(R, cts, rgsws):
    """what a caller could do before: 2 R troyhip_switch_key calls accumulating onto one ciphertext (existing code, not the code under test)"""
    ctx, N, K = R.ctx, R.N, R.ctx.key_limbs
    a0 = cts[0]
    limbs, batch = a0.limbs, a0.batch
    pw = limbs * N
    out = api.DeviceBuffer(batch * 2 * pw)
    out.zero()
    st = capi.CtStruct(out.ptr, 2 * pw, 2, limbs, 0, a0.scale, a0.correction_factor)
    for a, g in zip(cts, rgsws):
        for h in range(2):
            rc = ctx.lib.troyhip_switch_key(ctx.h, C.byref(st), C.c_void_p(a.buf.ptr + 8 * h * pw), C.c_uint64(a.bstride),
                                            C.c_void_p(g.buf.ptr + 8 * h * (K - 1) * 2 * K * N), C.c_uint64(batch), None)
            assert rc == capi.OK, ctx.lib.troyhip_last_error().decode()
    return out.to_numpy().reshape(batch, 2, limbs, N)


def check_real(scheme, N, bits, tbits, batch=2, fold=8):
    """fresh encryptions under generated keys, RGSWs from the device generator, everything decrypted exactly: m mu for m in {0, 1, x^5, a ternary
    polynomial}; cmux for both values of the bit; the fold sum_r RGSW(delta_{r, r*}) (.) ct_r; positive noise budgets, printed beside composition (b)'s"""
    R = Real(scheme, N, bits, tbits)
    t = R.t
    rng = np.random.default_rng(17)
    msgs = rng.integers(0, t, (fold, batch, N), dtype=np.uint64)
    cts = [R.encrypt(msgs[r]) for r in range(fold)]
    cf = cts[0].correction_factor
    x5 = np.zeros(6, dtype=np.uint64)
    x5[5] = 1
    tern = rng.integers(0, 3, N).astype(np.uint64)
    tern[tern == 2] = t - 1
    plains = {"0": np.zeros(1, dtype=np.uint64), "1": np.ones(1, dtype=np.uint64), "x^5": x5, "ternary": tern}
    G = dict(zip(plains, R.kg.createRGSWBatch(list(plains.values()))))

    def decrypts_to(got, exp, what):
        for b in range(batch):
            assert np.array_equal(R.dec.decrypt(got[b], correction_factor=cf), exp[b]), (scheme, N, what, "item", b)
            budget = R.dec.invariantNoiseBudget(got[b])
            assert budget > 0, (scheme, N, what, budget)
        return budget

    for name, m in plains.items():
        full = np.zeros(N, dtype=np.int64)
        full[:len(m)] = R.centred(m)
        exp = [XM.negacyclic_product(full, msgs[0, b], t) for b in range(batch)]
        got = R.ev.externalProduct(cts[0], G[name]).cpu()
        budget = decrypts_to(got, exp, "m = " + name)
        ref = composition_b(R, [cts[0]], [G[name]])
        for b in range(batch):
            assert np.array_equal(R.dec.decrypt(ref[b], correction_factor=cf), exp[b])
        print("scheme", scheme, "N", N, "m =", name, "noise budget", budget, "composition (b)", R.dec.invariantNoiseBudget(ref[batch - 1]),
              "fresh", R.dec.invariantNoiseBudget(cts[0].cpu()[batch - 1]))
    for bit in (0, 1):
        got = R.ev.cmux(G[str(bit)], cts[1], cts[2]).cpu()
        decrypts_to(got, msgs[2 if bit else 1], "cmux %d" % bit)
    for star in (0, fold - 1, 3):
        sel = [G["1" if r == star else "0"] for r in range(fold)]
        got = R.ev.externalProductSum(cts, sel).cpu()
        budget = decrypts_to(got, msgs[star], "fold onto %d" % star)
        ref = composition_b(R, cts, sel)
        print("scheme", scheme, "N", N, "fold of", fold, "noise budget", budget, "composition (b)", R.dec.invariantNoiseBudget(ref[batch - 1]))
    # a base: base + m mu
    got = R.ev.externalProductSum([cts[0]], [G["1"]], base=cts[3]).cpu()
    decrypts_to(got, (msgs[0] + msgs[3]) % np.uint64(t), "base")


# ---------------------------------------------------------------- the routes only large launches take, and the grid limit
def check_large_route(S, limbs, batch, R=2):
    """ONE call of `batch` items: three items against the model, EVERY item against the same call at batch 1 -> the path-counter deltas of the large call"""
    datas = [S.inputs(limbs, batch, 700 + r) for r in range(R)]
    seeds = list(range(R))
    base = synth.uniform_ct(707, S.primes[:limbs], 2, S.N, batch)
    s0 = HC.route_stats()
    got = run(S, datas, seeds, base=base)
    big = HC.delta(HC.route_stats(), s0)
    for b in range(batch):
        alone = run(S, [d[b:b + 1] for d in datas], seeds, base=base[b:b + 1])
        assert np.array_equal(alone[0], got[b]), (S.name, "item", b, "differs from the same call at batch 1")
    for b in sorted({0, batch // 2, batch - 1}):
        exp = XM.model_item(S, [d[b] for d in datas], [rgsw_of(S, s)[0] for s in seeds], base[b])
        assert np.array_equal(got[b], exp), (S.name, limbs, "item", b)
    print(S.name, "batch", batch, "counters of the large call", big)
    return big


def check_grid_limit(S, batch=65537):
    """more items than any grid dimension but x holds: the items at both ends and around 65535 equal the call on those items alone"""
    limbs = S.ctx.first_limbs
    rng = np.random.default_rng(65537)
    data = np.stack([rng.integers(0, S.primes[j], (batch, 2, S.N), dtype=np.uint64) for j in range(limbs)], axis=2)
    G = rgsw_of(S, 0)[1]
    big = S.ev.externalProduct(api.Ciphertext.from_numpy(S.ctx, data), G).cpu()
    pick = [0, 1, 65535, 65536]
    alone = S.ev.externalProduct(api.Ciphertext.from_numpy(S.ctx, data[pick]), G).cpu()
    for i, b in enumerate(pick):
        assert np.array_equal(big[b], alone[i]), ("item", b)
    exp = XM.model_item(S, [data[65536]], [rgsw_of(S, 0)[0]])
    assert np.array_equal(big[65536], exp)


# ---------------------------------------------------------------- refusals and the Python layer
def raw_call(S, sts, rgsws, out_ptr, out_stride, base=None, n=None, batch=1, limit=0, ctx=None):
    """sts: CtStruct per term (None: a null descriptor); rgsws: device pointers (None: null)"""
    so = capi.CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    R = len(sts)
    pa = (C.POINTER(capi.CtStruct) * max(R, 1))(*[C.pointer(st) if st is not None else None for st in sts])
    pg = (C.c_void_p * max(R, 1))(*rgsws)
    rc = S.lib.troyhip_external_product_sum((ctx or S.ctx).h, pa, pg, R if n is None else n, C.byref(base) if base is not None else None, C.byref(so), C.c_uint64(limit),
                                            C.c_uint64(batch), None)
    return rc, S.lib.troyhip_last_error().decode() if rc else "", so


def check_refusals(S):
    inv, logic = capi.INVALID_ARGUMENT, capi.LOGIC_ERROR
    limbs, N = S.ctx.first_limbs, S.N
    pw = limbs * N
    a = S.ct(S.inputs(limbs, 1, 5))
    st = a.struct()
    out = api.DeviceBuffer(2 * pw)
    out.zero()
    K = S.K
    if S.scheme == CKKS:
        g = api.DeviceBuffer(2 * (K - 1) * 2 * K * N)
        rc, msg, _ = raw_call(S, [st], [g.ptr], out.ptr, 2 * pw)
        assert rc == logic and msg.startswith("unsupported scheme"), (rc, msg)
        HC.with_raises(capi.LogicError, "unsupported scheme", lambda: S.ev.externalProductSum([a], [api.RGSWCiphertext(S.ctx, g)]))
        return
    g = rgsw_of(S, 0)[1].buf.ptr

    def refused(rc_msg, code, text=None):
        rc, msg = rc_msg[:2]
        assert rc == code and (text is None or msg.startswith(text)), (rc, msg)
        assert not out.to_numpy(2 * pw).any()  # the destination is untouched

    ntt = a.struct()
    ntt.is_ntt_form = 1
    refused(raw_call(S, [ntt], [g], out.ptr, 2 * pw), inv, "%s encrypted cannot be in NTT form" % ("BFV" if S.scheme == BFV else "BGV"))
    a3 = api.Ciphertext.from_numpy(S.ctx, synth.uniform_ct(6, S.primes[:limbs], 3, N, 1), False)
    refused(raw_call(S, [a3.struct()], [g], out.ptr, 3 * pw), inv, "encrypted size must be 2")
    one = a.struct()
    one.size = 1
    refused(raw_call(S, [one], [g], out.ptr, 2 * pw), inv, "encrypted size must be 2")
    refused(raw_call(S, [st, a3.struct()], [g, g], out.ptr, 2 * pw), inv, "encrypted size must be 2")
    refused(raw_call(S, [st], [g], out.ptr, 2 * pw, n=0), inv, "external_product_sum takes 1 to 64 terms")
    refused(raw_call(S, [st] * 65, [g] * 65, out.ptr, 2 * pw), inv, "external_product_sum takes 1 to 64 terms")
    refused(raw_call(S, [st], [g], out.ptr, 2 * pw, n=-1), inv, "external_product_sum takes 1 to 64 terms")
    refused(raw_call(S, [None], [g], out.ptr, 2 * pw), inv, "null ciphertext")
    refused(raw_call(S, [st, None], [g, g], out.ptr, 2 * pw), inv, "null ciphertext")
    refused(raw_call(S, [st], [None], out.ptr, 2 * pw), inv, "external_product_sum: null RGSW ciphertext")
    refused(raw_call(S, [st, st], [g, None], out.ptr, 2 * pw), inv, "external_product_sum: null RGSW ciphertext")
    nul = a.struct()
    nul.data = None
    refused(raw_call(S, [nul], [g], out.ptr, 2 * pw), inv)
    refused(raw_call(S, [st], [g], out.ptr, 2 * pw, base=nul), inv)
    refused(raw_call(S, [st], [g], None, 2 * pw), inv)
    rc = S.lib.troyhip_external_product_sum(S.ctx.h, None, None, 1, None, C.byref(capi.CtStruct(out.ptr, 2 * pw, 0, 0, 0, 0.0, 0)), C.c_uint64(0), C.c_uint64(1), None)
    refused((rc, ""), inv)
    pa = (C.POINTER(capi.CtStruct) * 1)(C.pointer(st))
    rc = S.lib.troyhip_external_product_sum(S.ctx.h, pa, (C.c_void_p * 1)(g), 1, None, None, C.c_uint64(0), C.c_uint64(1), None)
    refused((rc, ""), inv)
    # operands or a base at another level or, BGV, with another correction factor
    if limbs > S.ctx.last_limbs:
        lower = S.ct(S.inputs(limbs - 1, 1, 6)).struct()
        refused(raw_call(S, [st, lower], [g, g], out.ptr, 2 * pw), inv, "encrypted1 and encrypted2 parameter mismatch")
        refused(raw_call(S, [st], [g], out.ptr, 2 * pw, base=lower), inv, "encrypted1 and encrypted2 parameter mismatch")
    scaled = a.struct()
    scaled.scale = 2.0
    refused(raw_call(S, [st, scaled], [g, g], out.ptr, 2 * pw), inv, "scale mismatch")
    refused(raw_call(S, [st], [g], out.ptr, 2 * pw, base=scaled), inv, "scale mismatch")
    if S.scheme == BGV:
        other = a.struct()
        other.correction_factor = 2
        refused(raw_call(S, [st, other], [g, g], out.ptr, 2 * pw), inv, "correction factor mismatch")
        refused(raw_call(S, [st], [g], out.ptr, 2 * pw, base=other), inv, "correction factor mismatch")
    # the destination
    refused(raw_call(S, [st], [g], out.ptr, 2 * pw - 1), inv, "destination batch stride too small for the result size")
    b = S.ct(S.inputs(limbs, 1, 7))
    for alias in (a, b):  # the destination begins inside an operand, inside the base
        rc, msg, _ = raw_call(S, [st], [g], alias.buf.ptr + 8 * pw, 2 * pw, base=b.struct())
        assert rc == inv and "destination must be a distinct buffer" in msg, (rc, msg)
    refused((inv, ""), inv)
    w = S.ev.externalProductSumScratchWords(limbs, 1, 1)
    refused(raw_call(S, [st], [g], out.ptr, 2 * pw, limit=w - 1), inv, "scratch_limit_words is too small for one term of one ciphertext")
    # a host-only context, and one that cannot switch keys
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    rc, msg, _ = raw_call(S, [st], [g], out.ptr, 2 * pw, ctx=host)
    assert rc == logic and "host-only" in msg
    refused((rc, ""), logic)
    S1 = HC.Setup(*HC.adhoc(S.scheme, N, [40]))  # K = 1
    st1 = S1.ct(S1.inputs(1, 1, 5)).struct()
    rc, msg, _ = raw_call(S1, [st1], [g], out.ptr, 2 * N)
    assert rc == logic and msg == "keyswitching is not supported by the context", (rc, msg)
    refused((rc, ""), logic)
    # the scratch query
    v = C.c_uint64(0)
    q = S.lib.troyhip_external_product_sum_scratch_words
    assert q(S.ctx.h, limbs, 0, C.c_uint64(1), C.byref(v)) == inv
    assert q(S.ctx.h, limbs, 65, C.c_uint64(1), C.byref(v)) == inv
    assert q(S.ctx.h, 0, 1, C.c_uint64(1), C.byref(v)) == inv
    assert q(S.ctx.h, limbs, 1, C.c_uint64(1), None) == inv
    assert q(S.ctx.h, limbs, 1, C.c_uint64(1), C.byref(v)) == capi.OK and v.value == w == scratch_words(S, limbs, 1, 1)
    # a good call fills in the descriptor; an empty batch does nothing
    rc, _, so = raw_call(S, [st], [g], out.ptr, 2 * pw, batch=0)
    assert rc == capi.OK and not out.to_numpy(2 * pw).any()
    rc, _, so = raw_call(S, [st], [g], out.ptr, 2 * pw)
    assert rc == capi.OK and (so.size, so.limbs, so.is_ntt_form, so.scale, so.correction_factor) == (2, limbs, 0, a.scale, a.correction_factor)
    assert out.to_numpy(2 * pw).any()
    # the Python layer
    G = rgsw_of(S, 0)[1]
    HC.with_raises(capi.InvalidArgument, "external_product_sum takes 1 to 64 terms", lambda: S.ev.externalProductSum([], []))
    HC.with_raises(capi.InvalidArgument, "external_product_sum takes 1 to 64 terms", lambda: S.ev.externalProductSum([a, a], [G]))
    HC.with_raises(capi.InvalidArgument, "rgsw is not valid for encryption parameters", lambda: S.ev.externalProductSum([a], [rgsw_of(S, 0)[0]]))
    HC.with_raises(capi.InvalidArgument, "rgsw is not valid for encryption parameters", lambda: S.ev.externalProductSum([a], [rgsw_of(S1, 0) if S1.K > 1 else S1.gk]))
    HC.with_raises(capi.InvalidArgument, "rgsw is not valid for encryption parameters", lambda: api.RGSWCiphertext(S.ctx, api.DeviceBuffer(8)))
    HC.with_raises(capi.InvalidArgument, "encrypted size must be 2", lambda: S.ev.externalProduct(a3, G))
    HC.with_raises(capi.InvalidArgument, "one number of items", lambda: S.ev.externalProductSum([a, S.ct(S.inputs(limbs, 2, 5))], [G, G]))
