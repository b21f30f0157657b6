"""Shared checks of blind rotation (troyhip_blind_rotate, troyhip_blind_rotate_scratch_words, troyhip_lwe_mod_switch).  Every step
is exact arithmetic modulo p_i on canonical residues, so every comparison here is np.array_equal: against the exact model in Python integers built on
extprod_model, against the composition of negacyclicShift, sub and externalProductSum through the Python layer on every item alone (the byte anchor), of
the call against itself at another batch size or scratch limit, and of decryptions under real keys against tv x^phi in R_t.
Used by tests/test_device_blindrot.py (emulator build) and tests/test_gpu_blindrot.py (MI355X)."""
import ctypes as C

import numpy as np

import extprod_cases as XC
import extprod_model as XM
import hoist_cases as HC
from troy_amd import api, app, capi
from troy_amd.capi import BFV, BGV, CKKS

SYMBOLS = ("troyhip_blind_rotate", "troyhip_blind_rotate_scratch_words", "troyhip_lwe_mod_switch")
COUNTERS = ("blindrot_slabs", "blindrot_steps")
SETS = XC.SETS                                   # bfv_n64_k3, bgv_n128_k4
NARROW = XC.NARROW                               # primes below 2^33: the element-wise mod-down
MEDIUM = XC.MEDIUM
DIGITS = [1, 2]                                  # T: binary, ternary
DIMS = [1, 5]                                    # n
BATCHES = [1, 2, 5]                              # 5: a group of four items of the inner product and a ragged remainder
HIGH = (1 << 63) | (1 << 40)                     # bits above 2N: the kernels mask them


def stat(name):
    return capi.stat(name, api.KernelProvider.lib())


def check_symbols(lib, header_text):
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in capi.SYMBOLS and "int %s(" % sym in header_text, sym
    for name in COUNTERS:
        assert capi.stat(name, lib) >= 0


# ---------------------------------------------------------------- samples, keys, test vectors
def boundary_words(N):
    """0, 1, N - 1, N, N + 1, 2N - 1 and a word with bits above 2N set (N + 3 under the mask)"""
    return [0, 1, N - 1, N, N + 1, 2 * N - 1, HIGH | (N + 3)]


def samples(N, n, batch, seed=0):
    """[batch][n + 1] words: the shifts of the items of a batch DIFFER at every step, and shifts and beta run over the boundary words; item b does not
    depend on the batch size"""
    B = boundary_words(N)
    lwe = np.zeros((batch, n + 1), dtype=np.uint64)
    for b in range(batch):
        for i in range(n):
            lwe[b, i] = B[(3 * b + 5 * i + seed) % len(B)]
        lwe[b, n] = B[(b + 2 * seed + n) % len(B)]
    return lwe


def key_of(S, n, T):
    """a synthetic bootstrapping key [n][T] of the RGSWs extprod_cases.rgsw_of makes (the arithmetic is oblivious to their validity) -> (host, BlindRotationKey)"""
    cache = S.__dict__.setdefault("_brks", {})
    if (n, T) not in cache:
        g = np.stack([np.stack([XC.rgsw_of(S, (i * T + t) % 7)[0] for t in range(T)]) for i in range(n)])
        cache[(n, T)] = (g, api.BlindRotationKey.from_numpy(S.ctx, g))
    return cache[(n, T)]


def test_vectors(S, limbs, batch, seed=9300):
    """[batch][limbs][N] canonical residues, every row ending at p - 1 and starting at 0 (the negation of 0 stays 0)"""
    rng = np.random.default_rng(seed + limbs)
    tv = np.stack([rng.integers(0, S.primes[j], (batch, S.N), dtype=np.uint64) for j in range(limbs)], axis=1)
    for j in range(limbs):
        tv[:, j, 0] = 0
        tv[:, j, -1] = S.primes[j] - 1
    return tv


def shift_model(S, poly, u):
    """x^u poly for [..][limbs][N] canonical residues, u below 2N, in Python integers"""
    N = S.N
    limbs = poly.shape[-2]
    out = np.zeros_like(poly)
    m = [(n - u) % (2 * N) for n in range(N)]
    idx = [x % N for x in m]
    neg = np.array([x >= N for x in m])
    for j in range(limbs):
        p = S.primes[j]
        v = poly[..., j, idx].astype(object)
        out[..., j, :] = np.where(neg, (p - v) % p, v).astype(np.uint64)
    return out


def sub_model(S, a, b):
    out = np.zeros_like(a)
    for j in range(a.shape[-2]):
        out[..., j, :] = ((a[..., j, :].astype(object) - b[..., j, :].astype(object)) % S.primes[j]).astype(np.uint64)
    return out


_items = {}


def model_item(S, limbs, row, G, tv):
    """section 4.22 for one item in Python integers: row = (a_0 .. a_(n-1), beta), G host [n][T][2][K-1][2][K][N], tv [limbs][N] -> [2][limbs][N]; cached"""
    key = (S.name, S.ct_pattern, S.key_pattern, limbs, tuple(int(x) for x in row), G.shape[:2], G[:, :, 0, 0, 0, 0, :2].tobytes(), tv.tobytes())
    if key not in _items:
        N, n, T = S.N, G.shape[0], G.shape[1]
        acc = np.zeros((2, limbs, N), dtype=np.uint64)
        acc[0] = shift_model(S, tv, int(row[n]) % (2 * N))
        for i in range(n):
            a = int(row[i]) % (2 * N)
            us = [a, (2 * N - a) % (2 * N)][:T]
            ops = [sub_model(S, shift_model(S, acc, u), acc) for u in us]
            acc = XM.model_item(S, ops, [G[i, t] for t in range(T)], acc)
        acc.setflags(write=False)
        _items[key] = acc
    return _items[key]


def canonical(S, got):
    return all((got[:, :, j] < np.uint64(S.primes[j])).all() for j in range(got.shape[2]))


def run(S, lwe, BK, tv, limbs, limit=0, device_inputs=False):
    """blindRotate -> [batch][2][limbs][N]; the metadata is section 4.22's"""
    if device_inputs:
        lwe, tv = api.DeviceBuffer.from_numpy(lwe), api.DeviceBuffer.from_numpy(np.ascontiguousarray(tv))
    out = S.ev.blindRotate(lwe, BK, tv, limbs=limbs, scratch_limit_words=limit)
    assert (out.size(), out.limbs, out.is_ntt_form, out.scale, out.correction_factor) == (2, limbs, False, 1.0, 1)
    return out.cpu()


# ---------------------------------------------------------------- the model
def check_model(S, limbs, n, T, batch, per_item, seed=0):
    """every limb of every item equals the model and is canonical; one slab, n steps"""
    lwe = samples(S.N, n, batch, seed)
    G, BK = key_of(S, n, T)
    tvs = test_vectors(S, limbs, batch)
    tv = tvs if per_item else tvs[0]
    s0, c0 = stat("blindrot_slabs"), stat("blindrot_steps")
    got = run(S, lwe, BK, tv, limbs, device_inputs=bool(seed & 1))
    assert (stat("blindrot_slabs") - s0, stat("blindrot_steps") - c0) == (1, n), (S.name, n, batch)
    assert got.shape == (batch, 2, limbs, S.N)
    assert canonical(S, got)
    for b in range(batch):
        exp = model_item(S, limbs, lwe[b], G, tvs[b] if per_item else tvs[0])
        assert np.array_equal(got[b], exp), (S.name, "limbs", limbs, "n", n, "T", T, "batch", batch, "item", b, "per-item tv", per_item)
    if batch > 1:  # the shifts of the items differ at every step
        assert all(len({int(x) % (2 * S.N) for x in lwe[:, i]}) == batch for i in range(n))


def check_boundaries_covered(N=64):
    """across the cases of check_model the shifts and beta each run over every boundary word"""
    B = set(boundary_words(N))
    seen_a, seen_b = set(), set()
    for n in DIMS:
        for batch in BATCHES:
            for seed in (0, 1):
                lwe = samples(N, n, batch, seed)
                seen_a |= {int(x) for x in lwe[:, :n].reshape(-1)}
                seen_b |= {int(x) for x in lwe[:, n]}
    assert seen_a == B and seen_b == B


# ---------------------------------------------------------------- the byte anchor: the composition through existing public calls, item by item
def composition_item(ev, ctx, row, n, T, rgsws, tv, limbs):
    """the trivial ciphertext, then per step negacyclicShift, sub and externalProductSum(base=acc) -> Ciphertext of one item.  rgsws[i][t]: RGSWCiphertext"""
    N = ctx.N
    data = np.zeros((1, 2, limbs, N), dtype=np.uint64)
    data[0, 0] = tv
    acc = api.Ciphertext.from_numpy(ctx, data)
    acc = ev.negacyclicShift(acc, int(row[n]) % (2 * N))
    for i in range(n):
        a = int(row[i]) % (2 * N)
        us = [a, (2 * N - a) % (2 * N)][:T]
        ops = [ev.sub(ev.negacyclicShift(acc, u), acc) for u in us]
        acc = ev.externalProductSum(ops, [rgsws[i][t] for t in range(T)], base=acc)
    return acc


def rgsws_of(ctx, G):
    return [[api.RGSWCiphertext.from_numpy(ctx, G[i, t]) for t in range(G.shape[1])] for i in range(G.shape[0])]


def check_composition(S, limbs, n, T, batch, per_item=True, seed=1):
    lwe = samples(S.N, n, batch, seed)
    G, BK = key_of(S, n, T)
    tvs = test_vectors(S, limbs, batch)
    got = run(S, lwe, BK, tvs if per_item else tvs[0], limbs)
    R = rgsws_of(S.ctx, G)
    for b in range(batch):
        exp = composition_item(S.ev, S.ctx, lwe[b], n, T, R, tvs[b] if per_item else tvs[0], limbs).cpu()[0]
        assert np.array_equal(got[b], exp), (S.name, "limbs", limbs, "n", n, "T", T, "item", b)
    assert got.any() and canonical(S, got)


# ---------------------------------------------------------------- independence
def scratch_words(S, limbs, T, items):
    """what Evaluator::blind_rotate asks of the arena for a slab of `items` items (evaluator.cpp), restated: two accumulators, T operand pairs, and the
    external product's accumulator, second half and 2 T digit sets"""
    N, dl, rl = S.N, limbs, limbs + 1
    return items * N * ((4 + 2 * T) * dl + 2 * rl + 2 * dl + 4 + T * 2 * rl * dl) + 32 * 11 + 128


def check_independence(S, limbs, n=3, T=2):
    """the same bytes at batch 1, 2 and 5 and under the least limit the call accepts, where every item is a slab of its own"""
    G, BK = key_of(S, n, T)
    lwe = samples(S.N, n, 5, 1)
    tvs = test_vectors(S, limbs, 5)
    full = run(S, lwe, BK, tvs, limbs)
    for batch in (1, 2):
        assert np.array_equal(run(S, lwe[:batch], BK, tvs[:batch], limbs), full[:batch]), (S.name, limbs, "batch", batch)
    for b in range(5):
        assert np.array_equal(run(S, lwe[b:b + 1], BK, tvs[b], limbs)[0], full[b]), (S.name, limbs, "item alone", b)
    one = S.ev.blindRotateScratchWords(limbs, T, 1)
    assert one == scratch_words(S, limbs, T, 1)
    assert S.ev.blindRotateScratchWords(limbs, T, 5) == scratch_words(S, limbs, T, 5)
    s0, c0 = stat("blindrot_slabs"), stat("blindrot_steps")
    assert np.array_equal(run(S, lwe, BK, tvs, limbs, limit=one), full), (S.name, limbs, "one item per slab")
    assert (stat("blindrot_slabs") - s0, stat("blindrot_steps") - c0) == (5, 5 * n)
    two = scratch_words(S, limbs, T, 2)
    s0, c0 = stat("blindrot_slabs"), stat("blindrot_steps")
    assert np.array_equal(run(S, lwe, BK, tvs, limbs, limit=two), full), (S.name, limbs, "two items per slab")
    assert (stat("blindrot_slabs") - s0, stat("blindrot_steps") - c0) == (3, 3 * n)
    HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small for one ciphertext", lambda: run(S, lwe, BK, tvs, limbs, limit=one - 1))


# ---------------------------------------------------------------- real keys
def scaled_test_vector(ctx, scheme, t, f, limbs):
    """[limbs][N]: round(q f / t) modulo every prime for BFV (q the product of the level's primes), the plain lift of f for BGV"""
    primes = [int(p) for p in ctx.coeff_modulus[:limbs]]
    q = 1
    for p in primes:
        q *= p
    vals = [(q * int(v) + t // 2) // t if scheme == BFV else int(v) for v in f]
    return np.array([[v % p for v in vals] for p in primes], dtype=np.uint64)


def rotated(f, phi, t):
    """f x^phi in R_t, phi below 2N"""
    N = len(f)
    mono = np.zeros(N, dtype=np.int64)
    mono[phi % N] = -1 if phi >= N else 1
    return XM.negacyclic_product(mono, f, t)


def check_real(scheme, N=256, bits=(40, 40, 40, 40), tbits=14):
    """a binary and a ternary LWE secret of n = 6; samples built in integers mod 2N for chosen phases; every item decrypts EXACTLY to f x^phi.
    -> {(digits, limbs): least invariant noise budget}, printed"""
    R = XC.Real(scheme, N, bits, tbits)
    t, ctx = R.t, R.ctx
    rng = np.random.default_rng(23)
    f = rng.integers(0, t, N, dtype=np.uint64)
    phases = [0, N - 1, N, 2 * N - 1, 1, N + 77]
    budgets = {}
    for secret in ([1, 0, 1, 1, 0, 1], [1, -1, 0, 1, -1, -1]):
        n = len(secret)
        calls = R.kg.kswitch_calls
        BK = R.kg.createBlindRotationKey(secret)
        T = 2 if min(secret) < 0 else 1
        assert (BK.n, BK.T) == (n, T) and R.kg.kswitch_calls - calls == 2 * n * T
        lwe = rng.integers(0, 2 * N, (len(phases), n + 1), dtype=np.uint64)
        lwe[0, 0], lwe[1, 1], lwe[2, 2] = 0, N, 2 * N - 1
        for b, phi in enumerate(phases):
            lwe[b, n] = (phi - sum(int(a) * s for a, s in zip(lwe[b, :n], secret))) % (2 * N)
        lwe[3] |= np.uint64(HIGH)  # the bits above 2N do not count
        for limbs in sorted({ctx.first_limbs, ctx.last_limbs}, reverse=True):
            tv = scaled_test_vector(ctx, scheme, t, f, limbs)
            got = R.ev.blindRotate(lwe, BK, tv).cpu()
            least = None
            for b, phi in enumerate(phases):
                assert np.array_equal(R.dec.decrypt(got[b], correction_factor=1), rotated(f, phi, t)), (scheme, "T", T, "limbs", limbs, "phase", phi)
                budget = R.dec.invariantNoiseBudget(got[b])
                assert budget > 0, (scheme, T, limbs, budget)
                least = budget if least is None else min(least, budget)
            budgets[(T, limbs)] = least
            print("scheme", scheme, "N", N, "n", n, "T", T, "limbs", limbs, "least invariant noise budget", least)
    return budgets


def check_pipeline(N=256, bits=(40, 40, 40, 40), tbits=14, batch=3, terms=(0, 5)):
    """fresh BFV encryptions brought to one limb, two terms extracted, lweModSwitch, blindRotate under createBlindRotationKey() (n = N, ternary).  The test
    computes the switched phase of every sample in integers from the secret key and asserts decryption to tv x^phi: an exact condition"""
    R = XC.Real(BFV, N, bits, tbits)
    t, ctx = R.t, R.ctx
    s = R.kg.secretCoefficients()
    assert s.shape == (N,) and (s < 0).any() and (s > 0).any()
    calls = R.kg.kswitch_calls
    BK = R.kg.createBlindRotationKey()
    assert (BK.n, BK.T) == (N, 2) and R.kg.kswitch_calls - calls == 4 * N
    rng = np.random.default_rng(29)
    cts = R.encrypt(rng.integers(0, t, (batch, N), dtype=np.uint64))
    low = R.ev.modSwitchTo(cts, 1)
    lwes = R.ev.extractLWEs(low, terms)
    sw = R.ev.lweModSwitch(lwes)
    host = sw.to_numpy().reshape(len(terms) * batch, N + 1)
    assert (host < 2 * N).all()
    check_mod_switch_words(ctx, lwes, host)
    lut = app.LookupTable(ctx, lambda m: (t // 4, t // 8 + 1)[m], 1)  # a step function: two windows on [0, N), negated on [N, 2N)
    assert lut.table[0] == lut.table[N // 2 - 1] == t // 4 and lut.table[N // 2] == lut.table[N - 1] == t // 8 + 1
    f = lut.poly
    limbs = ctx.first_limbs
    assert np.array_equal(lut.test_vector(limbs), scaled_test_vector(ctx, BFV, t, f, limbs))
    got = R.ev.blindRotate(sw, BK, lut.test_vector(limbs), limbs=limbs).cpu()
    assert got.shape[0] == len(terms) * batch
    rot, out_lwes = lut.apply(R.ev, cts, terms, BK)  # the same pipeline through the helper
    assert np.array_equal(rot.cpu(), got) and (out_lwes.count, out_lwes.batch, out_lwes.limbs) == (1, len(terms) * batch, limbs)
    assert np.array_equal(out_lwes.c0_cpu()[0], got[:, 0, :, 0])
    least = None
    for r in range(got.shape[0]):
        phi = (int(host[r, N]) + sum(int(a) * int(d) for a, d in zip(host[r, :N], s))) % (2 * N)
        plain = R.dec.decrypt(got[r], correction_factor=1)
        assert np.array_equal(plain, rotated(f, phi, t)), ("sample", r, "phase", phi)
        assert int(plain[0]) == lut.value(phi)
        budget = R.dec.invariantNoiseBudget(got[r])
        least = budget if least is None else min(least, budget)
    print("pipeline N", N, "n", N, "limbs", limbs, "least invariant noise budget", least)
    assert least > 0
    return least


# ---------------------------------------------------------------- lweModSwitch
def mod_switch_word(x, q, N):
    return (4 * N * int(x) + q) // (2 * q) % (2 * N)


def check_mod_switch_words(ctx, lwes, host):
    q, N = int(ctx.coeff_modulus[0]), ctx.N
    c1 = lwes.c1_cpu().reshape(-1, N)
    c0 = lwes.c0_cpu().reshape(-1)
    exp = np.array([[mod_switch_word(x, q, N) for x in row] + [mod_switch_word(b, q, N)] for row, b in zip(c1, c0)], dtype=np.uint64)
    assert np.array_equal(host, exp)


def check_mod_switch(S, count=2, batch=3):
    """crafted words against Python integers: 0 and q - 1 (which wraps to 0), the rounding boundaries of several k and their predecessors, random words"""
    q, N = S.primes[0], S.N
    words = [0, q - 1, 1, q // 2, q // 2 + 1]
    for k in (0, 1, 2, N - 1, N, 2 * N - 2, 2 * N - 1):
        x = -(-(2 * q * (k + 1) - q) // (4 * N))  # the smallest x with 4N x + q >= 2 q (k + 1)
        assert mod_switch_word(x, q, N) == (k + 1) % (2 * N) and mod_switch_word(x - 1, q, N) == k
        words += [x, x - 1]
    assert mod_switch_word(q - 1, q, N) == 0
    rng = np.random.default_rng(31)
    c1 = rng.integers(0, q, (count, batch, 1, N), dtype=np.uint64)
    c0 = rng.integers(0, q, (count, batch, 1), dtype=np.uint64)
    flat = c1.reshape(-1)
    flat[:len(words)] = words                      # in the first rows ...
    flat[-len(words):] = words[::-1]               # ... and in the last
    c0.reshape(-1)[:count * batch] = (words * 2)[:count * batch]
    lwes = api.LWEBatch(S.ctx, count, batch, 1, c1=api.DeviceBuffer.from_numpy(c1), c0=api.DeviceBuffer.from_numpy(c0))
    host = S.ev.lweModSwitch(lwes).to_numpy().reshape(count * batch, N + 1)
    check_mod_switch_words(S.ctx, lwes, host)
    two = api.LWEBatch(S.ctx, 1, 1, 2)
    HC.with_raises(capi.InvalidArgument, "lwe_mod_switch takes samples of one limb", lambda: S.ev.lweModSwitch(two))


# ---------------------------------------------------------------- key generation
def check_key_generation(scheme, N=256, bits=(40, 40, 40, 40), tbits=14):
    """the key's RGSW [i][t] equals createRGSW (host form) of the constant with the seeds the counter rule assigns, and the counter advanced by 2 n T"""
    ctx, _ = XC.real_context(scheme, N, bits, tbits)
    for secret, ternary, T in (([1, 0, 1], None, 1), ([1, 0, -1, 0], None, 2), ([0, 1], True, 2)):
        kg = api.KeyGenerator(ctx, seed=(91, 7))
        kg.createRGSW(np.ones(1, dtype=np.uint64))  # the counter does not start at zero
        BK = kg.createBlindRotationKey(secret, ternary=ternary)
        n = len(secret)
        assert (BK.n, BK.T) == (n, T) and kg.kswitch_calls == 2 + 2 * n * T
        got = BK.cpu()
        ref = api.KeyGenerator(ctx, seed=(91, 7))
        ref.createRGSW(np.ones(1, dtype=np.uint64))
        for i in range(n):
            for tt in range(T):
                bit = int(secret[i] == (1, -1)[tt])
                assert np.array_equal(got[i, tt], ref.createRGSW(np.array([bit], dtype=np.uint64))), (scheme, secret, i, tt)
        assert ref.kswitch_calls == kg.kswitch_calls
    HC.with_raises(capi.InvalidArgument, "the LWE secret takes 1 to 65536 digits over {-1, 0, 1}", lambda: kg.createBlindRotationKey([]))
    HC.with_raises(capi.InvalidArgument, "the LWE secret takes 1 to 65536 digits over {-1, 0, 1}", lambda: kg.createBlindRotationKey([0, 2]))


# ---------------------------------------------------------------- refusals
def raw_call(S, lwe, n, brk, T, tv, tv_stride, limbs, out_ptr, out_stride, lwe_stride=None, batch=1, limit=0, ctx=None, out=True):
    so = capi.CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    rc = S.lib.troyhip_blind_rotate((ctx or S.ctx).h, C.c_void_p(lwe), C.c_uint64(n + 1 if lwe_stride is None else lwe_stride), C.c_uint64(n), C.c_void_p(brk), T,
                                    C.c_void_p(tv), C.c_uint64(tv_stride), limbs, C.byref(so) if out else None, C.c_uint64(limit), C.c_uint64(batch), None)
    return rc, S.lib.troyhip_last_error().decode() if rc else "", so


def check_refusals(S):
    inv, logic = capi.INVALID_ARGUMENT, capi.LOGIC_ERROR
    limbs, N, K = S.ctx.first_limbs, S.N, S.K
    pw = limbs * N
    n, T = 2, 2
    lwe = api.DeviceBuffer.from_numpy(samples(N, n, 2))
    out = api.DeviceBuffer(2 * 2 * pw)
    out.zero()
    if S.scheme == CKKS:
        g = api.DeviceBuffer(n * T * 2 * (K - 1) * 2 * K * N)
        tv = api.DeviceBuffer(pw)
        rc, msg, _ = raw_call(S, lwe.ptr, n, g.ptr, T, tv.ptr, 0, limbs, out.ptr, 2 * pw)
        assert rc == logic and msg.startswith("unsupported scheme"), (rc, msg)
        HC.with_raises(capi.LogicError, "unsupported scheme", lambda: S.ev.blindRotate(lwe, api.BlindRotationKey(S.ctx, g, n, T), tv, limbs=limbs))
        v = C.c_uint64(0)
        assert S.lib.troyhip_blind_rotate_scratch_words(S.ctx.h, limbs, T, C.c_uint64(1), C.byref(v)) == logic
        rc = S.lib.troyhip_lwe_mod_switch(S.ctx.h, C.c_void_p(tv.ptr), C.c_void_p(tv.ptr), C.c_uint64(1), C.c_uint64(1), C.c_void_p(out.ptr), None)
        assert rc == logic and S.lib.troyhip_last_error().decode().startswith("unsupported scheme")
        return
    G, BK = key_of(S, n, T)
    g = BK.buf.ptr
    tvb = api.DeviceBuffer.from_numpy(test_vectors(S, limbs, 2))
    tv = tvb.ptr

    def refused(rc_msg, code, text=None):
        rc, msg = rc_msg[:2]
        assert rc == code and (text is None or msg.startswith(text)), (rc, msg)
        assert not out.to_numpy(2 * 2 * pw).any()  # the destination is untouched

    refused(raw_call(S, lwe.ptr, n, g, 0, tv, 0, limbs, out.ptr, 2 * pw), inv, "blind_rotate takes 1 or 2 RGSW ciphertexts per digit")
    refused(raw_call(S, lwe.ptr, n, g, 3, tv, 0, limbs, out.ptr, 2 * pw), inv, "blind_rotate takes 1 or 2 RGSW ciphertexts per digit")
    refused(raw_call(S, lwe.ptr, 0, g, T, tv, 0, limbs, out.ptr, 2 * pw), inv, "blind_rotate takes 1 to 65536 LWE digits")
    refused(raw_call(S, lwe.ptr, 65537, g, T, tv, 0, limbs, out.ptr, 2 * pw), inv, "blind_rotate takes 1 to 65536 LWE digits")
    refused(raw_call(S, None, n, g, T, tv, 0, limbs, out.ptr, 2 * pw), inv, "blind_rotate: null pointer")
    refused(raw_call(S, lwe.ptr, n, None, T, tv, 0, limbs, out.ptr, 2 * pw), inv, "blind_rotate: null pointer")
    refused(raw_call(S, lwe.ptr, n, g, T, None, 0, limbs, out.ptr, 2 * pw), inv, "blind_rotate: null pointer")
    refused(raw_call(S, lwe.ptr, n, g, T, tv, 0, limbs, None, 2 * pw), inv, "destination batch stride too small for the result size")
    refused(raw_call(S, lwe.ptr, n, g, T, tv, 0, limbs, out.ptr, 2 * pw, out=False), inv, "null ciphertext")
    refused(raw_call(S, lwe.ptr, n, g, T, tv, 0, limbs, out.ptr, 2 * pw - 1), inv, "destination batch stride too small for the result size")
    refused(raw_call(S, lwe.ptr, n, g, T, tv, 1, limbs, out.ptr, 2 * pw), inv, "blind_rotate: test vector stride is neither 0 nor at least one test vector")
    refused(raw_call(S, lwe.ptr, n, g, T, tv, pw - 1, limbs, out.ptr, 2 * pw), inv, "blind_rotate: test vector stride is neither 0 nor at least one test vector")
    refused(raw_call(S, lwe.ptr, n, g, T, tv, 0, limbs, out.ptr, 2 * pw, lwe_stride=n, batch=2), inv, "blind_rotate: LWE stride is smaller than one sample")
    for bad in (0, S.K, 64, 70, -1):  # no level, the key level, past the 63 digits
        refused(raw_call(S, lwe.ptr, n, g, T, tv, 0, bad, out.ptr, 2 * pw), inv, "encrypted is not valid for encryption parameters")
    rc, msg, _ = raw_call(S, lwe.ptr, n, g, T, tv, pw, limbs, tv + 8 * pw, 2 * pw, batch=2)  # the destination begins inside the test vectors
    assert rc == inv and "destination must be a distinct buffer" in msg, (rc, msg)
    w = S.ev.blindRotateScratchWords(limbs, T, 1)
    refused(raw_call(S, lwe.ptr, n, g, T, tv, 0, limbs, out.ptr, 2 * pw, limit=w - 1), inv, "scratch_limit_words is too small for one ciphertext")
    # a host-only context, and one that cannot switch keys
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    rc, msg, _ = raw_call(S, lwe.ptr, n, g, T, tv, 0, limbs, out.ptr, 2 * pw, ctx=host)
    assert rc == logic and "host-only" in msg, (rc, msg)
    refused((rc, ""), logic)
    S1 = HC.Setup(*HC.adhoc(S.scheme, N, [40]))  # K = 1
    rc, msg, _ = raw_call(S1, lwe.ptr, n, g, T, tv, 0, 1, out.ptr, 2 * N)
    assert rc == logic and msg == "keyswitching is not supported by the context", (rc, msg)
    refused((rc, ""), logic)
    # the scratch query
    v = C.c_uint64(0)
    q = S.lib.troyhip_blind_rotate_scratch_words
    assert q(S.ctx.h, limbs, 0, C.c_uint64(1), C.byref(v)) == inv
    assert q(S.ctx.h, limbs, 3, C.c_uint64(1), C.byref(v)) == inv
    assert q(S.ctx.h, 0, T, C.c_uint64(1), C.byref(v)) == inv
    assert q(S.ctx.h, limbs, T, C.c_uint64(1), None) == inv
    assert q(S.ctx.h, limbs, T, C.c_uint64(1), C.byref(v)) == capi.OK and v.value == w == scratch_words(S, limbs, T, 1)
    # the modulus switch
    ms = S.lib.troyhip_lwe_mod_switch
    for args in ((None, tv, 1), (tv, None, 1), (tv, tv, 0)):
        rc = ms(S.ctx.h, C.c_void_p(args[0]), C.c_void_p(args[1]), C.c_uint64(args[2]), C.c_uint64(1), C.c_void_p(out.ptr), None)
        refused((rc, ""), inv)
    assert ms(S.ctx.h, C.c_void_p(tv), C.c_void_p(tv), C.c_uint64(1), C.c_uint64(1), None, None) == inv
    assert ms(host.h, C.c_void_p(tv), C.c_void_p(tv), C.c_uint64(1), C.c_uint64(1), C.c_void_p(out.ptr), None) == logic
    # a good call fills in the descriptor; an empty batch does nothing
    rc, _, so = raw_call(S, lwe.ptr, n, g, T, tv, 0, limbs, out.ptr, 2 * pw, batch=0)
    assert rc == capi.OK and not out.to_numpy(2 * 2 * pw).any()
    rc, _, so = raw_call(S, lwe.ptr, n, g, T, tv, pw, limbs, out.ptr, 2 * pw, batch=2)
    assert rc == capi.OK and (so.size, so.limbs, so.is_ntt_form, so.scale, so.correction_factor) == (2, limbs, 0, 1.0, 1)
    assert out.to_numpy(2 * 2 * pw).any()
    # the Python layer
    HC.with_raises(capi.InvalidArgument, "blind rotation key is not valid for encryption parameters", lambda: S.ev.blindRotate(lwe, G, tvb, limbs=limbs))
    HC.with_raises(capi.InvalidArgument, "blind rotation key is not valid for encryption parameters", lambda: api.BlindRotationKey(S.ctx, api.DeviceBuffer(8), 1, 1))
    HC.with_raises(capi.InvalidArgument, "blind rotation key is not valid for encryption parameters", lambda: api.BlindRotationKey(S.ctx, BK.buf, n, 3))
    HC.with_raises(capi.InvalidArgument, "blind_rotate: LWE samples take n . 1 words each", lambda: S.ev.blindRotate(np.zeros((2, n), dtype=np.uint64), BK, tvb, limbs=limbs))
    HC.with_raises(capi.InvalidArgument, "blind_rotate: a test vector takes limbs x N words", lambda: S.ev.blindRotate(lwe, BK, np.zeros((limbs, N - 1), dtype=np.uint64)))
