"""Shared checks of LWE key switching to a smaller dimension (troyhip_lwe_key_switch, troyhip_lwe_key_switch_scratch_words,
troyhip_lwe_kswitch_key_words, troyhip_host_lwe_kswitch_key).  Every step is exact arithmetic, so every comparison here is
np.array_equal: against the model in integers (lweks_model), of the call against itself at another batch size, split or scratch limit, of the key
generator against sampler_model's stream, of the phase under real keys against the operand's phase plus the recomputed key noise, and of decryptions
after a look-up against f(message).  Used by tests/test_device_lweks.py (emulator build) and tests/test_gpu_lweks.py (MI355X)."""
import ctypes as C

import numpy as np

import extprod_cases as XC
import hoist_cases as HC
import lweks_model as LM
from troy_amd import api, app, capi
from troy_amd.capi import BFV, CKKS

SYMBOLS = ("troyhip_lwe_key_switch", "troyhip_lwe_key_switch_scratch_words", "troyhip_lwe_kswitch_key_words", "troyhip_host_lwe_kswitch_key")
COUNTERS = ("lwe_ks_slabs", "lwe_ks_splits")
SETS = XC.SETS                                   # bfv_n64_k3 (the plan gives S = 1), bgv_n128_k4 (S = 2 at small batches)
NARROW = XC.NARROW                               # primes below 2^33
MEDIUM = XC.MEDIUM
DIMS = [1, 5, 63, 64]                            # n: n + 1 = 2 and 6 columns, exactly one wave of columns, and one past it
BASES = [1, 7, 16]                               # base_bits; 7 leaves a ragged top digit
SHAPES = [(1, 1), (1, 2), (2, 1), (1, 5), (5, 1)]  # (count, batch): R = 1, 2, 5 in both factorizations; the kernel's tiles of 1, 2 and 4 samples
SENTINEL = 0xA5A5A5A5A5A5A5A5                    # what the padding words of a row hold before and after the call
Z16 = [1, -1, 0, 1, 1, -1, -1, 1, 0, -1, 1, 1, -1, 0, 1, -1]  # the target secret of the real-key checks: n = 16, 13 digits are not zero


def stat(name):
    return capi.stat(name, api.KernelProvider.lib())


def check_symbols(lib, header_text):
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in capi.SYMBOLS and "int %s(" % sym in header_text, sym
    for name in COUNTERS:
        assert capi.stat(name, lib) >= 0 and '"%s"' % name in header_text


# ---------------------------------------------------------------- the plan, restated (evaluator.cpp: lwe_ks_splits)
def tile_of(R):
    return 8 if R >= 64 else 4 if R >= 4 else 2 if R >= 2 else 1


def splits_of(N, n, R):
    """S: a power of two, parts of at least 64 coefficients, 64 parts at the most, until the grid has 1024 waves"""
    waves = -(-(n + 1) // 64) * -(-R // tile_of(R))
    cap = min(max(N // 64, 1), 64)
    S = 1
    while S < cap and S * waves < 1024:
        S *= 2
    return S


def scratch_words(N, n, R):
    return R * splits_of(N, n, R) * (n + 1) + 32 + 128


# ---------------------------------------------------------------- samples and keys
def crafted_words(q, w):
    """0, q - 1, the word with every bit below q's top bit set (every digit below the top one is 2^w - 1), words at and above q with bits 61 - 63 set, the
    digit boundaries 2^(w j) and 2^(w j) - 1"""
    l = LM.digit_count(q, w)
    words = [0, q - 1, (1 << (q.bit_length() - 1)) - 1, q, q + 1, (1 << 64) - 1, (7 << 61) | 12345, (1 << 63) | (q - 1), (1 << 62) + 1, (1 << 61)]
    for j in range(l):
        words += [(1 << (w * j)) % q, ((1 << (w * j)) - 1) % q]
    return words


def samples(q, N, R, w, seed=0):
    """c1 [R][N] and c0 [R]: crafted words in the first and in the last row, random words below q elsewhere; row r does not depend on R"""
    c1 = np.stack([np.random.default_rng([seed, r, 77]).integers(0, q, N, dtype=np.uint64) for r in range(R)])
    c0 = np.array([int(np.random.default_rng([seed, r, 78]).integers(0, q)) for r in range(R)], dtype=np.uint64)
    words = crafted_words(q, w)
    m = min(len(words), N)
    c1[0, :m] = np.array(words[:m], dtype=np.uint64)
    c1[R - 1, N - m:] = np.array(words[::-1][:m], dtype=np.uint64)  # from the other end of the list: the two rows hold every word where N is short
    c0[0] = (1 << 63) | (q - 1)
    c0[R - 1] = q - 1 if R > 1 else c0[0]
    return c1, c0


def key_of(S, n, w, fill=None):
    """a synthetic key [N][l][n + 1] of uniform words below q_0 (the arithmetic is oblivious to its validity) -> (host, LWESwitchKey); fill: every word"""
    cache = S.__dict__.setdefault("_lwe_keys", {})
    if (n, w, fill) not in cache:
        q, N = S.primes[0], S.N
        l = LM.digit_count(q, w)
        k = np.random.default_rng([n, w, 79]).integers(0, q, (N, l, n + 1), dtype=np.uint64)
        if fill is not None:
            k[:] = fill
        else:
            k[0, 0, :] = q - 1
            k[-1, -1, :] = q - 1
            k[N // 2, 0, 0] = 0
        cache[(n, w, fill)] = (k, api.LWESwitchKey.from_numpy(S.ctx, k, w))
    return cache[(n, w, fill)]


def batch_of(S, c1, c0, count, batch):
    N = S.N
    return api.LWEBatch(S.ctx, count, batch, 1, c1=api.DeviceBuffer.from_numpy(c1.reshape(count, batch, 1, N)), c0=api.DeviceBuffer.from_numpy(c0.reshape(count, batch, 1)))


def run(S, c1, c0, LK, to_2n, count=None, batch=1, limit=0):
    """Evaluator.lweKeySwitch on an LWEBatch of count x batch samples -> [R][n + 1]"""
    R = c1.shape[0]
    count = R // batch if count is None else count
    assert count * batch == R
    out = S.ev.lweKeySwitch(batch_of(S, c1, c0, count, batch), LK, to_2n=to_2n, scratch_limit_words=limit)
    assert out.words == R * (LK.n + 1)
    return out.to_numpy().reshape(R, LK.n + 1)


def raw_call(S, c1, c0, samples_, key, n, w, to_2n, out, stride, limit=0, ctx=None):
    rc = S.lib.troyhip_lwe_key_switch((ctx or S.ctx).h, C.c_void_p(c1), C.c_void_p(c0), C.c_uint64(samples_), C.c_void_p(key), C.c_uint64(n), w, to_2n, C.c_void_p(out),
                                      C.c_uint64(stride), C.c_uint64(limit), None)
    return rc, S.lib.troyhip_last_error().decode() if rc else ""


def run_strided(S, c1, c0, LK, to_2n, stride):
    """the raw call with rows `stride` words apart -> [R][n + 1]; the padding words keep what they held"""
    R, n = c1.shape[0], LK.n
    d1, d0 = api.DeviceBuffer.from_numpy(c1), api.DeviceBuffer.from_numpy(c0)
    out = api.DeviceBuffer.from_numpy(np.full(R * stride, SENTINEL, dtype=np.uint64))
    rc, msg = raw_call(S, d1.ptr, d0.ptr, R, LK.buf.ptr, n, LK.base_bits, int(to_2n), out.ptr, stride)
    assert rc == capi.OK, msg
    api.synchronize()
    got = out.to_numpy().reshape(R, stride)
    assert (got[:, n + 1:] == np.uint64(SENTINEL)).all(), "padding words were written"
    return got[:, :n + 1]


_expected = {}


def expected(S, c1, c0, K, w, to_2n, what):
    """the model, computed once per case and shared by the forms of the call"""
    if what not in _expected:
        exp = LM.key_switch_fast(c1, c0, K, S.primes[0], w, to_2n)
        exp.setflags(write=False)
        _expected[what] = exp
    return _expected[what]


# ---------------------------------------------------------------- the model
def check_model_agrees_with_plain_integers():
    """the vectorised model against the definition word by word: no library involved"""
    for q, N, n, w in ((1099511590913, 16, 3, 7), ((1 << 60) - 93, 8, 2, 16), (40961, 8, 1, 1)):
        l = LM.digit_count(q, w)
        rng = np.random.default_rng(5)
        c1, c0 = samples(q, N, 3, w)
        K = rng.integers(0, q, (N, l, n + 1), dtype=np.uint64)
        K[0] = q - 1
        for to_2n in (False, True):
            assert np.array_equal(LM.key_switch_fast(c1, c0, K, q, w, to_2n), LM.key_switch(c1, c0, K, q, w, to_2n)), (q, w, to_2n)


def check_model(S, n, w):
    """every word equals the model: R = 1, 2, 5 in both factorizations, both forms of to_2n, rows n + 1 and n + 4 words apart"""
    q, N = S.primes[0], S.N
    K, LK = key_of(S, n, w)
    for count, batch in SHAPES:
        R = count * batch
        c1, c0 = samples(q, N, R, w)
        s0 = stat("lwe_ks_slabs")
        for to_2n in (False, True):
            exp = expected(S, c1, c0, K, w, to_2n, (S.name, n, w, R, to_2n))
            got = run(S, c1, c0, LK, to_2n, count, batch)
            assert np.array_equal(got, exp), (S.name, "n", n, "w", w, "count", count, "batch", batch, "to_2n", to_2n)
            assert (got < np.uint64(2 * N if to_2n else q)).all()
            if count == 1:
                assert np.array_equal(run_strided(S, c1, c0, LK, to_2n, n + 4), exp), (S.name, "n", n, "w", w, "R", R, "to_2n", to_2n, "stride n + 4")
        assert stat("lwe_ks_slabs") - s0 == (4 if count == 1 else 2) and stat("lwe_ks_splits") == splits_of(N, n, R)


def check_lazy_bound(S, n=5, R=5):
    """the lazy sum at its bound: every key word is q_0 - 1 and every sample word has every bit below q_0's top bit set, at 16-bit digits; and q_0 - 1"""
    q, N = S.primes[0], S.N
    for w in (16, 15):
        K, LK = key_of(S, n, w, fill=q - 1)
        assert (K == np.uint64(q - 1)).all()
        for word in ((1 << (q.bit_length() - 1)) - 1, q - 1):
            c1 = np.full((R, N), word, dtype=np.uint64)
            c0 = np.full(R, q - 1, dtype=np.uint64)
            for to_2n in (False, True):
                exp = LM.key_switch_fast(c1, c0, K, q, w, to_2n)
                assert np.array_equal(run(S, c1, c0, LK, to_2n), exp), (S.name, "w", w, "word", word, "to_2n", to_2n)
        total = N * LM.digit_count(q, w) * ((1 << w) - 1) * (q - 1)
        assert total < 1 << 99
    return q.bit_length()


# ---------------------------------------------------------------- the rounding boundaries of the switch to 2N
def check_rounding_boundaries(S, n=5, w=7):
    """out[r][n] is c0_r plus a constant the model knows: c0_r is chosen so that the word lands on x and on x - 1 for every boundary x (the smallest x with
    round(2N x / q_0) = k + 1); both sides are asserted"""
    q, N = S.primes[0], S.N
    K, LK = key_of(S, n, w)
    ks = (0, 1, 2, N - 1, N, 2 * N - 2, 2 * N - 1)
    R = 2 * len(ks)
    c1, c0 = samples(q, N, R, w, seed=3)
    const = LM.key_switch_fast(c1, np.zeros(R, dtype=np.uint64), K, q, w, False)[:, n]
    want = []
    for j, k in enumerate(ks):
        x = -(-(2 * q * (k + 1) - q) // (4 * N))  # the smallest x with 4N x + q >= 2 q (k + 1)
        assert LM.switch_word(x, q, N) == (k + 1) % (2 * N) and LM.switch_word(x - 1, q, N) == k
        for side, target in enumerate((x, x - 1)):
            r = 2 * j + side
            c0[r] = (target - int(const[r])) % q
            want.append(((k + 1) % (2 * N), k)[side])
    plain = run(S, c1, c0, LK, False)
    got = run(S, c1, c0, LK, True)
    for j, k in enumerate(ks):
        x = -(-(2 * q * (k + 1) - q) // (4 * N))
        assert (int(plain[2 * j, n]), int(plain[2 * j + 1, n])) == (x % q, x - 1), (S.name, k)
    assert [int(v) for v in got[:, n]] == want, (S.name, [int(v) for v in got[:, n]], want)
    assert np.array_equal(got, LM.key_switch_fast(c1, c0, K, q, w, True))


# ---------------------------------------------------------------- independence
def check_independence(S, expect_splits, n=5, w=7):
    """the same bytes alone, inside a larger batch, in a batch large enough for another S, and under limits that force slabs.  The plan does not depend on
    the device: expect_splits pins S at one sample for this set"""
    q, N = S.primes[0], S.N
    n1 = n + 1
    K, LK = key_of(S, n, w)
    c1, c0 = samples(q, N, 5, w, seed=1)
    for to_2n in (False, True):
        full = run(S, c1, c0, LK, to_2n)
        assert stat("lwe_ks_splits") == splits_of(N, n, 5)
        assert np.array_equal(full, LM.key_switch_fast(c1, c0, K, q, w, to_2n))
        for r in range(5):
            assert np.array_equal(run(S, c1[r:r + 1], c0[r:r + 1], LK, to_2n)[0], full[r]), (S.name, "sample alone", r)
            assert stat("lwe_ks_splits") == expect_splits == splits_of(N, n, 1)
        for R in (2, 3):
            assert np.array_equal(run(S, c1[:R], c0[:R], LK, to_2n), full[:R]), (S.name, "batch", R)
        words, sp = S.ev.lweKeySwitchScratchWords(n, w, 5)
        assert (words, sp) == (scratch_words(N, n, 5), splits_of(N, n, 5))
        one, sp1 = S.ev.lweKeySwitchScratchWords(n, w, 1)
        assert (one, sp1) == (scratch_words(N, n, 1), expect_splits)
        s0 = stat("lwe_ks_slabs")
        assert np.array_equal(run(S, c1, c0, LK, to_2n, limit=one), full), (S.name, "one sample per slab")
        assert stat("lwe_ks_slabs") - s0 == 5
        two = 2 * splits_of(N, n, 5) * n1 + 160
        s0 = stat("lwe_ks_slabs")
        assert np.array_equal(run(S, c1, c0, LK, to_2n, limit=two), full), (S.name, "two samples per slab")
        assert stat("lwe_ks_slabs") - s0 == 3
        HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small for one sample", lambda: run(S, c1, c0, LK, to_2n, limit=one - 1))


def check_other_split(S, R, expect_splits, n=63, w=16):
    """a batch large enough that the plan gives `expect_splits` (fewer parts than at one sample): its first and last samples equal the samples alone"""
    q, N = S.primes[0], S.N
    assert splits_of(N, n, R) == expect_splits != splits_of(N, n, 1)
    K, LK = key_of(S, n, w)
    c1, c0 = samples(q, N, R, w, seed=2)
    got = run(S, c1, c0, LK, True)
    assert stat("lwe_ks_splits") == expect_splits
    for r in (0, 1, R - 1):
        assert np.array_equal(run(S, c1[r:r + 1], c0[r:r + 1], LK, True)[0], got[r]), (S.name, "sample", r)
        assert stat("lwe_ks_splits") == splits_of(N, n, 1)
    assert np.array_equal(got, LM.key_switch_fast(c1, c0, K, q, w, True))


def check_many_samples(S, R=65537, n=1, w=8):
    """more samples than a grid dimension other than x could hold"""
    q, N = S.primes[0], S.N
    K, LK = key_of(S, n, w)
    c1, c0 = samples(q, N, R, w)
    got = run(S, c1, c0, LK, False)
    assert np.array_equal(got, LM.key_switch_fast(c1, c0, K, q, w, False))


# ---------------------------------------------------------------- key generation
def check_key_generation(scheme, N=64, bits=(40, 40, 40), tbits=10):
    """the key equals the model on sampler_model's stream (lo + kswitch_calls, hi, 10 << 32) byte for byte; every row has the phase u_i 2^(w j) + e with a
    centred-binomial e; the counter advances by 1 and a second key uses the next seed; extractionSecret() is the map of secretCoefficients()"""
    ctx, _ = XC.real_context(scheme, N, bits, tbits)
    q = int(ctx.coeff_modulus[0])
    lo, hi = 93, 11
    for z, w in (([1], 7), ([-1, 0, 1, 1, -1], 7), ([1], 16), ([0, -1, 1, 0, 1], 16)):
        kg = api.KeyGenerator(ctx, seed=(lo, hi))
        s = kg.secretCoefficients()
        u = kg.extractionSecret()
        assert u.dtype == np.int64 and np.array_equal(u, LM.extraction_secret(s)) and u[0] == s[0] and np.array_equal(u[1:], -s[:0:-1])
        kg.createRGSW(np.ones(1, dtype=np.uint64))  # the counter does not start at zero
        assert kg.kswitch_calls == 2
        n, l = len(z), LM.digit_count(q, w)
        LK = kg.createLWESwitchKey(z, base_bits=w)
        assert (LK.n, LK.base_bits, LK.digits, kg.kswitch_calls) == (n, w, l, 3)
        words = C.c_uint64(0)
        assert ctx.lib.troyhip_lwe_kswitch_key_words(ctx.h, C.c_uint64(n), w, C.byref(words)) == capi.OK and words.value == N * l * (n + 1) == LK.buf.words
        got = LK.cpu()
        assert got.shape == (N, l, n + 1)
        assert np.array_equal(got, LM.key_of(lo + 2, hi, q, s, z, w)), (scheme, z, w)
        e = LM.key_errors(got, q, s, z, w)
        assert np.abs(e).max() <= 21 and e.any()
        second = kg.createLWESwitchKey(z, base_bits=w).cpu()
        assert kg.kswitch_calls == 4 and np.array_equal(second, LM.key_of(lo + 3, hi, q, s, z, w)) and not np.array_equal(second, got)
    # the host form on a host-only context gives the same words
    host = api.SEALContext(scheme, N, [int(p) for p in ctx.coeff_modulus], int(ctx.plain_modulus), host_only=True)
    out = np.zeros((N, l, n + 1), dtype=np.uint64)
    z8 = np.array(z, dtype=np.int8)
    rc = ctx.lib.troyhip_host_lwe_kswitch_key(host.h, C.c_uint64(lo + 2), C.c_uint64(hi), api._u64p(kg.secretKey()), z8.ctypes.data_as(C.c_void_p), C.c_uint64(n), w,
                                              api._u64p(out))
    assert rc == capi.OK and np.array_equal(out, got)
    # a key that is not ternary is refused
    bad = kg.secretKey().copy()
    bad[0, 0] = (int(bad[0, 0]) + 1) % q
    rc = ctx.lib.troyhip_host_lwe_kswitch_key(ctx.h, C.c_uint64(1), C.c_uint64(2), api._u64p(bad), z8.ctypes.data_as(C.c_void_p), C.c_uint64(n), w, api._u64p(out))
    assert rc == capi.LOGIC_ERROR and ctx.lib.troyhip_last_error().decode() == "the secret key is not ternary"


# ---------------------------------------------------------------- real keys
def message_phases(R, lwes):
    """the phase c0 + c1[0] s_0 - sum_(i >= 1) c1[i] s_(N-i) mod q_0 of every sample of a one-limb LWEBatch, in integers"""
    q, N = int(R.ctx.coeff_modulus[0]), R.N
    u = [int(v) for v in R.kg.extractionSecret()]
    c1 = lwes.c1_cpu().reshape(-1, N)
    c0 = lwes.c0_cpu().reshape(-1)
    return [(int(b) + sum(int(a) * d for a, d in zip(row, u))) % q for row, b in zip(c1, c0)]


def check_phase(scheme, N=256, bits=(40, 40, 40, 40), tbits=14, w=8, terms=None, batch=2):
    """fresh encryptions brought to one limb, three terms extracted and switched to z with to_2n=False: the phase of every result under z equals the phase
    of the operand under the RLWE secret plus sum d e, recomputed from the key's recovered errors.  An exact condition"""
    R = XC.Real(scheme, N, bits, tbits)
    ctx, q = R.ctx, int(R.ctx.coeff_modulus[0])
    terms = (0, 5, N - 1) if terms is None else terms
    n = len(Z16)
    assert sum(1 for v in Z16 if v) == 13
    LK = R.kg.createLWESwitchKey(Z16, base_bits=w)
    e = LM.key_errors(LK.cpu(), q, R.kg.secretCoefficients(), Z16, w)
    assert np.abs(e).max() <= 21
    rng = np.random.default_rng(37)
    cts = R.encrypt(rng.integers(0, R.t, (batch, N), dtype=np.uint64))
    lwes = R.ev.extractLWEs(R.ev.modSwitchTo(cts, 1), list(terms))
    assert lwes.limbs == 1
    got = R.ev.lweKeySwitch(lwes, LK, to_2n=False).to_numpy().reshape(len(terms) * batch, n + 1)
    before = message_phases(R, lwes)
    c1 = lwes.c1_cpu().reshape(-1, N)
    worst = 0
    for r in range(got.shape[0]):
        after = (int(got[r, n]) + sum(int(a) * zk for a, zk in zip(got[r, :n], Z16))) % q
        noise = sum(d * int(e[i, j]) for i in range(N) for j, d in enumerate(LM.digits_of(c1[r, i], q, w)))
        assert (after - before[r]) % q == noise % q, (scheme, "sample", r)
        assert abs(noise) <= N * LM.digit_count(q, w) * ((1 << w) - 1) * 21
        worst = max(worst, abs(noise))
    print("scheme", scheme, "N", N, "n", n, "w", w, "largest |sum d e|", worst, "of q_0 =", q)
    # the same words through the model
    assert np.array_equal(got, LM.key_switch_fast(c1, lwes.c0_cpu().reshape(-1), LK.cpu(), q, w, False))


def TABLE(t):
    """f(k) for the four windows of t_bits = 2"""
    return (t // 4, 3, t - 5, t // 8 + 1)


def check_lookup(route, N=256, bits=(40, 40, 40, 40), tbits=14, w=8, terms=(0, 5, 255), batch=3):
    """f(message), end to end: LookupTable(t_bits = 2) has windows of N / 4 = 64 phases; the message coefficients sit at the windows' centres,
    m = (t (2k + 1) 64 + 2N) // (4N), so the phase error may reach 32 before a result is wrong -- the roundings give at most (1 + 13) / 2 and the scaled
    noise less than 1.  Every result's constant coefficient decrypts to f(k) exactly and the noise budget is positive.
    route "switch": LookupTable.apply(.., BK, lwe_key=LK) with LK = createLWESwitchKey(z), BK = createBlindRotationKey(z), n = 16.
    route "n=N": LookupTable.apply(.., createBlindRotationKey(kg.extractionSecret())), 256 steps (the MI355X only)."""
    R = XC.Real(BFV, N, bits, tbits)
    ctx, t = R.ctx, R.t
    f = TABLE(t)
    assert len(set(f)) == 4
    lut = app.LookupTable(ctx, lambda k: f[k], 2)
    assert N // 4 == 64 and all(int(lut.table[64 * k]) == int(lut.table[64 * k + 63]) == f[k] for k in range(4))
    rng = np.random.default_rng(41)
    msgs = rng.integers(0, t, (batch, N), dtype=np.uint64)
    ks = np.array([[(b + 2 * j + 1) % 4 for b in range(batch)] for j in range(len(terms))])
    for j, term in enumerate(terms):
        for b in range(batch):
            k = int(ks[j, b])
            msgs[b, term] = (t * (2 * k + 1) * 64 + 2 * N) // (4 * N)
            assert abs(2 * N * int(msgs[b, term]) / t - (64 * k + 32)) < 1
    assert set(ks.reshape(-1).tolist()) == {0, 1, 2, 3}
    cts = R.encrypt(msgs)
    if route == "switch":
        LK = R.kg.createLWESwitchKey(Z16, base_bits=w)
        BK = R.kg.createBlindRotationKey(Z16)
        assert (BK.n, BK.T) == (16, 2)
        s0 = stat("blindrot_steps")
        rot, out = lut.apply(R.ev, cts, list(terms), BK, lwe_key=LK)
        assert stat("blindrot_steps") - s0 == 16
    else:
        BK = R.kg.createBlindRotationKey(R.kg.extractionSecret())
        assert (BK.n, BK.T) == (N, 2)
        rot, out = lut.apply(R.ev, cts, list(terms), BK)
    got = rot.cpu()
    assert got.shape[0] == len(terms) * batch and (out.count, out.batch) == (1, len(terms) * batch)
    least = None
    for j in range(len(terms)):
        for b in range(batch):
            r = j * batch + b
            plain = R.dec.decrypt(got[r], correction_factor=1)
            assert int(plain[0]) == f[int(ks[j, b])], (route, "term", terms[j], "item", b, "window", int(ks[j, b]), int(plain[0]))
            budget = R.dec.invariantNoiseBudget(got[r])
            assert budget > 0
            least = budget if least is None else min(least, budget)
    print("lookup route", route, "N", N, "least invariant noise budget", least)
    if route == "switch":  # the dimensions must agree
        other = R.kg.createLWESwitchKey(Z16[:5], base_bits=w)
        HC.with_raises(capi.InvalidArgument, "LookupTable: the LWE switching key and the blind rotation key differ in dimension",
                       lambda: lut.apply(R.ev, cts, list(terms), BK, lwe_key=other))


# ---------------------------------------------------------------- refusals
def check_refusals(S):
    inv, logic = capi.INVALID_ARGUMENT, capi.LOGIC_ERROR
    N, n, w = S.N, 5, 7
    q = S.primes[0]
    l = LM.digit_count(q, w)
    R = 2
    c1 = api.DeviceBuffer(R * N)
    c0 = api.DeviceBuffer(R)
    c1.zero()
    c0.zero()
    out = api.DeviceBuffer(R * (n + 1))
    out.zero()
    v, sp = C.c_uint64(0), C.c_uint64(0)
    sw = S.lib.troyhip_lwe_key_switch_scratch_words
    kw = S.lib.troyhip_lwe_kswitch_key_words
    if S.scheme == CKKS:
        key = api.DeviceBuffer(N * l * (n + 1))
        rc, msg = raw_call(S, c1.ptr, c0.ptr, R, key.ptr, n, w, 1, out.ptr, n + 1)
        assert rc == logic and msg.startswith("unsupported scheme"), (rc, msg)
        LK = api.LWESwitchKey(S.ctx, key, n, w)
        HC.with_raises(capi.LogicError, "unsupported scheme", lambda: S.ev.lweKeySwitch(api.LWEBatch(S.ctx, 1, R, 1), LK))
        assert sw(S.ctx.h, C.c_uint64(n), w, C.c_uint64(1), C.byref(v), C.byref(sp)) == logic
        assert kw(S.ctx.h, C.c_uint64(n), w, C.byref(v)) == logic
        return
    K, LK = key_of(S, n, w)
    key = LK.buf.ptr

    def refused(rc_msg, code, text=None):
        rc, msg = rc_msg
        assert rc == code and (text is None or msg.startswith(text)), (rc, msg)
        assert not out.to_numpy(R * (n + 1)).any()  # the destination is untouched

    refused(raw_call(S, None, c0.ptr, R, key, n, w, 1, out.ptr, n + 1), inv, "lwe_key_switch: null pointer")
    refused(raw_call(S, c1.ptr, None, R, key, n, w, 1, out.ptr, n + 1), inv, "lwe_key_switch: null pointer")
    refused(raw_call(S, c1.ptr, c0.ptr, R, None, n, w, 1, out.ptr, n + 1), inv, "lwe_key_switch: null pointer")
    refused(raw_call(S, c1.ptr, c0.ptr, R, key, n, w, 1, None, n + 1), inv, "lwe_key_switch: null pointer")
    refused(raw_call(S, c1.ptr, c0.ptr, R, key, 0, w, 1, out.ptr, n + 1), inv, "lwe_key_switch takes 1 to 65536 LWE digits")
    refused(raw_call(S, c1.ptr, c0.ptr, R, key, 65537, w, 1, out.ptr, 65538), inv, "lwe_key_switch takes 1 to 65536 LWE digits")
    refused(raw_call(S, c1.ptr, c0.ptr, R, key, n, 0, 1, out.ptr, n + 1), inv, "lwe_key_switch takes 1 to 16 base bits")
    refused(raw_call(S, c1.ptr, c0.ptr, R, key, n, 17, 1, out.ptr, n + 1), inv, "lwe_key_switch takes 1 to 16 base bits")
    refused(raw_call(S, c1.ptr, c0.ptr, R, key, n, -1, 1, out.ptr, n + 1), inv, "lwe_key_switch takes 1 to 16 base bits")
    refused(raw_call(S, c1.ptr, c0.ptr, R, key, n, w, 1, out.ptr, n), inv, "lwe_key_switch: output stride is smaller than one sample")
    refused(raw_call(S, c1.ptr, c0.ptr, 0, key, n, w, 1, out.ptr, n + 1), inv, "lwe_key_switch: no samples, or too many")
    refused(raw_call(S, c1.ptr, c0.ptr, (1 << 40) + 1, key, n, w, 1, out.ptr, n + 1), inv, "lwe_key_switch: no samples, or too many")
    refused(raw_call(S, c1.ptr, c0.ptr, 1 << 63, key, n, w, 1, out.ptr, n + 1), inv, "lwe_key_switch: no samples, or too many")
    refused(raw_call(S, c1.ptr, c0.ptr, R, key, n, w, 1, out.ptr, (1 << 22) + 1), inv, "lwe_key_switch: no samples, or too many")
    # the destination inside the samples, on c0, inside the key
    for dst in (c1.ptr + 8 * (N - 1), c0.ptr, key + 8 * (N * l * (n + 1) - 1), key - 8 * (R * (n + 1) - 1)):
        refused(raw_call(S, c1.ptr, c0.ptr, R, key, n, w, 1, dst, n + 1), inv, "lwe_key_switch: destination must be a distinct buffer")
    one = scratch_words(N, n, 1)
    refused(raw_call(S, c1.ptr, c0.ptr, R, key, n, w, 1, out.ptr, n + 1, limit=one - 1), inv, "scratch_limit_words is too small for one sample")
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    rc, msg = raw_call(S, c1.ptr, c0.ptr, R, key, n, w, 1, out.ptr, n + 1, ctx=host)
    assert "host-only" in msg
    refused((rc, ""), logic)
    # the queries
    assert sw(S.ctx.h, C.c_uint64(0), w, C.c_uint64(1), C.byref(v), C.byref(sp)) == inv
    assert sw(S.ctx.h, C.c_uint64(n), 17, C.c_uint64(1), C.byref(v), C.byref(sp)) == inv
    assert sw(S.ctx.h, C.c_uint64(n), w, C.c_uint64(0), C.byref(v), C.byref(sp)) == inv
    assert sw(S.ctx.h, C.c_uint64(n), w, C.c_uint64(1), None, C.byref(sp)) == inv
    assert sw(S.ctx.h, C.c_uint64(n), w, C.c_uint64(1), C.byref(v), None) == capi.OK and v.value == one
    assert sw(host.h, C.c_uint64(n), w, C.c_uint64(3), C.byref(v), C.byref(sp)) == capi.OK and (v.value, sp.value) == (scratch_words(N, n, 3), splits_of(N, n, 3))
    assert kw(S.ctx.h, C.c_uint64(0), w, C.byref(v)) == inv and kw(S.ctx.h, C.c_uint64(n), 0, C.byref(v)) == inv and kw(S.ctx.h, C.c_uint64(n), w, None) == inv
    assert kw(host.h, C.c_uint64(n), w, C.byref(v)) == capi.OK and v.value == N * l * (n + 1)
    hk = S.lib.troyhip_host_lwe_kswitch_key
    sk = np.zeros((S.K, N), dtype=np.uint64)
    z8 = np.zeros(n, dtype=np.int8)
    buf = np.zeros(N * l * (n + 1), dtype=np.uint64)
    zp = z8.ctypes.data_as(C.c_void_p)
    assert hk(S.ctx.h, C.c_uint64(1), C.c_uint64(2), None, zp, C.c_uint64(n), w, api._u64p(buf)) == inv
    assert hk(S.ctx.h, C.c_uint64(1), C.c_uint64(2), api._u64p(sk), None, C.c_uint64(n), w, api._u64p(buf)) == inv
    assert hk(S.ctx.h, C.c_uint64(1), C.c_uint64(2), api._u64p(sk), zp, C.c_uint64(n), w, None) == inv
    assert hk(S.ctx.h, C.c_uint64(1), C.c_uint64(2), api._u64p(sk), zp, C.c_uint64(0), w, api._u64p(buf)) == inv
    assert hk(S.ctx.h, C.c_uint64(1), C.c_uint64(2), api._u64p(sk), zp, C.c_uint64(n), 17, api._u64p(buf)) == inv
    z8[1] = 2
    assert hk(S.ctx.h, C.c_uint64(1), C.c_uint64(2), api._u64p(sk), zp, C.c_uint64(n), w, api._u64p(buf)) == inv and not buf.any()
    # a good call writes; the Python layer
    rc, msg = raw_call(S, c1.ptr, c0.ptr, R, key, n, w, 1, out.ptr, n + 1)
    assert rc == capi.OK, msg
    good = api.LWEBatch(S.ctx, 1, R, 1)
    HC.with_raises(capi.InvalidArgument, "lwe_key_switch takes samples of one limb", lambda: S.ev.lweKeySwitch(api.LWEBatch(S.ctx, 1, 1, 2), LK))
    HC.with_raises(capi.InvalidArgument, "lwe_key_switch takes an LWEBatch", lambda: S.ev.lweKeySwitch(c1, LK))
    HC.with_raises(capi.InvalidArgument, "LWE switching key is not valid for encryption parameters", lambda: S.ev.lweKeySwitch(good, K))
    HC.with_raises(capi.InvalidArgument, "LWE switching key is not valid for encryption parameters", lambda: api.LWESwitchKey(S.ctx, api.DeviceBuffer(8), n, w))
    HC.with_raises(capi.InvalidArgument, "LWE switching key is not valid for encryption parameters", lambda: api.LWESwitchKey(S.ctx, LK.buf, n, 17))
    HC.with_raises(capi.InvalidArgument, "LWE switching key is not valid for encryption parameters", lambda: api.LWESwitchKey.from_numpy(S.ctx, K[:, :-1], w))
    kg = api.KeyGenerator(S.ctx, seed=(1, 2))
    HC.with_raises(capi.InvalidArgument, "the LWE secret takes 1 to 65536 digits over {-1, 0, 1}", lambda: kg.createLWESwitchKey([]))
    HC.with_raises(capi.InvalidArgument, "the LWE secret takes 1 to 65536 digits over {-1, 0, 1}", lambda: kg.createLWESwitchKey([0, 2]))
    HC.with_raises(capi.InvalidArgument, "lwe_key_switch takes 1 to 16 base bits", lambda: kg.createLWESwitchKey([0, 1], base_bits=0))
    assert kg.kswitch_calls == 0
