"""The library's randomness against an independent model (tests/sampler_model.py: ChaCha20 of RFC 8439 and the streams of DESIGN.md 4.6 / 4.8).

1. The model checks itself: the RFC's block, recorded stream words, and openssl's chacha20 where there is one.
2. Every form that consumes randomness is pinned to the model: the draws are recovered from the keys and ciphertexts with Python integers and the
   oracle's NTT and compared for equality -- host forms, and the device forms on the emulator build directly (not through their host siblings).
3. The distributions of draws already proved equal to the model (so a failure is a statement about the specification): CBD, ternary, uniform,
   independence.  Every seed is fixed, every test deterministic; a chi-square passes at a one-sided p >= 1e-6.
4. No two calls of one KeyGenerator / Encryptor share stream words."""
import os
import shutil
import subprocess
from math import comb

import numpy as np
import pytest
from scipy import stats

import cases
import enc_cases as E
import keygen_cases as G
import sampler_model as M
from conftest import ROOT
from oracle import oracle
from troy_amd.capi import BFV, BGV, CKKS

EMUL = os.path.join(ROOT, "tests", "emul", "libtroyhip_emul.so")
P_MIN = 1e-6  # acceptance level of every chi-square (one-sided)
SEEDS = [(0x5EED, 7), (0x8000000000000123, 0), (0xFFFFFFFFFFFFFFF0, 0x9000000000000001)]  # hi != 0; bit 63 of lo set; both, with lo near 2^64


@pytest.fixture(scope="module")
def emul_api():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    from troy_amd import api, capi
    lib = capi.load(EMUL)
    old = api.KernelProvider._lib
    api.KernelProvider.initialize(0, _lib=lib)
    yield api
    api.KernelProvider._lib = old


N_BIG = 4096
REJ_CFGS = {  # 60-bit primes where about one word in 17 is rejected by uniform_below(p)
    "ckks_n4096_rej60": dict(scheme=CKKS, N=N_BIG, tbits=0, primes=E.rejecting_primes(N_BIG, 3)),
    "bgv_n4096_rej60": dict(scheme=BGV, N=N_BIG, tbits=20, primes=E.rejecting_primes(N_BIG, 3)),
    "bfv_n256_rej60": dict(scheme=BFV, N=256, tbits=20, primes=E.rejecting_primes(256, 3)),
}
NAMES = cases.SMALL + ["cfgA_bfv_n4096_k3", "ckks_n4096_k4", "bgv_n4096_k3"] + sorted(REJ_CFGS)
DEVICE_NAMES = ["bfv_n128_k4", "ckks_n128_k6", "bgv_n128_k4", "bfv_n256_rej60"]


def params_of(name, api):
    cfg = REJ_CFGS.get(name) or cases.CONFIGS[name]
    N = cfg["N"]
    primes = cfg.get("primes") or api.CoeffModulus.Create(N, cfg["bits"])
    t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
    return cfg["scheme"], N, [int(p) for p in primes], t


def seed_of(name):
    return SEEDS[NAMES.index(name) % len(SEEDS)]


def scale_of(S):
    return S.t if S.scheme == BGV else 1


# ------------------------------------------------------------------ 1. the model against the RFC, recorded words and openssl
RFC_STATE = list(M.SIGMA) + [int.from_bytes(bytes(range(4 * i, 4 * i + 4)), "little") for i in range(8)] + [1, 0x09000000, 0x4A000000, 0]
RFC_BLOCK = "e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2"


def test_model_rfc8439_block():
    """RFC 8439 2.3.2: key 00 .. 1f, block counter 1, nonce 00000009 0000004a 00000000"""
    block = M.chacha20_blocks(RFC_STATE, RFC_STATE[12] | (RFC_STATE[13] << 32), 1)[0]
    assert " ".join("%08x" % w for w in block) == RFC_BLOCK


def test_model_stream_words():
    hexes = lambda w: " ".join("%016x" % int(x) for x in w)
    assert hexes(M.Stream(0x5EED, 7, 0).take(4)) == "0a57fa64c5c3615f 4b46c76648f3d0ae 2d153da87f4815a0 d80cfabdb6d08373"
    assert hexes(M.Stream(0x5EED, 7, 3 << 32).take(2)) == "c944f0764b8e1c92 22b87780b2a4f6e7"
    S = M.Stream(0x5EED, 7, 0)  # a stream grown in pieces is the stream grown at once
    pieces = np.concatenate([S.take(3), S.take(700), S.take(5000)])
    assert np.array_equal(pieces, M.Stream(0x5EED, 7, 0).take(5703))


def test_model_against_openssl():
    """64 blocks of the stream of SEEDS[2] against `openssl enc -chacha20` over zeros (its 16-byte IV is words 12 .. 15: counter, then nonce)"""
    if not shutil.which("openssl"):
        pytest.skip("no openssl on this machine")
    st = M.stream_state(*SEEDS[2], 5 << 32)
    pack = lambda words: b"".join(int(w).to_bytes(4, "little") for w in words).hex()
    out = subprocess.run(["openssl", "enc", "-chacha20", "-K", pack(st[4:12]), "-iv", pack(st[12:16])], input=bytes(64 * 64), capture_output=True, check=True).stdout
    assert out == M.chacha20_blocks(st, 0, 64).astype("<u4").tobytes()


def test_model_uniform_below_is_the_scalar_rule():
    """the vectorised rejection (accept mask, the first n accepted) against the rule word by word, at a bound that rejects one word in 17"""
    p = E.rejecting_primes(256, 1)[0]
    S = M.Stream(3, 4, 5)
    got = np.concatenate([S.uniform_below(p, 1000), S.uniform_below(3, 10), S.uniform_below(p, 1)])
    words = [int(w) for w in M.Stream(3, 4, 5).take(S.pos)]
    exp, k, rejected = [], 0, 0
    for bound, n in ((p, 1000), (3, 10), (p, 1)):
        limit = M.M64 - (M.M64 % bound + 1) % bound
        have = 0
        while have < n:
            r, k = words[k], k + 1
            if r > limit:
                rejected += 1
                continue
            exp.append(r % bound)
            have += 1
    assert k == S.pos and rejected == S.rejected and rejected > 30
    assert [int(v) for v in got] == exp


# ------------------------------------------------------------------ 2. every form against the model
def check_kswitch_key(S, key, stream_id, src, seed=None):
    """c1 of every digit and limb is the model's uniform draw; the recovered noise of every digit is the model's CBD vector in every limb.
    Returns the model's (a, e, stream)"""
    N, K, P = S.N, S.K, S.primes
    a, e, st = M.kswitch_key(*(seed or S.seed), stream_id, N, P)
    assert np.array_equal(key[:, 1], a)
    for j in range(K - 1):
        for l in range(K):
            assert np.array_equal(M.unscale(M.key_noise(key, S.sk, src, j, l, P, N), scale_of(S)), e[j]), (j, l)
    return a, e, st


def sources(S, s):
    """the source polynomials of a relin key and of Galois keys, from the model's secret s: s^2 and sigma_elt(s), NTT form [K][N]"""
    sn = M.lifted_ntt(s, S.N, S.primes)
    return np.stack([M.mulmod(sn[l], sn[l], p) for l, p in enumerate(S.primes)]), lambda elt: M.lifted_ntt(M.galois_coeffs(s, elt), S.N, S.primes)


def check_secret_and_public_key(S, seed, sk, pk):
    N, P = S.N, S.primes
    s, a, e, st = M.keygen(*seed, N, P)
    assert np.array_equal(M.centred(M.ntt(N, P[0], sk[0], inverse=True), P[0]), s)
    assert np.array_equal(sk, M.lifted_ntt(s, N, P))  # every limb is the same vector lifted
    if pk is not None:
        assert np.array_equal(pk[1], a)
        for l, p in enumerate(P):
            assert np.array_equal(M.unscale(M.noise_of(pk[0, l], pk[1, l], sk[l], p, N), scale_of(S)), e), l
    return s, st


@pytest.mark.parametrize("name", NAMES)
def test_keys_match_model(name, emul_api):
    """secret key, public key, relin key, Galois keys (3, 2N - 1 and the automorphism N + 1) and a key-switching key of the host forms"""
    scheme, N, primes, t = params_of(name, emul_api)
    S = G.Setup(scheme, N, primes, t, seed=seed_of(name))
    s, st = check_secret_and_public_key(S, S.seed, *S.host_keygen(S.seed))
    assert np.array_equal(S.sk, M.lifted_ntt(s, N, primes))  # KeyGenerator(seed) holds the same key
    s2, sigma = sources(S, s)
    rejected = st.rejected + check_kswitch_key(S, S.host_relin(), M.RELIN, s2)[2].rejected
    for elt in (3, 2 * N - 1, N + 1):
        rejected += check_kswitch_key(S, S.host_galois(elt), M.galois_stream(elt), sigma(elt))[2].rejected
    new_key = emul_api.KeyGenerator(S.ctx, seed=(99, 1)).secretKey()
    check_kswitch_key(S, S.host_kswitch(new_key), M.KSWITCH, new_key)
    if name in REJ_CFGS:  # the positions of these draws depend on the rejections before them
        assert rejected > 0.5 * 4 * (S.K - 1) * N * sum(E.rejection_rate(p) for p in primes), rejected


def check_symmetric(S, form, ct, seed, a_seed, limbs, plain):
    N, P = S.N, S.primes
    zero = form.endswith("0")
    if form.startswith("sks"):
        a, e = M.symmetric_seeded(*seed, a_seed, N, P[:limbs], zero)
        rejected = 0
    else:
        a, e, st = M.symmetric(*seed, N, P[:limbs], zero)
        rejected = st.rejected
    assert np.array_equal(ct[1], M.stored_uniform(S.scheme, a, P, N)), form
    for l in range(limbs):
        assert np.array_equal(M.symmetric_noise(S.scheme, ct, S.sk, l, limbs, P, S.t, N, plain), e), (form, l)
    return rejected


@pytest.mark.parametrize("name", NAMES)
def test_symmetric_forms_match_model(name, emul_api):
    """symmetric, zero-symmetric, both seeded forms and expand_seed: c1 and the recovered e, at every data level of CKKS, else at the first"""
    scheme, N, primes, t = params_of(name, emul_api)
    S = E.Setup(scheme, N, primes, t)
    seed, rng, rejected = seed_of(name), np.random.default_rng(5), 0
    for limbs in (S.data_levels() if scheme == CKKS else [S.ctx.first_limbs]):
        plain = S.plains(1, limbs, rng)[0]
        a_seed = (0xA5EED0000000001 * limbs) & M.M64
        for form in ("sk", "sk0", "sks", "sks0"):
            pl = None if form.endswith("0") else plain
            rejected += check_symmetric(S, form, S.host(form, seed, limbs, pl, a_seed), seed, a_seed, limbs, pl)
        assert np.array_equal(S.expand_host(a_seed, limbs), M.stored_uniform(scheme, M.expand_seed(a_seed, N, primes[:limbs]), primes, N))
    if name in REJ_CFGS:
        assert rejected > 0.5 * 2 * N * sum(E.rejection_rate(p) for p in primes[:S.ctx.first_limbs]), rejected


@pytest.mark.parametrize("name", NAMES)
def test_public_key_encryption_matches_model(name, emul_api):
    """The division by the extra prime rounds, so the expected ciphertext is built forward from the model's (u, e0, e1): products in NTT form through
    the oracle's NTT, the division through Oracle.rns_stage (pinned to the reference by test_oracle_golden.py); every byte, zero form and with a plaintext"""
    scheme, N, primes, t = params_of(name, emul_api)
    S = E.Setup(scheme, N, primes, t)
    O = oracle.Oracle(scheme, N, primes, t)
    seed, rng = seed_of(name), np.random.default_rng(6)
    for limbs in S.data_levels():
        exp = M.public_key_ciphertext(O, scheme, S.pk, *seed, limbs, primes, t, N)
        assert np.array_equal(S.host("pk0", seed, limbs), exp), ("pk0", limbs)
        if scheme == CKKS or limbs == S.ctx.first_limbs:
            plain = S.plains(1, limbs, rng)[0]
            exp = M.public_key_ciphertext(O, scheme, S.pk, *seed, limbs, primes, t, N, plain)
            assert np.array_equal(S.host("pk", seed, limbs, plain), exp), ("pk", limbs)


@pytest.mark.parametrize("name", DEVICE_NAMES)
def test_device_keygen_matches_model(name, emul_api):
    """troyhip_keygen at B = 3: the count / scan / scatter samplers against the model, not against their host sibling"""
    scheme, N, primes, t = params_of(name, emul_api)
    S = G.Setup(scheme, N, primes, t)
    sk, pk = S.device_keygen(np.array(SEEDS, dtype=np.uint64))
    for b, seed in enumerate(SEEDS):
        check_secret_and_public_key(S, seed, sk[b], pk[b])


@pytest.mark.parametrize("name", DEVICE_NAMES)
def test_device_galois_keys_match_model(name, emul_api):
    """troyhip_create_galois_keys with three elements in one call"""
    scheme, N, primes, t = params_of(name, emul_api)
    S = G.Setup(scheme, N, primes, t, seed=seed_of(name))
    s = M.keygen(*S.seed, N, primes)[0]
    sigma = sources(S, s)[1]
    elts = [3, 2 * N - 1, N + 1]
    for elt, buf in zip(elts, S.device_galois(elts)):
        check_kswitch_key(S, buf.to_numpy().reshape(S.ksk_shape()), M.galois_stream(elt), sigma(elt))


@pytest.mark.parametrize("name", DEVICE_NAMES)
def test_device_symmetric_matches_model(name, emul_api):
    """troyhip_encrypt_symmetric at B = 3 with per-item seeds, unseeded and seeded"""
    scheme, N, primes, t = params_of(name, emul_api)
    S = E.Setup(scheme, N, primes, t)
    limbs, seeds = S.ctx.first_limbs, np.array(SEEDS, dtype=np.uint64)
    plains = S.plains(3, limbs, np.random.default_rng(8))
    a_seeds = np.array([0xFEDCBA9876543210, 1, 0x8000000000000000], dtype=np.uint64)
    scale = 2.0**20 if scheme == CKKS else 1.0
    for form, a in (("sk", None), ("sks", a_seeds)):
        dev, _ = S.device(form, seeds, limbs, plains, True, a, scale=scale)
        for b in range(3):
            check_symmetric(S, form, dev[b], SEEDS[b], None if a is None else int(a[b]), limbs, plains[b])


# ------------------------------------------------------------------ 3. the distributions
N_POOL, K_POOL = N_BIG, 17  # a relin key of 16 digits: 2^16 pooled noise coefficients, 2^16 uniform residues per limb
CBD_PMF = np.array([comb(42, k + 21) for k in range(-21, 22)], dtype=float) / 2.0**42
_pool = {}


def relin_pool(scheme, api, primes=None):
    """(Setup, a [K-1][K][N], e [K-1][N]) of one relin key, seed SEEDS[0], proved equal to the model: c1 everywhere, the noise in limbs 0 and K - 1"""
    key = (scheme, None if primes is None else tuple(primes))
    if key not in _pool:
        P = [int(p) for p in (primes or api.CoeffModulus.Create(N_POOL, [30] * K_POOL))]
        S = G.Setup(scheme, N_POOL, P, 0 if scheme == CKKS else api.PlainModulus.Batching(N_POOL, 20), seed=SEEDS[0])
        rk = S.host_relin()
        a, e, st = M.kswitch_key(*S.seed, M.RELIN, N_POOL, P)
        assert np.array_equal(rk[:, 1], a)
        s2 = np.stack([M.mulmod(S.sk[l], S.sk[l], p) for l, p in enumerate(P)])
        for j in range(S.K - 1):
            for l in (0, S.K - 1):
                assert np.array_equal(M.unscale(M.key_noise(rk, S.sk, s2, j, l, P, N_POOL), scale_of(S)), e[j]), (j, l)
        _pool[key] = (S, a, e, st)
    return _pool[key]


def cbd_chisquare(e):
    """chi-square of a pool of CBD draws against C(42, k + 21) / 2^42, the tails pooled until every expected count is at least 5 -> (cells, p)"""
    e = np.asarray(e).reshape(-1)
    obs = np.array([(e == k).sum() for k in range(-21, 22)], dtype=float)
    exp = CBD_PMF * e.size
    lo = 0
    while exp[:lo + 1].sum() < 5:
        lo += 1
    hi = 42 - lo  # the pmf is symmetric
    o = np.concatenate([[obs[:lo + 1].sum()], obs[lo + 1:hi], [obs[hi:].sum()]])
    x = np.concatenate([[exp[:lo + 1].sum()], exp[lo + 1:hi], [exp[hi:].sum()]])
    assert x.min() >= 5 and o.sum() == e.size
    return len(o), stats.chisquare(o, x).pvalue


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_cbd_distribution(scheme, emul_api):
    """The noise of all 16 digits of one relin key at N = 4096 (2^16 coefficients) is Binomial(42, 1/2) - 21.
    The model alone, seed (0x5EED, 7): p = 0.957 over 25 cells and variance 10.428, for BFV and for BGV (the same stream; the noise enters as t e).
    The variance bound: the sample variance of n draws has standard error sqrt((mu4 - sigma^4) / n) with mu4 = sigma^4 (3 - 2 / 42), 0.0573 at n = 2^16; a two-sided normal tail of 1e-6, the level of the chi-square, is 4.9 standard errors: |variance - 10.5| <= 0.281."""
    S, a, e, st = relin_pool(scheme, emul_api)
    assert e.size >= 2**16 and np.abs(e).max() <= 21
    cells, p = cbd_chisquare(e)
    var = e.reshape(-1).astype(float).var()
    print("CBD scheme %d: %d cells, p = %.4f, variance %.4f, mean %.4f" % (scheme, cells, p, var, e.mean()))
    assert p >= P_MIN
    se = np.sqrt(10.5**2 * (2 - 2 / 42) / e.size)
    assert abs(var - 10.5) <= 4.9 * se


def test_ternary_distribution(emul_api):
    """the three counts of 8 secret keys of distinct seeds at N = 4096 against N / 3 each.  The model alone, seeds (0x5EED + i, 7 + i): p = 0.146"""
    scheme, N, primes, t = params_of("cfgA_bfv_n4096_k3", emul_api)
    S = G.Setup(scheme, N, primes, t)
    pool = []
    for i in range(8):
        seed = (0x5EED + i, 7 + i)
        pool.append(check_secret_and_public_key(S, seed, S.host_keygen(seed, with_pk=False)[0], None)[0])
    pool = np.concatenate(pool)
    counts = [(pool == v).sum() for v in (-1, 0, 1)]
    p = stats.chisquare(counts).pvalue
    print("ternary counts", counts, "p = %.4f" % p)
    assert sum(counts) == 8 * N and p >= P_MIN


def bucket_pvalue(v, p, buckets):
    """chi-square of residues v over `buckets` equal-width buckets of [0, p): bucket k is [ceil(k p / buckets), ceil((k + 1) p / buckets))"""
    edges = np.array([-(-k * p // buckets) for k in range(1, buckets)], dtype=np.uint64)
    counts = np.bincount(np.searchsorted(edges, v, side="right"), minlength=buckets)
    widths = np.diff(np.array([0] + [int(x) for x in edges] + [p], dtype=object)).astype(float)
    return stats.chisquare(counts, widths / p * v.size).pvalue, counts


def test_uniform_distribution(emul_api):
    """c1 of a 16-digit relin key, limb by limb: 2^16 residues, each below p, flat over 64 equal-width buckets.  The model alone: the smallest p of
    the 17 limbs is 0.135"""
    S, a, e, st = relin_pool(BFV, emul_api)
    worst = 1.0
    for l, p in enumerate(S.primes):
        v = a[:, l].reshape(-1)
        assert v.size >= 2**16 and int(v.max()) < p
        worst = min(worst, bucket_pvalue(v, p, 64)[0])
    print("uniform: smallest p over %d limbs %.4f" % (S.K, worst))
    assert worst >= P_MIN


def test_uniform_distribution_rejecting_primes(emul_api):
    """60-bit primes just above 2^64 / 17, where one word in 17 is rejected: 4 digits x 4096 residues per limb over 17 and over 64 buckets.  The
    model alone: the smallest p is 0.080 (17 buckets) and 0.085 (64 buckets); it rejected 5128 words.
    These primes leave 2^64 mod p within 3e-12 p of p itself, so a sampler WITHOUT the rejection would still be flat to this test's eye (every residue
    but the top few would be hit 17 times in 2^64 instead of 16): what a dropped rejection moves is the position of every later draw, and that is
    what the pins of part 2 catch at these primes."""
    S, a, e, st = relin_pool(CKKS, emul_api, primes=E.rejecting_primes(N_POOL, 5))
    assert st.rejected > 0.5 * (S.K - 1) * N_POOL * sum(E.rejection_rate(p) for p in S.primes), st.rejected
    worst = {17: 1.0, 64: 1.0}
    for l, p in enumerate(S.primes):
        v = a[:, l].reshape(-1)
        assert int(v.max()) < p
        for buckets in worst:
            worst[buckets] = min(worst[buckets], bucket_pvalue(v, p, buckets)[0])
    print("uniform, rejecting primes: smallest p", worst, "rejected words", st.rejected)
    assert min(worst.values()) >= P_MIN


def assert_independent(vectors, what):
    """no two of the vectors are equal, and the sample correlation of any two stays within 6 / sqrt(N)"""
    V = np.stack([np.asarray(v, dtype=float) for v in vectors])
    assert len({v.tobytes() for v in V}) == len(V), what
    c = np.corrcoef(V) - np.eye(len(V))
    assert np.abs(c).max() <= 6 / np.sqrt(V.shape[1]), (what, np.abs(c).max())


def test_noise_is_independent(emul_api):
    """across the digits of one key, the keys of one Galois call, the items of one batch and e0 / e1 of one encryption"""
    S, a, e, st = relin_pool(BFV, emul_api)
    assert_independent(e, "digits of a relin key")
    scheme, N, primes, t = params_of("bgv_n4096_k3", emul_api)
    Sg = G.Setup(scheme, N, primes, t)
    sigma = sources(Sg, M.keygen(*Sg.seed, N, primes)[0])[1]
    noise = []
    for elt in (3, 2 * N - 1, N + 1, 9):
        noise += list(check_kswitch_key(Sg, Sg.host_galois(elt), M.galois_stream(elt), sigma(elt))[1])
    assert_independent(noise, "keys and digits of one Galois set")
    scheme, N, primes, t = params_of("bfv_n256_rej60", emul_api)
    Se = E.Setup(scheme, N, primes, t)
    limbs, B = Se.ctx.first_limbs, 9
    seeds = E.seeds_for(B)
    dev, _ = Se.device("sk0", seeds, limbs)
    noise = []
    for b in range(B):
        check_symmetric(Se, "sk0", dev[b], [int(x) for x in seeds[b]], None, limbs, None)
        noise.append(M.symmetric(int(seeds[b][0]), int(seeds[b][1]), N, primes[:limbs], True)[1])
    assert_independent(noise, "items of one batch")
    # (u, e0, e1) of the encryptions that test_public_key_encryption_matches_model builds forward at this shape and seed
    name = "cfgA_bfv_n4096_k3"
    assert_independent(M.pk_encrypt(*seed_of(name), N_BIG, zero=True) + M.pk_encrypt(*seed_of(name), N_BIG), "u, e0, e1 of two encryptions")


# ------------------------------------------------------------------ 4. no two calls share stream words
def _c1_ntt(S, c1_limb0):
    return c1_limb0 if S.scheme == CKKS else M.ntt(S.N, S.primes[0], c1_limb0)


class Collector:
    """every uniform polynomial that leaves an object (limb 0, NTT form) and every recovered noise vector (with the secret key)"""

    def __init__(self, S, sk):
        self.S, self.sk, self.uniform, self.noise = S, sk, [], []
        self.noise.append(("secret key", M.centred(M.ntt(S.N, S.primes[0], sk[0], inverse=True), S.primes[0])))

    def key(self, tag, key, src):
        for j in range(self.S.K - 1):
            self.uniform.append(("%s digit %d" % (tag, j), key[j, 1, 0]))
            self.noise.append(("%s digit %d" % (tag, j), M.key_noise(key, self.sk, src, j, 0, self.S.primes, self.S.N)))

    def ct(self, tag, ct, symmetric, plain=None):
        S = self.S
        ct = np.asarray(ct)
        self.uniform.append((tag, _c1_ntt(S, ct[1, 0])))
        if symmetric:
            e = M.symmetric_noise(S.scheme, ct, self.sk, 0, ct.shape[1], S.primes, S.t, S.N, plain)
            assert e is not None and np.abs(e).max() <= 21, tag
            self.noise.append((tag, e))

    def check(self):
        for what, items in (("uniform", self.uniform), ("noise", self.noise)):
            seen = {}
            for tag, v in items:
                other = seen.setdefault(np.ascontiguousarray(v).tobytes(), tag)
                assert other == tag, "%s polynomial of '%s' is that of '%s'" % (what, tag, other)


def device_items(ct):
    return ct.cpu()


@pytest.mark.parametrize("name", ["bfv_n128_k4", "ckks_n128_k6", "bgv_n128_k4"])
def test_no_two_calls_share_stream_words(name, emul_api):
    """One seeded KeyGenerator and one seeded Encryptor issue every form they offer, in a mixed order, twice.  No two uniform polynomials and no
    two noise vectors that leave them are equal.  The one exception is documented: relin and Galois keys are functions of (seed, secret key,
    element) alone, so a repeated call returns the same key -- harmless, since it encrypts the same message each time; the test asserts that
    equality and counts such a key once.  Two createKeySwitchingKeys calls share nothing, whatever their arguments."""
    api = emul_api
    scheme, N, primes, t = params_of(name, api)
    S = G.Setup(scheme, N, primes, t, seed=(0xFFFFFFFFFFFFFFFE, 3))  # lo + call number wraps
    kg, sk = S.kg, S.sk
    k1, k2 = api.KeyGenerator(S.ctx, seed=(3, 4)).secretKey(), api.KeyGenerator(S.ctx, seed=(4, 3)).secretKey()
    enc = api.Encryptor(S.ctx, kg.createPublicKey(), seed=(77, 1))
    enc.setSecretKey(sk)
    limbs = S.ctx.first_limbs
    ES = E.Setup(scheme, N, primes, t)  # its plains() only
    rng = np.random.default_rng(11)
    s2, sigma = sources(S, M.keygen(*S.seed, N, primes)[0])
    scale = 2.0**20 if scheme == CKKS else 1.0
    host = lambda k: k.keys[0].to_numpy().reshape(S.ksk_shape()) if hasattr(k, "keys") else k
    elts = [3, 2 * N - 1]
    col = Collector(S, sk)
    first = {}
    for rnd in range(2):
        r = "round %d " % rnd
        keys = {"relin": (kg.createRelinKeys(device=bool(rnd)), s2)}
        gk = kg.createGaloisKeys(elts, device=bool(rnd))
        ak = kg.createAutomorphismKeys(device=not rnd)
        for e in elts + kg.automorphismElts():
            got = (gk if e in elts else ak)
            got = got[e] if isinstance(got, dict) else got.keys[api.GaloisKeys.getIndex(e)].to_numpy().reshape(S.ksk_shape())
            keys["galois %d" % e] = (got, sigma(e))
        for tag, (key, src) in keys.items():
            key = host(key)
            if rnd == 0:
                first[tag] = key
                col.key(tag, key, src)
            else:  # documented as deterministic: the same key again, host or device
                assert np.array_equal(key, first[tag]), tag
        col.key(r + "kswitch k1", host(kg.createKeySwitchingKeys(k1)), k1)
        col.key(r + "kswitch k2 (device)", host(kg.createKeySwitchingKeys(k2, device=True)), k2)
        col.key(r + "kswitch k1 again", host(kg.createKeySwitchingKeys(k1, device=bool(rnd))), k1)
        p = ES.plains(6, limbs, rng)
        col.ct(r + "encrypt", enc.encrypt(p[0]), False)
        for i, c in enumerate(device_items(enc.encryptBatch(p[1:3], scale))):
            col.ct(r + "encryptBatch %d" % i, c, False)
        col.ct(r + "encryptSymmetric", enc.encryptSymmetric(p[3]), True, p[3])
        for i, c in enumerate(device_items(enc.encryptSymmetricBatch(p[3:6], scale))):  # item 0 repeats the plaintext of the single call
            col.ct(r + "encryptSymmetricBatch %d" % i, c, True, p[3 + i])
        col.ct(r + "encryptZero", enc.encryptZero(), False)
        for i, c in enumerate(device_items(enc.encryptZeroBatch(2))):
            col.ct(r + "encryptZeroBatch %d" % i, c, False)
        col.ct(r + "encryptZeroSymmetric", enc.encryptZeroSymmetric(), True)
        for i, c in enumerate(device_items(enc.encryptZeroSymmetricBatch(3))):
            col.ct(r + "encryptZeroSymmetricBatch %d" % i, c, True)
        col.ct(r + "encrypt after the batches", enc.encrypt(p[0]), False)
        col.ct(r + "encryptSymmetric after the batches", enc.encryptSymmetric(p[3]), True, p[3])
    assert len(col.uniform) > 60 and len(col.noise) > 40
    col.check()


@pytest.mark.parametrize("name", ["bfv_n128_k4", "ckks_n128_k6", "bgv_n128_k4"])
def test_kswitch_calls_consume_their_own_seeds(name, emul_api):
    """call number k of createKeySwitchingKeys (host and device forms counted together) is the model's key of the seed (lo + k, hi) on stream
    5 << 32, whatever new_key is; the device form is the host form of the same call number"""
    api = emul_api
    scheme, N, primes, t = params_of(name, api)
    lo, hi = 0xFFFFFFFFFFFFFFFF, 5
    S = G.Setup(scheme, N, primes, t, seed=(lo, hi))
    twin = api.KeyGenerator(S.ctx, seed=(lo, hi))
    k1, k2 = api.KeyGenerator(S.ctx, seed=(3, 4)).secretKey(), api.KeyGenerator(S.ctx, seed=(4, 3)).secretKey()
    for call, (new_key, device) in enumerate(((k1, False), (k2, True), (k1, True), (k2, False))):
        key = S.kg.createKeySwitchingKeys(new_key, device=device)
        key = key.keys[0].to_numpy().reshape(S.ksk_shape()) if device else key
        check_kswitch_key(S, key, M.KSWITCH, new_key, seed=((lo + call) & M.M64, hi))
        other = twin.createKeySwitchingKeys(new_key, device=not device)
        assert np.array_equal(key, other if device else other.keys[0].to_numpy().reshape(S.ksk_shape()))


@pytest.mark.parametrize("name", ["bfv_n128_k4", "ckks_n128_k6", "bgv_n128_k4"])
def test_unseeded_generator_two_new_keys(name, emul_api):
    """the default path: a KeyGenerator seeded by the operating system, two new_keys -- nothing shared, and (c0 - c0') / (q_special mod p_j) is
    not new_key - new_key'"""
    api = emul_api
    scheme, N, primes, t = params_of(name, api)
    ctx = api.SEALContext(scheme, N, primes, t)
    kg = api.KeyGenerator(ctx)
    k1, k2 = api.KeyGenerator(ctx, seed=(3, 4)).secretKey(), api.KeyGenerator(ctx, seed=(4, 3)).secretKey()
    S = G.Setup(scheme, N, primes, t)
    col = Collector(S, kg.secretKey())
    A, B = kg.createKeySwitchingKeys(k1), kg.createKeySwitchingKeys(k2)
    col.key("k1", A, k1)
    col.key("k2", B, k2)
    col.key("k1, device", kg.createKeySwitchingKeys(k1, device=True).keys[0].to_numpy().reshape(S.ksk_shape()), k1)
    col.check()
    for tag, e in col.noise[1:]:
        assert M.unscale(e, scale_of(S)) is not None and np.abs(M.unscale(e, scale_of(S))).max() <= 21, tag
    K = len(primes)
    for j in range(K - 1):
        p = primes[j]
        finv = pow(primes[K - 1] % p, -1, p)
        leak = (A[j, 0, j].astype(object) - B[j, 0, j].astype(object)) * finv % p
        assert not np.array_equal(leak, (k1[j].astype(object) - k2[j].astype(object)) % p), j
        assert not any(np.array_equal(A[j, 0, l], B[j, 0, l]) for l in range(K))


def test_symmetric_calls_consume_their_own_seeds(emul_api):
    """At ONE call seed the seeded and the unseeded symmetric form read the same words of stream 4 << 32: the seeded call's noise is the CBD of
    the words whose residues the unseeded call publishes as c1 (shown here on the model, which both forms are pinned to).  The Encryptor never
    gives two calls one seed: call number k of ANY form takes (lo + k, hi), single calls and batch items alike"""
    api = emul_api
    scheme, N, primes, t = params_of("ckks_n128_k6", api)
    limbs = 2
    a, _, st = M.symmetric(9, 9, N, primes[:limbs])
    e = M.symmetric_seeded(9, 9, 1234, N, primes[:limbs])[1]
    words = M.Stream(9, 9, M.SYM).take(N)
    assert st.rejected == 0 and np.array_equal(words % np.uint64(primes[0]), a[0])  # c1 of the unseeded form publishes w mod p ...
    assert np.array_equal(M._popcount21(words) - M._popcount21(words >> np.uint64(21)), e)  # ... of the very words the seeded form's noise is made of
    S = E.Setup(scheme, N, primes, t)
    lo, hi = 0xFFFFFFFFFFFFFFFD, 2
    enc = api.Encryptor(S.ctx, S.pk, seed=(lo, hi))
    enc.setSecretKey(S.sk)
    rng = np.random.default_rng(3)
    p = S.plains(4, limbs, rng)
    call = 0
    for step in range(2):
        got = [("sk", enc.encryptSymmetric(p[0]), p[0]), ("pk", enc.encrypt(p[1]), p[1])]
        got += [("sk", c, p[2 + i]) for i, c in enumerate(enc.encryptSymmetricBatch(p[2:4], 2.0**20).cpu())]
        got += [("sk0", enc.encryptZeroSymmetric(limbs), None), ("pk0", enc.encryptZero(limbs), None)]
        got += [("sk0", c, None) for c in enc.encryptZeroSymmetricBatch(2, limbs).cpu()]
        for form, ct, plain in got:
            call += 1
            seed = ((lo + call) & M.M64, hi)
            assert np.array_equal(ct, S.host(form, seed, limbs, plain)), (step, call, form)
            if form.startswith("sk"):
                check_symmetric(S, form, np.asarray(ct), seed, None, limbs, plain)
    assert enc.counter == call == 16
