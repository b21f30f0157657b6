"""The reference for the library's randomness: a plain numpy restatement of the sampler specification of DESIGN.md 4.6 / 4.8 and of the ChaCha20
block function of RFC 8439.  It shares no code with the library (hostcrypto.cpp, sampler.hip): the tests of test_sampler_model.py, test_gpu_keygen.py
and test_gpu_encrypt.py recover the draws from the library's keys and ciphertexts with exact arithmetic and compare them with this model.

A Stream is the sequence of 64-bit words of one (seed, stream id); every draw advances one shared position.  One function per form returns the raw
draws in the order the form consumes them: ternary and CBD values as int64 in [-1, 1] / [-21, 21], uniform residues as uint64 [limbs][N]."""
import numpy as np

M64 = (1 << 64) - 1
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"

# stream ids
KEYGEN, RELIN = 0, 1
KSWITCH, PK, SYM, PK_ZERO, SYM_ZERO, A_SEED = 5 << 32, 3 << 32, 4 << 32, 6 << 32, 7 << 32, 9 << 32


def galois_stream(elt):
    return (2 << 32) | int(elt)


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def chacha20_blocks(state, first, count):
    """RFC 8439 2.3: `state` is 16 words, of which words 12 / 13 are replaced by the low / high half of the 64-bit block counter first .. first + count - 1
    (the RFC's own layout is the case of a counter below 2^32 with word 13 as the first nonce word) -> uint32 [count][16]"""
    init = np.empty((16, count), dtype=np.uint32)
    init[:] = np.array([int(w) for w in state], dtype=np.uint32)[:, None]
    ctr = np.uint64(first) + np.arange(count, dtype=np.uint64)
    init[12] = (ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    init[13] = (ctr >> np.uint64(32)).astype(np.uint32)
    x = init.copy()

    def quarter(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            quarter(0, 4, 8, 12); quarter(1, 5, 9, 13); quarter(2, 6, 10, 14); quarter(3, 7, 11, 15)
            quarter(0, 5, 10, 15); quarter(1, 6, 11, 12); quarter(2, 7, 8, 13); quarter(3, 4, 9, 14)
        x += init
    return np.ascontiguousarray(x.T)


def stream_state(lo, hi, stream_id):
    lo, hi, stream_id = int(lo) & M64, int(hi) & M64, int(stream_id) & M64
    words = list(SIGMA)
    for k in (lo, hi, lo ^ 0x9E3779B97F4A7C15, hi ^ 0xD1B54A32D192ED03):
        words += [k & 0xFFFFFFFF, k >> 32]
    return words + [0, 0, 0x74726F79 ^ (stream_id & 0xFFFFFFFF), 0x68697031 ^ (stream_id >> 32)]


def _popcount21(v):
    """popcount of the low 21 bits of every uint64 of v"""
    b = (v & np.uint64(0x1FFFFF)).astype("<u4").view(np.uint8).reshape(-1, 4)
    return np.unpackbits(b, axis=1).sum(axis=1).astype(np.int64)


class Stream:
    def __init__(self, lo, hi, stream_id):
        self.state = stream_state(lo, hi, stream_id)
        self.words = np.zeros(0, dtype=np.uint64)  # words 0 .. len - 1 of the stream, grown on demand
        self.pos, self.rejected = 0, 0

    def _upto(self, end):
        have = len(self.words)
        if end > have:
            first = have // 8
            blocks = max((end + 7) // 8 - first, first, 64)
            u = chacha20_blocks(self.state, first, blocks).reshape(-1).astype(np.uint64)
            self.words = np.concatenate([self.words, (u[0::2] << np.uint64(32)) | u[1::2]])

    def take(self, n):
        self._upto(self.pos + n)
        w = self.words[self.pos:self.pos + n]
        self.pos += n
        return w

    def uniform_below(self, bound, n):
        bound = int(bound)
        limit = np.uint64(M64 - (M64 % bound + 1) % bound)
        start, want = self.pos, n + 64
        while True:
            self._upto(start + want)
            ok = self.words[start:start + want] <= limit
            rank = np.cumsum(ok)
            if rank[-1] >= n:
                break
            want *= 2
        used = int(np.searchsorted(rank, n)) + 1 if n else 0  # the words up to and including the n-th accepted one
        w = self.words[start:start + used][ok[:used]]
        self.pos, self.rejected = start + used, self.rejected + used - n
        return w % np.uint64(bound)

    def ternary(self, n):
        return self.uniform_below(3, n).astype(np.int64) - 1

    def cbd(self, n):
        w = self.take(n)
        return _popcount21(w) - _popcount21(w >> np.uint64(21))

    def uniform_limbs(self, primes, n):
        return np.stack([self.uniform_below(p, n) for p in primes])


# ---- the forms.  `primes` are the primes the form draws residues for: the K key primes for keys, the level's primes for a symmetric ciphertext
def keygen(lo, hi, N, primes):
    """-> (s ternary [N], a uniform [K][N], e CBD [N], the stream)"""
    S = Stream(lo, hi, KEYGEN)
    return S.ternary(N), S.uniform_limbs(primes, N), S.cbd(N), S


def kswitch_key(lo, hi, stream_id, N, primes):
    """a key-switching key of K - 1 digits on one running stream -> (a [K-1][K][N], e [K-1][N], the stream)"""
    S = Stream(lo, hi, stream_id)
    a, e = [], []
    for _ in range(len(primes) - 1):
        a.append(S.uniform_limbs(primes, N))
        e.append(S.cbd(N))
    return np.stack(a), np.stack(e), S


def pk_encrypt(lo, hi, N, zero=False):
    """-> (u ternary, e0, e1)"""
    S = Stream(lo, hi, PK_ZERO if zero else PK)
    return S.ternary(N), S.cbd(N), S.cbd(N)


def symmetric(lo, hi, N, primes, zero=False):
    """-> (a [limbs][N], e [N], the stream)"""
    S = Stream(lo, hi, SYM_ZERO if zero else SYM)
    return S.uniform_limbs(primes, N), S.cbd(N), S


def expand_seed(a_seed, N, primes):
    return Stream(a_seed, 0, A_SEED).uniform_limbs(primes, N)


def symmetric_seeded(lo, hi, a_seed, N, primes, zero=False):
    """-> (a [limbs][N] from the public seed's stream, e [N] from word 0 of the call's own stream)"""
    return expand_seed(a_seed, N, primes), Stream(lo, hi, SYM_ZERO if zero else SYM).cbd(N)


# ---- recovering draws from the library's keys and ciphertexts: Python integers and the oracle's NTT, nothing of the library under test
def ntt(N, p, v, inverse=False):
    from oracle import oracle
    return oracle.ntt_standalone(N, int(p), np.ascontiguousarray(v, dtype=np.uint64), 3 if inverse else 1)


def lift(x, p):
    """signed integers -> residues mod p"""
    return np.array(np.asarray(x).astype(object) % int(p), dtype=np.uint64)


def centred(v, p):
    """residues mod p -> the representatives in (-p/2, p/2] as int64"""
    v, p = np.asarray(v).astype(object), int(p)
    return np.array([x - p if x > p // 2 else x for x in v], dtype=np.int64)


def mulmod(a, b, p):
    return np.array(np.asarray(a).astype(object) * np.asarray(b).astype(object) % int(p), dtype=np.uint64)


def lifted_ntt(x, N, primes):
    """signed coefficients -> [limbs][N] NTT form"""
    return np.stack([ntt(N, p, lift(x, p)) for p in primes])


def galois_coeffs(x, elt):
    """X -> X^elt on a signed coefficient vector"""
    N, out = len(x), np.zeros(len(x), dtype=np.int64)
    for i, v in enumerate(x):
        k = i * int(elt) % (2 * N)
        out[k - N if k >= N else k] = -v if k >= N else v
    return out


def noise_of(c0, c1, s, p, N, extra=None, ntt_form=True):
    """the centred coefficients of -(c0 + c1 s) + extra mod p; c0 / c1 in NTT form or (ntt_form=False) coefficient form; s and extra in NTT form"""
    if not ntt_form:
        c0, c1 = ntt(N, p, c0), ntt(N, p, c1)
    v = -(np.asarray(c0).astype(object) + np.asarray(c1).astype(object) * np.asarray(s).astype(object))
    if extra is not None:
        v = v + np.asarray(extra).astype(object)
    return centred(ntt(N, p, np.array(v % int(p), dtype=np.uint64), inverse=True), p)


def key_noise(key, sk, src, j, l, primes, N):
    """digit j, limb l of a key-switching key [K-1][2][K][N] under sk [K][N], whose source polynomial is src [K][N] (NTT form): e * e_scale, centred"""
    p = int(primes[l])
    extra = mulmod(src[l], int(primes[-1]) % p, p) if l == j else None
    return noise_of(key[j, 0, l], key[j, 1, l], sk[l], p, N, extra)


def unscale(e, scale):
    """e / scale where every coefficient is a multiple of scale (BGV: the noise enters as t e); else None"""
    e = np.asarray(e)
    return e // scale if not (e % scale).any() else None


def message_term(scheme, plain, l, limbs, primes, t, N):
    """what a fresh ciphertext of `plain` adds to limb l of c0, in the form the ciphertext is stored in: CKKS (scheme 2) the plaintext's own residues
    (NTT form); BGV (3) the coefficients m; BFV (1) round(q m / t), ties up, q the product of the level's primes (coefficient form)"""
    p = int(primes[l])
    if scheme == 2:
        return np.ascontiguousarray(plain[l], dtype=np.uint64)
    m = np.zeros(N, dtype=object)
    if scheme == 3:
        m[:len(plain)] = [int(v) for v in plain]
    else:
        q = 1
        for x in primes[:limbs]:
            q *= int(x)
        m[:len(plain)] = [(q * int(v) + (t + 1) // 2) // t for v in plain]
    return np.array(m % p, dtype=np.uint64)


def symmetric_noise(scheme, ct, sk, l, limbs, primes, t, N, plain=None):
    """e of limb l of a symmetric ciphertext [2][limbs][N] under sk (NTT form): -(c0 + c1 s) + message, centred, divided by t for BGV (None unless exact)"""
    p, ntt_form = int(primes[l]), scheme == 2
    extra = None
    if plain is not None:
        extra = message_term(scheme, plain, l, limbs, primes, t, N)
        extra = extra if ntt_form else ntt(N, p, extra)
    return unscale(noise_of(ct[0, l], ct[1, l], sk[l], p, N, extra, ntt_form=ntt_form), t if scheme == 3 else 1)


def stored_uniform(scheme, a, primes, N):
    """the model's uniform draw a [limbs][N] as a ciphertext stores it in c1: as drawn for CKKS, inverse-transformed for BFV / BGV"""
    return a if scheme == 2 else np.stack([ntt(N, p, a[l], inverse=True) for l, p in enumerate(primes[:len(a)])])


def public_key_ciphertext(O, scheme, pk, lo, hi, limbs, primes, t, N, plain=None):
    """the ciphertext [2][limbs][N] a public-key encryption must produce from the model's (u, e0, e1): u pk_j + e_j (t e_j for BGV) over the limbs + 1
    primes of the level above, the oracle's division by that level's last prime (O: an oracle.Oracle of the context), then the message"""
    from oracle import oracle
    el = limbs + 1
    u, e0, e1 = pk_encrypt(lo, hi, N, zero=plain is None)
    un = lifted_ntt(u, N, primes[:el])
    stage = {1: oracle.ST_DIVROUND_QLAST, 2: oracle.ST_DIVROUND_QLAST_NTT, 3: oracle.ST_MODT_DIV_QLAST}[scheme]
    polys = []
    for j, e in enumerate((e0, e1)):
        rows = []
        for l in range(el):
            p = int(primes[l])
            prod = mulmod(un[l], pk[j, l], p)
            if scheme == 2:
                r = prod.astype(object) + ntt(N, p, lift(e, p)).astype(object)
            else:
                r = ntt(N, p, prod, inverse=True).astype(object) + lift(e.astype(object) * (t if scheme == 3 else 1), p).astype(object)
            rows.append(np.array(r % p, dtype=np.uint64))
        polys.append(O.rns_stage(el, stage, np.stack(rows), el)[:limbs])
    ct = np.stack(polys)
    if plain is not None:
        for l in range(limbs):
            m = message_term(scheme, plain, l, limbs, primes, t, N)
            ct[0, l] = np.array((ct[0, l].astype(object) + m.astype(object)) % int(primes[l]), dtype=np.uint64)
    return ct
