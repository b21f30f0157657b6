"""Exact model of the lazy-range device primitives (bfly.h, fpmod.h, the key-switch fold) and the probes that hold the device to it.

Python integers only.  Every primitive is checked at the BOUND of its stated range, for residue and for range: the probe ops from 20 on
(troy_amd/csrc/selftest.hip) return the raw words a primitive left in its registers.  For the integer forms the model also restates the
documented quotient estimates (q~ = y1 q1 + floor((y1 q0 + y0 q1) / 2^32), the 32-bit estimates of lite_reduce / lean_final4), so the expected
words are exact; the contract (residue, range, the relations between the two outputs) is asserted on its own, from the device's words alone.
For the FP64 forms no rounding is replicated: the contract of fpmod.h is checked -- the result is an integer-valued double, congruent to the
exact product or sum, within the bound written next to the function.

tests/test_gpu_lazy.py runs check_* on the MI355X, tests/test_device_lazy.py on the emulator build (the plain-C forms) and tests the model itself.

One deviation from a literal reading of the comments: ct_bfly4_ng's second output is X + 3p - v with v in [0, 3p), so it REACHES X + 3p when
v = 0 (twiddle 0 or Y = 0, both in the lists).  bfly.h states the bound on bound(X), a strict bound of X: Y' <= X + 3p < bound(X) + 3p, and that
is what is asserted (X' < X + 3p strictly).

A second one: bfly.h writes "bound(X), bound(Y) <= kp / p" over gs_bfly4_last_ng.  The arithmetic spends kp on Y alone (X + kp - Y must not go below
zero; X enters only through X + kp < 2^64 and X + Y < 2^64), and inv_stages_lean (ntt1.hip) hands the _k forms kp[i] = p bound(Y's register) while X's
register may carry a larger bound.  The precondition held here is therefore the one the callers keep -- Y <= kp, X + kp < 2^64, X + Y < 2^64 -- and
the inputs include X above kp on purpose."""
import ctypes as C
import functools
import struct

import numpy as np

M = 1 << 64
M32 = (1 << 32) - 1

# ------------------------------------------------------------------ primes and their classes
# (prime, bit length, which side of which power of two): found on the CPU, p = 1 mod 2^14
PRIMES = [
    (8590163969, 34, "above", 33), (17179754497, 34, "below", 34), (17179967489, 35, "above", 34),
    (1125899906826241, 50, "below", 50), (1125899906990081, 51, "above", 50),
    (144115188075593729, 57, "below", 57), (144115188076167169, 58, "above", 57),
    (288230376150876161, 58, "below", 58), (288230376151760897, 59, "above", 58),
    (1152921504606830593, 60, "below", 60), (2305843009213317121, 61, "below", 61),
]
INT_PRIMES = [p for p, _, _, _ in PRIMES]
FP_PRIMES = [(8590163969, 34), (1099511480321, 40), (562949952847873, 49), (562949954093057, 50), (1125899906826241, 50)]


def is_prime(n):
    """Miller-Rabin, deterministic below 3.3 10^24 with the first twelve primes as bases"""
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for q in small:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:
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


def assert_int_prime_class(p):
    (bits, side, k), = [(b, s, k) for q, b, s, k in PRIMES if q == p]
    assert p.bit_length() == bits and is_prime(p) and p % (1 << 14) == 1
    assert 0 < ((1 << k) - p if side == "below" else p - (1 << k)) < 1 << 21, "the prime sits at its class edge"
    assert (1 << 33) <= p < (1 << 61)


def assert_fp_prime_class(p):
    (bits,), = [(b,) for q, b in FP_PRIMES if q == p]
    assert p.bit_length() == bits and is_prime(p) and p % (1 << 14) == 1 and p < (1 << 50)


def is_lean(p):
    return (1 << 33) <= p < (1 << 58)


# ------------------------------------------------------------------ the integer primitives, exactly
def shoup(w, p):
    return (w << 64) // p


def mulhi_approx(y, wq):
    """bfly.h: floor(y wq / 2^64) - {0, 1}, the low x low partial product dropped"""
    y0, y1, q0, q1 = y & M32, y >> 32, wq & M32, wq >> 32
    r = y1 * q1 + ((y1 * q0 + y0 * q1) >> 32)
    assert 0 <= (y * wq >> 64) - r <= 1
    return r


def lazy_mul(y, w, p, exact=False):
    """w y - q p for any 64-bit y and w < p: in [0, 3p) with the approximate quotient, in [0, 2p) with the exact one"""
    assert 0 <= y < M and 0 <= w < p
    q = (y * shoup(w, p)) >> 64 if exact else mulhi_approx(y, shoup(w, p))
    v = w * y - q * p
    assert 0 <= v < (2 if exact else 3) * p
    return v


def csub(x, m):
    return x - m if x >= m else x


def lite_reduce(x, p):
    assert p >= 1 << 33 and 0 <= x < M
    mu = (M // p) & M32
    assert mu == M // p
    return x - (((x >> 32) * mu) >> 32) * p


def lean_final(x, p):
    assert is_lean(p) and 0 <= x < 64 * p
    b = p.bit_length()
    sh, mu = b - 26, (M // p) >> (58 - b)
    assert x >> sh < 1 << 32
    return csub(x - ((((x >> sh) & M32) * mu) >> 32) * p, p)


def fold(lo, hi, p):
    """ks_fold4: (the value before the final step, the stored word)"""
    assert p >= 1 << 33
    r64 = M % p
    pre = lite_reduce(lo, p) + lazy_mul(hi, r64, p)
    word = lean_final(pre, p) if is_lean(p) else csub(csub(csub(pre, 4 * p), 2 * p), p)
    return pre, word


# butterfly ops: op -> (form, UNI, kp: None / "one" / "each", EXACT)
BFLY = {
    20: ("ct", 0, None, 0), 24: ("ct", 1, None, 0), 21: ("ct_ng", 0, None, 0), 25: ("ct_ng", 1, None, 0),
    22: ("gs", 0, None, 0), 27: ("gs", 1, None, 0), 23: ("gs_last", 0, None, 0), 28: ("gs_last", 1, None, 0),
    26: ("gs_ng", 0, "one", 0), 31: ("gs_ng", 1, "one", 0), 32: ("gs_ng", 0, "each", 0), 33: ("gs_ng", 1, "each", 0),
    29: ("gs_last_ng", 0, "one", 0), 30: ("gs_last_ng", 1, "one", 0),
    34: ("gs_last_ng", 0, "each", 0), 35: ("gs_last_ng", 1, "each", 0), 36: ("gs_last_ng", 0, "each", 1), 37: ("gs_last_ng", 1, "each", 1),
}
RAW_OF_CANONICAL = {6: 20, 7: 21, 8: 22, 9: 23, 11: 24, 12: 25, 13: 26}  # the existing canonical ops and their raw twins
NAMES = {op: "%s%s%s%s" % (f, "<UNI>" if u else "", "_k" if k == "each" else "", "<EXACT>" if e else "") for op, (f, u, k, e) in BFLY.items()}


def bfly_precondition(form, X, Y, w, ninv, kp, p):
    """what the caller owes the butterfly (bfly.h): no probe input may break it"""
    assert 0 <= w < p and 0 <= ninv < p and 0 <= X < M and 0 <= Y < M
    if form == "ct":
        assert X < 8 * p and Y < 8 * p
    elif form == "ct_ng":
        assert X + 3 * p < M
    elif form in ("gs", "gs_last"):
        assert X < 4 * p and Y < 4 * p
    else:
        assert kp % p == 0 and Y <= kp and X + kp < M and X + Y < M


def bfly_exact(form, exact, X, Y, w, ninv, kp, p):
    """the words the documented formulas leave"""
    if form == "ct":
        u = csub(X, 4 * p)
        v = lazy_mul(Y, w, p)
        return u + v, u + 3 * p - v
    if form == "ct_ng":
        v = lazy_mul(Y, w, p)
        return X + v, X + 3 * p - v
    if form == "gs":
        return csub(X + Y, 4 * p), lazy_mul(X + 4 * p - Y, w, p)
    if form == "gs_last":
        return lazy_mul(csub(X + Y, 4 * p), ninv, p), lazy_mul(X + 4 * p - Y, w, p)
    if form == "gs_ng":
        return X + Y, lazy_mul(X + kp - Y, w, p)
    assert form == "gs_last_ng"
    return lazy_mul(X + Y, ninv, p, exact), lazy_mul(X + kp - Y, w, p, exact)


def bfly_contract(form, exact, X, Y, w, ninv, kp, p, gx, gy):
    """residue and RANGE of the device's raw words (gx, gy), from bfly.h / ntt1.hip / ntt2.hip"""
    if form == "ct":
        assert gx < 7 * p and gy < 8 * p, "ct_bfly4: outputs < 8p, X' < 7p"
        assert gx % p == (X + w * Y) % p and gy % p == (X - w * Y) % p
    elif form == "ct_ng":
        v = gx - X
        assert 0 <= v < 3 * p and v % p == w * Y % p, "ct_bfly4_ng: X' = X + v, v in [0, 3p)"
        assert gy == X + 3 * p - v and gy <= X + 3 * p, "ct_bfly4_ng: Y' = X + 3p - v"
        assert max(gx, gy) < (X // p + 1 + 3) * p, "both outputs < bound(X) + 3p"
    elif form == "gs":
        assert gx < 4 * p and gy < 3 * p, "gs_bfly4: X' < 4p, Y' < 3p"
        assert gx % p == (X + Y) % p and gy % p == (X - Y) * w % p
    elif form == "gs_last":
        assert gx < 3 * p and gy < 3 * p, "gs_bfly4_last: both < 3p"
        assert gx % p == (X + Y) * ninv % p and gy % p == (X - Y) * w % p
    elif form == "gs_ng":
        assert gx == X + Y, "gs_bfly4_ng: X' = X + Y exactly"
        assert gy < 3 * p and gy % p == (X - Y) * w % p, "gs_bfly4_ng: Y' < 3p"
    else:
        lim = (2 if exact else 3) * p
        assert gx < lim and gy < lim, "gs_bfly4_last_ng: both < 3p, EXACT: both < 2p"
        assert gx % p == (X + Y) * ninv % p and gy % p == (X - Y) * w % p


# ------------------------------------------------------------------ inputs: the smallest that can still go wrong
def cap_of(p):
    return (M - 1) // p


def high_words(p):
    """the quotient-estimate extremes of lite_reduce and mulhi_approx"""
    return [(h << 32) | l for h in (0xFFFFFFFF, 0xFFFFFFFE, p >> 32, (p >> 32) + 1) for l in (0, 0xFFFFFFFF)]


def edge_values(p, K, limit=None, any_word=False):
    """0, 1, kp - 1, kp, kp + 1 for every k up to the op's bound K, the high-word extremes, 2^64 - 1 where any word is accepted; all below
    `limit` (default K p, never above 2^64)"""
    limit = min(K * p if limit is None else limit, M)
    v = [0, 1] + [k * p + d for k in range(1, K + 1) for d in (-1, 0, 1)] + high_words(p) + [limit - 1]
    if any_word:
        v += [M - 1, M - 2]
        limit = M
    out = []
    for x in v:
        if 0 <= x < limit and x not in out:
            out.append(x)
    return out


def randoms(rng, n, limit):
    return [int(v) % limit for v in rng.integers(0, 1 << 63, n, dtype=np.uint64).astype(object) * 2 + rng.integers(0, 2, n).astype(object)]


def twiddles(p, rng, n_random=3):
    """0, 1, p - 1, p / 3, a twiddle whose Shoup quotient has an all-ones low word and one with an all-zero low word, random ones"""
    i32 = pow(1 << 32, -1, p)
    ones, zeros = (-i32) % p, i32 % p  # w 2^32 = -1 / +1 (mod p): floor(w 2^64 / p) ends in 32 ones / 32 zeros (p > 2^32)
    assert shoup(ones, p) & M32 == M32 and shoup(zeros, p) & M32 == 0 and zeros != 0
    return [0, 1, p - 1, p // 3, ones, zeros] + randoms(rng, n_random, p)


@functools.lru_cache(maxsize=None)
def lite_worst(p, keep=8):
    """words that push lite_reduce towards its bound: among the 4096 largest high words, those that leave the most (the truncations of mu and of the
    product both near 1), under an all-ones low word (up to 2^32 / p <= 1/2 more)"""
    hs = sorted(range((1 << 32) - 4096, 1 << 32), key=lambda h: -lite_reduce(h << 32, p))[:keep]
    return tuple((h << 32) | M32 for h in hs)


@functools.lru_cache(maxsize=None)
def mul_worst(p, w, keep=4, among=2000, limit=M):
    """operands below `limit` that leave the largest lazy product w y - q~ p (the approximate quotient one short: towards 3p).  With
    w 2^64 = wq p + e the exact quotient already leaves (w y mod p) + p where (w y mod p) < y e / 2^64, and the approximate one is one short again
    where the dropped partial products carry: 2p and more needs both, so it takes y near 2^64 -- below 64p a 34-bit prime has no such operand"""
    rng = np.random.default_rng(p % 1000003)
    return tuple(sorted(randoms(rng, among, limit), key=lambda y: -lazy_mul(y, w, p))[:keep])


GROUP = 256  # butterflies per workgroup of the probe: the UNI forms take one twiddle (and one kp) per workgroup


def bfly_inputs(op, p, seed=1):
    """(X, Y, w, kp, checked) grouped by twiddle, every group padded to whole workgroups (the padding repeats the group's last butterfly
    and is not asserted again).  Every edge value meets every twiddle on a core subset; every edge value of X and of Y appears; a few hundred
    random butterflies on top.  The gs*_ng forms take any X with X + kp < 2^64, so they also get, per twiddle, the differences X + kp - Y and
    (last stage) the sums X + Y that mul_worst finds over the whole 64-bit range: products of 2p and more under the approximate quotient, which the
    EXACT forms must bring below 2p -- at every prime, which values below 32p cannot do for the small ones."""
    form, _uni, kpmode, _exact = BFLY[op]
    rng = np.random.default_rng(seed * 1000 + op)
    cap = cap_of(p)
    if form == "ct":
        xs, ys = edge_values(p, 8), edge_values(p, 8)
        xlim = ylim = min(8 * p, M)
    elif form == "ct_ng":
        KX = min(61, cap - 3)
        xlim, ylim = min(KX * p, M - 3 * p), M
        xs, ys = edge_values(p, KX, xlim), edge_values(p, min(64, cap), any_word=True)
    elif form in ("gs", "gs_last"):
        xs, ys = edge_values(p, 4), edge_values(p, 4)
        xlim = ylim = 4 * p
    else:
        KY = min(30, (cap - 1) // 2)
        KX = min(32, cap - 1 - KY)
        xs, ys = edge_values(p, KX), edge_values(p, KY)
        xlim, ylim = KX * p, KY * p
    tws = twiddles(p, rng)
    core_x = [xs[0], xs[1], xs[2], xs[3], xs[len(xs) // 2], xs[-2], xs[-1]]
    core_y = [ys[0], ys[1], ys[2], ys[3], ys[len(ys) // 2], ys[-2], ys[-1]]
    groups = [[(x, y) for x in core_x for y in core_y] for _ in tws]
    for i, x in enumerate(xs):
        groups[i % len(tws)].append((x, ys[(5 * i + 3) % len(ys)]))
    for j, y in enumerate(ys):
        groups[(j + 2) % len(tws)].append((xs[(7 * j + 1) % len(xs)], y))
    rx, ry = randoms(rng, 240, xlim), randoms(rng, 240, ylim)
    for i, (x, y) in enumerate(zip(rx, ry)):
        groups[i % len(tws)].append((x, y))
    hunted = [[] for _ in tws]  # (X, Y, kp) with kp = KY p, the largest any Y of the case needs
    if kpmode is not None:
        for g, w in enumerate(tws):
            hunted[g] += [(d, KY * p, KY * p) for d in mul_worst(p, w, among=400, limit=M - KY * p)]  # X + kp - Y = d, X + kp < 2^64
            if form == "gs_last_ng":
                hunted[g] += [(s - min(s, KY * p), min(s, KY * p), KY * p) for s in mul_worst(p, scale_of(op, p), among=400)]  # X + Y = s
    X, Y, W, KP, checked = [], [], [], [], []
    for g, (w, pairs) in enumerate(zip(tws, groups)):
        kps = []
        for i, (x, y) in enumerate(pairs):
            if kpmode is None:
                kps.append(0)
            elif kpmode == "one":
                kps.append(KY * p)  # one kp per workgroup: a multiple of p that bounds every Y of the case
            else:  # one per butterfly, from 3p to 61p with X + kp < 2^64
                kps.append((max(3, y // p + 1), max(3, KY), max(3, min(61, cap - x // p - 1)))[(i + g) % 3] * p)
        pairs = pairs + [(x, y) for x, y, _ in hunted[g]]
        kps += [kp for _, _, kp in hunted[g]]
        pad = (-len(pairs)) % GROUP
        for i in range(len(pairs) + pad):
            x, y = pairs[min(i, len(pairs) - 1)]
            X.append(x); Y.append(y); W.append(w); KP.append(kps[min(i, len(pairs) - 1)])
            checked.append(i < len(pairs))
    return X, Y, W, KP, checked


# ------------------------------------------------------------------ the probe
class Probe:
    def __init__(self, api):
        from troy_amd import capi
        self.api, self.capi = api, capi
        self.lib = api.KernelProvider._lib if getattr(api.KernelProvider, "_lib", None) is not None else capi.load()
        self.launches = 0

    def call(self, op, a, b, c, p, n_out, aux=1, n=None):
        """the status of one launch and its output words"""
        bufs = [self.api.DeviceBuffer.from_numpy(np.array(v, dtype=np.uint64)) if v is not None else None for v in (a, b, c)]
        out = self.api.DeviceBuffer(max(n_out, 1))
        rc = self.lib.troyhip_test_modarith(op, *[C.c_void_p(x.ptr) if x is not None else None for x in bufs], C.c_uint64(p), C.c_uint64(aux),
                                            C.c_void_p(out.ptr), C.c_uint64(len(a) if n is None else n), None)
        self.launches += 1
        return rc, [int(v) for v in out.to_numpy()[:n_out]]

    def run(self, *args, **kw):
        rc, out = self.call(*args, **kw)
        self.capi.check(self.lib, rc)
        return out


def ninv_of(p):
    return pow(32768, -1, p)


@functools.lru_cache(maxsize=None)
def generic_scale(p):
    """the first of a seeded sequence of residues under which some 64-bit operands leave 2p and more with the approximate quotient"""
    rng = np.random.default_rng(p % 1000003 + 1)
    return next(w for w in randoms(rng, 64, p) if w and all(lazy_mul(y, w, p) >= 2 * p for y in mul_worst(p, w, among=400)))


def scale_of(op, p):
    """the last stage's scale (aux).  N^-1 of a power of two N has the Shoup quotient 2^64 - 2^64 / N + floor(2^64 / (N p)): its low word is (next to)
    zero, no partial product is dropped, and the approximate quotient of the sum is never one short -- under a bare N^-1 nothing can tell the EXACT
    form's first multiplication from the approximate one (small multiples and fractions of N^-1 are hardly better: where their quotient is one short,
    the exact product sits below p).  The EXACT ops therefore run under a generic residue, as a scale with other factors folded in is; every other
    last stage under N^-1"""
    return generic_scale(p) if BFLY[op][3] else ninv_of(p)


def check_bfly(P, op, p):
    """ONE launch of one butterfly form at one prime: every butterfly asserted for the exact words and, separately, residue and range"""
    assert_int_prime_class(p)
    form, _uni, _kp, exact = BFLY[op]
    X, Y, W, KP, checked = bfly_inputs(op, p)
    ninv = scale_of(op, p)
    for x, y, w, kp in zip(X, Y, W, KP):
        bfly_precondition(form, x, y, w, ninv, kp, p)
    n = len(X)
    assert n % GROUP == 0
    out = P.run(op, X, Y, W + KP, p, 2 * n, aux=ninv, n=n)
    worst = 0
    for restated in (False, True):  # the contract of every butterfly first, from the device's words alone; then the model's restated formulas
        for i in range(n):
            if not checked[i]:
                continue
            gx, gy = out[2 * i], out[2 * i + 1]
            where = (NAMES[op], p, i, X[i], Y[i], W[i], KP[i], gx, gy)
            if restated:
                assert (gx, gy) == tuple(v % M for v in bfly_exact(form, exact, X[i], Y[i], W[i], ninv, KP[i], p)), ("the exact words", where)
                continue
            try:
                bfly_contract(form, exact, X[i], Y[i], W[i], ninv, KP[i], p, gx, gy)
            except AssertionError as e:
                raise AssertionError("%s at %r" % (e, where)) from None
            worst = max(worst, gy / p)
    return sum(checked), worst


def check_canonical_twin(P, op, p):
    """the existing canonical op and its raw twin agree: barrett64 of the raw words is what ops 6 .. 13 return.  Both launches run the primitive
    inside its contract, so equal words are right words (the raw twin is held to the model by check_bfly): op 13 has kp = 8p built in, and where
    8p leaves less than 8p below 2^64 (the prime below 2^61: 2^64 - 8p = 3014648) X is brought under 2^64 - 8p"""
    assert_int_prime_class(p)
    raw = RAW_OF_CANONICAL[op]
    form = BFLY[raw][0]
    X, Y, W, KP, _ = bfly_inputs(raw, p)
    n = GROUP  # the last workgroup: one twiddle (ops 11 and 12 read c[0]), a random one
    X, Y, W = X[-n:], Y[-n:], W[-n:]
    assert len(set(W)) == 1 and W[0] > 1
    kp = [0] * n
    if op == 13:
        kp = [8 * p] * n
        X, Y = [x % min(8 * p, M - 8 * p) for x in X], [y % (8 * p) for y in Y]
    ninv = ninv_of(p)
    for x, y, w, k in zip(X, Y, W, kp):
        bfly_precondition(form, x, y, w, ninv, k, p)  # the same butterflies go to both launches
    got = P.run(op, X, Y, W, p, 2 * n, aux=ninv)
    twin = P.run(raw, X, Y, W + kp, p, 2 * n, aux=ninv, n=n)
    for i in range(n):
        bfly_contract(form, 0, X[i], Y[i], W[i], ninv, kp[i], p, twin[2 * i], twin[2 * i + 1])
    assert got == [v % p for v in twin], (op, p)


REDUCTIONS = {40: "lite_reduce4", 41: "lite_reduce1", 42: "lean_final4", 43: "reduce4_from_8p", 44: "reduce4_from_4p"}


def reduction_inputs(op, p, seed=2):
    rng = np.random.default_rng(seed * 1000 + op)
    cap = cap_of(p)
    if op in (40, 41):
        return edge_values(p, min(64, cap), any_word=True) + list(lite_worst(p)) + randoms(rng, 300, M)
    K = {42: 64, 43: 8, 44: 4}[op]
    return edge_values(p, K) + randoms(rng, 300, K * p)


def check_reduction(P, op, p):
    """-> (values asserted, the largest result in units of p)"""
    assert_int_prime_class(p)
    xs = reduction_inputs(op, p)
    if op == 42:
        assert is_lean(p) and all(x < 64 * p for x in xs)
    out = P.run(op, xs, None, None, p, len(xs))
    worst = 0.0
    for x, g in zip(xs, out):
        where = (REDUCTIONS[op], p, x, g)
        assert g % p == x % p, where
        if op in (40, 41):
            assert g < 4 * p and g == lite_reduce(x, p), where
            assert (x - g) % p == 0 and 0 <= x // p - (x - g) // p <= 2, ("the quotient estimate is at most 2.5 below x / p, never above", where)
        else:
            assert g == x % p, where  # canonical
        worst = max(worst, g / p)
    return len(xs), worst


def fold_inputs(p, seed=3):
    rng = np.random.default_rng(seed * 1000 + 45)
    his = [0, 1, p - 1, M - 1] + high_words(p) + randoms(rng, 8, M)
    los = [0, M - 1] + high_words(p) + [k * p + d for k in (1, 2, 3, cap_of(p)) for d in (-1, 0, 1)] + randoms(rng, 8, M)
    pairs = [(lo % M, hi) for hi in his for lo in los]
    pairs += [(lo, hi) for lo in lite_worst(p)[:4] for hi in mul_worst(p, M % p)]  # both parts of the sum towards their bounds
    pairs += list(zip(randoms(rng, 300, M), randoms(rng, 300, M)))
    return [a for a, _ in pairs], [b for _, b in pairs]


def check_fold(P, p):
    """-> (sums asserted, the largest lite_reduce part and the largest value before the final step, in units of p)"""
    assert_int_prime_class(p)
    lo, hi = fold_inputs(p)
    out = P.run(45, lo, hi, None, p, 2 * len(lo))
    worst = 0.0
    for i, (l, h) in enumerate(zip(lo, hi)):
        pre, word = out[2 * i], out[2 * i + 1]
        where = ("ks_fold4", p, l, h, pre, word)
        assert pre < M and 2 * pre < 13 * p, ("the value before the final step is below 6.5p", where)
        assert pre % p == ((h << 64) + l) % p and word == ((h << 64) + l) % p, where
        assert (pre, word) == fold(l, h, p), where
        worst = max(worst, pre / p)
    return len(lo), worst


def mac_inputs(p, seed=4):
    """four accumulators (term k goes to accumulator k % 4): 0 -- seven lazy products at the evaluator's bound; 1 -- (2^64 - 1)^2 and what still fits;
    2 -- carries out of every 32-bit column; 3 -- random"""
    rng = np.random.default_rng(seed * 1000 + 46)
    bound = 8 * p if p < (1 << 60) else p
    cols = [[(bound - 1, p - 1)] * 7 + [(0, 0)],
            [(M - 1, M - 1), (M - 1, 1), (M32, M32), (0, M - 1), (1, 1), (0, 0), (1, 0), (0, 1)],
            [(M32, M32), (M32 << 32, M32), (M32, M32 << 32), (M32 << 32, M32 << 31), (M - 1, M32), (M32, M - 1), ((1 << 32) + 1, M - 1), (M - 1, 1 << 32)],
            list(zip(randoms(rng, 8, min(8 * p, M)), randoms(rng, 8, p)))]
    a = [cols[k % 4][k // 4][0] for k in range(32)]
    b = [cols[k % 4][k // 4][1] for k in range(32)]
    return a, b


def check_mac(P, p):
    assert_int_prime_class(p)
    a, b = mac_inputs(p)
    exp = [sum(a[k] * b[k] for k in range(j, len(a), 4)) for j in range(4)]
    assert all(e < 1 << 128 for e in exp), "acc < 2^128 is the caller's bound"
    out = P.run(46, a, b, None, p, 8)
    assert [out[2 * j] | (out[2 * j + 1] << 64) for j in range(4)] == exp, ("mac128x4", p)
    return len(a)


# ------------------------------------------------------------------ FP64 forms: the contract of fpmod.h, no rounding replicated
L52, L53 = 1 << 52, 1 << 53


def bits_of(values):
    """exact integers |v| < 2^53 as the bit patterns of their doubles"""
    assert all(abs(v) < L53 for v in values)
    return [int(b) for b in np.array([float(v) for v in values], dtype=np.float64).view(np.uint64)]


def int_of(bits, where):
    d = struct.unpack("<d", struct.pack("<Q", bits))[0]
    assert d == d and abs(d) != float("inf") and d.is_integer(), ("an integer-valued double", where)
    return int(d)


def lifts(r, p, limit):
    """r + m p at m = 0, mid-range and the largest with |value| < limit, in both signs"""
    top = (limit - 1 - r) // p
    bot = (limit - 1 + r) // p
    return [r, r + (top // 2) * p, r + top * p, r - p, r - (bot // 2) * p, r - bot * p]


def fp_mul_inputs(p, seed=5):
    """(y, w): y w = (p +- 1) / 2, (p +- 3) / 2, 0, 1, p - 1 (mod p), lifted to 0, mid-range and the largest |y| < 2^52, both signs"""
    rng = np.random.default_rng(seed * 1000 + 51)
    ws = [1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, p // 3] + randoms(rng, 3, p - 1)
    ys, wl = [], []
    for w in ws:
        w = max(w, 1)
        iw = pow(w, -1, p)
        for r in ((p + 1) // 2, (p - 1) // 2, (p + 3) // 2, (p - 3) // 2, 0, 1, p - 1):
            for y in lifts(r * iw % p, p, L52):
                assert abs(y) < L52 and y * w % p == r
                ys.append(y); wl.append(w)
        for y in (L52 - 1, -(L52 - 1)):
            ys.append(y); wl.append(w)
    ry = randoms(rng, 300, 2 * L52 - 1)
    ys += [v - (L52 - 1) for v in ry]
    wl += randoms(rng, 300, p)
    return ys, wl


def check_fp_convert(P, p):
    assert_fp_prime_class(p)
    rng = np.random.default_rng(50)
    xs = [0, 1, p - 1, p, L52 - 1, L52 - 2, 1 << 51, (1 << 51) - 1, M32, 1 << 32] + randoms(rng, 200, L52)
    out = P.run(50, xs, None, None, p, 2 * len(xs))
    for i, x in enumerate(xs):
        assert int_of(out[2 * i], ("fp_from_u64", x)) == x and out[2 * i + 1] == x, ("fp_from_u64 / fp_to_u64", x, out[2 * i:2 * i + 2])
    return len(xs)


def check_fp_mulmod(P, op, p):
    """op 51 fp_mulmod_wp: |r| <= (1/2 + |y| 2^-52) p;  op 52 fp_mulmod_pinv: |r| <= (1/2 + 3 |y| 2^-53) p.  -> (points, the largest |r| / bound)"""
    assert_fp_prime_class(p)
    ys, ws = fp_mul_inputs(p)
    yb = bits_of(ys)
    out = P.run(51, yb, None, ws, p, len(ys)) if op == 51 else P.run(52, yb, bits_of(ws), None, p, len(ys))
    tight = 0.0
    for y, w, g in zip(ys, ws, out):
        where = ("fp_mulmod_wp" if op == 51 else "fp_mulmod_pinv", p, y, w, hex(g))
        r = int_of(g, where)
        assert (r - y * w) % p == 0, where
        # in exact integers: |r| 2^53 <= (2^52 + c |y|) p with c = 2 (wp: 1/2 + |y| 2^-52) or 3 (pinv: 1/2 + 3 |y| 2^-53)
        c = 2 if op == 51 else 3
        assert abs(r) * L53 <= (L52 + c * abs(y)) * p, where
        tight = max(tight, abs(r) * L53 / ((L52 + c * abs(y)) * p))
    return len(ys), tight


def fp_reduce_inputs(p, seed=6):
    rng = np.random.default_rng(seed * 1000 + 53)
    kmax = (L53 - 1) // p
    xs = [L53 - 1, -(L53 - 1)]
    for k in sorted({0, 1, 2, 3, kmax // 2, kmax - 1, kmax}):
        for d in (0, 1, (p - 1) // 2, (p + 1) // 2, p - 1):
            for s in (1, -1):
                if abs(k * p + d) < L53:
                    xs.append(s * (k * p + d))
    return xs + [v - (L53 - 1) for v in randoms(rng, 300, 2 * L53 - 1)]


def check_fp_reduce(P, p):
    """fp_reduce: |r| <= p / 2 + 2;  fp_canonical: x mod p exactly"""
    assert_fp_prime_class(p)
    xs = fp_reduce_inputs(p)
    xb = bits_of(xs)
    red, can = P.run(53, xb, None, None, p, len(xs)), P.run(54, xb, None, None, p, len(xs))
    for x, g, c in zip(xs, red, can):
        r = int_of(g, ("fp_reduce", p, x))
        assert (r - x) % p == 0 and 2 * abs(r) <= p + 4, ("fp_reduce", p, x, r)
        assert c == x % p, ("fp_canonical", p, x, c)
    return len(xs)


def check_fp_bfly(P, op, p):
    """the butterflies of fp_fwd_stages (55) and fp_inv_stages (56, 57 = LAST with N^-1), as ntt1.hip writes them"""
    assert_fp_prime_class(p)
    ys, ws = fp_mul_inputs(p, seed=7 + op)
    rng = np.random.default_rng(op)
    ninv = ninv_of(p)
    if op == 55:  # |Y| < 2^52; X + v below 2^53
        Y = ys
        X = [(0, 1, -1, L52, -L52, p - 1, 1 - p)[i % 7] if i % 3 == 0 else v - L52 for i, v in enumerate(randoms(rng, len(ys), 2 * L52 + 1))]
    else:  # the difference takes the constructed value, the sum stays below 2^52: X - Y = y, |X + Y| < 2^52
        X, Y = [], []
        for i, y in enumerate(ys):
            lim = L52 - 1 - abs(y)  # |2 Y| <= lim
            yy = (0, lim // 2, -(lim // 2))[i % 3] if i % 2 == 0 else int(rng.integers(0, lim + 1)) - lim // 2
            yy = max(-(lim // 2), min(lim // 2, yy))
            X.append(y + yy); Y.append(yy)
            assert abs(X[-1] + Y[-1]) < L52 and abs(X[-1] - Y[-1]) < L52
    out = P.run(op, bits_of(X), bits_of(Y), ws, p, 2 * len(X), aux=ninv)
    for i, (x, y, w) in enumerate(zip(X, Y, ws)):
        where = (op, p, x, y, w, hex(out[2 * i]), hex(out[2 * i + 1]))
        gx, gy = int_of(out[2 * i], where), int_of(out[2 * i + 1], where)
        if op == 55:
            v = gx - x
            assert (v - y * w) % p == 0 and abs(v) * L53 <= (L52 + 2 * abs(y)) * p and gy == x - v, where
        else:
            d = x - y
            assert (gy - d * w) % p == 0 and abs(gy) * L53 <= (L52 + 2 * abs(d)) * p, where
            if op == 56:
                assert gx == x + y, where
            else:
                assert (gx - (x + y) * ninv) % p == 0 and abs(gx) * L53 <= (L52 + 2 * abs(x + y)) * p, where
    return len(X)


# ------------------------------------------------------------------ refusals: no primitive runs outside its class
def check_refusals(P):
    INV = P.capi.INVALID_ARGUMENT
    p = INT_PRIMES[0]
    one = [1, 1, 1, 1]
    for op in (14, 19, 38, 39, 47, 49, 58, 100, -1):
        assert P.call(op, one, one, one + one, p, 8)[0] == INV, ("unknown op", op)
    wide, fp_edge = 288230376151760897, 1125899906990081  # just above 2^58, just above 2^50
    below33 = next(q for q in range((1 << 33) - 1, 0, -2) if is_prime(q))  # lite_reduce, lean_final4 and the fold start at 2^33
    for op in (40, 41, 42, 45):
        assert P.call(op, one, one, None, below33, 8)[0] == INV, ("p < 2^33", op)
    assert P.call(42, one, None, None, wide, 4)[0] == INV, "lean_final4 with p >= 2^58"
    assert P.call(42, one, None, None, 288230376150876161, 4)[0] == P.capi.OK
    for op in range(50, 58):
        assert P.call(op, one, one, one, fp_edge, 8)[0] == INV, ("an FP64 op with p >= 2^50", op)
    assert P.call(46, one + [1], one + [1], None, p, 8)[0] == INV, "mac128x4 takes terms in fours"
    assert P.call(20, one, None, one + one, p, 8)[0] == INV and P.call(20, one, one, None, p, 8)[0] == INV, "missing buffers"
    assert P.call(0, one, None, None, 1 << 61, 4)[0] == INV
