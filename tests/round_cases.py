"""Shared checks of the divide-and-round steps on crafted rounding boundaries: the division by the last prime (troyhip_mod_switch_to_next of BFV and
BGV, troyhip_rescale_to_next of CKKS), the second half of the key switch (Evaluator::ks_acc_to_ct through troyhip_relinearize and
troyhip_relinearize_to) and the last step of decryption (troyhip_decrypt of BFV and BGV).
Used by tests/test_device_round.py (emulator build) and tests/test_gpu_round.py (MI355X).

Uniform residues meet none of the equalities these steps compare on (x_last + half == q_last, x_j == [t']_{q_j}, a lazy sum that is a multiple of p,
x_last mod t == 0, ...): each has probability 2^-30 or less per coefficient.  Here the inputs are BUILT so that a chosen integer sits at a chosen
coefficient, as tests/noise_cases.py does for the noise budget.  Every case has three parts:
  * a builder: seeded uniform residues with the boundary values written over seeded positions;
  * an exact model of the step in Python integers, restating the reference's formulas as hoist_cases.model_item does, held once per distinct item
    against the oracle (so the model and the reference cannot drift apart); it returns its intermediates;
  * a hit report (Hits): every named boundary is looked up in the model's intermediates OF THE BUILT INPUT, per polynomial and per data prime.  A
    boundary that no coefficient shows is a miss and fails the case, unless the parameter set cannot reach it: then the builder says why, and the
    case has to name it (`cannot`), so that nothing is dropped silently.
All comparisons are bit-exact, and every result is held canonical (below its prime)."""
import math

import numpy as np

import cases
import hoist_cases as HC
from oracle import oracle
from oracle import ref as R
from troy_amd import synth
from troy_amd.capi import BFV, BGV, CKKS

obj = HC.obj
W64 = 1 << 64


def u64(a):
    return np.asarray(a, dtype=object).astype(np.uint64)


def spots(N, count, seed):
    """`count` distinct positions of a row of N, seeded; the first and the last coefficient are always among them"""
    assert 2 <= count <= N, (count, N)
    rest = np.random.default_rng(seed).permutation(np.arange(1, N - 1))[:count - 2]
    return [0, N - 1] + [int(n) for n in rest]


class Hits:
    """the hit report of one case: boundary name -> met by at least one coefficient; names the parameter set cannot reach -> why"""

    def __init__(self):
        self.seen, self.unreachable = {}, {}

    def look(self, name, mask):
        self.seen[name] = self.seen.get(name, False) or bool(np.any(mask))

    def cannot(self, name, why):
        self.unreachable[name] = why

    def merge(self, prefix, other):
        for n, ok in other.seen.items():
            self.seen[prefix + n] = ok
        for n, why in other.unreachable.items():
            self.unreachable[n] = why  # without the polynomial: what a parameter set cannot reach, no polynomial of it can

    def misses(self):
        return sorted(n for n, ok in self.seen.items() if not ok)

    def check(self, cannot=(), what=""):
        """every boundary occurs, and what cannot is exactly what the case names"""
        assert not self.misses(), (what, "boundaries no coefficient meets", self.misses())
        assert sorted(self.unreachable) == sorted(cannot), (what, "unreachable here", self.unreachable, "the case names", sorted(cannot))
        assert self.seen and all(self.seen.values())
        return len(self.seen)


class Setup:
    """one parameter set on both sides: the library through cases.GpuBackend, the oracle through cases.oracle_backend"""

    def __init__(self, scheme, N, bits, tbits=None, name=None, primes=None):
        self.name, self.cfg = (name, cases.CONFIGS[name]) if name else HC.adhoc(scheme, N, bits, tbits)
        cfg = self.cfg
        if primes:  # an explicit list where CoeffModulus.Create does not give what the case needs
            cfg["primes"] = [int(p) for p in primes]
        self.scheme, self.N = cfg["scheme"], cfg["N"]
        self.be, self.orc = cases.GpuBackend(cfg), cases.oracle_backend(cfg)
        self.api, self.ctx, self.ev = self.be.api, self.be.ctx, self.be.ev
        self.primes = [int(p) for p in self.be.primes]
        assert self.primes == [int(p) for p in self.orc.primes] and [p.bit_length() for p in self.primes] == list(cfg["bits"])
        self.t, self.K, self.ntt = int(self.be.t), len(self.primes), self.scheme == CKKS

    def ct(self, data, cap=None, cf=1):
        return self.api.Ciphertext.from_numpy(self.ctx, data, self.ntt, 1.0, cf, capacity=cap)

    def canonical(self, got, limbs):
        return all((got[..., j, :] < np.uint64(self.primes[j])).all() for j in range(limbs))


def named(name):
    return Setup(None, None, None, name=name)


class Kernels:
    """the kernels the calls inside the block launch, name -> calls (troyhip_ktime_enable / troyhip_ktime_report: the names the launches carry, template
    arguments included).  The path counters cannot tell a fused epilogue from the element-wise form around a plain transform where both make one
    single-pass launch per prime class; the names can.  The emulator build records none: there `calls` stays empty and `on` is false"""

    def __init__(self, S):
        self.lib, self.calls, self.on = S.ctx.lib, {}, False

    def _report(self):
        import ctypes as C
        import json
        from troy_amd import capi
        buf = C.create_string_buffer(1 << 16)
        capi.check(self.lib, self.lib.troyhip_ktime_report(buf, C.c_size_t(len(buf))))
        return json.loads(buf.value.decode())

    def __enter__(self):
        from troy_amd import capi
        self._report()  # drops what was recorded before
        capi.check(self.lib, self.lib.troyhip_ktime_enable(1))
        return self

    def __exit__(self, *exc):
        from troy_amd import capi
        capi.check(self.lib, self.lib.troyhip_stream_synchronize(None))
        for k in self._report():
            self.calls[k["name"].strip()] = self.calls.get(k["name"].strip(), 0) + k["calls"]
        capi.check(self.lib, self.lib.troyhip_ktime_enable(0))
        self.on = bool(self.calls)


def calls_of(kernels, part):
    """launches of the kernels whose name contains `part`"""
    return sum(n for name, n in kernels.items() if part in name)


def epilogue_calls(kernels, direction):
    """launches of the single-pass kernels of `direction` ("fwd": the correction form Ntt1Corr, N = 2^15 only; "inv": the mod-down Ntt1ModDown) whose
    epilogue argument, the last one, is true: ntt1_fwd_kernel<LEAN, EP>, ntt1_fwd_fp_kernel<EP>, ntt1_inv_kernel<LEAN, EP>, ntt1_inv_fp_kernel<EP>,
    ntt1s_inv_kernel<LOGN, LEAN, EP>, ntt1s_inv_fp_kernel<LOGN, EP> (the small rings' forward kernels have no epilogue: their last argument is LEAN)"""
    import re
    pat = {"fwd": r"ntt1_fwd(_fp)?_kernel<(\w+, )?true>", "inv": r"ntt1_inv(_fp)?_kernel<(\w+, )?true>|ntt1s_inv_kernel<\d+, \w+, true>|ntt1s_inv_fp_kernel<\d+, true>"}[direction]
    return sum(n for name, n in kernels.items() if re.search(pat, name))


def prime_one_mod(bits, modulus):
    """the largest prime below 2^bits that is 1 modulo `modulus`"""
    q = ((1 << bits) - 2) // modulus * modulus + 1
    while not cases._is_prime(q):
        q -= modulus
    assert q.bit_length() == bits
    return q


def bgv_one_mod_t(N=4096, tbits=20):
    """BGV over [36 bits, q_1 of 50 bits, qk of 60 bits] with q_1 = qk = 1 (mod t): q_last^-1 mod t is 1 for the mod-switch, which drops q_1, and for the
    key switch, which divides by qk, so both kernels skip their multiplication by it and k_t = -x_last mod t goes on as negmod left it.  With any other
    inverse that multiplication reduces modulo t once more, and a k_t of t in place of 0 (x_last mod t = 0) would pass unseen"""
    from troy_amd import api
    t = int(api.PlainModulus.Batching(N, tbits))
    primes = [int(api.CoeffModulus.Create(N, [36])[0]), prime_one_mod(50, 2 * N * t), prime_one_mod(60, 2 * N * t)]
    S = Setup(BGV, N, [36, 50, 60], tbits, primes=primes)
    assert S.t == t and primes[1] % t == 1 and primes[2] % t == 1
    return S


# ---------------------------------------------------------------- the last-limb values both divisions are built on
TPRIME = ("p_j-1", "p_j", "p_j+1", "2p_j", "mp_j-1", "mp_j")  # mp_j: the largest multiple of p_j below the divisor


def last_targets(S, qd, data_primes, what):
    """the values the divided limb takes, qd = 2h + 1 the divisor: -> ([(name, x_last, key, value)], Hits with what qd cannot reach).  (key, value): where
    the hit report finds the boundary among the model's intermediates; entries whose x_last is None add no coefficient, they are met through another's.
      0, 1, h - 1, h, h + 1 (x_last + h wraps first), h + 2, qd - 2, qd - 1
      per data prime p_j: t' = (x_last + h) mod qd one of TPRIME (BGV has no t': x_last itself takes these values, where [x_last]_{p_j} wraps)
      BGV: x_last = t - 1, t, t + 1, and mt - 1, mt, mt + 1 around the largest multiple mt of t below qd: x_last mod t = 0, 1, t - 1, k_t = 0"""
    h = qd >> 1
    bgv = S.scheme == BGV
    out, H = [], Hits()
    for nm, v in (("0", 0), ("1", 1), ("h-1", h - 1), ("h", h), ("h+1", h + 1), ("h+2", h + 2), ("q-2", qd - 2), ("q-1", qd - 1)):
        out.append(("%s=%s" % (what, nm), v, "last", v))
    key = "last" if bgv else "t'"
    for j, p in enumerate(data_primes):
        m = (qd - 1) // p * p
        for nm, T in zip(TPRIME, (p - 1, p, p + 1, 2 * p, m - 1, m)):
            name = "p%d: %s=%s" % (j, what if bgv else "t'", nm)
            if 0 < T < qd:
                out.append((name, T if bgv else (T - h) % qd, key, T))
            else:
                H.cannot(name, "no such value below the divisor %d" % qd)
    if bgv:
        t = S.t
        mt = (qd - 1) // t * t
        for nm, v in (("t-1", t - 1), ("t", t), ("t+1", t + 1), ("mt-1", mt - 1), ("mt", mt), ("mt+1", mt + 1)):
            if v < qd:
                out.append(("%s=%s" % (what, nm), v, "last", v))
            else:
                H.cannot("%s=%s" % (what, nm), "not below the divisor")
        for nm, v in (("0", 0), ("1", 1), ("t-1", t - 1)):
            out.append(("%s mod t=%s" % (what, nm), None, "last mod t", v))
        out.append(("k_t=0", None, "k_t", 0))
    return out, H


def multiples(what, *js):
    """the names of the TPRIME boundaries of the data primes `js`: what a divisor below p_j cannot reach"""
    return ["p%d: %s=%s" % (j, what, v) for j in js for v in TPRIME]


def look_all(H, targets, I):
    for name, _, key, val in targets:
        H.look(name, I[key] == val)


# ================================================================ part 1: the division by the last prime
def divide_model(S, x):
    """one polynomial x [L][N] (CKKS: NTT form) -> (result uint64 [L - 1][N], intermediates).  rns.cpp:805-830 (BFV), 1097-1140 (BGV), 832-877 (CKKS) as
    hoist_cases.model_item restates them for the special prime:
      BFV   t' = (x_last + h) mod q_last,  s_j = [t']_{p_j} - [h]_{p_j},                    out_j = (x_j - s_j) q_last^-1 mod p_j
      BGV   k_t = -x_last q_last^-1 mod t, s_j = [x_last]_{p_j} + [k_t]_{p_j} q_last,       out_j = (x_j - s_j) q_last^-1 mod p_j
      CKKS  t' from the last limb in coefficient form, s_j = NTT_j([t']_{p_j} - [h]_{p_j}),  out_j = (x_j - s_j) q_last^-1 mod p_j"""
    L, N = x.shape
    primes = S.primes[:L]
    ql = primes[-1]
    h = ql >> 1
    xo = obj(x)
    last = obj(oracle.ntt_standalone(N, ql, x[L - 1], 3)) if S.ntt else xo[L - 1]
    I = {"last": last}
    if S.scheme == BGV:
        kt = (-last) % S.t * pow(ql, -1, S.t) % S.t
        I["last mod t"], I["k_t"] = last % S.t, kt
    else:
        tp = (last + h) % ql
        I["t'"] = tp
    out = np.zeros((L - 1, N), dtype=np.uint64)
    for j, p in enumerate(primes[:-1]):
        if S.scheme == BFV:
            s = (tp % p - h % p) % p
        elif S.scheme == BGV:
            s = (last % p + kt % p * (ql % p)) % p
        else:
            s = obj(oracle.ntt_standalone(N, p, u64((tp % p + p - h % p) % p), 1))
        diff = (xo[j] - s) % p
        out[j] = u64(diff * pow(ql, -1, p) % p)
        I["s", j], I["x", j], I["diff", j] = s, xo[j], diff
    return out, I


X_CHOICES = ("s_j", "s_j-1", "s_j+1", "0", "p_j-1")  # the data residue against the term the kernel subtracts from it


def craft_divide(S, L, seed):
    """one polynomial [L][N]: every last-limb value of last_targets crossed with every X_CHOICES value of the data residues (all data limbs of a
    coefficient take the same choice, each against its own s_j); CKKS, whose data limbs meet the correction in NTT form: the last limb is built in
    coefficient form and transformed, the data residues are set at seeded slots against the transformed correction.  -> (x, expected, Hits)"""
    N = S.N
    primes = S.primes[:L]
    ql, data = primes[-1], primes[:-1]
    targets, H = last_targets(S, ql, data, "x_last")
    vals = [v for _, v, _, _ in targets if v is not None]
    x = synth.uniform_rows(seed, primes, L, N)
    nc = len(X_CHOICES)
    if S.ntt:
        lastc = synth.uniform_rows(seed ^ 0x77, [ql], 1, N)[0]
        for a, n in enumerate(spots(N, len(vals), seed)):
            lastc[n] = vals[a]
        x[L - 1] = oracle.ntt_standalone(N, ql, lastc, 1)
        where = [(n, c) for c in range(nc) for n in spots(N, 4 * nc, seed + 1)[4 * c:4 * c + 4]]
    else:
        pos = spots(N, len(vals) * nc, seed)
        for a, v in enumerate(vals):
            for c in range(nc):
                x[L - 1, pos[a * nc + c]] = v
        where = [(pos[a * nc + c], c) for a in range(len(vals)) for c in range(nc)]
    _, I = divide_model(S, x)
    for j, p in enumerate(data):
        for n, c in where:
            s = int(I["s", j][n])
            x[j, n] = ((s) % p, (s - 1) % p, (s + 1) % p, 0, p - 1)[c]
    exp, I = divide_model(S, x)
    look_all(H, targets, I)
    for j, p in enumerate(data):
        for nm, key, v in (("x_j=s_j", "diff", 0), ("x_j=s_j-1", "diff", p - 1), ("x_j=s_j+1", "diff", 1), ("x_j=0", "x", 0), ("x_j=p_j-1", "x", p - 1)):
            H.look("p%d: %s" % (j, nm), I[key, j] == v)
    return x, exp, H


def check_divide(S, L, size, batch, cap=None, cf=1, distinct=2, seed=0, cannot=()):
    """`batch` items repeating `distinct` built ciphertexts of `size` polynomials at the level of L primes, dense or (cap) strided: every item against
    its own expected limbs; the model against the oracle and the hit report, once per distinct item.  -> the result"""
    op = R.OP_RESCALE_NEXT if S.ntt else R.OP_MODSWITCH_NEXT
    xs, exps, meta = [], [], None
    for i in range(distinct):
        polys = [craft_divide(S, L, seed + 16 * i + k) for k in range(size)]
        H = Hits()
        for k, (_, _, h) in enumerate(polys):
            H.merge("c%d: " % k, h)
        count = H.check(cannot, (S.name, L, size, "item", i))
        x, exp = np.stack([p[0] for p in polys]), np.stack([p[1] for p in polys])
        o = S.orc.impl.eval(op, R.Ct(x, S.ntt, 1.0, cf))
        assert np.array_equal(o.data, exp), (S.name, L, "the model differs from the oracle")
        meta = (o.is_ntt, o.scale, o.correction_factor)
        xs.append(x)
        exps.append(exp)
    print(S.name, "limbs", L, "size", size, "batch", batch, "boundaries met per item:", count, "unreachable:", sorted(cannot))
    c = S.ct(np.stack([xs[b % distinct] for b in range(batch)]), cap, cf)
    with Kernels(S) as K:
        got = S.ev.rescaleToNext(c) if S.ntt else S.ev.modSwitchToNext(c)
    S.kernels = K.calls
    g = got.cpu()
    assert g.shape == (batch, size, L - 1, S.N)
    for b in range(batch):
        assert np.array_equal(g[b], exps[b % distinct]), (S.name, L, size, "item", b)
    assert S.canonical(g, L - 1)
    assert (got.is_ntt_form, got.correction_factor) == (meta[0], meta[2]) and abs(got.scale - meta[1]) <= 1e-12 * abs(meta[1])
    return got


def check_divide_route(S, L, size, batch, cap=None, seed=0, cannot=()):
    """the call at `batch` and the same call at batch 1 -> their path-counter deltas and their kernels by name"""
    s0 = HC.route_stats()
    check_divide(S, L, size, batch, cap, seed=seed, cannot=cannot)
    big, kbig = HC.delta(HC.route_stats(), s0), S.kernels
    s0 = HC.route_stats()
    check_divide(S, L, size, 1, cap, distinct=1, seed=seed, cannot=cannot)
    one, kone = HC.delta(HC.route_stats(), s0), S.kernels
    print(S.name, "batch", batch, "counters", big, "at batch 1", one, "kernels", kbig, "at batch 1", kone)
    return big, one, kbig, kone


# ================================================================ part 2: the second half of the key switch
def share_targets(S, qk):
    """BGV, ks_bgv_share_kernel: S = a_last + k_t qk as a 128-bit integer; the carry out of the low word is taken by `low word < k_t qk's low word`.
    S is a multiple of t by construction (that is what k_t is for), so S = 2^64 c + d forces c = -d 2^-64 mod t:
      d = 0   needs c = 0 mod t, and c < t qk / 2^64 < t leaves c = 0, S = 0: a low word of exactly 0 AFTER a carry cannot occur (a_last = 0, the
              word where `<` and `<=` part, is on the x_last list)
      d = -1  (the sum misses the carry by one: low word 2^64 - 1) and d = +1 (clears it by one: low word 1) have one candidate c each, reachable
              where 2^64 c + d < t qk -- a chance of qk / 2^64 per parameter set, at most one in sixteen
    -> [(name, a_last, key, value)], unreachable {name: why}"""
    t = S.t
    out, no = [], {"share: low word 0 after a carry": "S = 0 mod t and S < t qk leave only S = 0"}
    if t * qk < W64:
        no["share: carries"] = "t qk < 2^64: the sum never leaves the low word"
    for nm, d in (("share: low word 2^64-1, one short of the carry", -1), ("share: low word 1, one past the carry", 1)):
        c = (-d * pow(W64, -1, t)) % t
        Sv = W64 * c + d
        al, kt = Sv % qk, Sv // qk
        if Sv > 0 and kt < t and (-al) % t * pow(qk, -1, t) % t == kt:
            out.append((nm, al, "share", Sv))
        else:
            no[nm] = "its only candidate, 2^64 * %d %+d, is not below t qk" % (c, d)
    return out, no


def relin_model(S, ct, key):
    """relinearization of one size-3 ciphertext ct [3][dl][N] under `key` [K-1][2][K][N] -> (result [2][dl][N], per-polynomial intermediates, v): the inner
    product of hoist_cases.model_item without the automorphism, its mod-down formulas (lines 146-167) onto (c0, c1); v [2][dl][N]: what is added"""
    N, K, primes = S.N, S.K, S.primes
    dl = ct.shape[1]
    qk = primes[K - 1]
    out_primes = primes[:dl] + [qk]
    key_limb = list(range(dl)) + [K - 1]
    d = [oracle.ntt_standalone(N, primes[j], ct[2, j], 3) if S.ntt else ct[2, j] for j in range(dl)]
    acc = np.zeros((2, dl + 1, N), dtype=object)
    for i, p in enumerate(out_primes):
        for j in range(dl):
            if not key[j, :, key_limb[i]].any():
                continue
            e = obj(oracle.ntt_standalone(N, p, d[j] % np.uint64(p), 1))
            for k in range(2):
                acc[k, i] += e * obj(key[j, k, key_limb[i]])
        acc[:, i] %= p
    half = qk >> 1
    v = np.zeros((2, dl, N), dtype=object)
    Is = []
    for k in range(2):
        last = obj(oracle.ntt_standalone(N, qk, u64(acc[k, dl]), 3))
        I = {"last": last}
        if S.scheme == BGV:
            kt = (-last) % S.t * pow(qk, -1, S.t) % S.t
            I["last mod t"], I["k_t"], I["share"] = last % S.t, kt, kt * qk + last
            I["carry"] = (kt * qk) % W64 + last >= W64
        else:
            tl = (last + half) % qk
            I["t'"] = tl
        for j in range(dl):
            q = primes[j]
            inv = pow(qk, -1, q)
            if S.ntt:
                a = acc[k, j]
                diff = (a - obj(oracle.ntt_standalone(N, q, u64((tl % q + (q - half % q)) % q), 1))) % q
            else:
                a = obj(oracle.ntt_standalone(N, q, u64(acc[k, j]), 3))
                diff = (a - tl % q + half % q) % q if S.scheme == BFV else (a - kt % q * (qk % q) - last % q) % q
            v[k, j] = diff * inv % q
            I["a", j], I["diff", j] = a, diff
        Is.append(I)
    return Is, v


def relin_finish(S, ct, Is, v):
    dl = ct.shape[1]
    out = np.zeros((2, dl, S.N), dtype=np.uint64)
    for k in range(2):
        for j in range(dl):
            r = (obj(ct[k, j]) + v[k, j]) % S.primes[j]
            Is[k]["out", j] = r
            out[k, j] = u64(r)
    return out


class Selector:
    """the key that puts chosen integers into the accumulator.  key[j0][k][i][:] = w is the same word at every position of an NTT-form row, a constant
    polynomial, so in coefficient form digit j0 adds w (d_n mod p_i) to limb i, d_n coefficient n of limb j0 of c2.  The special limb takes w = 1: its
    coefficient is d_n mod qk.  Where q_j0 < qk (CoeffModulus.Create gives that for every set here), d_n < q_j0 cannot reach the values of qk's upper range
    alone, so a second digit j1 carries the high bits with w = 2^s, s = bits(q_j0) - 1:  a_last = (d_j0 + 2^s d_j1) mod qk, any value below qk.
    The data limbs take w = p_i - 1 from digit j0 (a_i = -d_n: 0 where d_n = 0, p_i - 1 where d_n = 1) and a seeded word from digit j1.
    Every other digit is zero -- or, `live`, a seeded uniform key (digit j0 keeps its selector rows): the accumulator is then no longer chosen, the
    stored results still are, and the model is computed anew; that case is there so that the selector hides no indexing error"""

    def __init__(self, S, live=False, seed=900):
        K, N, primes = S.K, S.N, S.primes
        dl = self.dl = K - 1
        qk = primes[K - 1]
        self.live = live
        self.j0 = max(range(dl), key=lambda j: primes[j])
        self.two = primes[self.j0] < qk and dl >= 2 and not live
        self.j1 = (self.j0 + 1) % dl if self.two else None
        self.s = primes[self.j0].bit_length() - 1
        key = synth.uniform_kswitch_key(seed, primes, N) if live else np.zeros((K - 1, 2, K, N), dtype=np.uint64)
        rng = np.random.default_rng(seed)
        for k in range(2):
            key[self.j0, k, K - 1] = 1
            for i in range(dl):
                key[self.j0, k, i] = primes[i] - 1
            if self.two:
                key[self.j1, k, K - 1] = 1 << self.s
                for i in range(dl):
                    key[self.j1, k, i] = int(rng.integers(1, primes[i]))
        self.key = key
        S.be.rlk.set(0, key)
        S.orc.impl.set_kswitch_key(0, key)

    def digits(self, S, v):
        """(d_j0, d_j1) that make the special limb's coefficient v, or None"""
        if self.two:
            return v & ((1 << self.s) - 1), v >> self.s
        return (v, None) if v < S.primes[self.j0] else None


CKKS_A = "a_j=0, a_j=p_j-1: not placed by the selector in NTT form"
R_CHOICES = ("0", "1", "p_j-1")  # the stored result: 0 means the lazy sum before the last conditional subtractions is an exact multiple of p_j


def craft_relin(S, sel, seed):
    """one size-3 ciphertext at the first level: c2 holds the digits that put every value of last_targets (and, BGV, of share_targets) into the special
    limb of both accumulator polynomials; the base (c0, c1) is then chosen against the model's v so that the stored result is each of R_CHOICES at each
    of those coefficients (CKKS, whose data limbs stay in NTT form: at seeded slots).  -> (ct, expected, Hits)"""
    N, dl, primes = S.N, sel.dl, S.primes
    qk = primes[S.K - 1]
    targets, H = last_targets(S, qk, primes[:dl], "a_last") if not sel.live else ([], Hits())
    if S.scheme == BGV and not sel.live:
        more, no = share_targets(S, qk)
        targets += more
        for n, why in no.items():
            H.cannot(n, why)
    d = synth.uniform_rows(seed, primes[:dl], dl, N)
    nr = len(R_CHOICES) + 1  # and one coefficient whose base stays uniform
    where = []
    if not sel.live:
        placed = []
        for name, val, _, _ in targets:
            dig = sel.digits(S, val) if val is not None else None
            if val is not None and dig is None:
                H.cannot(name, "a single digit below q_j0 < qk")
            elif val is not None:
                placed.append(dig)
        pos = spots(N, len(placed) * (1 if S.ntt else nr), seed)
        for a, (d0, d1) in enumerate(placed):
            for c in range(1 if S.ntt else nr):
                n = pos[a * (1 if S.ntt else nr) + c]
                d[sel.j0, n] = d0
                if d1 is not None:
                    d[sel.j1, n] = d1
                where.append((n, c))
    if S.ntt or sel.live:
        where = [(n, c) for c in range(len(R_CHOICES)) for n in spots(N, 8 * len(R_CHOICES), seed + 1)[8 * c:8 * c + 8]]
    c2 = np.stack([oracle.ntt_standalone(N, primes[j], d[j], 1) for j in range(dl)]) if S.ntt else d
    ct = np.concatenate([synth.uniform_rows(seed + 2, primes[:dl], 2 * dl, N).reshape(2, dl, N), c2[None]])
    Is, v = relin_model(S, ct, sel.key)
    for k in range(2):
        for j in range(dl):
            p = primes[j]
            for n, c in where:
                if c < len(R_CHOICES):
                    ct[k, j, n] = ((0, 1, p - 1)[c] - int(v[k, j, n])) % p
    exp = relin_finish(S, ct, Is, v)
    for k in range(2):
        Hk, I = Hits(), Is[k]
        if not sel.live:
            look_all(Hk, [t for t in targets if t[0] not in H.unreachable], I)
            if S.scheme == BGV:
                if "share: carries" not in H.unreachable:
                    Hk.look("share: carries", I["carry"])
                Hk.look("share: does not carry", ~I["carry"].astype(bool))
        for j in range(dl):
            p = primes[j]
            for nm, val in zip(R_CHOICES, (0, 1, p - 1)):
                Hk.look("p%d: result=%s" % (j, nm), I["out", j] == val)
            if not sel.live and not S.ntt:
                Hk.look("p%d: a_j=0" % j, I["a", j] == 0)
                Hk.look("p%d: a_j=p_j-1" % j, I["a", j] == p - 1)
                Hk.look("p%d: difference=0" % j, I["diff", j] == 0)
        H.merge("c%d: " % k, Hk)
    if S.ntt and not sel.live:
        H.cannot(CKKS_A, "a limit of this construction, not of the parameter set: the CKKS accumulator's data limbs stay in NTT form, a_j = w NTT_j(d), "
                         "where the selector's constant w places no single value; the coefficient-form schemes cover the accumulator's ends")
    return ct, exp, H


def check_relin(S, sel, batch, cap=None, distinct=2, seed=0, cannot=(), to=True, inplace=True):
    """`batch` items repeating `distinct` built ciphertexts through troyhip_relinearize_to (`to`, Evaluator.relinearize: the operand is read where it lies,
    the base is taken by the epilogue) and troyhip_relinearize_keys (`inplace`, Evaluator.relinearizeInplace: the entry the Python layer calls; with one
    key it is Evaluator::relinearize, as troyhip_relinearize is: accumulated onto the operand's own c0 / c1), dense or (cap 4) strided: every item
    against its own expected limbs.  -> {route: path-counter deltas}; S.kernels: {route: kernels by name}"""
    cts, exps = [], []
    for i in range(distinct):
        ct, exp, H = craft_relin(S, sel, seed + 16 * i)
        count = H.check(cannot, (S.name, "item", i))
        o = S.orc.impl.eval(R.OP_RELIN, R.Ct(ct, S.ntt))
        assert np.array_equal(o.data, exp), (S.name, "the model differs from the oracle")
        cts.append(ct)
        exps.append(exp)
    print(S.name, "batch", batch, "live" if sel.live else "selector", "boundaries met per item:", count, "unreachable:", sorted(cannot))
    data = np.stack([cts[b % distinct] for b in range(batch)])
    dl = sel.dl
    stats, S.kernels = {}, {}
    for route in ("to",) * to + ("inplace",) * inplace:
        a = S.ct(data, cap)
        s0 = HC.route_stats()
        with Kernels(S) as K:
            if route == "to":
                got = S.ev.relinearize(a, S.be.rlk)
            else:
                S.ev.relinearizeInplace(a, S.be.rlk)
                got = a
        stats[route], S.kernels[route] = HC.delta(HC.route_stats(), s0), K.calls
        if route == "to":
            assert np.array_equal(a.cpu(), data), (S.name, "operand modified")
        g = got.cpu()
        assert g.shape == (batch, 2, dl, S.N) and got.is_ntt_form == S.ntt
        for b in range(batch):
            assert np.array_equal(g[b], exps[b % distinct]), (S.name, route, "item", b)
        assert S.canonical(g, dl)
    return stats


# the small-launch cases of both test files, batch 2 at N = 4096, and what each parameter set cannot reach (the tests' docstrings say why)
MEDIUM = {
    "cfgA_bfv_n4096_k3": [],
    # t qk < 2^57: the 128-bit share never leaves its low word
    "bgv_n4096_k3": ["share: carries", "share: low word 0 after a carry", "share: low word 1, one past the carry", "share: low word 2^64-1, one short of the carry"],
    # twice the 40-bit p_0 lies above the 40-bit special prime; the accumulator's data limbs stay in NTT form
    "ckks_n4096_k4": ["p0: t'=2p_j", CKKS_A],
}
TWICE_P0 = {BFV: ["p0: t'=2p_j"], BGV: ["p0: a_last=2p_j"], CKKS: ["p0: t'=2p_j", CKKS_A]}  # [60, .., 60]: 2 p_0 lies above the 60-bit special prime
SHARE_60 = ["share: low word 0 after a carry", "share: low word 1, one past the carry"]  # [60, 50, 50, 60], t of 20 bits: share_targets


def check_relin_medium(name, live=False):
    """the small-launch case of `name`: the selector dense and strided, or every digit live"""
    S = named(name)
    if live:
        return check_relin(S, Selector(S, live=True), 2, seed=500)
    sel = Selector(S)
    for cap in (None, 4):
        check_relin(S, sel, 2, cap, seed=400, cannot=MEDIUM[name])


def run_in_child(body, env, lib=None, timeout=600):
    """`body` (Python source; round_cases is RC, hoist_cases HC) in a fresh process under `env`: the library reads its switches once per process.
    lib: the path of another build of the library (the emulator's), else what troy_amd loads by itself (TROYHIP_LIB in `env`: the probe build)"""
    import os
    import subprocess
    import sys
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from troy_amd import api, capi\n"
            "api.KernelProvider.initialize(0, **(dict(_lib=capi.load(%r)) if %r else {}))\n"
            "import hoist_cases as HC, round_cases as RC\n" % (tests_dir, os.path.dirname(tests_dir), lib, lib)) + body + "\nprint('child ok')\n"
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.split()[-2:] == ["child", "ok"], (out.stdout[-2000:], out.stderr[-2000:])
    return out.stdout


def single_pass_at_small_batch():
    """for a process started with TROYHIP_NTT=single, which lets batch 2 at N = 4096 take the single-pass inverse with the BFV mod-down as its epilogue
    (Ntt1ModDown; the FP64 instance for [36, 36, 37], the guarded and the guard-free integer ones for [60, 58, 58, 60]), which only a large launch
    reaches otherwise, on the built inputs.  Its conditional subtractions are bfly.h's csub4: the C form on the emulator build, where no small-launch
    route runs it on a built value.  (The correction form of the CKKS transforms, Ntt1Corr, exists at N = 2^15 only and is not forced by the switch:
    tests/test_gpu_round.py runs it.)  The route: exactly one single-pass launch over the special limb and one per prime class of the data limbs --
    the first half of a BFV key switch makes none, and the element-wise form behind a plain single-pass inverse would make one per class of ALL
    limbs: 1 and 2 in place of 2 and 3 -- and, where the build records kernel names, the epilogue instances themselves"""
    for S, cannot, launches in ((named("cfgA_bfv_n4096_k3"), [], 2), (Setup(BFV, 4096, (60, 58, 58, 60)), TWICE_P0[BFV], 3)):
        for cap in (None, 4):
            st = check_relin(S, Selector(S), 2, cap, seed=800, cannot=cannot)
            assert st["to"] == st["inplace"] and HC.single_pass(st["to"]) == launches and HC.two_pass(st["to"]) == 0, (S.name, st)
            for k in S.kernels.values():
                assert not k or (epilogue_calls(k, "inv") == launches - 1 and calls_of(k, "ks_moddown_kernel") == 0), (S.name, k)


def probe_fallback(which):
    """for a process on the probe build under TROYHIP_MODDOWN=split or TROYHIP_CORR=split (tests/test_gpu_round.py test_probe_build_fallbacks)"""
    if which == "moddown_split":
        for name in ("cfgA_bfv_n4096_k3", "bgv_n4096_k3"):
            S = named(name)
            check_relin(S, Selector(S), 2, seed=400, cannot=MEDIUM[name])
            for k in S.kernels.values():
                assert calls_of(k, "ks_moddown_kernel") == 1, (name, k)
        cache = {}
        bgv_one_mod_t_case(cache)
        assert all(calls_of(k, "ks_moddown_kernel") == 1 for k in cache["one_mod_t"].kernels.values())
        return
    cus = HC.device_cus()
    S = Setup(CKKS, 32768, (60, 40, 40, 60))
    batch = HC.items_for(HC.single_pass_rows(S.N, cus), 2 * 3)
    st = check_relin(S, Selector(S), batch, seed=750, cannot=TWICE_P0[CKKS], inplace=False)
    k = S.kernels["to"]
    assert HC.single_pass(st["to"]) == 2 and epilogue_calls(k, "fwd") == 0 and calls_of(k, "ks_ckks_corr_kernel") == calls_of(k, "ks_ckks_combine_kernel") == 1, (st, k)
    S = Setup(CKKS, 32768, (60, 40, 58, 50, 60))
    s0 = HC.route_stats()
    check_divide(S, 4, 2, batch, 3, seed=700, cannot=multiples("t'", 0, 2))
    d, k = HC.delta(HC.route_stats(), s0), S.kernels
    assert HC.single_pass(d) == 3 and epilogue_calls(k, "fwd") == 0 and calls_of(k, "rescale_stepA") == calls_of(k, "rescale_stepB") == 1, (d, k)


def check_relin_route(S, sel, batch, cap=None, seed=0, cannot=()):
    """-> (counter deltas of the call at `batch`, of the same call at batch 1, their kernels by name), both through troyhip_relinearize_to and
    troyhip_relinearize_keys, which must agree in the counters and in the epilogue launches"""
    big, kbig = check_relin(S, sel, batch, cap, seed=seed, cannot=cannot), S.kernels
    one, kone = check_relin(S, sel, 1, cap, distinct=1, seed=seed, cannot=cannot), S.kernels
    print(S.name, "batch", batch, "counters", big, "at batch 1", one, "kernels", kbig, "at batch 1", kone)
    assert big["to"] == big["inplace"] and one["to"] == one["inplace"], (big, one)
    for d in ("fwd", "inv"):
        assert epilogue_calls(kbig["to"], d) == epilogue_calls(kbig["inplace"], d), kbig
    return big["to"], one["to"], kbig["to"], kone["to"]


# ================================================================ part 3: the last step of decryption
def level_q(S, limbs):
    q = 1
    for p in S.primes[:limbs]:
        q *= p
    return q


def bfv_values(q, t):
    """[(name, V, exact k or None, tie)]: the ends and the middle of the range; per k the plateau centre round(k q / t), where the reference's
    algorithm is exact by its own bound, and the two neighbours of the tie (2k + 1) q / (2t): the last V that rounds to k, the first that rounds to k + 1"""
    out = [("V=0", 0, 0, False), ("V=1", 1, None, False), ("V=q-1", q - 1, None, False), ("V=(q-1)/2", (q - 1) // 2, None, False),
           ("V=(q+1)/2", (q + 1) // 2, None, False)]
    for nm, k in (("0", 0), ("1", 1), ("(t-1)/2", (t - 1) // 2), ("t-2", t - 2), ("t-1", t - 1)):
        out.append(("centre of k=%s" % nm, (2 * k * q + t) // (2 * t), k, False))
        lo = ((2 * k + 1) * q) // (2 * t)  # q is odd and t prime: the tie itself is no integer
        assert (2 * t * lo + q) // (2 * q) == k and (2 * t * (lo + 1) + q) // (2 * q) == k + 1
        out.append(("last V of k=%s" % nm, lo, None, True))
        out.append(("first V of k=%s + 1" % nm, lo + 1, None, True))
    return out


def bgv_values(q, t):
    """where sum_l v_l / p_l + 0.5 of decrypt_bgv_kernel sits within an ulp of an integer: around q / 2; and the ends of the range"""
    hm = (q - 1) // 2
    vals = [("V=0", 0), ("V=1", 1), ("V=t-1", t - 1), ("V=t", t), ("V=(q-1)/2-2", hm - 2), ("V=(q-1)/2-1", hm - 1), ("V=(q-1)/2", hm), ("V=(q+1)/2", hm + 1),
            ("V=(q+1)/2+1", hm + 2), ("V=q-t", q - t), ("V=q-1", q - 1)]
    # for a q of a hundred bits these all give the double k + 0.5 itself; the doubles next to it belong to V / q = 1/2 - j 2^-54 (k < 4: the sum's
    # ulp is 2^-53 .. 2^-51), where `sum + 0.5` is the last double below an integer, or a tie between it and the integer
    if 2 * q >= 1 << 53:
        vals += [("V=q(1/2 - %d/2^54)" % j, (q * ((1 << 53) - j)) >> 54) for j in range(-8, 17) if j]
    return [(n, v % q, None, False) for n, v in vals]


def double_sum(S, limbs, res):
    """the kernel's rounding term for one coefficient's residues: sum_l (x_l (q / p_l)^-1 mod p_l) / p_l in double precision, limb order"""
    q = level_q(S, limbs)
    agg = 0.0
    for l, p in enumerate(S.primes[:limbs]):
        agg += float(int(res[l]) * pow(q // p, -1, p) % p) / float(p)
    return agg


DOUBLE_SUM = "the double sum within an ulp of k + 0.5"
DOUBLE_BELOW = "the double sum + 0.5 is the last double below an integer"
DOUBLE_EXACT = "the double sum is k + 0.5 exactly"


def craft_decrypt(S, limbs, seed, shift=0):
    """one size-2 ciphertext with c1 = 0 and c0 = CRT(V) at seeded coefficients, as noise_cases.crafted builds them; uniform residues elsewhere in c0
    -> (ct, [(name, position, V, exact, tie)], Hits)"""
    N, t = S.N, S.t
    q = level_q(S, limbs)
    vals = (bfv_values if S.scheme == BFV else bgv_values)(q, t)
    vals = vals[shift % len(vals):] + vals[:shift % len(vals)]
    ct = np.zeros((2, limbs, N), dtype=np.uint64)
    ct[0] = synth.uniform_rows(seed, S.primes[:limbs], limbs, N)
    pos = spots(N, len(vals), seed)
    H = Hits()
    placed = []
    for (name, V, exact, tie), n in zip(vals, pos):
        for l, p in enumerate(S.primes[:limbs]):
            ct[0, l, n] = V % p
        placed.append((name, n, V, exact, tie))
    # the report reads the ciphertext back: the integer the written residues stand for (CRT), and for BFV where exact rounding puts it and its neighbours
    rnd = lambda X: (2 * t * X + q) // (2 * q)  # noqa: E731
    for name, n, V, exact, tie in placed:
        X = sum(int(ct[0, l, n]) * (q // p) * pow(q // p, -1, p) for l, p in enumerate(S.primes[:limbs])) % q
        ok = X == V
        if name.startswith("centre"):
            ok = ok and rnd(X - 1) == rnd(X) == rnd(X + 1) == exact
        elif name.startswith("last V"):
            ok = ok and rnd(X) + 1 == rnd(X + 1)
        elif name.startswith("first V"):
            ok = ok and rnd(X - 1) + 1 == rnd(X)
        H.look(name, ok)
    if S.scheme == BGV:
        aggs = [double_sum(S, limbs, ct[0, :, n]) for _, n, _, _, _ in placed]
        sums = [a + 0.5 for a in aggs]
        near = [abs(a - round(a)) <= math.ulp(a) for a in sums]
        if 2 * q < 1 << 53:
            for name in (DOUBLE_SUM, DOUBLE_BELOW, DOUBLE_EXACT):
                H.cannot(name, "the sum nearest to k + 0.5, that of V = (q - 1) / 2, lies 1 / (2q) > 2^-53 below it")
        else:
            H.look(DOUBLE_SUM, near)
            H.look(DOUBLE_BELOW, [a == math.nextafter(math.ceil(a), 0.0) for a in sums])
            H.look(DOUBLE_EXACT, [a - math.floor(a) == 0.5 for a in aggs])
    return ct, placed, H


def check_decrypt(S, limbs, batch=3, cap=None, cf=1, seed=0, cannot=()):
    """`batch` built ciphertexts (each its own positions, the value list rotated), an all-zero key: every coefficient against the oracle's decrypt;
    at the plateau centres the exact integer too.  -> (tie neighbours, those the reference's algorithm places differently from exact rounding)"""
    N, t = S.N, S.t
    q = level_q(S, limbs)
    sk = np.zeros((S.K, N), dtype=np.uint64)
    built = [craft_decrypt(S, limbs, seed + 16 * b, shift=5 * b) for b in range(batch)]
    for _, _, H in built:
        H.check(cannot, (S.name, limbs))
    data = np.stack([b[0] for b in built])
    got = S.ev.decrypt(S.ct(data, cap, cf), S.api.DeviceBuffer.from_numpy(sk))
    assert got.shape == (batch, N)
    ties = off = 0
    inv_cf = pow(cf, -1, t)
    for b, (ct, placed, _) in enumerate(built):
        exp = S.orc.impl.decrypt(R.Ct(ct, False, 1.0, cf), sk)
        assert np.array_equal(got[b], exp), (S.name, limbs, cf, "item", b, [p[0] for p in placed if got[b, p[1]] != exp[p[1]]])
        assert (got[b] < np.uint64(t)).all()
        for name, n, V, exact, tie in placed:
            if exact is not None:
                assert int(got[b, n]) == exact, (S.name, limbs, name)
            if S.scheme == BGV and name in ("V=0", "V=1", "V=t-1", "V=t", "V=q-1"):  # small centred values decrypt to themselves, times cf^-1
                assert int(got[b, n]) == (V if V < q // 2 else V - q) % t * inv_cf % t, (S.name, limbs, name)
            if tie:
                ties += 1
                off += int(exp[n]) != (2 * t * V + q) // (2 * q) % t
    return ties, off


# ================================================================ the cases both test files run (each file keeps its own setups: its own library)
def setup_in(cache, *key):
    if key not in cache:
        cache[key] = named(key[0]) if len(key) == 1 else Setup(*key)
    return cache[key]


def divide_wide(cache, scheme, size, batch, cap):
    S = setup_in(cache, scheme, 4096, (36, 40, 50, 60))
    for L in (3, 2):
        for cf in ((1, 3) if scheme == BGV else (1,)):
            check_divide(S, L, size, batch, cap, cf=cf, seed=100 + L)


def divide_narrow(cache, scheme, size, batch, cap):
    S = setup_in(cache, scheme, 4096, (50, 45, 30, 60))
    what = "x_last" if scheme == BGV else "t'"
    for L, cannot in ((3, multiples(what, 0, 1)), (2, multiples(what, 0))):
        for cf in ((1, 3) if scheme == BGV else (1,)):
            check_divide(S, L, size, batch, cap, cf=cf, seed=200 + L, cannot=cannot)


def divide_ckks(cache, size, batch, cap):
    S = setup_in(cache, CKKS, 4096, (60, 40, 58, 50, 60))
    for L, cannot in ((4, multiples("t'", 0, 2)), (2, multiples("t'", 0))):
        check_divide(S, L, size, batch, cap, seed=300 + L, cannot=cannot)


def decrypt_boundaries(cache, name):
    S = setup_in(cache, name)
    ties = off = 0
    for limbs in range(S.K - 1, S.be.last_limbs - 1, -1):
        for cap in (None, 3):
            for cf in ((1, 5) if S.scheme == BGV else (1,)):
                cannot = [DOUBLE_SUM, DOUBLE_BELOW, DOUBLE_EXACT] if S.scheme == BGV and limbs == 1 else []
                a, b = check_decrypt(S, limbs, 3, cap, cf, seed=600 + limbs, cannot=cannot)
                ties, off = ties + a, off + b
    print(name, "tie neighbours", ties, "placed differently from exact rounding by the reference's algorithm", off)


def bgv_one_mod_t_case(cache):
    if "one_mod_t" not in cache:
        cache["one_mod_t"] = bgv_one_mod_t()
    S = cache["one_mod_t"]
    for size, batch, cap in ((2, 3, 3), (3, 2, None)):
        for cf in (1, 3):
            check_divide(S, 2, size, batch, cap, cf=cf, seed=900, cannot=["x_last=mt+1"])
    sel = Selector(S)
    for cap in (None, 4):
        check_relin(S, sel, 2, cap, seed=910, cannot=["a_last=mt+1"] + SHARE_60)
