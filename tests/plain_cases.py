"""Shared checks of the plaintext operands on crafted boundaries against exact models: troyhip_add_plain (add_plain_kernel<KIND, SUB>,
add_plain_rows_kernel<SUB>), troyhip_plain_to_ntt (plain_lift_kernel), troyhip_multiply_plain, troyhip_multiply_plain_ntt (mul_plain_kernel) and
troyhip_multiply_plain_accumulate (mul_plain_acc_kernel), and what leans on them (troyhip_encrypt's message, the constant of troyhip_scalar_combine).
Used by tests/test_device_plain.py (emulator build) and tests/test_gpu_plain.py (MI355X).

A uniform plaintext under a 20-bit batching prime meets none of what these kernels decide on: the BFV scaling round(q m / t) is computed as
m Delta + floor((m r + thr) / t), r = q mod t, thr = (t + 1) >> 1, with div128, a Barrett quotient corrected once -- a quotient off by one shows only
where m r + thr lies within one of a multiple of t, a chance of 3 / t per coefficient; the lift compares m with thr; the BGV form multiplies by the
correction factor only where it is not 1.  Here the plaintexts are BUILT (boundary_values, craft_plain), the models are Python integers written from the
definitions (none calls the oracle's plaintext operations or the library's host forms; the transform itself, pinned elsewhere, is oracle.ntt_standalone),
and every boundary class is counted in the built plaintext (round_cases.Hits): a class no coefficient shows fails the case unless the parameter set
cannot reach it, and then the case has to name it.  All comparisons are bit-exact, and every result is held canonical (below its prime)."""
import ctypes as C
import math

import numpy as np

import hoist_cases as HC
import round_cases as RC
from oracle import oracle
from troy_amd import api, capi, synth
from troy_amd.capi import BFV, BGV, CKKS

obj, u64, Hits = HC.obj, RC.u64, RC.Hits


def _batching(bits):
    return lambda N: int(api.PlainModulus.Batching(N, bits))


# name -> (prime bits, t, the data levels in limbs)
SETS = {
    "small": ([36, 40, 50, 60], _batching(17), (3, 2, 1)),        # every level: q mod t and Delta_l change per level
    # LinearHelper's modulus: t no prime, its Barrett constant 2^87 exact -- div128's estimate is the quotient itself here and its correction never fires
    "pow2": ([60, 60, 60], lambda N: 1 << 41, (2, 1)),
    "wide60": ([60, 60, 60, 60], lambda N: (1 << 60) - 1, (3, 2)),  # the largest t accepted, composite: numerator near 2^120, quotient near 2^60
    "wide59": ([60, 60, 60, 60], _batching(59), (3, 2, 1)),
    "above": ([30, 50, 60], _batching(40), (2,)),                 # t above the 30-bit data prime: barrett64(pc, m) and t % p really reduce
}
INT_SETS = sorted(SETS)
CKKS_BITS = [60, 40, 58, 50, 60]  # the guarded, the FP64 and the guard-free class of prime


class Setup:
    """one parameter set with an explicit plain modulus (hoist_cases.Setup only makes batching primes)"""

    def __init__(self, scheme, name, N=128):
        bits, t, levels = SETS[name] if scheme != CKKS else (CKKS_BITS, lambda N: 0, None)
        self.name, self.scheme, self.N = "%s_%s_n%d" % ({BFV: "bfv", BGV: "bgv", CKKS: "ckks"}[scheme], name, N), scheme, N
        self.primes = [int(p) for p in api.CoeffModulus.Create(N, bits)]
        self.t = t(N)
        self.thr = (self.t + 1) >> 1
        self.ctx = api.SEALContext(scheme, N, self.primes, self.t)
        self.lib, self.ev, self.K, self.ntt = self.ctx.lib, api.Evaluator(self.ctx), len(self.primes), scheme == CKKS
        self.levels = list(range(self.ctx.first_limbs, self.ctx.last_limbs - 1, -1))
        assert levels is None or tuple(self.levels) == levels, (self.name, "data levels", self.levels, "the case expects", levels)
        self.sk, self.set = None, name

    def q(self, limbs):
        return math.prod(self.primes[:limbs])

    def ct(self, data, cap=None, cf=1, scale=1.0, seed=77):
        """a batch [B][size][limbs][N]; strided (cap): the padding polynomials hold seeded 64-bit words, nobody's residues -> (Ciphertext, the whole buffer)"""
        data = np.asarray(data, dtype=np.uint64)
        B, size, limbs, N = data.shape
        cap = cap or size
        full = synth.splitmix64_stream(seed, B * cap * limbs * N).reshape(B, cap, limbs, N)
        full[:, :size] = data
        return api.Ciphertext(self.ctx, B, size, limbs, self.ntt, scale, cf, cap, api.DeviceBuffer.from_numpy(full)), full

    def whole(self, c):
        return c.buf.to_numpy().reshape(c.batch, c.capacity, c.limbs, self.N)

    def canonical(self, got, limbs):
        return all((got[..., j, :] < np.uint64(self.primes[j])).all() for j in range(limbs))

    def secret(self):
        if self.sk is None:  # any key: every ciphertext decrypted here has c1 = 0
            self.sk = api.DeviceBuffer.from_numpy(synth.uniform_rows(7, self.primes, self.K, self.N))
        return self.sk


def setup_in(cache, scheme, name, N=128):
    key = (scheme, name, N)
    if key not in cache:
        cache[key] = Setup(scheme, name, N)
    return cache[key]


# ================================================================ the crafted plaintexts
M_CLASSES = ("m=0", "m=1", "m=thr-1", "m=thr", "m=thr+1", "m=t-1")
REM_CLASSES = ("rem=0", "rem=1", "rem=t-1", "rem=thr-1", "rem=thr")  # rem = (m r + thr) mod t: 0 is the first numerator of a quotient, t - 1 the last


def rem_targets(S):
    return dict(zip(REM_CLASSES, (0, 1, S.t - 1, S.thr - 1, S.thr)))


def boundary_values(S, limbs):
    """-> ([(class, m)], {class: why no m of this level meets it}).  The plain values 0, 1, thr - 1, thr, thr + 1, t - 1; and per target remainder the m
    with m r + thr = target (mod t): m = (target - thr) r^-1.  Where r is no unit (possible for the composite 2^60 - 1 only: a prime t never divides q,
    and q is odd) the congruence is solved modulo t / g, g = gcd(r, t), and has no solution at all where g does not divide target - thr"""
    t, thr = S.t, S.thr
    r = S.q(limbs) % t
    g = math.gcd(r, t)
    out, no = list(zip(M_CLASSES, (0, 1, thr - 1, thr, thr + 1, t - 1))), {}
    for name, target in rem_targets(S).items():
        d = (target - thr) % t
        if d % g:
            no[name] = "gcd(q mod t, t) = %d does not divide target - thr" % g
        else:
            m = d // g * pow(r // g, -1, t // g) % (t // g)
            assert (m * r + thr) % t == target
            out.append((name, m))
    return out, no


def look_classes(S, limbs, H, m):
    """the hit report reads the built plaintext back"""
    t, thr = S.t, S.thr
    r = S.q(limbs) % t
    mo = obj(m).reshape(-1)
    _, no = boundary_values(S, limbs)
    for name, v in zip(M_CLASSES, (0, 1, thr - 1, thr, thr + 1, t - 1)):
        H.look(name, mo == v)
    rem = (mo * r + thr) % t
    for name, target in rem_targets(S).items():
        if name in no:
            H.cannot(name, no[name])
        else:
            H.look(name, rem == target)


UNREACHABLE = {}  # (set, limbs) -> the classes no plaintext of that level meets.  Empty: q mod t is a unit in every set, 2^60 - 1 at both of its levels included


def cannot(S, limbs):
    """what the case names as unreachable; Hits.check holds it against what boundary_values found"""
    return sorted(UNREACHABLE.get((S.set, limbs), ()))


def positions(count, seed):
    """every coefficient of a plaintext of `count`, the first, the second and the last in front, the rest in seeded order"""
    first = list(dict.fromkeys(n for n in (0, 1, count - 1) if 0 <= n < count))
    rest = [int(n) for n in np.random.default_rng(seed).permutation(np.arange(count)) if n not in first]
    return first + rest


def craft_plain(S, limbs, count, seed, shift=0, sparse=False):
    """one plaintext of `count` coefficients: the boundary values, their list rotated by `shift`, at coefficients 0, 1, count - 1 and seeded spots; uniform
    residues elsewhere, or (sparse) zeros, with at most eight coefficients set"""
    vals = [v for _, v in boundary_values(S, limbs)[0]]
    vals = vals[shift % len(vals):] + vals[:shift % len(vals)]
    m = np.zeros(count, dtype=np.uint64) if sparse else synth.uniform_rows(seed, [S.t], 1, count)[0]
    for n, v in zip(positions(count, seed), vals[:8] if sparse else vals):
        m[n] = v
    return m


def craft_batch(S, limbs, count, batch, seed, per_item=True, sparse=False):
    """[batch][count]: every item its own placement and its own rotation of the values; shared: one plaintext for all"""
    if not per_item:
        return np.stack([craft_plain(S, limbs, count, seed, seed, sparse)] * batch)
    return np.stack([craft_plain(S, limbs, count, seed + 101 * b, seed + 4 * b + 1, sparse) for b in range(batch)])


def device_plain(pts, per_item):
    return api.DeviceBuffer.from_numpy(pts if per_item else pts[0])


# ================================================================ the exact models (Python integers)
def add_value(S, limbs, m, cf):
    """what add_plain adds to c0, before the reduction modulo q_l.  BFV: round(q m / t) = (q m + thr) // t; BGV: m cf mod t"""
    mo = obj(m)
    return (S.q(limbs) * mo + S.thr) // S.t if S.scheme == BFV else mo * cf % S.t


def add_model(S, x, m, cf, sub):
    """x [size][limbs][N], m [count]: c0_l[j] +- v_j mod q_l for j < count; c1 and any third polynomial unchanged"""
    limbs = x.shape[1]
    v = add_value(S, limbs, m, cf)
    out = x.copy()
    for l, p in enumerate(S.primes[:limbs]):
        out[0, l, :len(m)] = u64((obj(x[0, l, :len(m)]) + (-v if sub else v)) % p)
    return out


def centred(S, m):
    mo = obj(m)
    return np.where(mo < S.thr, mo, mo - S.t)


def lift_model(S, limbs, m):
    """[limbs][N]: m for m < thr, else m - t, modulo q_l; zero from the plaintext's coefficient count on"""
    out = np.zeros((limbs, S.N), dtype=np.uint64)
    c = centred(S, m)
    for l, p in enumerate(S.primes[:limbs]):
        out[l, :len(m)] = u64(c % p)
    return out


def ntt_model(S, rows, inverse=False):
    return np.stack([oracle.ntt_standalone(S.N, S.primes[l], rows[l], 3 if inverse else 1) for l in range(len(rows))])


def negacyclic_sparse(S, x, m):
    """x [size][limbs][N] times the centred plaintext m, whose nonzero coefficients are few, modulo X^N + 1 and q_l: a signed rotation per coefficient"""
    N = S.N
    c = centred(S, m)
    nz = [int(k) for k in np.nonzero(np.asarray(m))[0]]
    assert len(nz) <= 8
    out = np.zeros(x.shape, dtype=np.uint64)
    xo = obj(x)
    acc = np.zeros(x.shape, dtype=object)
    for k in nz:
        rot = np.roll(xo, k, axis=-1)
        rot[..., :k] = -rot[..., :k]  # X^N = -1
        acc += rot * int(c[k])
    for l, p in enumerate(S.primes[:x.shape[1]]):
        out[:, l] = u64(acc[:, l] % p)
    return out


# ================================================================ check 1: add / sub on the boundaries
def edge_c0(S, x, m, cf):
    """c0 written over at half of the plaintext's coefficients, against the value v the call adds or subtracts: -v (the sum is q_l itself, stored 0),
    -v - 1 (stored q_l - 1), v (the difference is 0), v - 1 (the difference is -1, stored q_l - 1)"""
    limbs = x.shape[1]
    v = add_value(S, limbs, m, cf)
    j = np.arange(len(m))
    for l, p in enumerate(S.primes[:limbs]):
        for k, val in enumerate((-v, -v - 1, v, v - 1)):
            sel = j % 8 == k
            x[0, l, :len(m)][sel] = u64(val[sel] % p)


LAYOUTS = ((2, None), (2, 3), (3, None))  # (size, capacity): dense, strided, and a third polynomial


def check_add(S, limbs, batch=3, counts=None, cfs=None, layouts=LAYOUTS, per_items=(False, True), seed=0):
    """add and sub at one level: dense and strided, one plaintext for the batch and one per item, plain_coeff_count 1, N - 3, N, BGV under the correction
    factors 1, 3, t - 1: the whole buffer -- c0, c1, a third polynomial, the padding of a strided batch -- against the model.  -> boundary classes met"""
    N, primes = S.N, S.primes[:limbs]
    H, calls = Hits(), 0
    for count in counts or (1, N - 3, N):
        for cf in cfs or ((1, 3, S.t - 1) if S.scheme == BGV else (1,)):
            for per_item in per_items:
                pts = craft_batch(S, limbs, count, batch, seed + count + cf % 7, per_item)
                if count >= 16:
                    for b in range(batch if per_item else 1):  # every full-size plaintext by itself shows every class
                        Hb = Hits()
                        look_classes(S, limbs, Hb, pts[b])
                        Hb.check(cannot(S, limbs), (S.name, limbs, "plaintext", b))
                look_classes(S, limbs, H, pts)
                for size, cap in layouts:
                    for sub in (False, True):
                        xs = synth.uniform_ct(seed + 31 * size + sub, primes, size, N, batch)
                        for b in range(batch):
                            edge_c0(S, xs[b], pts[b], cf)
                        c, full = S.ct(xs, cap, cf)
                        (S.ev.subPlainInplace if sub else S.ev.addPlainInplace)(c, device_plain(pts, per_item), count, per_item=per_item)
                        for b in range(batch):
                            full[b, :size] = add_model(S, xs[b], pts[b], cf, sub)
                        got = S.whole(c)
                        assert np.array_equal(got[:, :size, :, :], full[:, :size]), (S.name, limbs, "count", count, "cf", cf, "per item", per_item, size, cap, "sub", sub)
                        assert np.array_equal(got, full), (S.name, limbs, "the padding of a strided batch changed", count, cf, per_item, size, cap, sub)
                        assert S.canonical(got[:, :size], limbs) and (c.size(), c.correction_factor, c.is_ntt_form) == (size, cf, False)
                        calls += 1
    n = H.check(cannot(S, limbs), (S.name, limbs))
    print(S.name, "limbs", limbs, "add/sub calls", calls, "boundary classes met", n, "unreachable", cannot(S, limbs))
    return n


# ================================================================ check 2: the round trip through decryption
def check_roundtrip(S, limbs, batch=3, seed=40):
    """a zero ciphertext plus the crafted plaintext decrypts to the plaintext: the scaling against the decrypt rounding, without either model.
    BGV adds V = m cf mod t as it stands, and decryption reads c0 centred: a V above (q - 1) / 2 -- which exists only where 2 t > q + 1, here at the last
    level of wide59 (a 59-bit t under one 60-bit prime), for the 9600 values from (q + 1) / 2 to t - 1, m = t - 1 among them -- stands for V - q there, so
    such a coefficient returns (V - q) cf^-1 mod t by the definition of the scheme and not m; everywhere else the plaintext itself is asserted"""
    N, t, q = S.N, S.t, S.q(limbs)
    cfs = (1, 3, 5) if math.gcd(15, t) == 1 else (1, 2, 17)  # 2^60 - 1 is a multiple of 3 and of 5: decryption refuses a factor without an inverse
    assert all(math.gcd(cf, t) == 1 for cf in cfs)
    if S.scheme == BGV and cfs != (1, 3, 5):  # and that is what happens: the sum is formed, its decryption refused
        c, _ = S.ct(np.zeros((batch, 2, limbs, N), dtype=np.uint64), None, 3)
        S.ev.addPlainInplace(c, device_plain(craft_batch(S, limbs, N, batch, seed), True), N, per_item=True)
        HC.with_raises(capi.LogicError, "invalid correction factor", lambda: S.ev.decrypt(c, S.secret()))
    for cf in (cfs if S.scheme == BGV else (1,)):
        for count in (N, N - 3):
            pts = craft_batch(S, limbs, count, batch, seed + cf)
            H = Hits()
            look_classes(S, limbs, H, pts)
            H.check(cannot(S, limbs), (S.name, limbs))
            c, _ = S.ct(np.zeros((batch, 2, limbs, N), dtype=np.uint64), None, cf)
            S.ev.addPlainInplace(c, device_plain(pts, True), count, per_item=True)
            got = S.ev.decrypt(c, S.secret())
            exp = np.zeros((batch, N), dtype=np.uint64)
            exp[:, :count] = pts
            if S.scheme == BGV and 2 * t > q + 1:
                V = obj(pts) * cf % t
                wraps = V > (q - 1) // 2
                assert wraps.any() and wraps.sum() <= batch * 2, (S.name, limbs, "coefficients that stand for V - q", int(wraps.sum()))
                exp[:, :count] = u64(np.where(wraps, (V - q) % t * pow(cf, -1, t) % t, obj(pts)))
            else:
                assert S.scheme == BFV or 2 * t <= q + 1
            assert np.array_equal(got, exp), (S.name, limbs, "cf", cf, "count", count, np.argwhere(got != exp)[:8])


# ================================================================ check 3: the lift and plain_to_ntt
def dirty_arena(S, limbs, batch, size=2, seed=5):
    """a multiply_plain with a FULL uniform plaintext per item: the arena words a later call's lifted plaintexts take are nonzero afterwards"""
    c, _ = S.ct(synth.uniform_ct(seed, S.primes[:limbs], size, S.N, batch))
    S.ev.multiplyPlainNormalInplace(c, api.DeviceBuffer.from_numpy(synth.uniform_rows(seed + 1, [S.t], batch, S.N)), S.N, per_item=True)


def plain_to_ntt_into(S, plain, count_coeffs, stride, limbs, out, count):
    capi.check(S.lib, S.lib.troyhip_plain_to_ntt(S.ctx.h, C.c_void_p(plain.ptr), C.c_uint64(count_coeffs), C.c_uint64(stride), int(limbs), C.c_void_p(out.ptr),
                                                 C.c_uint64(count), None))


def check_lift(S, limbs, count=3, seed=60):
    """troyhip_plain_to_ntt of `count` plaintexts with a per-item stride (and of one shared plaintext) at plain_coeff_count 1, 4, N - 3, N, into a
    destination that holds 64-bit junk: NTT of the lifted rows, zero from plain_coeff_count on.  Through Evaluator.transformPlainToNtt too"""
    N = S.N
    H = Hits()
    for pcc in (1, 4, N - 3, N):
        pts = craft_batch(S, limbs, pcc, count, seed + pcc)
        look_classes(S, limbs, H, pts)
        exp = np.stack([ntt_model(S, lift_model(S, limbs, pts[b])) for b in range(count)])
        dirty_arena(S, limbs, count)
        for n_items, stride in ((count, pcc), (1, 0)):
            out = api.DeviceBuffer.from_numpy(synth.splitmix64_stream(seed + pcc, n_items * limbs * N) | np.uint64(1 << 63))
            plain_to_ntt_into(S, api.DeviceBuffer.from_numpy(pts), pcc, stride, limbs, out, n_items)
            got = out.to_numpy().reshape(n_items, limbs, N)
            assert np.array_equal(got, exp[:n_items]), (S.name, limbs, "plain_coeff_count", pcc, "items", n_items)
            assert S.canonical(got, limbs)
        got = S.ev.transformPlainToNtt(api.DeviceBuffer.from_numpy(pts), limbs, pcc, count=count).to_numpy().reshape(count, limbs, N)
        assert np.array_equal(got, exp), (S.name, limbs, "transformPlainToNtt", pcc)
    return H.check(cannot(S, limbs), (S.name, limbs))


# ================================================================ check 4: multiply_plain in coefficient form
MUL_LAYOUTS = ((2, None), (2, 3), (3, None), (3, 4))


def check_multiply(S, limbs, batch=3, seed=80):
    """sizes 2 and 3, dense and strided, a shared and a per-item SPARSE boundary plaintext (at most eight coefficients set: the model is that many
    signed rotations), after a call that left the arena nonzero.  The strided per-item form is the host loop over `temp + b * pw`"""
    N, primes = S.N, S.primes[:limbs]
    H = Hits()
    for a, (size, cap) in enumerate(MUL_LAYOUTS):
        for per_item in (False, True):
            pcc = (N - 3, N, 4, N - 3)[(a + per_item) % 4]
            pts = craft_batch(S, limbs, pcc, batch, seed + 8 * a + per_item, per_item, sparse=True)
            look_classes(S, limbs, H, pts)
            xs = synth.uniform_ct(seed + a, primes, size, N, batch)
            dirty_arena(S, limbs, batch, size)
            c, full = S.ct(xs, cap)
            S.ev.multiplyPlainNormalInplace(c, device_plain(pts, per_item), pcc, per_item=per_item)
            for b in range(batch):
                full[b, :size] = negacyclic_sparse(S, xs[b], pts[b])
            got = S.whole(c)
            assert np.array_equal(got[:, :size], full[:, :size]), (S.name, limbs, size, cap, "per item", per_item, "plain_coeff_count", pcc)
            assert np.array_equal(got, full), (S.name, limbs, "the padding of a strided batch changed", size, cap, per_item)
            assert S.canonical(got[:, :size], limbs) and not c.is_ntt_form
    return H.check(cannot(S, limbs), (S.name, limbs))


# ================================================================ check 5: CKKS rows and NTT-form products
def pattern_rows(primes, rows, N, seed, shift):
    """[rows][N] of row r's prime: coefficient n takes pattern (n // 4^shift) % 4 of 0, 1, 2, p - 1 for n < 16, uniform residues elsewhere -- two operands
    with shifts 0 and 1 meet in all sixteen pairs (0, 1, p - 1 alone never sum to p + 1: that takes the 2)"""
    out = synth.uniform_rows(seed, primes, rows, N)
    for r in range(rows):
        p = primes[r % len(primes)]
        for n in range(min(16, N)):
            out[r, n] = (0, 1, 2, p - 1)[(n // 4 ** shift) % 4]
    return out


def check_ckks_rows(S, limbs, batch=3, seed=120):
    """add_plain_rows_kernel<SUB> and mul_plain_kernel at one CKKS level on residue pairs from 0, 1, 2, p - 1: a + b = p - 1, p, p + 1 (wraps exactly and by one),
    a - b = -1, 0, 1, (p - 1)(p - 1), (p - 1) 1 and 0: limb-wise sums and products modulo p_l.  Sizes 2 and 3, dense and strided; the sums also with one
    plaintext per item"""
    N, primes = S.N, S.primes[:limbs]
    H = Hits()
    scale = 2.0 ** 20
    for a, (size, cap) in enumerate(MUL_LAYOUTS):
        xs = pattern_rows(primes, batch * size * limbs, N, seed + a, 0).reshape(batch, size, limbs, N)
        for per_item in (False, True):
            pl = pattern_rows(primes, batch * limbs, N, seed + 50 + a + per_item, 1).reshape(batch, limbs, N)
            if not per_item:
                pl[:] = pl[0]
            for op in ("add", "sub", "mul"):
                if op == "mul" and per_item:
                    continue  # troyhip_multiply_plain_ntt takes one plaintext for the batch
                c, full = S.ct(xs, cap, scale=scale)
                buf = api.DeviceBuffer.from_numpy(pl if per_item else pl[0])
                if op == "mul":
                    S.ev.multiplyPlainInplace(c, buf, scale)
                else:
                    (S.ev.subPlainInplace if op == "sub" else S.ev.addPlainInplace)(c, buf, plain_scale=scale, per_item=per_item)
                for l, p in enumerate(primes):
                    A, Bv = obj(xs[:, :, l]), obj(pl[:, None, l])
                    if op == "mul":
                        full[:, :size, l] = u64(A * Bv % p)
                        H.look("p%d: (p-1)(p-1)" % l, (A == p - 1) & (Bv == p - 1))
                        H.look("p%d: (p-1) 1" % l, (A == p - 1) & (Bv == 1))
                        H.look("p%d: 0" % l, (A == 0) | (Bv == 0))
                    else:
                        full[:, 0, l] = u64((A[:, 0] + (-Bv[:, 0] if op == "sub" else Bv[:, 0])) % p)
                        for nm, v in (("p-1", p - 1), ("p", p), ("p+1", p + 1)):
                            H.look("p%d: a+b=%s" % (l, nm), A[:, 0] + Bv[:, 0] == v)
                        for nm, v in (("-1", -1), ("0", 0), ("1", 1)):
                            H.look("p%d: a-b=%s" % (l, nm), A[:, 0] - Bv[:, 0] == v)
                got = S.whole(c)
                assert np.array_equal(got, full), (S.name, limbs, op, size, cap, "per item", per_item)
                assert S.canonical(got[:, :size], limbs) and c.is_ntt_form and c.scale == (scale * scale if op == "mul" else scale)
    return H.check((), (S.name, limbs))


# ================================================================ check 6: multiply_plain_accumulate at its bound
def check_accumulate(N, size, uniform=False, batch=3, terms=16, seed=160):
    """CKKS over [60, 60, 60] at ring size N, 16 terms: every ciphertext and plaintext residue p - 1 -- the exact sum 16 (p - 1)^2 exceeds 2^123 -- or
    (uniform) seeded residues, against sum_i ct_i plain_i mod p_l.  One operand is strided, one operand buffer serves two terms.  N = 2 and 4: the
    kernel's `span` takes another shape"""
    primes = [int(p) for p in api.CoeffModulus.Create(N, [60, 60, 60])]
    ctx = api.SEALContext(CKKS, N, primes, 0)
    ev = api.Evaluator(ctx)
    limbs = ctx.first_limbs
    q = primes[:limbs]
    assert limbs == 2 and all(p.bit_length() == 60 for p in q)
    cts, pls, hx, hp = [], [], [], []
    for i in range(terms):
        if i == 5:  # the operand buffer of term 2 once more, under another plaintext
            cts.append(cts[2])
            hx.append(hx[2])
        else:
            x = synth.uniform_ct(seed + i, q, size, N, batch) if uniform else synth.edge_ct("max", seed + i, q, size, N, batch)
            cts.append(api.Ciphertext.from_numpy(ctx, x, True, 2.0 ** 20, capacity=size + 1 if i == 1 else None))
            hx.append(x)
        w = synth.uniform_rows(seed + 100 + i, q, limbs, N) if uniform else synth.edge_rows("max", seed + 100 + i, q, limbs, N)
        pls.append(api.DeviceBuffer.from_numpy(w))
        hp.append(w)
    got = ev.multiplyPlainAccumulate(cts, pls, 2.0 ** 10).cpu()
    exp = np.zeros((batch, size, limbs, N), dtype=np.uint64)
    for l, p in enumerate(q):
        total = sum(obj(hx[i][:, :, l]) * obj(hp[i][None, None, l]) for i in range(terms))
        if not uniform:
            assert (total == 16 * (p - 1) ** 2).all() and 16 * (p - 1) ** 2 > 1 << 123
        exp[:, :, l] = u64(total % p)
    assert got.shape == exp.shape and np.array_equal(got, exp), ("N", N, "size", size, "uniform", uniform)
    assert all((got[:, :, l] < np.uint64(p)).all() for l, p in enumerate(q))


# ================================================================ check 7: what leans on these kernels
def check_encrypt(S, batch=3, seed=200):
    """troyhip_encrypt and troyhip_encrypt_symmetric of the crafted plaintexts (first level, one per item, plain_coeff_count N - 3 and N, dense and
    strided results) against troyhip_host_encrypt / _symmetric with the same seeds, byte for byte: the host form divides in 128 bits directly"""
    import enc_cases as E
    ES = E.Setup(S.scheme, S.N, S.primes, S.t)
    limbs = ES.ctx.first_limbs
    assert limbs == S.levels[0]
    for k, (count, pad) in enumerate(((S.N - 3, 0), (S.N, S.N), (1, 0))):
        pts = craft_batch(S, limbs, count, batch, seed + k)
        if count > 16:
            H = Hits()
            look_classes(S, limbs, H, pts)
            H.check(cannot(S, limbs), (S.name, limbs))
        for form in ("pk", "sk"):
            seeds = E.seeds_for(batch, base=seed + k)
            dev, st = ES.device(form, seeds, limbs, pts, True, None, pad=pad)
            for b in range(batch):
                assert np.array_equal(dev[b], ES.host(form, seeds[b], limbs, pts[b])), (S.name, form, "count", count, "item", b)
        dev, _ = ES.device("pk", seeds, limbs, pts, False, None, pad=pad)  # one plaintext for every item
        for b in range(batch):
            assert np.array_equal(dev[b], ES.host("pk", seeds[b], limbs, pts[0])), (S.name, "shared", count, b)


def check_combine_constant(S, limbs, seed=220):
    """Evaluator.linearCombination on a zero weight: coefficient 0 of c0 is the model's value of the constant, for the constants crafted by the same rule
    -- computed on the host, a third implementation of the rounding -- and equals what add_plain adds for the one-coefficient plaintext"""
    N, primes = S.N, S.primes[:limbs]
    vals, _ = boundary_values(S, limbs)
    H = Hits()
    for cf in ((1, 3) if S.scheme == BGV else (1,)):
        for name, cst in vals:
            look_classes(S, limbs, H, np.array([cst], dtype=np.uint64))
            x = synth.uniform_ct(seed, primes, 2, N, 2)
            c, _ = S.ct(x, None, cf)
            got = S.ev.linearCombination([c], [0], constant=cst).cpu()
            exp = np.zeros_like(x)
            v = int(add_value(S, limbs, np.array([cst], dtype=np.uint64), cf)[0])
            for l, p in enumerate(primes):
                exp[:, 0, l, 0] = v % p
            assert np.array_equal(got, exp), (S.name, limbs, name, "cf", cf)
            z, _ = S.ct(np.zeros_like(x), None, cf)
            S.ev.addPlainInplace(z, api.DeviceBuffer.from_numpy(np.array([cst], dtype=np.uint64)), 1)
            assert np.array_equal(z.cpu(), exp), (S.name, limbs, name, "add_plain of the constant")
    return H.check(cannot(S, limbs), (S.name, limbs))


# ================================================================ check 8: the refusals
def check_refusals(S, SC):
    """S: a BFV set, SC: the CKKS set.  The status class and the message evaluator.cpp gives"""
    N, L = S.N, S.levels[0]
    inv = capi.InvalidArgument
    x = synth.uniform_ct(1, S.primes[:L], 2, N, 2)
    pt = api.DeviceBuffer.from_numpy(synth.uniform_rows(2, [S.t], 2, N))
    fresh = lambda ntt=False: api.Ciphertext.from_numpy(S.ctx, x, ntt)  # noqa: E731

    class Null:
        ptr = None
    bad = "plain is not valid for encryption parameters"
    HC.with_raises(inv, bad, lambda: S.ev.addPlainInplace(fresh(), Null))
    HC.with_raises(inv, bad, lambda: S.ev.subPlainInplace(fresh(), Null))
    HC.with_raises(inv, bad, lambda: S.ev.multiplyPlainNormalInplace(fresh(), Null))
    HC.with_raises(inv, bad, lambda: S.ev.transformPlainToNtt(Null, L))
    HC.with_raises(inv, "plain_ntt is not valid for encryption parameters", lambda: S.ev.multiplyPlainInplace(fresh(True), Null))
    for fn in (S.ev.addPlainInplace, S.ev.subPlainInplace, S.ev.multiplyPlainNormalInplace):
        HC.with_raises(inv, bad, lambda: fn(fresh(), pt, N + 1))
    HC.with_raises(inv, bad, lambda: S.ev.transformPlainToNtt(pt, L, N + 1))
    HC.with_raises(inv, "BFV encrypted cannot be in NTT form", lambda: S.ev.addPlainInplace(fresh(True), pt))
    HC.with_raises(inv, "NTT form mismatch", lambda: S.ev.multiplyPlainNormalInplace(fresh(True), pt))
    HC.with_raises(inv, "encrypted_ntt is not in NTT form", lambda: S.ev.multiplyPlainInplace(fresh(), pt))
    out = api.DeviceBuffer((S.K + 1) * N)
    for limbs in (0, S.K + 1, -1):
        HC.with_raises(inv, "parms_id is not valid for the current context", lambda: plain_to_ntt_into(S, pt, N, 0, limbs, out, 1))
    for limbs in (1, S.K):  # the ends of 1 .. K are accepted
        S.ev.transformPlainToNtt(pt, limbs)
    a = fresh()
    S.ev.addPlainInplace(a, pt, N)  # and nothing above left the context unusable
    assert np.array_equal(a.cpu()[0], add_model(S, x[0], pt.to_numpy(N), 1, False))
    # CKKS
    Lc = SC.levels[0]
    xc = synth.uniform_ct(3, SC.primes[:Lc], 2, N, 2)
    pc = api.DeviceBuffer.from_numpy(synth.uniform_rows(4, SC.primes[:Lc], Lc, N))
    scale = 2.0 ** 20
    cc = lambda ntt=True: api.Ciphertext.from_numpy(SC.ctx, xc, ntt, scale)  # noqa: E731
    HC.with_raises(inv, "CKKS encrypted must be in NTT form", lambda: SC.ev.multiplyPlainNormalInplace(cc(False), pc))
    HC.with_raises(inv, "CKKS encrypted must be in NTT form", lambda: SC.ev.addPlainInplace(cc(False), pc, plain_scale=scale))
    HC.with_raises(inv, bad, lambda: SC.ev.transformPlainToNtt(pc, Lc))
    eps = 2.0 ** -23
    below = eps - 2.0 ** -32  # the largest difference below the bound that a scale of 2^20 can show
    assert (scale + eps) - scale == eps and (scale + below) - scale == below < eps
    HC.with_raises(inv, "scale mismatch", lambda: SC.ev.addPlainInplace(cc(), pc, plain_scale=scale + eps))   # at the bound: refused
    HC.with_raises(inv, "scale mismatch", lambda: SC.ev.subPlainInplace(cc(), pc, plain_scale=scale - eps))
    b = cc()
    SC.ev.addPlainInplace(b, pc, plain_scale=scale + below)  # just below it: accepted, and the scale stays the ciphertext's
    assert b.scale == scale
    exp = xc.copy()
    for l, p in enumerate(SC.primes[:Lc]):
        exp[:, 0, l] = u64((obj(xc[:, 0, l]) + obj(pc.to_numpy(N, l * N))[None]) % p)
    assert np.array_equal(b.cpu(), exp)


# ================================================================ check 9 (device only): the route a large launch takes
def check_large_launch(S, limbs, count, seed=300):
    """plain_to_ntt over `count` plaintexts, one per item, then multiply_plain of a size-2 batch with the same plaintexts: the crafted rows (the first and
    the last three items) and every 37th item against the models (the product through the transform: pointwise in NTT form).  -> the path-counter deltas
    of the two calls"""
    N, primes = S.N, S.primes[:limbs]
    pts = synth.uniform_rows(seed, [S.t], count, N)
    crafted = [0, 1, 2, count - 3, count - 2, count - 1]
    for k, b in enumerate(crafted):
        pts[b] = craft_plain(S, limbs, N, seed + b, 3 * k)
        if k & 1:
            pts[b, N - 3:] = 0
    H = Hits()
    look_classes(S, limbs, H, pts[crafted])
    H.check(cannot(S, limbs), (S.name, limbs))
    sample = sorted(set(crafted) | set(range(0, count, 37)))
    dpts = api.DeviceBuffer.from_numpy(pts)
    s0 = HC.route_stats()
    out = S.ev.transformPlainToNtt(dpts, limbs, N, count=count)
    d_ntt = HC.delta(HC.route_stats(), s0)
    lifted = {}
    for b in sample:
        lifted[b] = ntt_model(S, lift_model(S, limbs, pts[b]))
        assert np.array_equal(out.to_numpy(limbs * N, b * limbs * N).reshape(limbs, N), lifted[b]), (S.name, "plain_to_ntt, item", b)
    del out
    x = synth.uniform_rows(seed + 1, primes, 2 * limbs, N).reshape(2, limbs, N)
    xs = np.broadcast_to(x, (count, 2, limbs, N)).copy()
    xs[:, 0, 0, 0] = np.arange(count, dtype=np.uint64)  # every item its own operand
    c = api.Ciphertext.from_numpy(S.ctx, xs)
    s0 = HC.route_stats()
    S.ev.multiplyPlainNormalInplace(c, dpts, N, per_item=True)
    d_mul = HC.delta(HC.route_stats(), s0)
    for b in sample:
        got = c.buf.to_numpy(2 * limbs * N, b * c.bstride).reshape(2, limbs, N)
        for i in range(2):
            xn = ntt_model(S, xs[b, i])
            prod = np.stack([u64(obj(xn[l]) * obj(lifted[b][l]) % p) for l, p in enumerate(primes)])
            assert np.array_equal(got[i], ntt_model(S, prod, inverse=True)), (S.name, "multiply_plain, item", b, "polynomial", i)
    print(S.name, "count", count, "counters: plain_to_ntt", d_ntt, "multiply_plain", d_mul)
    return d_ntt, d_mul


# ================================================================ the cases both test files run (each file keeps its own setups: its own library)
def add_case(cache, scheme, name, limbs):
    check_add(setup_in(cache, scheme, name), limbs)


def add_many_workgroups(cache, scheme):
    """N = 4096, batch 2: items x plain_coeff_count coefficients make 32 workgroups, the last one ragged at N - 3"""
    S = setup_in(cache, scheme, "small", 4096)
    for limbs in S.levels:
        check_add(S, limbs, batch=2, counts=(S.N - 3, S.N) if limbs == S.levels[0] else (S.N - 3,), cfs=(1, S.t - 1) if scheme == BGV else (1,),
                  layouts=((2, 3), (3, None)), per_items=(True,), seed=11)


def per_level(fn, cache, scheme, name):
    S = setup_in(cache, scheme, name)
    for limbs in S.levels:
        fn(S, limbs)


def at_level(fn, cache, scheme, name, limbs):
    fn(setup_in(cache, scheme, name), limbs)
