"""Shared checks of the two BEHZ base conversions inside BFV multiply -- the extension q -> Bsk with its small Montgomery step and the floor with the
Shenoy-Kumaresan step back to q -- on crafted boundaries, for the three kernel families (behz3.hip FP64, behz2.hip matrix cores, behz.hip VALU).
Used by tests/test_device_behz.py (emulator build) and tests/test_gpu_behz.py (MI355X).

Uniform residues meet none of the values these kernels branch or round on (a centred m~ residue of 2^31, a sum that is an exact multiple of the
output prime, a digit row near its bound).  As tests/round_cases.py does for the divide-and-round steps, the inputs are BUILT:
  * the second operand is a constant ciphertext b = (c, 0), c an integer written to coefficient 0 of b's first polynomial; the negacyclic product
    then maps coefficient n of a to coefficient n of the result, polynomial for polynomial, and the third result polynomial is zero: the whole
    multiply is coefficient-wise, and every coefficient of a can carry its own boundary;
  * Model restates the reference's step sequence per coefficient in Python integers (rns.cpp fastbconvmTilde + smMrq, times t, fastFloor,
    fastbconvSk) over the bases the LIBRARY chose (ctx.behz_bases: the auxiliary primes are its own) and returns its intermediates.  The result of
    the sequence does not depend on the auxiliary base, so the model is held against the oracle's multiply (reference base), once per distinct
    item, bit for bit;
  * the hit report (round_cases.Hits) looks every named boundary up in the model's intermediates of the built input, per family and per prime.
All comparisons are bit-exact, and every output word is held below its prime."""
import math

import numpy as np

import grid_cases as G
import hoist_cases as HC
import round_cases as RC
from troy_amd import capi, synth
from troy_amd.capi import BFV

obj = HC.obj
MT = 1 << 32                 # m~
C_BOUND = 2.0 ** 21.4        # behz2.hip: |C_s| < 2^21.4
TRIES = 64                   # seeded candidates per (family, prime, boundary)
UNREACHABLE = ("alpha<0", "a=(m_sk-1)/2", "a=(m_sk+1)/2")  # the only names a case may pass as `cannot`

ROWS = {  # id -> (bits, family, variant inside the family)
    "fp": ([45, 40, 45], "fp", None),
    "fp_wide": ([50] * 7, "fp", None),
    "fp_low": ([35, 34, 35], "fp", None),
    "mfma_small": ([60, 55, 55, 55, 60], "mfma", dict(ext_small=True, floor_small=True, f2_fast=True)),
    "mfma_large": ([60] + [55] * 14 + [60], "mfma", dict(ext_small=False, floor_small=False, f2_fast=True)),
    "mfma_mid": ([45] + [40] * 10 + [45], "mfma", dict(ext_small=False, floor_small=False, f2_fast=True)),
    "mfma_slow": ([32] + [30] * 4 + [32], "mfma", dict(ext_small=True, floor_small=True, f2_fast=False)),
    "valu": ([45] + [40] * 15 + [45], "valu", None),
}

# rows whose base has t q / B >= 1 (the library sizes B m_sk, not B, above t q): there a negative Shenoy-Kumaresan quotient is reachable and is built
NEGATIVE_ALPHA = (("fp_wide", 256), ("mfma_small", 256), ("mfma_small", 4096), ("fp", 4096))  # (fp at N = 4096: t has 20 bits there)


def cannot_for(row, N):
    return UNREACHABLE[1:] if (row, N) in NEGATIVE_ALPHA else UNREACHABLE


PATTERNS = (("7F", 0x7F7F7F7F7F7F7F7F), ("80", 0x8080808080808080), ("7F80", 0x7F807F807F807F80), ("807F", 0x807F807F807F807F),
            ("FF", 0xFFFFFFFFFFFFFFFF), ("lowFF", 0x00000000FFFFFFFF))


def clip(v, q):
    """the byte pattern v cut to the bytes of q and, where it is not below q, its top digit lowered"""
    nb = (q.bit_length() + 7) // 8
    v &= (1 << 8 * nb) - 1
    if v >= q:
        v = (v & ((1 << 8 * (nb - 1)) - 1)) | (((q >> 8 * (nb - 1)) - 1) << 8 * (nb - 1))
    assert 0 <= v < q
    return v


def digits(v):
    """balanced base-256 digits of 64-bit words as the kernels take them (b2_digits; context.cpp balanced_digit): object / uint64 [..] -> int64 [.., 8]"""
    c80 = np.uint64(0x8080808080808080)
    w = np.ascontiguousarray(np.asarray([int(x) % (1 << 64) for x in np.ravel(v)], dtype=np.uint64))
    with np.errstate(over="ignore"):
        d = ((w + c80) ^ c80)
    return d.view(np.int8).reshape(np.shape(v) + (8,)).astype(np.int64)  # little endian: byte k is digit k


class Model:
    """the reference's step sequence per coefficient, in Python integers, over the library's bases of one level"""

    def __init__(self, S, limbs):
        self.S, self.L, self.t = S, limbs, S.t
        self.q = [int(p) for p in S.primes[:limbs]]
        bsk, _ = S.ctx.behz_bases(limbs)
        self.bsk = [int(p) for p in bsk]
        self.B, self.msk = self.bsk[:-1], self.bsk[-1]
        self.nB, self.nBsk = len(self.B), len(self.bsk)
        self.Q, self.PB = math.prod(self.q), math.prod(self.B)
        assert len(set(self.q + self.bsk)) == limbs + self.nBsk and all(p % 2 for p in self.bsk)
        self.punct = [self.Q // p for p in self.q]
        self.ipunct = [pow(self.punct[l] % p, -1, p) for l, p in enumerate(self.q)]
        self.ext_pre = [MT % p * self.ipunct[l] % p for l, p in enumerate(self.q)]          # y_l = x_l m~ (q/q_l)^-1
        self.floor_pre = [self.t % p * self.ipunct[l] % p for l, p in enumerate(self.q)]     # z_l = t dq_l (q/q_l)^-1
        self.neg_inv_q_mt = (-pow(self.Q, -1, MT)) % MT
        self.inv_mt = [pow(MT, -1, p) for p in self.bsk]
        self.inv_q = [pow(self.Q % p, -1, p) for p in self.bsk]
        self.bpunct = [self.PB // p for p in self.B]
        self.ibpunct = [pow(self.bpunct[b] % p, -1, p) for b, p in enumerate(self.B)]
        self.inv_B_msk = pow(self.PB % self.msk, -1, self.msk)
        self.tq_over_B = self.t * self.Q / self.PB
        # the folded rows of the matrix-core form (behz2.hip header; context.cpp): extension E[o][l] = (q/q_l) m~^-1, its extra column q m~^-1
        # against the centred r; floor stage 1 F[o][l] = -(q/q_l) q^-1 [(B/B_o)^-1 | B^-1 mod m_sk]
        self.rows_ext = [[self.punct[l] % p * self.inv_mt[o] % p for l in range(limbs)] + [self.Q % p * self.inv_mt[o] % p] for o, p in enumerate(self.bsk)]
        self.rows_floor = []
        for o, p in enumerate(self.bsk):
            fs = self.inv_q[o] * (self.ibpunct[o] if o < self.nB else self.inv_B_msk % p) % p
            self.rows_floor.append([(-(self.punct[l] % p * fs)) % p for l in range(limbs)])
        self.wd_ext, self.wd_floor = self._wdigits(self.rows_ext), self._wdigits(self.rows_floor)
        self.sums = True  # whether extend / floor also return the digit sums (the builders' candidate runs leave them out)

    def _wdigits(self, rows):
        """[o][l][k][s]: balanced digit s of W[o][l][k] = M[o][l] 2^(8k) mod p_o, canonical"""
        return np.stack([digits(np.array([[m * (1 << 8 * k) % p for k in range(8)] for m in rows[o]], dtype=object)) for o, p in enumerate(self.bsk)])

    # ---- the extension of one operand: x object [L][n] -> intermediates
    def extend(self, x):
        L, I = self.L, {}
        y = np.stack([x[l] * self.ext_pre[l] % p for l, p in enumerate(self.q)])
        conv_mt = sum(y[l] * (self.punct[l] % MT) for l in range(L)) % MT
        r = conv_mt * self.neg_inv_q_mt % MT
        rc = np.where(r >= MT >> 1, r - MT, r)                                           # rns.cpp:973 '>=' (m~ is a power of two)
        ext = []
        for o, p in enumerate(self.bsk):
            conv = sum(y[l] * (self.punct[l] % p) for l in range(L)) % p
            temp = np.where(r >= MT >> 1, r + p - MT, r)
            ext.append((temp * (self.Q % p) + conv) % p * self.inv_mt[o] % p)
        big = (sum(y[l] * self.punct[l] for l in range(L)) + self.Q * rc)
        assert not np.any(big % MT)
        I.update(y=y, r=r, rc=rc, ext=np.stack(ext), big=big // MT)                      # big: the integer the extension stands for, x + (hidden) q
        if self.sums:
            d = np.concatenate([digits(y), digits(rc)[None]])                            # [L + 1][n][8]
            I["C_ext"] = np.einsum("lnk,olks->osn", d, self.wd_ext)                      # the accumulators C_s of the matrix-core form
        return I

    # ---- times t, floor, Shenoy-Kumaresan: dq object [L][n], db object [nBsk][n]
    def floor(self, dq, db):
        L, nB, I = self.L, self.nB, {}
        z = np.stack([dq[l] * self.floor_pre[l] % p for l, p in enumerate(self.q)])
        u = []
        for o, p in enumerate(self.bsk):
            conv = sum(z[l] * (self.punct[l] % p) for l in range(L)) % p
            u.append((self.t % p * db[o] % p + p - conv) % p * self.inv_q[o] % p)
        u = np.stack(u)
        w = [u[b] * self.ibpunct[b] % p for b, p in enumerate(self.B)]
        a = (sum(w[b] * (self.bpunct[b] % self.msk) for b in range(nB)) % self.msk + self.msk - u[nB]) * self.inv_B_msk % self.msk
        alpha = np.where(a > self.msk >> 1, a - self.msk, a)                             # rns.cpp:928 '>'
        out = np.stack([(sum(w[b] * (self.bpunct[b] % p) for b in range(nB)) - alpha * (self.PB % p)) % p for p in self.q])
        I.update(z=z, u=u, a=a, alpha=alpha, out=out)
        if self.sums:
            I["C_floor"] = np.einsum("lnk,olks->osn", digits(z), self.wd_floor)
        return I

    def residues(self, v):
        """integers object [n] -> [L][n]"""
        return np.stack([v % p for p in self.q])

    def times_constant(self, x, c):
        """a coefficient row set x [L][n] of operand a against the constant c of operand b -> intermediates of the result coefficients"""
        X, Cc = self.extend(x), self.extend(self.residues(np.array([c], dtype=object)))
        dq = np.stack([x[l] * (c % p) % p for l, p in enumerate(self.q)])
        db = np.stack([X["ext"][o] * Cc["ext"][o, 0] % p for o, p in enumerate(self.bsk)])
        I = self.floor(dq, db)
        I.update(X)
        I["hidden"] = (X["big"] - self.crt(x)) // self.Q
        I["c_big"] = Cc["big"][0]
        return I

    def crt(self, x):
        return sum(x[l] * self.ipunct[l] % p * self.punct[l] for l, p in enumerate(self.q)) % self.Q

    def fraction(self, I, stage):
        return float(np.abs(I["C_" + stage]).max()) / C_BOUND

    def bias_fraction(self, I, stage):
        """the largest |sum_{s >= 4} C_s 2^(8 (s - 4))|, the high half of the recombined sum, as a fraction of the bias that keeps it positive
        (context.cpp make_k2: bias1 = 2^(8 (nd - 5) + 22), nd the digits of a residue of the output prime)"""
        worst = 0.0
        for o, p in enumerate(self.bsk):
            nd = min(8, p.bit_length() // 8 + 1)
            high = sum(I["C_" + stage][o, s].astype(object) << 8 * (s - 4) for s in range(4, 8))
            worst = max(worst, float(max(abs(int(high.max())), abs(int(high.min())))) / float(1 << (8 * (nd - 5) + 22 if nd >= 5 else 22)))
        return worst


def u64(a):
    return np.asarray(a, dtype=object).astype(np.uint64)


# ================================================================ builders
class Built:
    """coefficient rows of operand a in base q with the name each was built for"""

    def __init__(self, M, c, seed):
        self.M, self.c, self.rng, self.cols, self.names, self.dropped = M, c, np.random.default_rng(seed), [], [], []
        self.inv_ext = [pow(M.ext_pre[l], -1, p) for l, p in enumerate(M.q)]
        self.inv_z = [pow(M.floor_pre[l] * (c % p) % p, -1, p) for l, p in enumerate(M.q)]

    def rand(self, l):
        return int(self.rng.integers(0, self.M.q[l]))

    def add_y(self, name, y):
        self.cols.append([y[l] * self.inv_ext[l] % p for l, p in enumerate(self.M.q)])
        self.names.append(name)

    def add_z(self, name, z):
        self.cols.append([z[l] * self.inv_z[l] % p for l, p in enumerate(self.M.q)])
        self.names.append(name)

    def add_a(self, name, a):
        self.cols.append([a % p for p in self.M.q])
        self.names.append(name)


def constant_for(M, seed):
    """c near q / (2 t), non-zero modulo every q prime: t c / q in (1/2 + 1/64, 1/2 + 1/32), seeded.  (Right at 1/2 the floored value of an even a and
    the conversion's excess are tied to each other, and a small q then skips some values for every multiple.)"""
    step = M.Q // (64 * M.t)
    c = M.Q // (2 * M.t) + step + int(np.random.default_rng(seed).integers(1, 1 << 30)) * step // (1 << 30)
    while any(c % p == 0 for p in M.q):
        c += 1
    return c


def build_centred_r(Bd):
    """r in {0, 2^31 - 1, 2^31, 2^32 - 1}: (q/q_0) mod 2^32 is odd, so the low 32 bits of y_0 follow from the other y_l and the target; a candidate
    whose y_0 is not below q_0 (q_0 of 32 bits) is drawn again"""
    M = Bd.M
    inv_p0 = pow(M.punct[0] % MT, -1, MT)
    inv_nq = pow(M.neg_inv_q_mt, -1, MT)
    for name, r in (("r=0", 0), ("r=2^31-1", (MT >> 1) - 1), ("r=2^31", MT >> 1), ("r=2^32-1", MT - 1)):
        for _ in range(TRIES):
            y = [0] + [Bd.rand(l) for l in range(1, M.L)]
            low = (r * inv_nq - sum(y[l] * (M.punct[l] % MT) for l in range(1, M.L))) * inv_p0 % MT
            y[0] = low + (int(Bd.rng.integers(0, M.q[0] >> 32)) << 32 if M.q[0] >> 32 else 0)
            if y[0] < M.q[0]:
                Bd.add_y(name, y)
                break


def limb_values(q):
    return [("0", 0), ("1", 1), ("q-1", q - 1)] + [(n, clip(v, q)) for n, v in PATTERNS]


def build_limb_patterns(Bd, floor_side=True):
    """y_l (extension input) and z_l (floor stage-1 input) at 0, 1, q_l - 1 and the byte patterns, in every limb position, the others seeded; and every
    limb at q_l - 1 at once, the largest sums a conversion adds up (the FP64 form's are then closest to 2^53)"""
    M = Bd.M
    Bd.add_y("y*=q-1", [p - 1 for p in M.q])
    if floor_side:
        Bd.add_z("z*=q-1", [p - 1 for p in M.q])
    for l, p in enumerate(M.q):
        for n, v in limb_values(p):
            y = [Bd.rand(j) for j in range(M.L)]
            y[l] = v
            Bd.add_y("y%d=%s" % (l, n), y)
            if n != "1" and floor_side:
                z = [Bd.rand(j) for j in range(M.L)]
                z[l] = v
                Bd.add_z("z%d=%s" % (l, n), z)


def pick(Bd, names_targets, cand, key):
    """runs the model on the candidate integers once and keeps, per (name, index into the intermediate `key`, target), the first candidate that shows
    the target"""
    M = Bd.M
    M.sums = False
    I = M.times_constant(M.residues(np.array(cand, dtype=object)), Bd.c)
    M.sums = True
    for name, idx, target in names_targets:
        v = I[key] if idx is None else I[key][idx]
        hit = np.nonzero(v == target)[0]
        if len(hit):
            Bd.add_a(name, cand[int(hit[0])])
        else:
            Bd.dropped.append(name)  # stays a miss in the hit report: nothing is dropped silently
    return I


def build_ext_multiples(Bd):
    """ext_o in {0, p_o - 1}: a = j p_o or j p_o - 1 below q for seeded j; the hidden multiple of q is 0 for about half of them"""
    M = Bd.M
    for o, p in enumerate(M.bsk):
        for name, off in (("ext%d=0" % o, 0), ("ext%d=p-1" % o, 1)):
            hi = max(2, min(M.Q // p, 1 << 62))
            cand = [int(Bd.rng.integers(1, hi)) * p - off for _ in range(TRIES)]
            pick(Bd, [(name, o, (p - off) % p)], [a for a in cand if 0 <= a < M.Q], "ext")


def quotient_one_values(M, count):
    """values V below q / 2^15 whose Shenoy-Kumaresan quotient is exactly 1: V = d B / P, P the product of the first j primes of B (the fewest that
    bring V under q), has w_b = 0 for b >= j and sum_{b < j} w_b P / B_b = d + m P with w_b = d (P / B_b)^-1 mod B_b: the d with m = 1"""
    for j in range(2, M.nB + 1):
        P = math.prod(M.B[:j])
        unit = M.PB // P
        if unit << 27 < M.Q:
            break
    else:
        return []
    out = []
    for d in range(1, 4096):
        if sum(d * pow(P // p, -1, p) % p * (P // p) for p in M.B[:j]) // P == 1:
            out.append(d * unit)
            if len(out) == count:
                break
    return out


def build_floor_multiples(Bd):
    """u_o in {0, p_o - 1}, out_l in {0, q_l - 1}, alpha in {0, 1, the largest the candidates reach}: with c near q / (2 t) the floored value V moves by
    about 1/2 per unit of a, below it by the fast conversion's excess e in [0, L), about L / 2: four multiples k p, sixteen a around
    (k p + L / 2) q / (t c) each (64 candidates per prime and boundary), kept where the model confirms"""
    M, c = Bd.M, Bd.c
    pool, alphas = [], []
    for kind, primes in (("u", M.bsk), ("out", M.q)):
        for i, p in enumerate(primes):
            cand = []
            for k in range(1, 5):
                centre = ((2 * k * p + M.L) * M.Q) // (2 * M.t * c)
                cand += [(centre + d) % M.Q for d in range(-8, 8)]
            assert len(cand) <= TRIES
            I = pick(Bd, [("%s%d=0" % (kind, i), i, 0), ("%s%d=p-1" % (kind, i), i, p - 1)], cand, kind)
            pool += cand
            alphas += [int(v) for v in I["alpha"]]
    top = max(alphas)
    Bd.alpha_top = top  # the largest quotient the candidates reach: |B| - 1 and |B| need a floored value near -B, far outside t q
    Bd.add_a("alpha=top", pool[alphas.index(top)])
    if 1 in alphas:
        Bd.add_a("alpha=1", pool[alphas.index(1)])
    else:
        # a large base: the quotient of a generic value is a sum of |B| uniform fractions, never 1 among a few thousand candidates: four built values,
        # sixteen a around each
        cand = []
        for V in quotient_one_values(M, 4):
            centre = ((2 * V + M.L) * M.Q) // (2 * M.t * c)
            cand += [(centre + e) % M.Q for e in range(-8, 8)]
        pick(Bd, [("alpha=1", None, 1)], cand, "alpha") if cand else Bd.dropped.append("alpha=1")
    Bd.add_a("alpha=0", 0)
    for name, a in (("a=1", 1), ("a=2", 2), ("a=q-1", M.Q - 1), ("a=q-2", M.Q - 2), ("a=q/2", M.Q // 2), ("a=q/2+1", M.Q // 2 + 1)):
        Bd.add_a(name, a)


def signed_row(M, wd, o, s, sign, primes):
    """the input whose digits push accumulator C_s of output o as far as they can: digit k of limb l is +127 where digit s of W[o][l][k] has the wanted
    sign and -128 elsewhere, clipped into [0, q_l) through the top digit.  -> (values per limb, the C_s they give without the extra column)"""
    vals, total = [], 0
    for l, p in enumerate(primes):
        nk = min(8, p.bit_length() // 8 + 1)
        w = [int(wd[o, l, k, s]) * sign for k in range(nk)]
        d = [127 if w[k] > 0 else -128 for k in range(nk)]
        top = 1 << 8 * (nk - 1)
        fits = lambda low: (max(-128, -(low // top)), min(127, (p - 1 - low) // top))  # noqa: E731  the top digits t with 0 <= low + t top < p
        low = sum(d[k] << 8 * k for k in range(nk - 1))
        if fits(low)[0] > fits(low)[1]:  # a negative low part just under a prime just under 2^(8 (nk - 1))
            d[nk - 2] = 127
            low = sum(d[k] << 8 * k for k in range(nk - 1))
        best = fits(low)[1 if w[nk - 1] > 0 else 0]
        d[nk - 1] = best
        v = low + best * top
        assert 0 <= v < p and [int(x) for x in digits(np.array([v], dtype=object))[0]] == d + [0] * (8 - nk)
        vals.append(v)
        total += sum(d[k] * w[k] for k in range(nk)) * sign
    return vals, total


def build_signed_rows(Bd, floor_side=True):
    """section 3: for every Bsk output o, shift s and sign, the sign-matched input of the extension (y_l) and of floor stage 1 (z_l)"""
    M = Bd.M
    Bd.rows = {}
    for o in range(M.nBsk):
        for s in range(8):
            for sign, sn in ((1, "+"), (-1, "-")):
                y, cy = signed_row(M, M.wd_ext, o, s, sign, M.q)
                Bd.add_y("ext row o%d s%d %s" % (o, s, sn), y)
                Bd.rows[len(Bd.cols) - 1] = ("ext", o, s, cy)
                if floor_side:
                    z, cz = signed_row(M, M.wd_floor, o, s, sign, M.q)
                    Bd.add_z("floor row o%d s%d %s" % (o, s, sn), z)
                    Bd.rows[len(Bd.cols) - 1] = ("floor", o, s, cz)


def build_all(M, seed, floor_side=True):
    Bd = Built(M, constant_for(M, seed), seed)
    build_centred_r(Bd)
    build_limb_patterns(Bd, floor_side)
    build_ext_multiples(Bd)
    if floor_side:
        build_floor_multiples(Bd)
    build_signed_rows(Bd, floor_side)
    return Bd


def place(Bd, N, seed, items=None):
    """the built coefficients over both polynomials of `items` items of seeded uniform residues (as many as they need, two at least), at seeded
    positions, the first and the last coefficient among them -> (a [items][2][L][N], {(item, poly, n): index of the built coefficient})"""
    M = Bd.M
    n = len(Bd.cols)
    items = items or max(2, -(-n // N))  # at most half of a polynomial is built, the rest stays uniform
    per = -(-n // (2 * items))
    assert 2 <= per <= N, (n, items, N)
    a = synth.uniform_ct(seed, M.q, 2, N, items)
    where = {}
    for g in range(2 * items):
        it, poly = g % items, g // items  # consecutive coefficients go to different items, then to the other polynomial
        for i, pos in zip(range(g, n, 2 * items), RC.spots(N, per, seed + g)):
            a[it, poly, :, pos] = u64(Bd.cols[i])
            where[(it, poly, pos)] = i
    return a, where


def constant_ct(M, c, N, items):
    b = np.zeros((items, 2, M.L, N), dtype=np.uint64)
    b[:, 0, :, 0] = u64([c % p for p in M.q])
    return b


# ================================================================ the hit report
def report(M, Bd, I, at, rows=True):
    """I: the model's intermediates of ALL coefficients of the built input ([.., n]); at: index of a built coefficient -> the flat coefficient index
    where it was placed; rows: whether the sign-matched rows are looked up too"""
    H = RC.Hits()
    for name in Bd.dropped:
        H.look(name, False)
    col = lambda k, i=None: (I[k] if i is None else I[k][i])  # noqa: E731
    for name, r in (("r=0", 0), ("r=2^31-1", (MT >> 1) - 1), ("r=2^31", MT >> 1), ("r=2^32-1", MT - 1)):
        H.look(name, col("r") == r)
    top = obj([p - 1 for p in M.q])[:, None]
    H.look("y*=q-1", np.all(I["y"] == top, axis=0))
    if "z" in I:
        H.look("z*=q-1", np.all(I["z"] == top, axis=0))
    H.look("hidden=0", I["hidden"] == 0)
    H.look("hidden=-1", I["hidden"] == -1)
    for l, p in enumerate(M.q):
        for n, v in limb_values(p):
            H.look("y%d=%s" % (l, n), col("y", l) == v)
            if n != "1" and "z" in I:
                H.look("z%d=%s" % (l, n), col("z", l) == v)
        if "out" in I:
            H.look("out%d=0" % l, col("out", l) == 0)
            H.look("out%d=p-1" % l, col("out", l) == p - 1)
    for o, p in enumerate(M.bsk):
        H.look("ext%d=0" % o, col("ext", o) == 0)
        H.look("ext%d=p-1" % o, col("ext", o) == p - 1)
        if "u" in I:
            H.look("u%d=0" % o, col("u", o) == 0)
            H.look("u%d=p-1" % o, col("u", o) == p - 1)
    if "alpha" in I:
        for name, v in (("alpha=0", 0), ("alpha=1", 1), ("alpha=top", Bd.alpha_top)):
            H.look(name, I["alpha"] == v)
        for name, v in (("a=1", 1), ("a=2", 2), ("a=q-1", M.Q - 1), ("a=q-2", M.Q - 2), ("a=q/2", M.Q // 2), ("a=q/2+1", M.Q // 2 + 1)):
            H.look(name, I["a_int"] == v)
        # the floored value V is within t q (|V| < t q / 4 + L) and the conversion's sum S in [0, |B| B): the quotient (S - V) / B is in
        # (-t q / B - 1, |B| + 1).  Computed from the base the library built:
        ratio = M.tq_over_B
        small = "t q / B = 2^%.1f < 1: the quotient (S - V) / B of S in [0, |B| B) and |V| < t q is in [0, |B|]" % math.log2(ratio)
        far = "t q / B = 2^%.1f: |alpha| < t q / B + |B| + 1, far below m_sk / 2 = 2^%.1f" % (math.log2(ratio), math.log2(M.msk) - 1)
        for name, mask in zip(UNREACHABLE, (I["alpha"] < 0, I["a"] == (M.msk - 1) // 2, I["a"] == (M.msk + 1) // 2)):
            if np.any(mask):
                H.look(name, mask)
            elif ratio < 1:
                H.cannot(name, small)
            elif name != "alpha<0" and ratio + M.nB + 1 < M.msk // 4:
                H.cannot(name, far)
            else:
                H.look(name, mask)
    for i, (stage, o, s, want) in (Bd.rows if rows else {}).items():
        if stage == "floor" and "z" not in I:
            continue
        got = int(I["C_" + stage][o, s, at[i]])
        if stage == "ext":  # the builder's sum leaves the extra column out: the centred r against q m~^-1
            got -= int(np.dot(digits(I["rc"][at[i]:at[i] + 1])[0], M.wd_ext[o, M.L, :, s]))
        H.look(Bd.names[i], got == want)
    return H


# ================================================================ the checks
def counters(S):
    return [capi.stat(n, S.ctx.lib) for n in G.BEHZ_COUNTERS]


def variant_of(M):
    """the conditions of behz2.hip's launchers, restated: the everything-in-registers kernels (behz2s_*) for the extension (kb <= 2 && nBsk <= 8, tables
    built when KB2 <= 2) and for the floor (kb2 <= 2), and the one-step q-side reduction (f2_fast: every q prime >= 2^33)"""
    kb, kb2 = (M.L + 1 + 3) // 4, (M.nB + 1 + 3) // 4
    return dict(ext_small=kb2 <= 2 and kb <= 2 and M.nBsk <= 8, floor_small=kb2 <= 2, f2_fast=all(p >= 1 << 33 for p in M.q))


def run_family(S, family, fn):
    before = counters(S)
    got = fn()
    delta = [x - b for x, b in zip(counters(S), before)]
    i = G.FAMILY_INDEX[family]
    assert delta[i] >= 2 and sum(delta) == delta[i], (S.name, family, dict(zip(G.BEHZ_COUNTERS, delta)))
    return got


def setup_for(cache, row, N):
    S = RC.setup_in(cache, BFV, N, tuple(ROWS[row][0]), 14 if N < 4096 else 20)
    M = Model(S, S.K - 1)
    if ROWS[row][2] is not None:
        assert variant_of(M) == ROWS[row][2], (row, variant_of(M), M.L, M.nB)
    return S, M


def oracle_multiply(S, a, b=None):
    e = S.orc.square(S.orc.ct(a, False)) if b is None else S.orc.multiply(S.orc.ct(a, False), S.orc.ct(b, False))
    return S.orc.export(e).data


def canonical(S, got, limbs):
    return all((got[..., j, :] < np.uint64(S.primes[j])).all() for j in range(limbs))


def model_items(M, a, cs):
    """the model over every coefficient of a [items][2][L][N], item i against the constant cs[i] -> (expected [items][3][L][N], intermediates over the
    flat index (item, poly, n))"""
    items, _, L, N = a.shape
    parts = []
    for i in range(items):
        x = obj(a[i]).reshape(2, L, N).transpose(1, 0, 2).reshape(L, -1)
        I = M.times_constant(x, cs[i])
        I["a_int"] = M.crt(x)
        del I["c_big"]
        parts.append(I)
    I = {k: np.concatenate([p[k] for p in parts], axis=-1) for k in parts[0]}
    exp = np.zeros((items, 3, L, N), dtype=np.uint64)
    exp[:, :2] = u64(I["out"]).reshape(L, items, 2, N).transpose(1, 2, 0, 3)
    return exp, I


def wide_constant(M, seed):
    """c just below q / 2: the floored value of a uniform a then spreads over (-t q / 4, t q / 4), beyond B where t q / B > 4 |B|"""
    c = M.Q // 2 - int(np.random.default_rng(seed).integers(1, 1 << 16))
    while any(c % p == 0 for p in M.q):
        c -= 1
    return c


def check_row(cache, row, N=256, batch=None, seed=1000, merged=None, cannot=UNREACHABLE):
    """one row of ROWS: builds the input, holds the model against the oracle item by item, the library against the oracle (all words) and the model,
    asserts the family, checks the hit report.  batch None: one call of batch 1 per item; else the items repeated up to that many in one call (the
    routes of large launches).  merged: whether a call is expected to extend both operands in one launch (the family counter: two launches with the
    floor against three).  Where t q / B >= 1 for the base the library built, the Shenoy-Kumaresan quotient CAN be negative: one more item, uniform
    against a constant near q / 2, reaches it, and the case may not name "alpha<0" in `cannot`
    -> the record of the case"""
    S, M = setup_for(cache, row, N)
    if ("built", row, N, seed) not in cache:  # built, modelled and held against the oracle once; the tests that share a shape share it, unchanged
        Bd = build_all(M, seed)
        a, where = place(Bd, N, seed + 1)
        cs = [Bd.c] * a.shape[0]
        if M.tq_over_B >= 1:
            a = np.concatenate([a, synth.uniform_ct(seed + 2, M.q, 2, N, 1)])
            cs.append(wide_constant(M, seed + 2))
        b = np.concatenate([constant_ct(M, c, N, 1) for c in cs])
        exp, I = model_items(M, a, cs)
        for i in range(a.shape[0]):
            ref = oracle_multiply(S, a[i], b[i])
            assert np.array_equal(ref, exp[i]), (row, "the model against the oracle, item", i, np.argwhere(ref != exp[i])[:4])
        for arr in (a, b, exp):
            arr.setflags(write=False)
        cache["built", row, N, seed] = (Bd, a, where, b, exp, I)
    Bd, a, where, b, exp, I = cache["built", row, N, seed]
    items = a.shape[0]
    reps = -(-(batch or items) // items)
    A, Bb = np.tile(a, (reps, 1, 1, 1))[:batch or items], np.tile(b, (reps, 1, 1, 1))[:batch or items]
    kernels = RC.Kernels(S)
    with kernels:
        if batch is None:  # batch 1: one call per item
            got, launches = [], set()
            for i in range(items):
                before = counters(S)
                got.append(run_family(S, ROWS[row][1], lambda: S.ev.multiply(S.ct(A[i:i + 1]), S.ct(Bb[i:i + 1])).cpu())[0])
                launches.add(sum(counters(S)) - sum(before))
            got = np.stack(got)
            assert len(launches) == 1, launches
            launches = launches.pop()
        else:
            before = counters(S)
            got = run_family(S, ROWS[row][1], lambda: S.ev.multiply(S.ct(A), S.ct(Bb)).cpu())
            launches = sum(counters(S)) - sum(before)
    assert got.shape == (len(A), 3, M.L, N)
    for j in range(M.L):
        high = np.argwhere(got[:, :, j] >= np.uint64(S.primes[j]))
        assert not len(high), (row, "words not below their prime, limb", j, "at (item, polynomial, n)", high[:4])
    for i in range(len(A)):
        assert np.array_equal(got[i], exp[i % items]), (row, "item", i, np.argwhere(got[i] != exp[i % items])[:4])
    if merged is not None:
        assert launches == (2 if merged else 3), (row, "extend + floor launches", launches)
    if kernels.on and ROWS[row][2] is not None:  # the names the launches carry (the emulator build records none)
        v = ROWS[row][2]
        assert (RC.calls_of(kernels.calls, "behz2s_extend") > 0) == v["ext_small"] and (RC.calls_of(kernels.calls, "behz2_extend") > 0) != v["ext_small"], kernels.calls
        assert (RC.calls_of(kernels.calls, "behz2s_floor") > 0) == v["floor_small"] and (RC.calls_of(kernels.calls, "behz2_floor") > 0) != v["floor_small"], kernels.calls
        fl = {n: k for n, k in kernels.calls.items() if "floor_sk" in n}
        assert fl and all(("true>" if v["f2_fast"] else "false>") in n for n in fl), kernels.calls  # the floor kernels' last template argument
    at = {i: (it * 2 + poly) * N + pos for (it, poly, pos), i in where.items()}
    H = report(M, Bd, I, at)
    count = H.check(cannot=cannot, what=row)
    rec = dict(log2_tq_over_B=round(math.log2(M.tq_over_B), 1), alpha_min=int(I["alpha"].min()), row=row, N=N, items=items, batch=len(A), built=len(Bd.cols), boundaries=count, nB=M.nB, aux_bits=M.bsk[0].bit_length(), alpha_top=Bd.alpha_top,
               frac_ext=round(M.fraction(I, "ext"), 4), frac_floor=round(M.fraction(I, "floor"), 4), launches=launches,
               bias_ext=round(M.bias_fraction(I, "ext"), 5), bias_floor=round(M.bias_fraction(I, "floor"), 5))
    assert max(rec["frac_ext"], rec["frac_floor"], rec["bias_ext"], rec["bias_floor"]) < 1, rec  # an input that breaks the documented bound is no test of the kernel
    print("behz", rec)
    return rec


def check_square(cache, row, N=256, seed=2000):
    """the same operand twice: one extension serves both factors.  The operand's only non-zero coefficient is coefficient 0 of both polynomials, so the
    product is (a0 a0, 2 a0 a1, a1 a1) at coefficient 0; the extension-side boundaries (centred r, limb patterns, ext_o, the sign-matched rows of the
    extension) are written there across a batch of items"""
    S, M = setup_for(cache, row, N)
    Bd = build_all(M, seed, floor_side=False)
    n = len(Bd.cols)
    items = -(-n // 2)
    cols = Bd.cols + [Bd.cols[0]] * (2 * items - n)
    a = np.zeros((items, 2, M.L, N), dtype=np.uint64)
    a[:, :, :, 0] = u64(cols).reshape(items, 2, M.L)
    x = obj(a[:, :, :, 0]).transpose(2, 0, 1).reshape(M.L, -1)  # flat index: item * 2 + poly
    X = M.extend(x)
    X["hidden"] = (X["big"] - M.crt(x)) // M.Q
    e0, e1 = X["ext"][:, 0::2], X["ext"][:, 1::2]
    x0, x1 = x[:, 0::2], x[:, 1::2]
    exp = np.zeros((items, 3, M.L, N), dtype=np.uint64)
    for k, (fq, fb) in enumerate(((x0 * x0, e0 * e0), (2 * x0 * x1, 2 * e0 * e1), (x1 * x1, e1 * e1))):
        dq = np.stack([fq[l] % p for l, p in enumerate(M.q)])
        db = np.stack([fb[o] % p for o, p in enumerate(M.bsk)])
        exp[:, k, :, 0] = u64(M.floor(dq, db)["out"]).T
    for i in sorted({0, 1, items // 2, items - 1}):
        ref = oracle_multiply(S, a[i])
        assert np.array_equal(ref, exp[i]), (row, "square: the model against the oracle, item", i)
    ct = S.ct(a)
    got = run_family(S, ROWS[row][1], lambda: S.ev.square(ct).cpu())
    assert canonical(S, got, M.L) and np.array_equal(got, exp), (row, "square", np.argwhere(got != exp)[:4])
    both = run_family(S, ROWS[row][1], lambda: S.ev.multiply(ct, ct).cpu())
    assert np.array_equal(both, exp), (row, "multiply(a, a)")
    H = report(M, Bd, X, {i: i for i in range(n)})
    count = H.check(what=row + " square")
    rec = dict(row=row, square=True, items=items, boundaries=count, frac_ext=round(M.fraction(X, "ext"), 4))
    print("behz", rec)
    return rec


def check_multiply_sum(cache, row="mfma_small", N=256, seed=3000):
    """troyhip_multiply_sum with R = 2 pairs, each a built operand against a constant: the tensor sums a0 c0 + a1 c1 go through ONE floor, so the model's
    floor takes the summed products; held against the oracle's stages over the summed products (mulsum_cases.BfvModel, the reference's base)"""
    import mulsum_cases as MS
    S, M = setup_for(cache, row, N)
    limbs = M.L
    assert S.ev.multiplySumMaxTerms(limbs) >= 2
    Bds = [build_all(M, seed + 10 * r) for r in range(2)]
    As = [place(Bd, N, seed + 10 * r + 1, items=2)[0] for r, Bd in enumerate(Bds)]
    Bs = [constant_ct(M, Bd.c, N, 2) for Bd in Bds]
    L = M.L
    xs = [obj(a).transpose(2, 0, 1, 3).reshape(L, -1) for a in As]
    Xs = [M.extend(x) for x in xs]
    Cs = [M.extend(M.residues(np.array([Bd.c], dtype=object))) for Bd in Bds]
    dq = np.stack([sum(xs[r][l] * (Bds[r].c % p) for r in range(2)) % p for l, p in enumerate(M.q)])
    db = np.stack([sum(Xs[r]["ext"][o] * Cs[r]["ext"][o, 0] for r in range(2)) % p for o, p in enumerate(M.bsk)])
    F = M.floor(dq, db)
    exp = np.zeros((2, 3, L, N), dtype=np.uint64)
    exp[:, :2] = u64(F["out"]).reshape(L, 2, 2, N).transpose(1, 2, 0, 3)
    orc = MS.model_of(S, limbs)
    for i in range(2):
        assert np.array_equal(orc.item([(As[r][i], Bs[r][i]) for r in range(2)]), exp[i]), ("multiply_sum: the model against the oracle's stages, item", i)
    got = run_family(S, ROWS[row][1], lambda: MS.mulsum(S, As, Bs))
    assert canonical(S, got, L) and np.array_equal(got, exp), ("multiply_sum", np.argwhere(got != exp)[:4])
    H = RC.Hits()  # the extension side of either pair keeps its boundaries; the floor sees the SUMMED products, whose values are not built
    for r in range(2):
        Xs[r]["hidden"] = (Xs[r]["big"] - M.crt(xs[r])) // M.Q
        Bds[r].dropped = [n for n in Bds[r].dropped if n.startswith("ext")]
        H.merge("pair %d: " % r, report(M, Bds[r], Xs[r], {}, rows=False))
    H.check(what="multiply_sum")
    rec = dict(row=row, multiply_sum=2, frac_ext=round(max(M.fraction(X, "ext") for X in Xs), 4), frac_floor=round(M.fraction(F, "floor"), 4))
    print("behz", rec)
    return rec


def reference_base_child(row="mfma_small", N=256):
    """for a process started under TROYHIP_AUX_BASE=reference: the reference's 61-bit auxiliary primes (nd = 8 digit rows, the largest bias); there
    t q / B < 1, so all three of UNREACHABLE are out of reach"""
    cache = {}
    S, M = setup_for(cache, row, N)
    assert all(p.bit_length() == 61 for p in M.bsk) and [int(p) for p in S.orc.impl.behz_bases(M.L)[0]] == M.bsk, M.bsk
    return check_row(cache, row, N, seed=4000, merged=False)
