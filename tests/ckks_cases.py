"""Shared checks of the CKKS slot encoder and decoder against the definition (tests/ckks_model.py), run on the host forms
(tests/test_ckks_model.py), on the emulator build of the kernels (tests/test_device_ckks.py) and on the MI355X (tests/test_gpu_ckks.py).

A Form is how a check reaches the code: the host form called with one item, or the device form called with a batch of BATCH items whose
plaintexts lie PAD words apart; item ITEM is the one examined, so the item stride and the pad are in play.  The device checks also run
encode_cases.check_ckks over the same batch, which ties every word of every item to the host form, while the model pins the host.

Every expected value, every tolerance and every refusal comes from the model; nothing here reads the library's tables."""
import math
from fractions import Fraction

import numpy as np

import ckks_model as M
import encode_cases as E
from troy_amd import api, capi
from troy_amd.capi import CKKS

BATCH, ITEM, PAD = 3, 2, 7
TOO_LARGE, NOT_FINITE = "encoded values are too large", "encoded values are not finite"

# levels for the constant-slot and crafted-boundary checks (N = 128: every level of each)
CONST_CONFIGS = {  # (their levels: every prefix of the primes, LEVELS below)
    "n128_30x6": dict(scheme=CKKS, N=128, bits=[30] * 6, tbits=0),           # up to 180 bits: wider than 128
    "n128_narrow": dict(scheme=CKKS, N=128, bits=[28, 25, 32, 31], tbits=0),  # narrow primes; the last level is one 28-bit prime
    "n128_60x3": dict(scheme=CKKS, N=128, bits=[60, 60, 60], tbits=0),        # 60-bit primes
}
LEVELS = [(name, limbs) for name in sorted(CONST_CONFIGS) for limbs in range(len(CONST_CONFIGS[name]["bits"]), 0, -1)]
# the smallest ring sizes that reach each kernel route (ENC_LOGS = 11)
ROUTE_CONFIGS = {
    128: dict(scheme=CKKS, N=128, bits=[30] * 6, tbits=0),            # one LDS tile
    2048: dict(scheme=CKKS, N=2048, bits=[40, 30, 30, 40], tbits=0),  # the largest all-LDS run, FINAL
    4096: dict(scheme=CKKS, N=4096, bits=[40, 30, 30, 40], tbits=0),  # first split: the LDS kernel on 2 tiles, the final stage kernel, one decode stage
    8192: dict(scheme=CKKS, N=8192, bits=[60, 40, 40, 60], tbits=0),  # first non-final stage kernel, two decode stages
}


class Form:
    def __init__(self, ctx, device, transform_ctx=None):
        """transform_ctx: a context with device tables for the NTTs that bring plaintexts to and from coefficient form (ctx itself unless it is
        host-only)"""
        self.ctx, self.device, self.tctx, self.N = ctx, device, transform_ctx or ctx, ctx.N
        self.suffix = " (item %d)" % ITEM if device else ""

    def primes(self, limbs):
        return [int(p) for p in self.ctx.coeff_modulus[:limbs]]

    def encode(self, V3, limbs, scale):
        """V3 [BATCH][count][2] -> (status, plaintext [limbs][N] of item ITEM, or the message)"""
        if not self.device:
            return E.ckks_host_encode(self.ctx, V3[ITEM], limbs, scale)
        rc, enc = E.ckks_device_encode(self.ctx, V3, limbs, scale, pad=PAD)
        return (rc, enc[ITEM]) if rc == capi.OK else (rc, enc)

    def decode(self, P3, limbs, scale):
        """P3 [BATCH][limbs][N] -> (status, slots [N/2][2] of item ITEM, or the message)"""
        if not self.device:
            return E.ckks_host_decode(self.ctx, P3[ITEM], limbs, scale)
        rc, dec = E.ckks_device_decode(self.ctx, P3, limbs, scale, pad=PAD)
        return (rc, dec[ITEM]) if rc == capi.OK else (rc, dec)

    def encode_tied(self, V3, limbs, scale):
        """encode; the device form goes through encode_cases.check_ckks, which also ties every word of every item to the host form, encode and
        decode (or finds both refusing alike), and hands back the plaintexts of that same call"""
        if self.device:
            r = E.check_ckks(self.ctx, BATCH, V3.shape[1], limbs, scale, None, pad=PAD, V=V3)
            if r is not None:
                return capi.OK, r[1][ITEM]
        return self.encode(V3, limbs, scale)

    def transform(self, rows, limbs, inverse):
        buf = api.DeviceBuffer.from_numpy(np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1))
        self.tctx.ntt(buf, limbs, self.primes(limbs), inverse=inverse)
        return buf.to_numpy().reshape(limbs, self.N)

    def coefficients(self, plain, limbs):
        """the N centred integers of a plaintext [limbs][N] in NTT form.  A limb that is not a residue of the same integer as the others gives a
        value of the size of Q here, which no bound below lets through."""
        return M.crt_centred_rows(self.transform(plain, limbs, True), self.primes(limbs))

    def plaintext(self, c, limbs):
        """NTT form [limbs][N] of the integer polynomial c"""
        rows = np.array([[int(x) % p for x in c] for p in self.primes(limbs)], dtype=np.uint64)
        return self.transform(rows, limbs, False)


def batch_values(V, scale):
    """V [count][2] as item ITEM of a batch whose other items are of magnitude 1 once scaled, so that no level refuses them"""
    V3 = np.zeros((BATCH,) + V.shape)
    V3[0, :, 0], V3[1, :, 0], V3[1, :, 1] = 1.25 / scale, -0.75 / scale, 0.5 / scale
    V3[ITEM] = V
    return V3


def batch_plains(P):
    P3 = np.zeros((BATCH,) + P.shape, dtype=np.uint64)
    P3[1] = np.roll(P, 1, axis=1)
    P3[ITEM] = P
    return P3


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---------------------------------------------------------------- a. real constant slots: exact
def constant_cases(primes):
    """(v, scale) pairs for a level of these primes"""
    tb = M.total_bits(primes)
    out = []
    for p in primes:  # multiples of a prime, both signs: the residue 0 of a negative value stays 0 (a 60-bit prime has no multiple among the doubles)
        if p < 2**53:
            out += [(float(p), 1.0), (-float(p), 1.0), (-3.0 * p, 1.0), (-float(p) / 4, 4.0)]
    for x in (0.5, 1.5, 2.5, 3.5, 1234566.5, 0.49999999999999994, 2.0**52 - 0.5, 2.0**51 + 0.5):  # ties k + 1/2 at scale 1, and the double below 1/2
        out += [(x, 1.0), (-x, 1.0)]
    for k in (52, 53, 63, 64):  # both sides of 2^k: the branches E < 52, E >= 52 and e > 64 of ckks_split
        for x in (2.0**k, math.nextafter(2.0**k, 0.0), math.nextafter(2.0**k, math.inf), 2.0**k + 2.0**(k - 30) * 3):
            out += [(x, 1.0), (-x, 1.0)]
    out += [(2.0**51 + 0.75, 4.0), (-(2.0**61 + 2.0**20), 8.0)]
    for v in (3.0, -7.77, 1.2345678):
        out += [(v, 2.0**20), (v, 2.0**40), (v, 2.0**80), (-v, 2.0**80)]
    # products that are not representable: the one rounding of v * scale decides (0.3 * 5 lies below 1.5 and rounds to the tie, hence to 2)
    out += [(0.3, 5.0), (-0.3, 5.0), (1.8333333333333333, 3.0), (3.3333333333333335, 1048577.3), (-1.2345678, 1e15 / 3)]
    edge = 2.0**(tb - 2)  # the refusal boundary: 2^(tb-2) is the largest accepted magnitude
    for x in (edge, math.nextafter(edge, math.inf), math.nextafter(edge, 0.0), 2 * edge, edge * 1.5):
        out += [(x, 1.0), (-x, 1.0)]
    out += [(edge / 2.0**20, 2.0**20), (math.nextafter(edge, math.inf) / 2.0**20, 2.0**20)]
    return out


def check_constant_slots(form, limbs):
    """all N/2 slots equal to a real v: every butterfly is x + x or x - x, so coefficient 0 is exactly round_half_away(fl(v * scale)) =: R, the
    others are 0, and the NTT-form plaintext is R mod q_j in every word of limb j; or the call is refused, as the model's rule says"""
    N, primes = form.N, form.primes(limbs)
    tb = M.total_bits(primes)
    assert Fraction(0.3) * 5 < Fraction(3, 2) and 0.3 * 5.0 == 1.5  # the tie that only the rounded product reaches
    seen = set()
    for v, scale in constant_cases(primes):
        V = np.zeros((N // 2, 2))
        V[:, 0] = v
        V3 = batch_values(V, scale)
        x = M.scaled(v, scale)
        refusal = M.encode_refusal(x, tb)
        rc, got = form.encode_tied(V3, limbs, scale)
        what = (limbs, v.hex() if isinstance(v, float) else v, scale)
        if refusal:
            assert (rc, got) == (capi.INVALID_ARGUMENT, refusal + form.suffix), (what, rc, got)
        else:
            assert rc == capi.OK, (what, got)
            R = M.round_half_away(x)
            want = np.array([[R % p] * N for p in primes], dtype=np.uint64)
            assert np.array_equal(got, want), (what, R, [int(got[j, 0]) for j in range(limbs)], [int(np.count_nonzero(got[j] != want[j])) for j in range(limbs)])
        seen.add(refusal)
    assert seen == {None, TOO_LARGE}  # both outcomes occur at every level
    # the boundary itself, by its definition and not through the model's rule: 2^(tb-2) is taken, the next double is not
    edge = 2.0**(tb - 2)
    for sign in (1.0, -1.0):
        V = np.zeros((N // 2, 2))
        V[:, 0] = sign * edge
        assert form.encode(batch_values(V, 1.0), limbs, 1.0)[0] == capi.OK
        V[:, 0] = sign * edge * (1 + 2.0**-52)
        assert form.encode(batch_values(V, 1.0), limbs, 1.0) == (capi.INVALID_ARGUMENT, TOO_LARGE + form.suffix)


def check_not_finite(form, limbs):
    """one infinity or NaN in one slot of one item: refused, and the device names the item"""
    rng = np.random.default_rng(5)
    for bad in (np.inf, -np.inf, np.nan):
        for part in (0, 1):
            V = E.ckks_values(rng, 1, form.N // 2)[0]
            V[form.N // 4 + 1, part] = bad
            V3 = batch_values(V, 2.0**20)
            assert M.encode_refusal(bad, 64) == NOT_FINITE
            assert form.encode_tied(V3, limbs, 2.0**20) == (capi.INVALID_ARGUMENT, NOT_FINITE + form.suffix), (bad, part)


# ---------------------------------------------------------------- b. crafted decode boundaries
def crafted_integers(primes):
    Q = math.prod(primes)
    q0, q1 = primes[0], primes[1] if len(primes) > 1 else 1
    low = Q % 2**64
    out = [0, 1, -1, 2**53 - 1, -(2**53 - 1), 2**52 + 1,
           (Q - 1) // 2, -((Q - 1) // 2), (Q - 1) // 2 - 1,  # the last positive value; `half` itself (cmp == 0); the one before the last
           2**64, -2**64, 2**64 + 1, 2**64 - 1, -(2**64 + 1), -(2**64 - 1),
           -low, -low - 1, -low + 1,  # the no-borrow word differences change sign between words around here
           q0 - 1, q0, -q0, q0 * q1 - 1]  # Garner digits 0 and q_i - 1
    return out


def check_crafted_decode(form, limbs):
    """the plaintext with the constant word R mod q_j in limb j is the constant polynomial R in NTT form: every slot is the same real number, its
    imaginary part exactly 0, within the tolerance of the word-by-word composition -- and exactly R / scale where one conversion is all there is"""
    N, primes = form.N, form.primes(limbs)
    worst = Fraction(0)
    exact_seen = 0
    for R in crafted_integers(primes):
        P = np.array([[R % p] * N for p in primes], dtype=np.uint64)
        Rc = M.crt_centred([R % p for p in primes], primes)
        d = M.word_differences(R, primes)
        assert sum(dw << (64 * w) for w, dw in enumerate(d)) == Rc
        for scale in (1.0, 2.0**20):
            rc, got = form.decode(batch_plains(P), limbs, scale)
            assert rc == capi.OK, got
            assert np.all(got[:, 1] == 0.0), (limbs, R, scale)
            assert np.all(got[:, 0] == got[0, 0]), (limbs, R, scale)
            err = abs(Fraction(float(got[0, 0])) - Fraction(Rc) / Fraction(scale))
            tol = M.compose_tolerance(R, primes, scale)
            assert err <= tol, (limbs, R, scale, float(err), float(tol))
            if abs(Rc) < 2**53 and not any(d[1:]):  # one word, converted exactly, times a power of two
                assert err == 0, (limbs, R, scale, float(err))
                exact_seen += 1
            elif tol:
                worst = max(worst, err / tol)
            if form.device:
                hrc, host = E.ckks_host_decode(form.ctx, P, limbs, scale)
                assert hrc == capi.OK and bits_equal(got, host), (limbs, R, scale)
    assert exact_seen >= 6
    return float(worst)


def check_decode_scale_bound(form, limbs):
    """decode takes the scale 2^(tb-1) and refuses 2^tb"""
    primes = form.primes(limbs)
    tb = M.total_bits(primes)
    P3 = batch_plains(np.array([[1] * form.N for _ in primes], dtype=np.uint64))
    assert not M.decode_scale_refused(2.0**(tb - 1), tb) and M.decode_scale_refused(2.0**tb, tb)
    rc, got = form.decode(P3, limbs, 2.0**(tb - 1))
    assert rc == capi.OK and np.all(got[:, 0] == 2.0**-(tb - 1)) and np.all(got[:, 1] == 0.0)
    assert form.decode(P3, limbs, 2.0**tb) == (capi.INVALID_ARGUMENT, "scale out of bounds")


# ---------------------------------------------------------------- c. against the definition
def spots(N, rng):
    """(coefficients, slots) to examine: all of them at N <= 256, else the fixed ones around the tile and half boundaries plus 8 seeded random"""
    if N <= 256:
        return list(range(N)), list(range(N // 2))
    cs = {j for j in (0, 1, 2047, 2048, 2049, N // 2 - 1, N // 2, N - 1) if j < N} | {int(x) for x in rng.integers(0, N, 8)}
    ss = {0, 1, N // 4 - 1, N // 4, N // 2 - 1} | {int(x) for x in rng.integers(0, N // 2, 8)}
    return sorted(cs), sorted(ss)


def value_sets(N, rng):
    """(name, V [count][2], heavy): the slot vectors of section c"""
    half = N // 2
    out = [("complex", E.ckks_values(rng, 1, half)[0], True),
           ("real, N/2 - 1 slots", E.ckks_values(rng, 1, half - 1, complex_=False)[0], True),
           ("one slot", E.ckks_values(rng, 1, 1)[0], False),
           ("no slot", np.zeros((0, 2)), False)]
    for i in (0, 1, N // 4, half - 1):  # unit vectors: they pin the 3^i slot order
        V = np.zeros((i + 1, 2))
        V[i, 0] = 1.0
        out.append(("e_%d" % i, V, False))
    V = np.zeros((half, 2))
    V[N // 4, 1] = 1.0  # i e_(N/4): an imaginary unit vector through the conjugate half
    out.append(("i e_%d" % (N // 4), V, False))
    return out


def check_encode_definition(form, limbs, V, scales, coeff_spots):
    """|R_j - scale exact_coeff_j| <= 1/2 + (t eta + u) scale max|v| at the examined coefficients.  Returns {scale: (worst |R - exact|, worst
    share of the bound, the integer polynomial)}"""
    N = form.N
    exact = {j: Fraction(M.exact_coeff(V, N, j)) for j in coeff_spots}
    vmax = M.vmax(V)
    out = {}
    for scale in scales:
        V3 = batch_values(V, scale)
        rc, plain = form.encode_tied(V3, limbs, scale)
        assert rc == capi.OK, plain
        c = form.coefficients(plain, limbs)
        bound = Fraction(1, 2) + M.encode_bound(N, scale, vmax)
        worst = Fraction(0)
        for j in coeff_spots:
            err = abs(c[j] - Fraction(scale) * exact[j])
            assert err <= bound, ("coefficient", j, "scale", scale, "error", float(err), "bound", float(bound), c[j])
            worst = max(worst, err)
        out[scale] = (float(worst), float(worst / bound), c)
    return out


def check_decode_definition(form, limbs, c, scale, slot_spots):
    """|got_i - exact_slot_i / scale| <= (t eta + 2 limbs u) sqrt N ||c||_2 / scale in both parts at the examined slots; returns the worst share"""
    N = form.N
    P = form.plaintext(c, limbs)
    rc, got = form.decode(batch_plains(P), limbs, scale)
    assert rc == capi.OK, got
    bound = M.decode_bound(N, limbs, scale, c)
    worst = Fraction(0)
    for i in slot_spots:
        re, im = M.exact_slot(c, N, i)
        for part, want in ((0, re), (1, im)):
            err = abs(Fraction(float(got[i, part])) - Fraction(want) / Fraction(scale))
            assert err <= bound, ("slot", i, part, "scale", scale, "error", float(err), "bound", float(bound))
            worst = max(worst, err)
    if form.device:
        hrc, host = E.ckks_host_decode(form.ctx, P, limbs, scale)
        assert hrc == capi.OK and bits_equal(got, host)
    return float(worst / bound) if bound else 0.0


def route_scales(form, limbs):
    """2^20 and 2^40, plus 2^60 and 2^80 where the level takes slots of magnitude 8 sqrt 2 at that scale"""
    tb = M.total_bits(form.primes(limbs))
    return [s for s in (2.0**20, 2.0**40, 2.0**60, 2.0**80) if s <= 2.0**40 or M.encode_refusal(16.0 * s, tb) is None]


def check_definition(form, limbs, seed=1):
    """section c at one level: encode every value set at every scale against the definition, decode the integer polynomials so obtained and one
    crafted polynomial.  Returns a dict of the worst figures."""
    N = form.N
    rng = np.random.default_rng(seed + N)
    coeff_spots, slot_spots = spots(N, rng)
    scales = route_scales(form, limbs)
    assert len(scales) >= 3
    fig = {"encode |R - exact| at 2^20": 0.0, "encode share": 0.0, "encode share, scale >= 2^60": 0.0, "decode share": 0.0}
    for name, V, heavy in value_sets(N, rng):
        res = check_encode_definition(form, limbs, V, scales if heavy else scales[:2], coeff_spots)
        for scale, (worst, share, c) in res.items():
            if scale == 2.0**20:
                fig["encode |R - exact| at 2^20"] = max(fig["encode |R - exact| at 2^20"], worst)
            key = "encode share, scale >= 2^60" if scale >= 2.0**60 else "encode share"
            fig[key] = max(fig[key], share)
        for scale in (scales if name == "complex" else [2.0**40] if heavy or name.startswith("e_") else []):
            fig["decode share"] = max(fig["decode share"], check_decode_definition(form, limbs, res[scale][2], scale, slot_spots))
    # a polynomial that is no encoder's output: seeded centred integers near scale * 8
    c = [int(x) for x in rng.integers(-8 * 2**40, 8 * 2**40, N, endpoint=True)]
    fig["decode share"] = max(fig["decode share"], check_decode_definition(form, limbs, c, 2.0**40, slot_spots))
    return fig


def report(label, fig):
    print("ckks %s: %s" % (label, ", ".join("%s %.3g" % kv for kv in sorted(fig.items()))))
