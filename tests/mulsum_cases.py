"""Shared checks of the sum of ciphertext products (troyhip_multiply_sum): the acceptance rule of the auxiliary base restated,
byte equality with the composition of existing calls (CKKS, BGV), an exact host model of the BFV definition, the bounds of the lazy sums, the
independence of the result from how it is asked for, real keys, the refusals.  Used by tests/test_device_mulsum.py (emulator build) and
tests/test_gpu_mulsum.py (MI355X).

The BFV model restates the definition independently of the device code and of the library's auxiliary base: the oracle's extension and small Montgomery
step per operand polynomial IN THE REFERENCE'S BASE (61-bit primes), a transform per prime, the tensor sums as Python integers, ONE inverse transform,
the oracle's floor and Shenoy-Kumaresan steps.  The device runs its own base (58- or 50-bit primes where they cost no limb): equal limbs show that the
result does not depend on the base."""
import ctypes as C

import numpy as np

import grid_cases as G
import hoist_cases as HC
from hoist_cases import obj, with_raises
from oracle import oracle
from troy_amd import api, capi, synth
from troy_amd.capi import BFV, BGV, CKKS, CtStruct

ST_FASTBCONV_MTILDE, ST_SMMRQ, ST_FASTFLOOR, ST_FASTBCONV_SK = 0, 1, 2, 3  # oracle/troy_oracle.h ORC_ST_*
MAX_TERMS = 16


def chunks():
    return capi.stat("mulsum_chunks", api.KernelProvider.lib())


# ---------------------------------------------------------------- the acceptance rule, restated
def expected_max_terms(S, limbs):
    """16, or for BFV the largest R <= 16 with 32 + bits(t) + bits(q) + ceil(log2 R) < aux_bits (|B| + 1), from what the context reports"""
    if S.scheme != BFV:
        return MAX_TERMS
    bsk, _ = S.ctx.behz_bases(limbs)
    aux_bits = max(int(p).bit_length() for p in bsk)
    assert all(int(p).bit_length() == aux_bits for p in bsk)
    q = 1
    for p in S.primes[:limbs]:
        q *= p
    need = 32 + S.t.bit_length() + q.bit_length()
    room = aux_bits * len(bsk)  # |Bsk| = |B| + 1
    assert need < room
    best = 0
    for R in range(1, MAX_TERMS + 1):
        if need + (R - 1).bit_length() < room:  # (R - 1).bit_length() == ceil(log2 R)
            best = R
    return best


# ---------------------------------------------------------------- calls
def operands(S, limbs, batch, R, seed, pattern=None):
    """R pairs of host batches [batch][2][limbs][N]"""
    pat = pattern or S.ct_pattern
    mk = lambda s: synth.edge_ct(pat, s, S.primes[:limbs], 2, S.N, batch, ntt_form=S.ntt)  # noqa: E731
    return [mk(seed + 2 * r) for r in range(R)], [mk(seed + 2 * r + 1) for r in range(R)]


def to_cts(S, datas, scale=1.0):
    """one device batch per DISTINCT host array (the same array twice is the same buffer twice); an odd batch is strided (Setup.ct)"""
    made = {}
    out = []
    for d in datas:
        if id(d) not in made:
            made[id(d)] = S.ct(d)
            made[id(d)].scale = scale
        out.append(made[id(d)])
    return out


def mulsum(S, As, Bs, limit=0, scale=1.0):
    """-> [batch][3][limbs][N] through the Python layer"""
    cts = to_cts(S, list(As) + list(Bs), scale)
    out = S.ev.multiplySum(cts[:len(As)], cts[len(As):], scratch_limit_words=limit)
    assert (out.size(), out.limbs, out.is_ntt_form, out.batch) == (3, As[0].shape[2], S.ntt, As[0].shape[0])
    return out.cpu()


def composed(S, As, Bs):
    """multiply per pair, size-3 adds"""
    cts = to_cts(S, list(As) + list(Bs))
    acc = None
    for a, b in zip(cts[:len(As)], cts[len(As):]):
        p = S.ev.multiply(a, b)
        if acc is None:
            acc = p
        else:
            S.ev.addInplace(acc, p)
    return acc.cpu()


def check_composition(S, limbs, batch, R, seed):
    As, Bs = operands(S, limbs, batch, R, seed)
    got, exp = mulsum(S, As, Bs), composed(S, As, Bs)
    assert np.array_equal(got, exp), (S.name, limbs, batch, R)
    assert all((got[:, :, j] < np.uint64(S.primes[j])).all() for j in range(limbs))
    return got


# ---------------------------------------------------------------- the definitions in exact integers
def exact_sum(pairs, primes, trace=None):
    """sum_r a_r (x) b_r of residues that are multiplied as they stand: [3][limbs][N] (CKKS; BGV in the transformed domain)"""
    limbs, N = pairs[0][0].shape[1], pairs[0][0].shape[2]
    acc = np.zeros((3, limbs, N), dtype=object)
    for a, b in pairs:
        a, b = obj(a), obj(b)
        acc[0] += a[0] * b[0]
        acc[1] += a[0] * b[1] + a[1] * b[0]
        acc[2] += a[1] * b[1]
    if trace is not None:
        trace["max_sum"] = max(trace.get("max_sum", 0), int(acc.max()))
        trace["max_middle"] = max(trace.get("max_middle", 0), int(acc[1].max()))
    out = np.zeros((3, limbs, N), dtype=np.uint64)
    for j in range(limbs):
        out[:, j] = (acc[:, j] % primes[j]).astype(np.uint64)
    return out


class BfvModel:
    """out = (floor(t sum_r D_r / q) - alpha') mod q through the oracle's stages in the reference's auxiliary base"""

    def __init__(self, S, limbs):
        self.S, self.L, self.N = S, limbs, S.N
        self.O = oracle.Oracle(oracle.BFV, S.N, S.primes, S.t)
        self.Bsk, _ = self.O.behz_bases(limbs)
        self.nb = len(self.Bsk)
        self.primes = [int(p) for p in S.primes[:limbs]] + [int(p) for p in self.Bsk]
        self.seen = {}

    def transformed(self, poly):
        """R' of one operand polynomial [L][N] in base q u Bsk, transformed: object [L + nb][N]"""
        key = poly.tobytes()
        if key not in self.seen:
            L, nb, N = self.L, self.nb, self.N
            ext = self.O.rns_stage(L, ST_SMMRQ, self.O.rns_stage(L, ST_FASTBCONV_MTILDE, poly, nb + 1), nb)
            rows = list(poly) + list(ext)
            self.seen[key] = np.stack([obj(oracle.ntt_standalone(N, p, rows[i], 1)) for i, p in enumerate(self.primes)])
        return self.seen[key]

    def item(self, pairs, trace=None):
        """pairs [(a [2][L][N], b [2][L][N])] of one item -> [3][L][N]"""
        L, nb, N, t = self.L, self.nb, self.N, self.S.t
        acc = np.zeros((3, L + nb, N), dtype=object)
        for a, b in pairs:
            a0, a1, b0, b1 = (self.transformed(x) for x in (a[0], a[1], b[0], b[1]))
            acc[0] += a0 * b0
            acc[1] += a0 * b1 + a1 * b0
            acc[2] += a1 * b1
        if trace is not None:
            trace["max_sum"] = max(trace.get("max_sum", 0), int(acc.max()))
            trace["max_middle"] = max(trace.get("max_middle", 0), int(acc[1].max()))
        out = np.zeros((3, L, N), dtype=np.uint64)
        for k in range(3):
            rows = []
            for i, p in enumerate(self.primes):
                coeff = obj(oracle.ntt_standalone(N, p, (acc[k, i] % p).astype(np.uint64), 3))
                rows.append((coeff * (t % p) % p).astype(np.uint64))
            out[k] = self.O.rns_stage(L, ST_FASTBCONV_SK, self.O.rns_stage(L, ST_FASTFLOOR, np.stack(rows), nb), L)
        return out


_models = {}


def model_of(S, limbs):
    if (S.name, limbs) not in _models:
        _models[(S.name, limbs)] = BfvModel(S, limbs)
    return _models[(S.name, limbs)]


def check_bfv_model(S, limbs, batch, R, seed, items=None, pattern=None, trace=None):
    As, Bs = operands(S, limbs, batch, R, seed, pattern)
    got = mulsum(S, As, Bs)
    M = model_of(S, limbs)
    for b in (range(batch) if items is None else items):
        exp = M.item([(As[r][b], Bs[r][b]) for r in range(R)], trace)
        assert np.array_equal(got[b], exp), (S.name, limbs, "batch", batch, "R", R, "item", b)
    if R == 1:
        assert np.array_equal(got, composed(S, As, Bs)), (S.name, "R = 1 is troyhip_multiply")
    return got


def check_single_is_multiply(S, limbs, batch, seed):
    As, Bs = operands(S, limbs, batch, 1, seed)
    assert np.array_equal(mulsum(S, As, Bs), composed(S, As, Bs)), (S.name, limbs, batch)


# ---------------------------------------------------------------- bounds of the lazy sums
def check_bounds_ckks(pattern="max"):
    """R = 16 pairs of 60-bit residues p - 1: thirty-two products in the middle sum"""
    S = HC.Setup(*HC.adhoc(CKKS, 64, [60, 60, 60]), patterns=(pattern, "uniform", "uniform"))
    limbs = S.ctx.first_limbs
    As, Bs = operands(S, limbs, 2, MAX_TERMS, 40)
    trace = {}
    got = mulsum(S, As, Bs)
    for b in range(2):
        assert np.array_equal(got[b], exact_sum([(As[r][b], Bs[r][b]) for r in range(MAX_TERMS)], S.primes[:limbs], trace)), (pattern, b)
    assert trace["max_middle"] < 1 << 128 and trace["max_sum"] == trace["max_middle"]
    if pattern == "max":
        assert trace["max_middle"] == 2 * MAX_TERMS * (max(S.primes[:limbs]) - 1) ** 2 > 1 << 123
    return trace


def check_bounds_bfv(pattern):
    S = HC.Setup("bfv_n128_k5_60", patterns=(pattern, "uniform", "uniform"))
    limbs = S.ctx.first_limbs
    R = S.ev.multiplySumMaxTerms(limbs)
    trace = {}
    check_bfv_model(S, limbs, 2, R, 50, trace=trace)
    assert trace["max_middle"] < 1 << 128
    return R, trace


# ---------------------------------------------------------------- independence
def plan(S, limbs, batch, R, limit=0):
    """(items per run, pairs per chunk) as Evaluator::multiply_sum plans them (evaluator.cpp), restated"""
    nb = len(S.ctx.behz_bases(limbs)[0]) if S.scheme == BFV else 0
    mw = S.N * (limbs + nb)
    limit = limit or 1 << 28
    slack = 32 * 8 + 128
    per_item, per_pair_item = 3 * mw, 4 * mw
    if batch * (per_item + per_pair_item) + slack <= limit:
        return batch, min(R, (limit - slack - batch * per_item) // (batch * per_pair_item))
    return (limit - slack) // (per_item + per_pair_item), 1


def scratch_words(S, limbs, items, pairs):
    nb = len(S.ctx.behz_bases(limbs)[0]) if S.scheme == BFV else 0
    return items * S.N * (limbs + nb) * (3 + 4 * pairs) + 32 * 8 + 128


def check_independence(S, limbs, seed, batch=5):
    R = min(3, S.ev.multiplySumMaxTerms(limbs))
    As, Bs = operands(S, limbs, batch, R, seed)
    c0 = chunks()
    ref = mulsum(S, As, Bs)
    assert chunks() - c0 == 1
    # the pairs permuted; a_r and b_r swapped within a pair
    perm = list(range(R))[::-1]
    assert np.array_equal(mulsum(S, [As[i] for i in perm], [Bs[i] for i in perm]), ref), "permuted"
    assert np.array_equal(mulsum(S, [Bs[0]] + As[1:], [As[0]] + Bs[1:]), ref), "swapped"
    # every item alone
    for b in range(batch):
        assert np.array_equal(mulsum(S, [a[b:b + 1] for a in As], [x[b:b + 1] for x in Bs])[0], ref[b]), ("item alone", b)
    if S.scheme != CKKS:  # the chunking (CKKS holds no transformed operands: one launch whatever the limit)
        limit = scratch_words(S, limbs, batch, 1)
        assert plan(S, limbs, batch, R, limit) == (batch, 1)
        c0 = chunks()
        assert np.array_equal(mulsum(S, As, Bs, limit=limit), ref), "one pair per chunk"
        assert chunks() - c0 == R
        limit = scratch_words(S, limbs, 2, 1)
        assert plan(S, limbs, batch, R, limit) == (2, 1)
        c0 = chunks()
        assert np.array_equal(mulsum(S, As, Bs, limit=limit), ref), "runs of two items"
        assert chunks() - c0 == R * -(-batch // 2)
        with_raises(capi.InvalidArgument, "scratch_limit_words is too small", lambda: mulsum(S, As, Bs, limit=scratch_words(S, limbs, 1, 1) - 1))
    if R < S.ev.multiplySumMaxTerms(limbs):
        # a pair whose a_r is all zero changes nothing (BFV: the extension of 0 is 0)
        zero = np.zeros_like(As[0])
        assert np.array_equal(mulsum(S, As[:1] + [zero] + As[1:], Bs[:1] + [Bs[1]] + Bs[1:]), ref), "zero pair"
    # a_r and b_r the same buffer == two copies
    sq = mulsum(S, [As[0]] + As[1:], [As[0]] + Bs[1:])
    assert np.array_equal(sq, mulsum(S, [As[0]] + As[1:], [As[0].copy()] + Bs[1:])), "square"
    # an operand shared by every pair (a vector against the rows of a matrix)
    assert np.array_equal(mulsum(S, As, [Bs[0]] * R), mulsum(S, As, [Bs[0].copy() for _ in range(R)])), "shared operand"
    return ref


# ---------------------------------------------------------------- real ring sizes without a model (device only)
def check_real_size(name, batch=2):
    S = HC.Setup(name)
    limbs = S.ctx.first_limbs
    As, Bs = operands(S, limbs, batch, 4, 60)
    if S.scheme == CKKS:
        assert np.array_equal(mulsum(S, As, Bs), composed(S, As, Bs)), name
        return
    one = composed(S, As[:1], Bs[:1])
    assert np.array_equal(mulsum(S, As[:1], Bs[:1]), one), (name, "R = 1")
    zero = np.zeros_like(As[0])
    assert np.array_equal(mulsum(S, [zero, As[0], zero], [Bs[1], Bs[0], Bs[2]]), one), (name, "R = 3 with two zero pairs")


# ---------------------------------------------------------------- the grid limit
def check_grid_limit(seed=360):
    """launch_tensor_sum (CKKS, N = 16, ONE limb: the last level of a K = 3 modulus), R = 2, more than 65535 items: tensor_sum_kernel's grid z = batch"""
    S = G.setup(CKKS, [50, 40, 50])
    limbs, R = S.ctx.last_limbs, 2
    assert limbs == 1
    batch = G.batch_past()
    assert G.LIMIT + 50 <= batch <= G.LIMIT + 100
    words = 2 * limbs * S.N
    names = ["a0", "b0", "a1", "b1"]
    inputs = {k: (G.fill_ct(S, limbs, 2, batch, seed + i, "alt" if i == 0 else "top"), words) for i, k in enumerate(names)}

    def call(src, dst, lo, n):
        sa = [G.ct_struct(S, src("a%d" % r), 2, limbs, ntt=True) for r in range(R)]
        sb = [G.ct_struct(S, src("b%d" % r), 2, limbs, ntt=True) for r in range(R)]
        pa = (C.POINTER(CtStruct) * R)(*[C.pointer(x) for x in sa])
        pb = (C.POINTER(CtStruct) * R)(*[C.pointer(x) for x in sb])
        out = CtStruct(dst("out"), 3 * limbs * S.N, 0, 0, 0, 0.0, 0)
        capi.check(S.lib, S.lib.troyhip_multiply_sum(S.ctx.h, pa, pb, R, C.byref(out), C.c_uint64(n), C.c_uint64(0), None))
        assert (out.size, out.limbs, out.is_ntt_form) == (3, limbs, 1)

    def ref(b, h):  # the composition's definition in exact integers
        return {"out": exact_sum([(h["a%d" % r].reshape(2, limbs, S.N), h["b%d" % r].reshape(2, limbs, S.N)) for r in range(R)], S.primes[:limbs]).reshape(-1)}

    return G.run(S.name + " multiply_sum", S.lib, batch, inputs, {"out": 3 * limbs * S.N}, call, ref, G.boundary_items(batch))


# ---------------------------------------------------------------- under real keys
class RealSetup(HC.RealSetup):
    def __init__(self, name, cfg=None):
        if cfg is not None:
            HC.BENCH.setdefault(name, cfg)
        super().__init__(name, ())
        self.rlk = api.RelinKeys(self.ctx)
        self.rlk.set(0, self.kg.createRelinKeys())


def check_real_bfv_bgv(name, R=3, batch=2, cfg=None):
    """-> [(fused, composed)] invariant noise budgets (BFV) per item"""
    S = RealSetup(name, cfg)
    rng = np.random.default_rng(11)
    benc = api.BatchEncoder(S.ctx)
    R = min(R, S.ev.multiplySumMaxTerms())
    ma = [[rng.integers(0, S.t, S.N, dtype=np.uint64) for _ in range(batch)] for _ in range(R)]
    mb = [[rng.integers(0, S.t, S.N, dtype=np.uint64) for _ in range(batch)] for _ in range(R)]
    enc = lambda ms: api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(benc.encode(m)) for m in ms]))  # noqa: E731
    As, Bs = [enc(m) for m in ma], [enc(m) for m in mb]
    got = S.ev.innerProduct(As, Bs, S.rlk)
    assert (got.size(), got.limbs, got.is_ntt_form, got.batch) == (2, As[0].limbs, False, batch)
    acc = None
    for a, b in zip(As, Bs):
        p = S.ev.multiply(a, b)
        if acc is None:
            acc = p
        else:
            S.ev.addInplace(acc, p)
    S.ev.relinearizeInplace(acc, S.rlk)
    f, q = got.cpu(), acc.cpu()
    budgets = []
    for b in range(batch):
        cf_f, cf_q = got.correction_factor, acc.correction_factor
        df, dq = S.dec.decrypt(f[b], correction_factor=cf_f), S.dec.decrypt(q[b], correction_factor=cf_q)
        assert np.array_equal(df, dq), (name, b)
        exp = sum(obj(ma[r][b]) * obj(mb[r][b]) for r in range(R)) % S.t
        assert np.array_equal(benc.decode(df), exp.astype(np.uint64)), (name, b)
        if S.scheme == BFV:
            bf, bq = S.dec.invariantNoiseBudget(f[b]), S.dec.invariantNoiseBudget(q[b])
            print(name, "R", R, "item", b, "invariant noise budget fused", bf, "composed", bq)
            assert bq > 0 and bf >= bq - 1, (name, b, bf, bq)
            budgets.append((bf, bq))
    return budgets


def check_real_ckks(name, R=3, batch=2, scale=2.0 ** 25):
    S = RealSetup(name)
    rng = np.random.default_rng(12)
    cenc = api.CKKSEncoder(S.ctx)
    n = S.N // 2
    va = [[rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in range(batch)] for _ in range(R)]
    vb = [[rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in range(batch)] for _ in range(R)]
    enc = lambda vs: api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(cenc.encode(v, scale)) for v in vs]), True, scale)  # noqa: E731
    As, Bs = [enc(v) for v in va], [enc(v) for v in vb]
    got = S.ev.innerProduct(As, Bs, S.rlk)
    assert got.scale == scale * scale and got.is_ntt_form and got.size() == 2
    acc = None
    for a, b in zip(As, Bs):
        p = S.ev.multiply(a, b)
        if acc is None:
            acc = p
        else:
            S.ev.addInplace(acc, p)
    S.ev.relinearizeInplace(acc, S.rlk)
    assert np.array_equal(got.cpu(), acc.cpu()), name
    f = got.cpu()
    for b in range(batch):
        exact = sum(va[r][b] * vb[r][b] for r in range(R))
        err = np.abs(cenc.decode(S.dec.decrypt(f[b]), scale * scale) - exact).max()
        print(name, "item", b, "max slot error", err)
        assert err < 0.1, (name, b, err)  # a smoke check: the limbs are the composition's


# ---------------------------------------------------------------- symbol, counter, query
def check_query(S):
    for limbs in S.levels():
        assert S.ev.multiplySumMaxTerms(limbs) == expected_max_terms(S, limbs), (S.name, limbs)
    assert S.ev.multiplySumMaxTerms() == expected_max_terms(S, S.ctx.first_limbs)


def check_headline_margin():
    """the headline parameters at N = 64: four bits of margin under the library's own base (R <= 8), room for 16 under the reference's"""
    S = HC.Setup(*HC.adhoc(BFV, 64, [60] + [58] * 13 + [60], tbits=20))
    limbs = S.ctx.first_limbs
    mt = S.ev.multiplySumMaxTerms(limbs)
    assert mt == expected_max_terms(S, limbs) and 1 <= mt < MAX_TERMS
    bsk, _ = S.ctx.behz_bases(limbs)
    if max(int(p).bit_length() for p in bsk) == 58:  # the library's own base (not TROYHIP_AUX_BASE=reference)
        assert mt == 8
    As, Bs = operands(S, limbs, 1, mt + 1, 70)
    with_raises(capi.InvalidArgument, "too many products for the auxiliary base", lambda: mulsum(S, As, Bs))
    got = mulsum(S, As[:mt], Bs[:mt])
    assert np.array_equal(got[0], model_of(S, limbs).item([(As[r][0], Bs[r][0]) for r in range(mt)]))
    return mt


# ---------------------------------------------------------------- refusals
def raw_call(S, sa, sb, out_ptr, out_stride, n=None, batch=1, limit=0, ctx=None):
    R = len(sa)
    pa = (C.POINTER(CtStruct) * max(R, 1))(*[C.pointer(x) if x is not None else None for x in sa])
    pb = (C.POINTER(CtStruct) * max(R, 1))(*[C.pointer(x) if x is not None else None for x in sb])
    so = CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    rc = S.lib.troyhip_multiply_sum((ctx or S.ctx).h, pa, pb, R if n is None else n, C.byref(so), C.c_uint64(batch), C.c_uint64(limit), None)
    return (rc, S.lib.troyhip_last_error().decode() if rc else "", so)


def check_refusals(S):
    inv = capi.INVALID_ARGUMENT
    limbs, N = S.ctx.first_limbs, S.N
    item = 3 * limbs * N
    a, b = S.ct(S.inputs(limbs, 1, 5)), S.ct(S.inputs(limbs, 1, 6))
    a3 = api.Ciphertext.from_numpy(S.ctx, synth.uniform_ct(7, S.primes[:limbs], 3, N, 1), S.ntt)
    out = api.DeviceBuffer(item)
    sa, sb = a.struct(), b.struct()
    rc, _, so = raw_call(S, [sa], [sb], out.ptr, item)
    assert rc == capi.OK and (so.size, so.limbs, bool(so.is_ntt_form)) == (3, limbs, S.ntt)
    assert raw_call(S, [sa], [sb], out.ptr, item, n=0)[:2] == (inv, "multiply_sum takes 1 to 16 products")
    assert raw_call(S, [sa] * 16, [sb] * 16, out.ptr, item, n=17)[:2] == (inv, "multiply_sum takes 1 to 16 products")
    assert raw_call(S, [sa, None], [sb, sb], out.ptr, item)[:2] == (inv, "null ciphertext descriptor")
    assert raw_call(S, [sa], [None], out.ptr, item)[:2] == (inv, "null ciphertext descriptor")
    assert raw_call(S, [sa], [a3.struct()], out.ptr, item)[:2] == (inv, "multiply_sum takes size-2 operands")
    assert raw_call(S, [a3.struct()], [sb], out.ptr, item)[:2] == (inv, "multiply_sum takes size-2 operands")
    if S.ctx.last_limbs < limbs:
        low = S.ct(S.inputs(limbs - 1, 1, 8))
        assert raw_call(S, [sa, sa], [sb, low.struct()], out.ptr, item)[:2] == (inv, "encrypted1 and encrypted2 parameter mismatch")
    wrong = a.struct()
    wrong.is_ntt_form = 0 if S.ntt else 1
    msg = {BFV: "encrypted1 or encrypted2 cannot be in NTT form", BGV: "encryped1 or encrypted2 must be not in NTT form", CKKS: "encrypted1 or encrypted2 must be in NTT form"}[S.scheme]
    assert raw_call(S, [sa, wrong], [sb, sb], out.ptr, item)[:2] == (inv, msg)
    if S.scheme == CKKS:
        s2 = a.struct()
        s2.scale = 2.0
        assert raw_call(S, [sa, s2], [sb, sb], out.ptr, item)[:2] == (inv, "scale mismatch")
        two = S.ct(S.inputs(limbs, 2, 10))  # the kernel reads 16 bytes at a time: an item on an odd word is refused
        odd = two.struct()
        odd.batch_stride -= 1
        wide = api.DeviceBuffer(2 * item)
        assert raw_call(S, [two.struct()], [odd], wide.ptr, item, batch=2)[:2] == (inv, "batch stride is smaller than one ciphertext")
        big = api.Ciphertext.from_numpy(S.ctx, S.inputs(limbs, 3, 11), True, capacity=3)
        odd = big.struct()
        odd.batch_stride -= 1  # 3 polynomials less a word: room for a size-2 item, odd
        assert raw_call(S, [two.struct()], [odd], wide.ptr, item, batch=2)[:2] == (inv, "multiply_sum: batch strides must be even")
        s3 = a.struct()
        s3.scale = 2.0 ** 400
        assert raw_call(S, [s3], [sb], out.ptr, item)[:2] == (inv, "scale out of bounds")
    if S.scheme == BGV:
        s2 = a.struct()
        s2.correction_factor = 3
        assert raw_call(S, [sa, s2], [sb, sb], out.ptr, item)[:2] == (inv, "correction factor mismatch")
        rc, _, so = raw_call(S, [s2, s2], [sb, sb], out.ptr, item)
        assert rc == capi.OK and so.correction_factor == 3
    assert raw_call(S, [sa], [sb], out.ptr, item - 1)[:2] == (inv, "destination batch stride too small for the result size")
    assert raw_call(S, [sa], [sb], None, item)[0] == inv
    for alias in (a, b):  # the destination is one of the operands (Setup.ct of one item leaves room for three polynomials)
        assert alias.capacity == 3
        assert raw_call(S, [sa], [sb], alias.buf.ptr, item)[:2] == (inv, "the destination cannot be one of the operands")
    # a level the context does not have; a host-only context
    bad = a.struct()
    bad.limbs = S.K + 1
    assert raw_call(S, [bad], [bad], out.ptr, item)[:2] == (inv, "encrypted is not valid for encryption parameters")
    other = HC.Setup("other", dict(S.cfg, bits=S.cfg["bits"] + [S.cfg["bits"][-1]]))  # one more prime: its first level is no level here
    foreign = other.ct(other.inputs(other.ctx.first_limbs, 1, 9)).struct()
    assert raw_call(S, [foreign], [foreign], out.ptr, item)[:2] == (inv, "encrypted is not valid for encryption parameters")
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    rc, msg, _ = raw_call(S, [sa], [sb], out.ptr, item, ctx=host)
    assert rc == capi.LOGIC_ERROR and "host-only" in msg
    n = C.c_int(0)
    assert S.lib.troyhip_multiply_sum_max_terms(S.ctx.h, S.K + 1, C.byref(n)) == inv
    # the Python layer: the same messages as exceptions
    with_raises(capi.InvalidArgument, "1 to 16 products", lambda: S.ev.multiplySum([], []))
    with_raises(capi.InvalidArgument, "1 to 16 products", lambda: S.ev.multiplySum([a] * 17, [b] * 17))
    with_raises(capi.InvalidArgument, "size-2 operands", lambda: S.ev.multiplySum([a3], [b]))


def check_strided_destination(S, seed=90):
    """batch 2, R = 2 into a destination whose items lie 3 polynomials + padding apart: the CKKS path through the arena, the BFV floor into scratch and
    the BGV sums in scratch, each followed by the strided copy; equal to the dense call, the padding untouched"""
    limbs, N, batch = S.ctx.first_limbs, S.N, 2
    As, Bs = operands(S, limbs, batch, 2, seed)
    ref = mulsum(S, As, Bs)
    cts = to_cts(S, As + Bs)
    item, pad = 3 * limbs * N, 2 * N
    ones = np.uint64(2**64 - 1)
    out = api.DeviceBuffer.from_numpy(np.full(batch * (item + pad), ones, dtype=np.uint64))
    rc, msg, so = raw_call(S, [c.struct() for c in cts[:2]], [c.struct() for c in cts[2:]], out.ptr, item + pad, batch=batch)
    assert rc == capi.OK, msg
    got = out.to_numpy().reshape(batch, item + pad)
    assert np.array_equal(got[:, :item].reshape(ref.shape), ref), (S.name, "strided destination")
    assert (got[:, item:] == ones).all(), (S.name, "the padding between the items was written")


def check_python_layer(S):
    limbs = S.ctx.first_limbs
    As, Bs = operands(S, limbs, 3, 2, 80)
    cts = to_cts(S, As + Bs)
    out = S.ev.multiplySum(cts[:2], cts[2:])
    assert isinstance(out, api.Ciphertext) and out.size() == 3 and out.capacity == 3
    if S.scheme != BFV:
        assert np.array_equal(out.cpu(), composed(S, As, Bs))
    rk = api.RelinKeys(S.ctx)
    rk.set(0, synth.uniform_kswitch_key(81, S.primes, S.N))
    got = S.ev.innerProduct(cts[:2], cts[2:], rk)
    S.ev.relinearizeInplace(out, rk)
    assert got.size() == 2 and np.array_equal(got.cpu(), out.cpu())
