"""Shared checks of the hoisted linear transform (troyhip_galois_plain_sum_hoisted): an exact host model of the definition, the
independence of the result from how it was asked for, the comparison with the composition of existing calls under real keys, DiagonalMatvec, the
refusals and the layers.  Used by tests/test_device_hoist_lt.py (emulator build) and tests/test_gpu_hoist_lt.py (MI355X).

The model restates the definition independently of the device code, as hoist_cases.model_item does: every automorphism is applied in the COEFFICIENT
domain (oracle.apply_galois modulo the output prime) and transformed (oracle.ntt_standalone), where the device permutes transformed rows; the inner
products, the plaintext products, the sums and the mod-down are Python integers."""
import ctypes as C

import numpy as np
import pytest

import hoist_cases as HC
from hoist_cases import obj
from oracle import oracle
from troy_amd import api, app, capi, synth
from troy_amd.capi import BFV, BGV, CKKS

PLAIN_SEED = 8200


def plains_of(S, R, seed=PLAIN_SEED):
    """R synthetic plaintexts [R][K][N], uniform residues of all K key primes (the arithmetic is oblivious to what they encode)"""
    return synth.edge_rows(S.pt_pattern, seed, S.primes, R * S.K, S.N).reshape(R, S.K, S.N)


def fused(S, data, elts, pts, limit=0, rows_only=None, ct=None, bufs=None):
    """-> [batch][2][limbs][N] through the Python layer (bufs: the plaintexts `pts` already on the device)"""
    for g in elts:
        if g != 1:
            S.key(g, rows_only)
    bufs = [api.DeviceBuffer.from_numpy(p) for p in pts] if bufs is None else bufs
    out = S.ev.applyGaloisPlainSumHoisted(S.ct(data) if ct is None else ct, elts, bufs, S.gk, scratch_limit_words=limit)
    assert (out.size(), out.limbs, out.is_ntt_form, out.batch) == (2, data.shape[2], S.ntt, data.shape[0])
    return out.cpu()


# ---------------------------------------------------------------- the definition, in exact integers
MAC_TERMS, MAC_OPERAND = 63, 1 << 61   # poly.hip MacAcc: fewer than 64 terms of operands below 2^61
BOUNDS = {"inner": MAC_TERMS * MAC_OPERAND ** 2, "base": MAC_TERMS * MAC_OPERAND ** 2,  # the sums a MacAcc holds
          "outer128": 1 << 124,  # hoist_lt_kernel<true>: at most 16 products of canonical words per launch, "below 2^124"
          "outer64": 1 << 64}    # hoist_lt_kernel<false>: at most 16 reduced products per launch, "below 2^64"
LAUNCH = 16                      # HOIST_MAX_ROT


def note(trace, name, values):
    if trace is not None:
        trace[name] = max(trace.get(name, 0), int(np.max(values)))


def model_item(S, ct, elts, keys, pts, trace=None):
    """sum_r pts[r] * (element elts[r] of the ciphertext ct [2][dl][N]) under keys[r] [K-1][2][K][N] -> [2][dl][N]
    trace: a dict that receives the largest value each lazy accumulator of the kernels holds for these inputs, as exact integers ("inner": the sum
    over the digits before its reduction; "outer128" / "outer64": the sum over the rotations of one launch of hoist_lt_kernel<true> / <false>;
    "base": the sum over the elements of one launch of hoist_lt_base_kernel) -- to be held against BOUNDS"""
    N, K, primes = S.N, S.K, S.primes
    dl = ct.shape[1]
    qk = primes[K - 1]
    out_primes = primes[:dl] + [qk]
    key_limb = list(range(dl)) + [K - 1]
    # c in coefficient form (what the automorphism is defined on) and in NTT form (what the plaintexts multiply)
    coeff = [[oracle.ntt_standalone(N, primes[j], ct[k, j], 3) if S.ntt else ct[k, j] for j in range(dl)] for k in range(2)]
    d = coeff[1]
    # steps 1 - 3: per rotation the inner product over the rotated digits, canonical, times the plaintext row of the output prime, summed
    acc = np.zeros((2, dl + 1, N), dtype=object)
    launch = np.zeros((2, 2, dl + 1, N), dtype=object)  # [128-bit form, 64-bit form]: what the outer accumulators of the current launch hold
    in_launch = 0
    for g, key, pt in zip(elts, keys, pts):
        if g == 1:
            continue
        if in_launch == LAUNCH:
            launch[:] = 0
            in_launch = 0
        in_launch += 1
        for i, p in enumerate(out_primes):
            inner = np.zeros((2, N), dtype=object)
            for j in range(dl):
                e = oracle.ntt_standalone(N, p, oracle.apply_galois(N, g, p, d[j] % np.uint64(p)), 1)
                for k in range(2):
                    inner[k] += obj(e) * obj(key[j, k, key_limb[i]])
            note(trace, "inner", inner)
            inner %= p
            for k in range(2):
                acc[k, i] += obj(pt[key_limb[i]]) * inner[k]
                if trace is not None:
                    launch[0, k, i] += obj(pt[key_limb[i]]) * inner[k]
                    launch[1, k, i] += obj(pt[key_limb[i]]) * inner[k] % p
        if trace is not None:
            note(trace, "outer128", launch[0])
            note(trace, "outer64", launch[1])
    for i, p in enumerate(out_primes):
        acc[:, i] %= p
    # steps 4 - 6: the base in NTT form, back in the ciphertext's own form
    base = np.zeros((2, dl, N), dtype=object)
    for j in range(dl):
        q = primes[j]
        launch = np.zeros((2, N), dtype=object)
        for r, (g, pt) in enumerate(zip(elts, pts)):
            if r % LAUNCH == 0:
                launch[:] = 0
            rot = oracle.ntt_standalone(N, q, oracle.apply_galois(N, g, q, coeff[0][j]) if g != 1 else coeff[0][j], 1)
            base[0, j] += obj(pt[j]) * obj(rot)
            launch[0] += obj(pt[j]) * obj(rot)
            if g == 1:
                one = obj(pt[j]) * obj(oracle.ntt_standalone(N, q, coeff[1][j], 1))
                base[1, j] += one
                launch[1] += one
            note(trace, "base", launch)
        base[:, j] %= q
        if not S.ntt:
            for k in range(2):
                base[k, j] = obj(oracle.ntt_standalone(N, q, base[k, j].astype(np.uint64), 3))
    if all(g == 1 for g in elts):
        return base.astype(np.uint64)
    # step 7: the scheme's mod-down by the special prime, added to the base
    half = qk >> 1
    out = np.zeros((2, dl, N), dtype=np.uint64)
    for k in range(2):
        if S.ntt:
            last = obj(oracle.ntt_standalone(N, qk, acc[k, dl].astype(np.uint64), 3))
        else:
            cf = [obj(oracle.ntt_standalone(N, p, acc[k, i].astype(np.uint64), 3)) for i, p in enumerate(out_primes)]
            last = cf[dl]
        for j in range(dl):
            q = primes[j]
            inv = pow(qk, -1, q)
            if S.scheme == BFV:
                tl = (last + half) % qk
                v = (cf[j] - tl % q + half % q) * inv
            elif S.scheme == BGV:
                kt = (-last) % S.t * pow(qk, -1, S.t) % S.t
                v = (cf[j] - kt % q * (qk % q) - last % q) * inv
            else:
                tl = (last + half) % qk
                corr = ((tl % q) + (q - half % q)) % q
                v = (acc[k, j] - obj(oracle.ntt_standalone(N, q, corr.astype(np.uint64), 1))) * inv
            out[k, j] = ((base[k, j] + v) % q).astype(np.uint64)
    return out


def check_model(S, limbs, batch, elts, seed, items=None, rows_only=None, limit=0, trace=None):
    """every limb of every output item (or of `items`) equals the model and is canonical; trace: see model_item"""
    data = S.inputs(limbs, batch, seed)
    pts = plains_of(S, len(elts), PLAIN_SEED + seed)
    got = fused(S, data, elts, pts, limit=limit, rows_only=rows_only)
    assert got.shape == (batch, 2, limbs, S.N)
    keys = [S.host_keys.get(g) for g in elts]
    for b in (range(batch) if items is None else items):
        exp = model_item(S, data[b], elts, keys, pts, trace)
        for name, v in (trace or {}).items():  # a pattern past a documented precondition is no test of the kernel: this comes first
            assert v < BOUNDS[name], (S.name, "the inputs break the documented bound of", name, v, BOUNDS[name])
        assert np.array_equal(got[b], exp), (S.name, limbs, "item", b, elts)
        assert all((got[b, :, j] < np.uint64(S.primes[j])).all() for j in range(limbs))
    return got, data, pts


def elts_crossing_a_launch(S):
    """R = 18: seventeen elements other than 1 (three distinct ones, repeated with different plaintexts) and element 1 in their middle -- more than
    HOIST_MAX_ROT = 16 of either kind, so both kernels run a second, accumulating launch"""
    e = S.elts(5)
    three = [e[0], e[1], e[4]]
    rots = (three * 6)[:17]
    return rots[:9] + [1] + rots[9:]


# ---------------------------------------------------------------- independence
def scratch_words(S, limbs, items):
    """what Evaluator::galois_plain_sum_hoisted asks of the arena for a slab of `items` (evaluator.cpp; include/troyhip.h documents the formula)"""
    N, dl, rl = S.N, limbs, limbs + 1
    return items * N * (rl * dl + (dl if S.ntt else 0) + 2 * rl + 2 * dl + (0 if S.ntt else dl) + 2 * dl + 4) + 32 * 8 + 128


def slabs():
    return capi.stat("hoist_lt_slabs", api.KernelProvider.lib())


def check_independence(S, limbs, batch, seed):
    data = S.inputs(limbs, batch, seed)
    elts = S.elts(5)
    pts = plains_of(S, 5, PLAIN_SEED + seed)
    s0 = slabs()
    ref = fused(S, data, elts, pts)  # an odd batch: Setup.ct makes it a strided operand (capacity 3)
    assert slabs() - s0 == 1
    # a dense operand
    assert np.array_equal(fused(S, data, elts, pts, ct=api.Ciphertext.from_numpy(S.ctx, data, S.ntt)), ref), "strided against dense"
    # the pair list permuted
    perm = [3, 0, 4, 2, 1]
    assert np.array_equal(fused(S, data, [elts[i] for i in perm], pts[perm]), ref), "permuted"
    # batch 1 per item
    for b in range(batch):
        assert np.array_equal(fused(S, data[b:b + 1], elts, pts)[0], ref[b]), ("item alone", b)
    # a scratch limit of one item: one slab per item
    s0 = slabs()
    assert np.array_equal(fused(S, data, elts, pts, limit=scratch_words(S, limbs, 1)), ref)
    assert slabs() - s0 == batch == 3
    HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small", lambda: fused(S, data, elts, pts, limit=scratch_words(S, limbs, 1) - 1))
    # one plaintext word changed (a rotation's special-prime row, then element 1's first data row): another result
    for r, row in ((0, S.K - 1), (3, 0)):
        other = pts.copy()
        other[r, row, 5] = (other[r, row, 5] + np.uint64(1)) % np.uint64(S.primes[row])
        assert not np.array_equal(fused(S, data, elts, other), ref), ("plaintext word", r, row)


# ---------------------------------------------------------------- against the composition of existing calls, with real keys
STEPS = (1, -2, 0, 5)


def check_composition_bfv_bgv(name, steps=STEPS, batch=2):
    """decrypt(fused) == decrypt(sum_r multiplyPlainNormal(rotateRows(a, s_r), d_r)) == the slot-wise sum; differing limbs; the noise budget of the
    fused result within 2 bits of the composition's (what hoist_cases.check_sequential_bfv_bgv asserts for hoisting); -> [(fused, sequential)] budgets"""
    S = HC.RealSetup(name, steps)
    rng = np.random.default_rng(3)
    benc = api.BatchEncoder(S.ctx)
    K, N = S.ctx.key_limbs, S.N
    msgs = [rng.integers(0, S.t, N, dtype=np.uint64) for _ in range(batch)]
    diags = [rng.integers(0, S.t, N, dtype=np.uint64) for _ in steps]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(benc.encode(m)) for m in msgs]))
    d_coeff = [api.DeviceBuffer.from_numpy(benc.encode(d)) for d in diags]
    d_ntt = [S.ev.transformPlainToNtt(p, K) for p in d_coeff]
    got = S.ev.rotateRowsPlainSumHoisted(a, steps, d_ntt, S.gk)
    assert (got.size(), got.limbs, got.is_ntt_form, got.batch, got.scale, got.correction_factor) == (2, a.limbs, False, batch, a.scale, a.correction_factor)
    seq = None
    for s, p in zip(steps, d_coeff):
        term = S.ev.rotateRows(a, s, S.gk) if s else a.copy()
        S.ev.multiplyPlainNormalInplace(term, p)
        if seq is None:
            seq = term
        else:
            S.ev.addInplace(seq, term)
    f, q = got.cpu(), seq.cpu()
    assert not np.array_equal(f, q), "the fused limbs are the library's own: one rounding instead of one per rotation"
    budgets = []
    for b in range(batch):
        df, ds = S.dec.decrypt(f[b]), S.dec.decrypt(q[b])
        assert np.array_equal(df, ds), (name, b)
        m = msgs[b].reshape(2, -1).astype(object)
        exp = sum(d.reshape(2, -1).astype(object) * np.roll(m, -s, axis=1) for s, d in zip(steps, diags)) % S.t
        assert np.array_equal(benc.decode(df).reshape(2, -1), exp.astype(np.uint64)), (name, b)
        bf, bq = S.dec.invariantNoiseBudget(f[b]), S.dec.invariantNoiseBudget(q[b])
        fresh = S.dec.invariantNoiseBudget(a.cpu()[b])
        print(name, "item", b, "budget fused", bf, "sequential", bq, "fresh", fresh)
        assert bq > 0 and bf >= bq - 2, (name, b, bf, bq)
        budgets.append((bf, bq))
    return budgets


def ckks_errors(S, cenc, vals, diags, steps, got, seq, scale):
    """slot errors of the fused result and of the composition against the exact complex sum, over the batch"""
    exact = [sum(d * np.roll(v, -s) for s, d in zip(steps, diags)) for v in vals]
    f, q = got.cpu(), seq.cpu()
    d_f = np.concatenate([np.abs(cenc.decode(S.dec.decrypt(f[b]), scale) - exact[b]) for b in range(len(vals))])
    d_s = np.concatenate([np.abs(cenc.decode(S.dec.decrypt(q[b]), scale) - exact[b]) for b in range(len(vals))])
    return d_f, d_s


def ckks_composition(S, a, steps, plains_np, plain_scale):
    """sum_r multiplyPlain(rotateVector(a, s_r), d_r) by the existing calls, the plaintexts at the ciphertext's level"""
    seq = None
    for s, p in zip(steps, plains_np):
        term = S.ev.rotateVector(a, s, S.gk) if s else a.copy()
        S.ev.multiplyPlainInplace(term, api.DeviceBuffer.from_numpy(p[:a.limbs]), plain_scale)
        if seq is None:
            seq = term
        else:
            S.ev.addInplace(seq, term)
    return seq


def check_composition_ckks(name, steps=STEPS, batch=2, scale=2.0 ** 25):
    """fused median slot error <= 1.5 x the composition's and fused maximum <= 4 x the composition's, both against the exact complex sum"""
    S = HC.RealSetup(name, steps)
    rng = np.random.default_rng(3)
    cenc = api.CKKSEncoder(S.ctx)
    K, n = S.ctx.key_limbs, S.N // 2
    vals = [rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in range(batch)]
    diags = [rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in steps]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(cenc.encode(v, scale)) for v in vals]), True, scale)
    plains_np = [cenc.encode(d, scale, limbs=K) for d in diags]
    got = S.ev.rotateVectorPlainSumHoisted(a, steps, [api.DeviceBuffer.from_numpy(p) for p in plains_np], S.gk, plain_scale=scale)
    assert got.scale == a.scale * scale and got.is_ntt_form and (got.size(), got.limbs, got.batch) == (2, a.limbs, batch)
    seq = ckks_composition(S, a, steps, plains_np, scale)
    assert seq.scale == got.scale
    d_f, d_s = ckks_errors(S, cenc, vals, diags, steps, got, seq, scale * scale)
    print(name, "max slot error fused", d_f.max(), "sequential", d_s.max(), "medians", np.median(d_f), np.median(d_s))
    assert d_s.max() < 0.1, "the composition itself is expected to be right"
    assert np.median(d_f) <= 1.5 * np.median(d_s), (name, np.median(d_f), np.median(d_s))
    assert d_f.max() <= 4 * d_s.max(), (name, d_f.max(), d_s.max())
    return (d_f.max(), d_s.max(), np.median(d_f), np.median(d_s))


# ---------------------------------------------------------------- DiagonalMatvec
def matvec_matrix(rng, d, draw):
    """d x d with the diagonals 2, 5 and 6 zero: five rotations (one of them step 0) are requested"""
    k = np.arange(d)
    m = np.zeros((d, d), dtype=np.asarray(draw(1)).dtype)
    for r in (0, 1, 3, 4, 7):
        m[k, (k + r) % d] = draw(d)
    return m


def check_matvec_bfv(name="bfv_n64_k3", d=8, batch=2):
    rng = np.random.default_rng(5)
    M = matvec_matrix(rng, d, lambda n: rng.integers(1, 1 << 9, n, dtype=np.uint64))
    cfg = HC.config(name)
    probe = api.SEALContext(cfg["scheme"], cfg["N"], api.CoeffModulus.Create(cfg["N"], cfg["bits"]), api.PlainModulus.Batching(cfg["N"], cfg["tbits"]))
    mv = app.DiagonalMatvec(probe, M)
    assert mv.steps == [0, 1, 3, 4, 7] and mv.requiredSteps() == [1, 3, 4, 7]
    S = HC.RealSetup(name, mv.requiredSteps())
    mv = app.DiagonalMatvec(S.ctx, M)
    benc = api.BatchEncoder(S.ctx)
    assert len(mv.encodeDiagonals(benc)) == 5
    xs = [rng.integers(0, S.t, d, dtype=np.uint64) for _ in range(batch)]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(benc.encode(np.tile(x, S.N // d))) for x in xs]))
    y = mv.apply(S.ev, a, S.gk).cpu()
    for b in range(batch):
        exp = (M.astype(object).dot(xs[b].astype(object)) % S.t).astype(np.uint64)
        assert np.array_equal(benc.decode(S.dec.decrypt(y[b])), np.tile(exp, S.N // d)), (name, b)


def check_matvec_ckks(name="ckks_n128_k6", d=8, batch=2, scale=2.0 ** 25):
    rng = np.random.default_rng(6)
    M = matvec_matrix(rng, d, lambda n: rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n))
    S = HC.RealSetup(name, (1, 3, 4, 7))
    mv = app.DiagonalMatvec(S.ctx, M)
    assert mv.requiredSteps() == [1, 3, 4, 7]
    cenc = api.CKKSEncoder(S.ctx)
    plains = mv.encodeDiagonals(cenc, scale)
    n = S.N // 2
    xs = [rng.uniform(-1, 1, d) + 1j * rng.uniform(-1, 1, d) for _ in range(batch)]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(cenc.encode(np.tile(x, n // d), scale)) for x in xs]), True, scale)
    got = mv.apply(S.ev, a, S.gk)
    assert got.scale == scale * scale
    K = S.ctx.key_limbs
    seq = ckks_composition(S, a, mv.steps, [p.to_numpy().reshape(K, S.N) for p in plains], scale)
    diags = [mv.diagonals[r] for r in mv.steps]
    d_f, d_s = ckks_errors(S, cenc, [np.tile(x, n // d) for x in xs], diags, mv.steps, got, seq, scale * scale)
    exact = [np.tile(M.dot(x), n // d) for x in xs]
    f = got.cpu()
    direct = np.concatenate([np.abs(cenc.decode(S.dec.decrypt(f[b]), scale * scale) - exact[b]) for b in range(batch)])
    print(name, "matvec max slot error fused", d_f.max(), "sequential", d_s.max(), "medians", np.median(d_f), np.median(d_s))
    assert np.allclose(direct, d_f, atol=1e-9), "the sum over the diagonals is M x"
    assert d_s.max() < 0.1 and np.median(d_f) <= 1.5 * np.median(d_s), (name, np.median(d_f), np.median(d_s))


# ---------------------------------------------------------------- refusals and the layers
def raw_call(S, st_in, out_ptr, out_stride, elts, keys, pls, n=None, batch=1, limit=0, plain_scale=1.0, ctx=None):
    so = capi.CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    R = len(elts)
    e = (C.c_uint32 * max(R, 1))(*elts)
    k = (C.c_void_p * max(R, 1))(*keys)
    p = (C.c_void_p * max(R, 1))(*pls)
    rc = S.lib.troyhip_galois_plain_sum_hoisted(S.ctx.h if ctx is None else ctx.h, C.byref(st_in), C.byref(so), e, k, p, R if n is None else n, C.c_double(plain_scale),
                                                C.c_uint64(limit), C.c_uint64(batch), None)
    return (rc, S.lib.troyhip_last_error().decode() if rc else "", so)


def check_refusals(S):
    inv = capi.INVALID_ARGUMENT
    limbs, N, K = S.ctx.first_limbs, S.N, S.K
    item = 2 * limbs * N
    g = S.ctx.galois_elt_from_step(1)
    S.key(g)
    kp = S.gk.keys[api.GaloisKeys.getIndex(g)].ptr
    pts = plains_of(S, 2)
    pl = [api.DeviceBuffer.from_numpy(p) for p in pts]
    pp = pl[0].ptr
    data = S.inputs(limbs, 1, 5)
    a = S.ct(data)
    a3 = api.Ciphertext.from_numpy(S.ctx, synth.uniform_ct(6, S.primes[:limbs], 3, N, 1), S.ntt)
    out = api.DeviceBuffer(3 * item)
    st = a.struct()
    assert raw_call(S, st, out.ptr, item, [g], [kp], [pp], n=0)[:2] == (inv, "hoisted linear transform takes at least one Galois element")
    assert raw_call(S, st, out.ptr, item, [g], [kp], [pp], n=-1)[0] == inv
    assert raw_call(S, st, out.ptr, item, [2], [kp], [pp])[:2] == (inv, "Galois element is not valid")
    assert raw_call(S, st, out.ptr, item, [2 * N + 1], [kp], [pp])[:2] == (inv, "Galois element is not valid")
    assert raw_call(S, st, out.ptr, item, [g], [None], [pp])[:2] == (inv, "Galois key not present")
    assert raw_call(S, st, out.ptr, item, [1, g], [None, None], [pp, pp])[:2] == (inv, "Galois key not present")
    assert raw_call(S, st, out.ptr, item, [g], [kp], [None])[:2] == (inv, "plain_ntt is not valid for encryption parameters")
    assert raw_call(S, st, out.ptr, item, [g, 1], [kp, None], [pp, None])[:2] == (inv, "plain_ntt is not valid for encryption parameters")
    assert raw_call(S, a3.struct(), out.ptr, item, [g], [kp], [pp])[:2] == (inv, "encrypted size must be 2")
    wrong = a.struct()
    wrong.is_ntt_form = 0 if S.ntt else 1
    msg = {BFV: "BFV encrypted cannot be in NTT form", BGV: "BGV encrypted cannot be in NTT form", CKKS: "CKKS encrypted must be in NTT form"}[S.scheme]
    assert raw_call(S, wrong, out.ptr, item, [g], [kp], [pp])[:2] == (inv, msg)
    # a host-only context and one with a single prime (no special prime: no key switching)
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    rc, text, _ = raw_call(S, st, out.ptr, item, [g], [kp], [pp], ctx=host)
    assert rc == capi.LOGIC_ERROR and "host-only" in text
    single = api.SEALContext(S.scheme, N, S.primes[:1], S.t)
    one = api.Ciphertext.from_numpy(single, synth.uniform_ct(7, S.primes[:1], 2, N, 1), S.ntt)
    assert raw_call(S, one.struct(), out.ptr, 2 * N, [g], [kp], [pp], ctx=single)[:2] == (capi.LOGIC_ERROR, "keyswitching is not supported by the context")
    # the destination: overlapping the operand, missing, too narrow
    assert raw_call(S, st, a.buf.ptr, item, [g], [kp], [pp])[:2] == (inv, "hoisted linear transform: destination must be a distinct buffer")
    assert raw_call(S, st, None, item, [g], [kp], [pp])[0] == inv
    assert raw_call(S, st, out.ptr, item - 1, [g], [kp], [pp])[:2] == (inv, "destination batch stride too small for the result size")
    if S.scheme == CKKS:
        assert raw_call(S, st, out.ptr, item, [g], [kp], [pp], plain_scale=2.0 ** 400)[:2] == (inv, "scale out of bounds")
    rc, text, _ = raw_call(S, st, out.ptr, item, [g], [kp], [pp], limit=scratch_words(S, limbs, 1) - 1)
    assert rc == inv and text.startswith("scratch_limit_words is too small")
    # element 1 alone needs no key; the call fills in the descriptor, the scale is the product
    rc, _, so = raw_call(S, st, out.ptr, item, [1], [None], [pp], plain_scale=4.0)
    assert rc == capi.OK and (so.size, so.limbs, bool(so.is_ntt_form), so.scale, so.correction_factor) == (2, limbs, S.ntt, 4.0 * a.scale, a.correction_factor)
    assert np.array_equal(out.to_numpy(item).reshape(2, limbs, N), model_item(S, data[0], [1], [None], pts[:1]))
    # the Python layer: the same refusals as exceptions
    HC.with_raises(capi.InvalidArgument, "Galois key not present", lambda: S.ev.applyGaloisPlainSumHoisted(a, [1, g], pl, api.GaloisKeys(S.ctx)))
    HC.with_raises(capi.InvalidArgument, "at least one", lambda: S.ev.applyGaloisPlainSumHoisted(a, [], [], S.gk))
    HC.with_raises(capi.InvalidArgument, "one plaintext per element", lambda: S.ev.applyGaloisPlainSumHoisted(a, [g, 1], pl[:1], S.gk))
    HC.with_raises(capi.InvalidArgument, "plain_ntt is not valid", lambda: S.ev.applyGaloisPlainSumHoisted(a, [g, 1], [pl[0], None], S.gk))
    HC.with_raises(capi.InvalidArgument, r"\[K\]\[N\] words", lambda: S.ev.applyGaloisPlainSumHoisted(a, [g], [api.DeviceBuffer((K - 1) * N)], S.gk))
    HC.with_raises(capi.InvalidArgument, "encrypted size must be 2", lambda: S.ev.applyGaloisPlainSumHoisted(a3, [g], pl[:1], S.gk))
    HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small", lambda: S.ev.applyGaloisPlainSumHoisted(a, [g], pl[:1], S.gk, scratch_limit_words=1000))
    HC.with_raises(capi.LogicError, "unsupported scheme", lambda: (S.ev.rotateRowsPlainSumHoisted if S.ntt else S.ev.rotateVectorPlainSumHoisted)(a, [1], pl[:1], S.gk))
    if S.scheme == CKKS:
        HC.with_raises(capi.InvalidArgument, "scale out of bounds", lambda: S.ev.applyGaloisPlainSumHoisted(a, [g], pl[:1], S.gk, plain_scale=2.0 ** 400))


def check_python_layer(S):
    """rotate*PlainSumHoisted map steps through galois_elt_from_step, step 0 to element 1, and equal applyGaloisPlainSumHoisted"""
    limbs = S.ctx.first_limbs
    data = S.inputs(limbs, 3, 21)
    steps = [1, 0, -1]
    elts = [S.ctx.galois_elt_from_step(s) if s else 1 for s in steps]
    pts = plains_of(S, 3)
    ref = fused(S, data, elts, pts)
    fn = S.ev.rotateVectorPlainSumHoisted if S.ntt else S.ev.rotateRowsPlainSumHoisted
    got = fn(S.ct(data), steps, [api.DeviceBuffer.from_numpy(p) for p in pts], S.gk, plain_scale=2.0)
    assert isinstance(got, api.Ciphertext) and got.scale == 2.0
    assert np.array_equal(got.cpu(), ref)


# ---------------------------------------------------------------- the routes only large launches take
def check_both_calls(S, limbs, seed, batch=3):
    """both hoisted calls at R = 3 against the model on item 0: rotations by (step 1, the conjugation, step 1 again), the linear transform over
    (step 1, element 1, the conjugation)"""
    e = S.elts(3)
    HC.check_model(S, limbs, batch, 3, seed, items=[0])
    check_model(S, limbs, batch, [e[0], 1, e[1]], seed, items=[0])


def check_large_route(S, limbs, batch, elts, seed, rows_only=None, limit=0):
    """ONE call of `batch` items: items 0, the middle one and the last against the model; EVERY item bit-for-bit against the same call at batch 1 (the
    small-launch routes, which the model pins at the small shapes).  -> the path-counter deltas (the large call, the first batch-1 call)"""
    data = S.inputs(limbs, batch, seed)
    pts = plains_of(S, len(elts), PLAIN_SEED + seed)
    for g in elts:
        if g != 1:
            S.key(g, rows_only)
    bufs = [api.DeviceBuffer.from_numpy(p) for p in pts]
    s0 = HC.route_stats()
    got = fused(S, data, elts, pts, limit=limit, rows_only=rows_only, bufs=bufs)
    big = HC.delta(HC.route_stats(), s0)
    one = None
    for b in range(batch):
        s0 = HC.route_stats()
        alone = fused(S, data[b:b + 1], elts, pts, rows_only=rows_only, bufs=bufs)[0]
        one = one or HC.delta(HC.route_stats(), s0)
        assert np.array_equal(alone, got[b]), (S.name, "item", b, "differs from the same call at batch 1")
    keys = [S.host_keys.get(g) for g in elts]
    for b in sorted({0, batch // 2, batch - 1}):
        assert np.array_equal(got[b], model_item(S, data[b], elts, keys, pts)), (S.name, limbs, "item", b, elts)
    print(S.name, "batch", batch, "elements", elts, "counters of the large call", big, "of the call at batch 1", one)
    return big, one


# ---------------------------------------------------------------- both hoisted calls as one hash, for the library's switches
def hoisted_hash(name, cfg=None, batch=3, seed=4343):
    """SHA-256 over the limbs of one applyGaloisHoisted and one applyGaloisPlainSumHoisted call (synthetic keys, R = 5 with element 1, first level): what
    a child process under one of the library's switches must reproduce (cases.mul_relin_hash is the counterpart for multiply, relinearize, rotate)"""
    import cases
    S = HC.Setup(name, cfg)
    limbs = S.ctx.first_limbs
    data = S.inputs(limbs, batch, seed)
    elts = S.elts(5)
    return cases.sha(S.hoisted(data, elts)) + ":" + cases.sha(fused(S, data, elts, plains_of(S, 5, PLAIN_SEED + seed)))


def hoisted_hashes_in_child(sets, env, timeout=900):
    """hoisted_hash of every (name, cfg) of `sets` in a child process under `env` (the library reads its switches once per process)"""
    import os
    import subprocess
    import sys
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import troy_amd as ta, hoist_lt_cases as LT\n"
            "ta.KernelProvider.initialize(0)\n"
            "print(' '.join(LT.hoisted_hash(n, c) for n, c in %r))\n") % (tests_dir, os.path.dirname(tests_dir), list(sets))
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split()[-len(sets):]


# ---------------------------------------------------------------- residues at the ends of their range
EDGE_SETS = [[60, 60, 60], [50, 49, 50]]  # the widest primes of the integer instances; the last FP64 width (49 bits) and the first integer one (50)


def edge_placements(pattern, every=True):
    """(ciphertext, keys, plaintexts) patterns: `pattern` on each operand alone, the others uniform, and on all three"""
    u = "uniform"
    alone = [(pattern, u, u), (u, pattern, u), (u, u, pattern)] if pattern != "zero" else [(pattern, u, u)]  # a zero key or plaintext alone: a zero sum
    return (alone if every else []) + [(pattern,) * 3]


def check_edges(S, limbs, batch, seed, R=16):
    """both calls with R = 16 elements other than 1 (sixteen terms per launch: the stated bound of both outer accumulators) on the edge patterns S was made
    with: first the model's own accumulators against the documented bounds (check_model: a pattern past a precondition would be no test of the kernel),
    then the limbs against the model -- every item and rotation at batch 1, the first and the last item (of the first and the last rotation) of a
    batch.  -> the largest accumulator values the model saw, as fractions of their bounds"""
    elts = HC.many_elts(S, R)
    trace = {}
    items = None if batch == 1 else [0, batch - 1]
    check_model(S, limbs, batch, elts, seed, items=items, trace=trace)
    HC.check_model(S, limbs, batch, R, seed, elts=elts, items=items, rots=None if batch == 1 else [0, R - 1])
    return {n: trace[n] / BOUNDS[n] for n in trace}


def check_edge_pattern(scheme, bits, pattern, N=128, batches=(1, 5), alone_batches=None, every=None, seed=900):
    """check_edges for every placement of `pattern` (BGV, whose inner product and outer sums are BFV's: all three operands only) at batch 1 (four
    rotations per thread, 128-bit outer sums) and batch 5 (the batched instance, 64-bit outer sums); alone_batches: the batches of the placements on
    one operand alone, where they differ.  -> {placement: fractions}"""
    seen = {}
    for pats in edge_placements(pattern, every=scheme != "bgv" if every is None else every):
        S = HC.Setup(*HC.adhoc(HC.SCHEMES[scheme], N, bits, 40 if bits[0] == 60 and N == 128 else None), patterns=pats)
        for batch in (batches if len(set(pats)) == 1 or alone_batches is None else alone_batches):
            f = check_edges(S, S.ctx.first_limbs, batch, seed + batch)
            seen[pats] = {n: max(f[n], seen.get(pats, {}).get(n, 0)) for n in f}
    return seen
