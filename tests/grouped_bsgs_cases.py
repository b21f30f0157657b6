"""Shared checks of the baby-step / giant-step linear transform with grouped keys (troyhip_galois_plain_sum_bsgs_grouped): an exact
host model of the definition in Python integers, the identities with the two grouped hoisted calls, the equality with the per-prime call at one special
prime, the independence of the result from batch, order and scratch limit, decryption and noise under real keys, the app, the refusals and the launch
geometry.  Used by tests/test_device_grouped_bsgs.py (emulator build) and tests/test_gpu_grouped_bsgs.py (MI355X).

The model is made of what tests/grouped_hoist_cases.py exports: u_i = model_sum over the present pairs of row i; the giant stage is model_ext(u_i.c1), then
model_inner with G_i and its key, summed over i modulo p_o; the base is sum_i sigma_{G_i}(u_i.c0) and sum_{i: G_i = 1} u_i.c1; the last step is
model_moddown.  Everything is exact: no test of limbs has a tolerance."""
import ctypes as C

import numpy as np

import bsgs_cases as BC
import grouped_cases as GC
import grouped_hoist_cases as GH
import hoist_cases as HC
import hoist_lt_cases as LC
from troy_amd import api, app, capi, synth
from troy_amd.capi import BFV, BGV, CKKS

obj = GC.obj
LAUNCH, MAX_ROWS = 16, 8  # HOIST_MAX_ROT, BSGS_MAX_ROWS
SYMBOLS = ("troyhip_galois_plain_sum_bsgs_grouped", "troyhip_galois_plain_sum_bsgs_grouped_scratch_words")
PLAIN_SEED = 9700


# ---------------------------------------------------------------- the definition, in exact integers
def giant_model(S, alpha, us, Gs, keys):
    """sum_i galois_{Gs[i]}(us[i]) with ONE mod-down by all special primes: us[i] [2][dl][N] in the scheme's form, keys[i] grouped (not read for element 1)"""
    N, primes = S.N, S.primes
    dl = us[0].shape[1]
    acc = None
    for u, G, key in zip(us, Gs, keys):
        if G == 1:
            continue
        ext, out_ids = GH.model_ext(S, alpha, u[1])
        inner = GH.model_inner(S, ext, out_ids, G, key)
        acc = inner if acc is None else {k: (acc[k] + inner[k]) % primes[k[1]] for k in acc}
    base = np.zeros((2, dl, N), dtype=np.uint64)
    for j in range(dl):
        b = np.zeros((2, N), dtype=object)
        for u, G in zip(us, Gs):
            b[0] += obj(GH.sigma(S, G, u[0, j], j) if G != 1 else u[0, j])
            if G == 1:
                b[1] += obj(u[1, j])
        base[:, j] = (b % primes[j]).astype(np.uint64)
    return base if acc is None else GH.model_moddown(S, alpha, acc, base)


def model_item(S, alpha, ct, babies, giants, table, keys):
    """the definition for one ciphertext ct [2][dl][N]; keys: element -> grouped key"""
    us, Gs, gkeys = [], [], []
    for G, row in zip(giants, table):
        present = [j for j, p in enumerate(row) if p is not None]
        if not present:
            continue
        us.append(GH.model_sum(S, alpha, ct, [babies[j] for j in present], [keys.get(babies[j]) for j in present], [row[j] for j in present]))
        Gs.append(G)
        gkeys.append(keys.get(G))
    return giant_model(S, alpha, us, Gs, gkeys)


# ---------------------------------------------------------------- the library, through the Python layer
def table_of(S, n2, n1, absent=(), seed=PLAIN_SEED):
    return BC.table_of(S, n2, n1, absent=absent, seed=seed)


def host_keys(S, alpha, babies, giants, table):
    """the grouped keys of the elements a present plaintext uses (only those are made): element -> host key"""
    ub, ug = BC.used(babies, giants, table)
    K = GH.keys_of(S, alpha)
    return {g: K.key(g) for g in sorted(ub | ug) if g != 1}


def bsgs(S, alpha, data, babies, giants, table, limit=0, gk=None, bufs=None):
    """-> [batch][2][limbs][N]"""
    host_keys(S, alpha, babies, giants, table)
    out = S.ev.applyGaloisPlainSumBsgsGrouped(S.ct(data), babies, giants, BC.to_device(table) if bufs is None else bufs, GH.keys_of(S, alpha).gk if gk is None else gk,
                                              scratch_limit_words=limit)
    assert (out.size(), out.limbs, out.is_ntt_form, out.batch) == (2, data.shape[2], S.ntt, data.shape[0])
    return out.cpu()


def slabs():
    return capi.stat("grouped_bsgs_slabs", api.KernelProvider.lib())


def check_model(S, alpha, dl, batch, babies, giants, table, seed, items=None, limit=0):
    data = S.inputs(dl, batch, seed)
    got = bsgs(S, alpha, data, babies, giants, table, limit=limit)
    assert got.shape == (batch, 2, dl, S.N) and GH.canonical(S, got)
    keys = host_keys(S, alpha, babies, giants, table)
    for b in (range(batch) if items is None else items):
        assert np.array_equal(got[b], model_item(S, alpha, data[b], babies, giants, table, keys)), (S.name, alpha, dl, "item", b, babies, giants)
    return got, data


def small_case(S, seed=PLAIN_SEED):
    """n1 = 4 babies with element 1 and a repeated element, n2 = 3 giants with element 1; one absent entry, and row 2 whose only present baby is 1"""
    e = S.elts(5)
    babies, giants = [e[0], 1, e[2], e[4]], [e[4], 1, e[1]]
    assert babies[0] == babies[2] and babies[1] == 1 and giants[1] == 1
    return babies, giants, table_of(S, 3, 4, absent={(0, 3), (2, 0), (2, 2), (2, 3)}, seed=seed)


def check_model_small(S, tag):
    """batch 5 (a group of four and a remainder: the four-items mapping of the giant sum) and batch 2 (the four-giants mapping) at the levels of
    grouped_hoist_cases.small_levels; then a table whose used giants are all 1 (no second mod-down, no giant key read) and one whose babies are all 1
    (no baby key read)"""
    babies, giants, table = small_case(S, PLAIN_SEED + 1)
    for dl in GH.small_levels(S, tag):
        for batch in (5, 2):
            check_model(S, S.alpha, dl, batch, babies, giants, table, seed=400 + dl + batch)
    lmax = S.K - S.alpha
    e = S.elts(5)
    # the giants are 1 (a row of another giant has no present plaintext: its key is not made)
    t1 = table_of(S, 3, 3, absent={(1, 1), (2, 0), (2, 1), (2, 2)}, seed=PLAIN_SEED + 2)
    data = S.inputs(lmax, 2, 71)
    empty_g = api.GaloisKeys(S.ctx, special_primes=S.alpha)
    K = GH.keys_of(S, S.alpha)
    for g in (e[0], e[4]):
        K.key(g)
        empty_g.set_elt(g, K.key(g))
    got = bsgs(S, S.alpha, data, [e[0], 1, e[4]], [1, 1, e[1]], t1, gk=empty_g)  # no key of e[1] in the set
    keys = {e[0]: K.key(e[0]), e[4]: K.key(e[4])}
    for b in range(2):
        assert np.array_equal(got[b], model_item(S, S.alpha, data[b], [e[0], 1, e[4]], [1, 1, e[1]], t1, keys)), (S.name, "giants all 1", b)
    # the babies are 1
    t2 = table_of(S, 3, 2, absent={(1, 0)}, seed=PLAIN_SEED + 3)
    only_g = api.GaloisKeys(S.ctx, special_primes=S.alpha)
    for g in (e[0], e[1]):
        only_g.set_elt(g, K.key(g))
    got = bsgs(S, S.alpha, data, [1, 1], [e[0], 1, e[1]], t2, gk=only_g)
    keys = {e[0]: K.key(e[0]), e[1]: K.key(e[1])}
    for b in range(2):
        assert np.array_equal(got[b], model_item(S, S.alpha, data[b], [1, 1], [e[0], 1, e[1]], t2, keys)), (S.name, "babies all 1", b)
    # babies and giants all 1: no key at all
    none = api.GaloisKeys(S.ctx, special_primes=S.alpha)
    got = bsgs(S, S.alpha, data, [1, 1], [1, 1], table_of(S, 2, 2, absent={(1, 0)}, seed=PLAIN_SEED + 4), gk=none)
    for b in range(2):
        assert np.array_equal(got[b], model_item(S, S.alpha, data[b], [1, 1], [1, 1], table_of(S, 2, 2, absent={(1, 0)}, seed=PLAIN_SEED + 4), {})), (S.name, "all 1", b)


def check_model_large(S, ragged):
    """N = 4096, the two-pass transforms: batch 3, n1 = 4, n2 = 2, one absent entry, items 0 and 2, the first level and a ragged one"""
    e = S.elts(5)
    babies, giants = [e[0], 1, e[1], e[4]], [e[4], 1]
    table = table_of(S, 2, 4, absent={(0, 2)}, seed=PLAIN_SEED + 5)
    for dl in (S.K - S.alpha, ragged):
        check_model(S, S.alpha, dl, 3, babies, giants, table, seed=500 + dl, items=[0, 2])


# ---------------------------------------------------------------- chunk boundaries
def scratch_formula(S, alpha, dl, batch, rot_babies, rows, gc):
    """DESIGN.md section 4.18"""
    N, rl, d, ckks = S.N, dl + alpha, -(-dl // alpha), int(S.ntt)
    per_item = ckks * dl + d * rl + min(rot_babies, LAUNCH) * 2 * rl + rows * 2 * rl + (1 - ckks) * 2 * dl + 2 * rl + 2 * dl
    per_row = 4 * dl + d * rl + ckks * (3 * dl + 2 * alpha)
    return batch * N * per_item + min(gc, rows, LAUNCH) * batch * N * per_row + 32 * 16 + 128


def scratch_query(S, alpha, dl, batch, rot_babies, rows, gc, ctx=None):
    w = C.c_uint64(0)
    capi.check(S.lib, S.lib.troyhip_galois_plain_sum_bsgs_grouped_scratch_words((ctx or S.ctx).h, dl, alpha, C.c_uint64(batch), rot_babies, rows, gc, C.byref(w)))
    return w.value


def check_chunks(S, batch, many_babies, seed=81):
    """n1 = 17 used babies other than 1 (two baby chunks: the inner kernel's `accumulate`), or n2 = 18 rows with 17 giants other than 1 (three inner
    launches of at most 8 rows; giant-sum launches of 16 and 1 giants, the second accumulating) against the model, one slab"""
    alpha, dl = S.alpha, S.K - S.alpha
    if many_babies:
        babies, giants = HC.many_elts(S, 17), [S.elts(2)[0], 1]
        absent = {(0, 3), (1, 16)}
    else:
        babies, giants = [S.elts(2)[0], 1], HC.many_elts(S, 17, one_at=5)
        assert sum(1 for g in giants if g != 1) == 17 and len(giants) == 18
        absent = {(2, 1), (17, 0)}
    table = table_of(S, len(giants), len(babies), absent=absent, seed=PLAIN_SEED + seed)
    s0 = slabs()
    got, data = check_model(S, alpha, dl, batch, babies, giants, table, seed, items=sorted({0, batch - 1}))  # a full group of four and the ragged one
    assert slabs() - s0 == 1
    if not many_babies:  # five rows per chunk: giant-sum launches of 5, 5, 5 and 2 giants, three of them accumulating
        rot_babies = sum(1 for g in babies if g != 1)
        limit = scratch_query(S, alpha, dl, batch, rot_babies, len(giants), 5)
        assert limit < scratch_query(S, alpha, dl, batch, rot_babies, len(giants), 6)
        s0 = slabs()
        assert np.array_equal(bsgs(S, alpha, data, babies, giants, table, limit=limit), got), (S.name, "five rows per chunk")
        assert slabs() - s0 == 1


# ---------------------------------------------------------------- the identities with the two grouped hoisted calls, byte for byte
def check_identities(S, dl, batch, seed):
    alpha = S.alpha
    data = S.inputs(dl, batch, seed)
    e = S.elts(5)
    babies = [e[0], 1, e[1], e[4]]
    row = table_of(S, 1, 4, seed=PLAIN_SEED + seed)[0]
    u = GH.transform(S, alpha, data, babies, np.stack(row))
    assert np.array_equal(bsgs(S, alpha, data, babies, [1], [row]), u), "giants = [1] is the grouped hoisted linear transform"
    G = e[1]
    assert np.array_equal(bsgs(S, alpha, data, babies, [G], [row]), GH.rotations(S, alpha, u, [G])[0]), "one giant is the grouped hoisted rotation of the transform"
    # a present subset of the babies only
    sub = [row[0], None, row[2], None]
    u = GH.transform(S, alpha, data, [babies[0], babies[2]], np.stack([row[0], row[2]]))
    assert np.array_equal(bsgs(S, alpha, data, babies, [G], [sub]), GH.rotations(S, alpha, u, [G])[0]), "the present pairs of the row"


# ---------------------------------------------------------------- alpha = 1 is the existing call
def check_alpha1(S, batch=3, seed=9):
    """special_primes = 1 with the per-prime keys: the bytes of troyhip_galois_plain_sum_bsgs, at every level"""
    babies, giants, table = BC.small_case(S, PLAIN_SEED + seed)
    gk1 = api.GaloisKeys(S.ctx, special_primes=1)
    for g in set(babies + giants) - {1}:
        gk1.set_elt(g, S.key(g))  # the per-prime key [K-1][2][K][N]: its shape is the grouped shape at alpha = 1
    bufs = BC.to_device(table)
    for dl in S.all_levels():
        for nb in (batch, 2):
            data = S.inputs(dl, nb, seed + dl)
            want = BC.bsgs(S, data, babies, giants, table, bufs=bufs)
            got = S.ev.applyGaloisPlainSumBsgsGrouped(S.ct(data), babies, giants, bufs, gk1)
            assert np.array_equal(got.cpu(), want), (S.name, dl, nb)


# ---------------------------------------------------------------- independence
def check_scratch_formula(S, alpha, dl):
    for batch, rot_babies, rows, gc in ((1, 1, 1, 1), (5, 3, 3, 2), (2, 40, 20, 64)):
        assert scratch_query(S, alpha, dl, batch, rot_babies, rows, gc) == scratch_formula(S, alpha, dl, batch, rot_babies, rows, gc), (batch, rot_babies, rows, gc)


def check_independence(S, alpha, dl, seed=31, batch=5):
    """the same bytes at batch 1 and batch 5, with babies and rows permuted, and under the scratch limit of (one item, one row per chunk): one item per
    slab; one word less is refused"""
    check_scratch_formula(S, alpha, dl)
    data = S.inputs(dl, batch, seed)
    babies, giants, table = small_case(S, PLAIN_SEED + seed)
    s0 = slabs()
    ref = bsgs(S, alpha, data, babies, giants, table)
    assert slabs() - s0 == 1
    assert np.array_equal(bsgs(S, alpha, data, babies, giants, table, gk=None, bufs=BC.to_device(table)), ref)
    pb, pr = [2, 0, 3, 1], [2, 0, 1]
    assert np.array_equal(bsgs(S, alpha, data, [babies[j] for j in pb], giants, [[row[j] for j in pb] for row in table]), ref), "babies permuted"
    assert np.array_equal(bsgs(S, alpha, data, babies, [giants[i] for i in pr], [table[i] for i in pr]), ref), "rows permuted"
    for b in range(batch):
        assert np.array_equal(bsgs(S, alpha, data[b:b + 1], babies, giants, table)[0], ref[b]), ("item alone", b)
    rot_babies = sum(1 for g in babies if g != 1)
    one = scratch_query(S, alpha, dl, 1, rot_babies, len(giants), 1)
    s0 = slabs()
    assert np.array_equal(bsgs(S, alpha, data, babies, giants, table, limit=one), ref), "tight limit"
    assert slabs() - s0 == batch
    HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small for one giant step of one ciphertext",
                   lambda: bsgs(S, alpha, data, babies, giants, table, limit=one - 1))
    # a null entry is an absent term: a zero plaintext in its place adds nothing before the mod-down
    zero = [list(row) for row in table]
    zero[0][3] = np.zeros_like(table[0][0])
    assert np.array_equal(bsgs(S, alpha, data, babies, giants, zero), ref), "absent against zero"


# ---------------------------------------------------------------- real keys
BABY_STEPS, GIANT_STEPS = BC.BABY_STEPS, BC.GIANT_STEPS  # (0, 1, 2), (0, 3, 6)


def real_of(S, alpha):
    return GH.Real(S, alpha, steps=tuple(sorted(set(BABY_STEPS + GIANT_STEPS))))


def check_real_bfv_bgv(S, alpha, batch=2):
    """decryption equals the slot-wise sum exactly; invariant noise budget >= the per-prime BSGS call's on the same operand - the derived margin of section
    4.16 - 2 bits of floor jitter (the floor section 4.17 asserts).  -> [(item, grouped budget, per-prime budget, margin)]"""
    R = real_of(S, alpha)
    ev, N, dl = S.ev, S.N, S.K - alpha
    rng = np.random.default_rng(13)
    benc = api.BatchEncoder(S.ctx)
    K = S.ctx.key_limbs
    msgs = [rng.integers(0, S.t, N, dtype=np.uint64) for _ in range(batch)]
    diags = [[rng.integers(0, S.t, N, dtype=np.uint64) for _ in BABY_STEPS] for _ in GIANT_STEPS]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([R.enc.encrypt(benc.encode(m)) for m in msgs]))
    a = ev.modSwitchTo(a, dl) if a.limbs > dl else a
    assert a.limbs == dl
    d_ntt = [[ev.transformPlainToNtt(api.DeviceBuffer.from_numpy(benc.encode(d)), K) for d in row] for row in diags]
    got = ev.rotateRowsPlainSumBsgsGrouped(a, BABY_STEPS, GIANT_STEPS, d_ntt, R.gk_g)
    per = ev.rotateRowsPlainSumBsgs(a, BABY_STEPS, GIANT_STEPS, d_ntt, R.gk)
    assert (got.size(), got.limbs, got.is_ntt_form, got.batch, got.scale, got.correction_factor) == (2, dl, False, batch, a.scale, a.correction_factor)
    margin = GC.noise_margin_bits(S.primes, alpha, dl, N)
    g, p = got.cpu(), per.cpu()
    out = []
    for b in range(batch):
        m = msgs[b].reshape(2, -1).astype(object)
        exp = sum(np.roll(sum(d.reshape(2, -1).astype(object) * np.roll(m, -s, axis=1) for s, d in zip(BABY_STEPS, row)), -G, axis=1)
                  for G, row in zip(GIANT_STEPS, diags)) % S.t
        dg = benc.decode(R.dec.decrypt(g[b], correction_factor=got.correction_factor))
        assert np.array_equal(dg.reshape(2, -1), exp.astype(np.uint64)), (S.name, alpha, b, "decryption")
        bg, bp = R.dec.invariantNoiseBudget(g[b]), R.dec.invariantNoiseBudget(p[b])
        print(S.name, "alpha", alpha, "item", b, "budget bsgs grouped", bg, "bsgs per-prime", bp, "margin", margin, "fresh at this level", R.dec.invariantNoiseBudget(a.cpu()[b]))
        assert bp > 0 and bg >= bp - margin - 2, (S.name, b, bg, bp, margin)
        out.append((b, bg, bp, margin))
    return out


def check_real_ckks(S, alpha, batch=2, scale=2.0 ** 40):
    """median slot error <= 1.5 x the per-prime BSGS median on the same operand (the statistic of sections 4.10 / 4.12), both maxima below 0.1"""
    R = real_of(S, alpha)
    ev, N, dl = S.ev, S.N, S.K - alpha
    n = N // 2
    rng = np.random.default_rng(14)
    cenc = api.CKKSEncoder(S.ctx)
    K = S.ctx.key_limbs
    ps = 2.0 ** 20  # the plaintexts, as grouped_hoist_cases.check_real_ckks: the product's scale stays inside the modulus at this level
    vals = [rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in range(batch)]
    diags = [[rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in BABY_STEPS] for _ in GIANT_STEPS]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([R.enc.encrypt(cenc.encode(v, scale)) for v in vals]), True, scale)
    a = ev.modSwitchTo(a, dl) if a.limbs > dl else a
    assert a.limbs == dl
    plains = BC.to_device([[cenc.encode(d, ps, limbs=K) for d in row] for row in diags])
    got = ev.rotateVectorPlainSumBsgsGrouped(a, BABY_STEPS, GIANT_STEPS, plains, R.gk_g, plain_scale=ps)
    per = ev.rotateVectorPlainSumBsgs(a, BABY_STEPS, GIANT_STEPS, plains, R.gk, plain_scale=ps)
    assert got.scale == a.scale * ps == per.scale and got.is_ntt_form and (got.size(), got.limbs, got.batch) == (2, dl, batch)
    exact = [sum(np.roll(sum(d * np.roll(v, -s) for s, d in zip(BABY_STEPS, row)), -G) for G, row in zip(GIANT_STEPS, diags)) for v in vals]
    g, p = got.cpu(), per.cpu()
    d_g = np.concatenate([np.abs(cenc.decode(R.dec.decrypt(g[b]), scale * ps) - exact[b]) for b in range(batch)])
    d_p = np.concatenate([np.abs(cenc.decode(R.dec.decrypt(p[b]), scale * ps) - exact[b]) for b in range(batch)])
    print(S.name, "alpha", alpha, "median slot error bsgs grouped", np.median(d_g), "bsgs per-prime", np.median(d_p), "maxima", d_g.max(), d_p.max())
    assert d_g.max() < 0.1 and d_p.max() < 0.1, (S.name, d_g.max(), d_p.max())
    assert np.median(d_g) <= 1.5 * np.median(d_p), (S.name, np.median(d_g), np.median(d_p))
    return float(np.median(d_g)), float(np.median(d_p))


def check_matvec(S, alpha, d=16, batch=2):
    """app.DiagonalMatvecBSGS.apply picks the grouped member for a key set with the grouped tag; BFV: exact against M x mod t"""
    rng = np.random.default_rng(15)
    M = BC.matvec_matrix(rng, d, lambda n: rng.integers(1, 1 << 9, n, dtype=np.uint64))
    mv = app.DiagonalMatvecBSGS(S.ctx, M, baby_steps=4)
    assert mv.steps == list(BC.MATVEC_DIAGONALS)
    R = GH.Real(S, alpha, steps=tuple(mv.requiredSteps()))
    benc = api.BatchEncoder(S.ctx)
    mv.encodeDiagonals(benc)
    xs = [rng.integers(0, S.t, d, dtype=np.uint64) for _ in range(batch)]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([R.enc.encrypt(benc.encode(np.tile(x, S.N // d))) for x in xs]))
    a = S.ev.modSwitchTo(a, S.K - alpha) if a.limbs > S.K - alpha else a
    s0, p0 = slabs(), BC.slabs()
    y = mv.apply(S.ev, a, R.gk_g)
    assert slabs() - s0 == 1 and BC.slabs() == p0
    yc = y.cpu()
    for b in range(batch):
        exp = (M.astype(object).dot(xs[b].astype(object)) % S.t).astype(np.uint64)
        assert np.array_equal(benc.decode(R.dec.decrypt(yc[b], correction_factor=y.correction_factor)), np.tile(exp, S.N // d)), (S.name, b)
    # a per-prime set still takes the per-prime member
    y = mv.apply(S.ev, a, R.gk)
    assert slabs() - s0 == 1 and BC.slabs() - p0 == 1


# ---------------------------------------------------------------- refusals
def raw_call(S, st_in, out_ptr, out_stride, babies, bkeys, giants, gkeys, pls, alpha, n1=None, n2=None, batch=1, limit=0, plain_scale=1.0, ctx=None):
    so = capi.CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    be, ge = (C.c_uint32 * max(len(babies), 1))(*babies), (C.c_uint32 * max(len(giants), 1))(*giants)
    bk, gk = (C.c_void_p * max(len(babies), 1))(*bkeys), (C.c_void_p * max(len(giants), 1))(*gkeys)
    p = (C.c_void_p * max(len(pls), 1))(*pls)
    rc = S.lib.troyhip_galois_plain_sum_bsgs_grouped((ctx or S.ctx).h, C.byref(st_in), C.byref(so), be, bk, len(babies) if n1 is None else n1, ge, gk,
                                                     len(giants) if n2 is None else n2, p, C.c_double(plain_scale), alpha, C.c_uint64(limit), C.c_uint64(batch), None)
    return rc, (S.lib.troyhip_last_error().decode() if rc else ""), so


def check_refusals(S, alpha):
    inv = capi.INVALID_ARGUMENT
    N, K, lmax = S.N, S.K, S.K - alpha
    item = 2 * lmax * N
    g = S.ctx.galois_elt_from_step(1)
    G = GH.keys_of(S, alpha)
    G.key(g)
    kp = G.gk.keys[api.GaloisKeys.getIndex(g)].ptr
    pts = LC.plains_of(S, 2)
    pl = [api.DeviceBuffer.from_numpy(p) for p in pts]
    pp = pl[0].ptr
    data = S.inputs(lmax, 1, 5)
    a = S.ct(data)
    st = a.struct()
    out = api.DeviceBuffer(3 * 2 * (lmax + 1) * N)
    call = lambda *args, al=alpha, **kw: raw_call(S, *args, al, **kw)[:2]
    pre = "baby-step / giant-step transform "
    assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp]) == (capi.OK, "")
    # what troyhip_galois_plain_sum_bsgs refuses, with its messages
    assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], n1=0) == (inv, pre + "takes at least one baby and one giant element")
    assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], n2=0) == (inv, pre + "takes at least one baby and one giant element")
    assert call(st, out.ptr, item, [g] * 65, [kp] * 65, [1], [None], [pp] * 65) == (inv, pre + "takes at most 64 baby and 64 giant elements")
    assert call(st, out.ptr, item, [1], [None], [g] * 65, [kp] * 65, [pp] * 65) == (inv, pre + "takes at most 64 baby and 64 giant elements")
    assert call(st, out.ptr, item, [g, 1], [kp, None], [g], [kp], [None, None]) == (inv, pre + "takes at least one plaintext")  # an empty table
    assert call(st, out.ptr, item, [2], [kp], [g], [kp], [pp]) == (inv, "Galois element is not valid")
    assert call(st, out.ptr, item, [g], [kp], [2 * N + 1], [kp], [pp]) == (inv, "Galois element is not valid")
    assert call(st, out.ptr, item, [g], [None], [1], [None], [pp]) == (inv, "Galois key not present")  # a null key for a used baby
    assert call(st, out.ptr, item, [1], [None], [g], [None], [pp]) == (inv, "Galois key not present")  # ... for a used giant
    assert call(st, out.ptr, item, [1, g], [None, None], [1, g], [None, None], [pp, None, None, None])[0] == capi.OK  # an unused element needs no key
    a3 = api.Ciphertext.from_numpy(S.ctx, synth.uniform_ct(6, S.primes[:lmax], 3, N, 1), S.ntt)
    assert call(a3.struct(), out.ptr, item, [g], [kp], [g], [kp], [pp]) == (inv, "encrypted size must be 2")
    wrong = a.struct()
    wrong.is_ntt_form = 0 if S.ntt else 1
    msg = {BFV: "BFV encrypted cannot be in NTT form", BGV: "BGV encrypted cannot be in NTT form", CKKS: "CKKS encrypted must be in NTT form"}[S.scheme]
    assert call(wrong, out.ptr, item, [g], [kp], [g], [kp], [pp]) == (inv, msg)
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    rc, text = call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], ctx=host)
    assert rc == capi.LOGIC_ERROR and "host-only" in text
    # the destination: overlapping the operand, missing, too narrow
    assert call(st, a.buf.ptr, item, [g], [kp], [g], [kp], [pp]) == (inv, pre[:-1] + ": destination must be a distinct buffer")
    assert call(st, None, item, [g], [kp], [g], [kp], [pp])[0] == inv
    assert call(st, out.ptr, item - 1, [g], [kp], [g], [kp], [pp]) == (inv, "destination batch stride too small for the result size")
    if S.scheme == CKKS:
        assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], plain_scale=2.0 ** 400) == (inv, "scale out of bounds")
    # the grouped refusals: a level above K - alpha, special_primes out of range
    if S.ctx.first_limbs >= lmax + 1:
        big = S.ct(S.inputs(lmax + 1, 1, 6))
        assert call(big.struct(), out.ptr, 2 * (lmax + 1) * N, [g], [kp], [g], [kp], [pp]) == (inv, "operand has more limbs than the grouped key serves")
    for bad in (0, -1, 9, K):
        assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], al=bad) == (inv, "special_primes must lie in 1 .. min(8, key limbs - 1)"), bad
    # the scratch limit and its query
    one = scratch_query(S, alpha, lmax, 1, 1, 1, 1)
    rc, text = call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], limit=one - 1)
    assert (rc, text) == (inv, "scratch_limit_words is too small for one giant step of one ciphertext")
    assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], limit=one)[0] == capi.OK
    w = C.c_uint64(0)
    q = S.lib.troyhip_galois_plain_sum_bsgs_grouped_scratch_words
    assert q(S.ctx.h, lmax + 1, alpha, C.c_uint64(1), 1, 1, 1, C.byref(w)) == inv and q(S.ctx.h, lmax, K, C.c_uint64(1), 1, 1, 1, C.byref(w)) == inv
    assert q(S.ctx.h, lmax, alpha, C.c_uint64(1), 65, 1, 1, C.byref(w)) == inv and q(S.ctx.h, lmax, alpha, C.c_uint64(1), 1, 0, 1, C.byref(w)) == inv
    assert q(S.ctx.h, lmax, alpha, C.c_uint64(1), 1, 1, 1, None) == inv
    assert scratch_query(S, alpha, lmax, 1, 1, 1, 1, ctx=host) == one  # host-only
    # elements 1 alone need no key; the call fills in the descriptor, the scale is the product
    rc, _, so = raw_call(S, st, out.ptr, item, [1], [None], [1], [None], [pp], alpha, plain_scale=4.0)
    assert rc == capi.OK and (so.size, so.limbs, bool(so.is_ntt_form), so.scale, so.correction_factor) == (2, lmax, S.ntt, 4.0 * a.scale, a.correction_factor)
    assert np.array_equal(out.to_numpy(item).reshape(2, lmax, N), GH.model_sum(S, alpha, data[0], [1], [None], pts[:1]))
    # the Python layer: a per-prime set is refused by the *Grouped members, a grouped one by the existing members; a key of another alpha by its shape
    per_prime = api.GaloisKeys(S.ctx)
    text = "this call takes keys with grouped digits"
    HC.with_raises(capi.InvalidArgument, text, lambda: S.ev.applyGaloisPlainSumBsgsGrouped(a, [g], [1], [pl[:1]], per_prime))
    HC.with_raises(capi.InvalidArgument, text, lambda: (S.ev.rotateVectorPlainSumBsgsGrouped if S.ntt else S.ev.rotateRowsPlainSumBsgsGrouped)(a, [0], [0], [pl[:1]], per_prime))
    HC.with_raises(capi.InvalidArgument, "grouped keys are not supported by this call", lambda: S.ev.applyGaloisPlainSumBsgs(a, [g], [1], [pl[:1]], G.gk))
    fn = S.ev.rotateVectorPlainSumBsgs if S.ntt else S.ev.rotateRowsPlainSumBsgs
    HC.with_raises(capi.InvalidArgument, "grouped keys are not supported by this call", lambda: fn(a, [1], [0], [pl[:1]], G.gk))
    other = api.GaloisKeys(S.ctx, special_primes=alpha + 1)  # a key of another alpha: its shape is not this set's
    assert other.digits != G.gk.digits
    HC.with_raises(capi.InvalidArgument, "kswitch_keys is not valid for encryption parameters", lambda: other.set_elt(g, G.key(g)))
    HC.with_raises(capi.InvalidArgument, "kswitch_keys is not valid for encryption parameters", lambda: G.gk.set_elt(g, GC.synth_key(S, alpha + 1, g)))
    empty = api.GaloisKeys(S.ctx, special_primes=alpha)
    HC.with_raises(capi.InvalidArgument, "Galois key not present", lambda: S.ev.applyGaloisPlainSumBsgsGrouped(a, [1, g], [1], [pl], empty))
    HC.with_raises(capi.InvalidArgument, "at least one baby", lambda: S.ev.applyGaloisPlainSumBsgsGrouped(a, [], [1], [[]], G.gk))
    HC.with_raises(capi.InvalidArgument, "one row of plaintexts per giant", lambda: S.ev.applyGaloisPlainSumBsgsGrouped(a, [g, 1], [1], [pl[:1]], G.gk))
    HC.with_raises(capi.InvalidArgument, "at most 64", lambda: S.ev.applyGaloisPlainSumBsgsGrouped(a, [1] * 65, [1], [[pl[0]] * 65], G.gk))
    HC.with_raises(capi.LogicError, "unsupported scheme", lambda: (S.ev.rotateRowsPlainSumBsgsGrouped if S.ntt else S.ev.rotateVectorPlainSumBsgsGrouped)(a, [0], [0], [pl[:1]], G.gk))
    # the step members equal the element members
    fn = S.ev.rotateVectorPlainSumBsgsGrouped if S.ntt else S.ev.rotateRowsPlainSumBsgsGrouped
    got = fn(a, [1, 0], [0, 1], [pl, [pl[1], None]], G.gk, plain_scale=2.0)
    want = S.ev.applyGaloisPlainSumBsgsGrouped(a, [g, 1], [1, g], [pl, [pl[1], None]], G.gk, plain_scale=2.0)
    assert got.scale == 2.0 * a.scale and np.array_equal(got.cpu(), want.cpu())


# ---------------------------------------------------------------- launch geometry
def check_large_grid(S, alpha, dl, batch, seed=41):
    """n1 = n2 = 2 and a batch whose launches all pass 65535 blocks in x, in ONE slab: a handful of items against the model, every item against the same
    call on a slice"""
    N = S.N
    e = S.elts(2)
    babies, giants = [e[0], e[1]], [e[1], e[0]]
    table = table_of(S, 2, 2, seed=PLAIN_SEED + seed)
    block = S.inputs(dl, 64, seed)
    data = np.tile(block, (-(-batch // 64), 1, 1, 1))[:batch].copy()
    data[batch // 2], data[batch - 1] = block[5][::-1], block[7][::-1]  # the sampled items are no copies of their neighbours in the tiling
    # the smallest launch: the giant sum (four items per thread over rl * N coefficients)
    assert -(-(dl + alpha) * N // 256) * -(-batch // 4) > 65535
    limit = scratch_query(S, alpha, dl, batch, 2, 2, 2)
    bufs = BC.to_device(table)
    s0 = slabs()
    got = bsgs(S, alpha, data, babies, giants, table, limit=limit, bufs=bufs)
    assert slabs() - s0 == 1
    keys = host_keys(S, alpha, babies, giants, table)
    for b in (0, batch // 2, batch - 1):
        assert np.array_equal(got[b], model_item(S, alpha, data[b], babies, giants, table, keys)), (S.name, "item", b)
    # the tiling repeats the first 64 items: the call on that slice gives every other item
    small = bsgs(S, alpha, data[:64], babies, giants, table, bufs=bufs)
    untouched = np.ones(batch, dtype=bool)
    untouched[[batch // 2, batch - 1]] = False
    idx = np.arange(batch) % 64
    for b0 in range(0, batch, 4096):
        sl = slice(b0, min(b0 + 4096, batch))
        assert np.array_equal(got[sl][untouched[sl]], small[idx[sl]][untouched[sl]]), (S.name, "items from", b0)
    for b in (batch // 2, batch - 1):
        assert np.array_equal(bsgs(S, alpha, data[b:b + 1], babies, giants, table, bufs=bufs)[0], got[b]), (S.name, "item alone", b)
