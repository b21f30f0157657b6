"""Shared checks of the baby-step / giant-step linear transform (troyhip_galois_plain_sum_bsgs): an exact host model of the
definition in two stages, the identities with the two hoisted calls, the chunk boundaries, the independence of the result from how it was asked for, the
composition of existing calls under real keys, DiagonalMatvecBSGS, the refusals and the layers.
Used by tests/test_device_bsgs.py (emulator build) and tests/test_gpu_bsgs.py (MI355X).

The model: stage 3 (the inner sum of a giant row) is hoist_lt_cases.model_item itself; stage 4 (giant_model) restates the definition independently of the
device code -- every automorphism is applied in the COEFFICIENT domain (oracle.apply_galois) and transformed (oracle.ntt_standalone), where the device
permutes transformed rows; the inner products, the sums and the mod-down are Python integers."""
import ctypes as C

import numpy as np

import hoist_cases as HC
import hoist_lt_cases as LT
from hoist_cases import obj
from oracle import oracle
from troy_amd import api, app, capi, synth
from troy_amd.capi import BFV, BGV, CKKS

PLAIN_SEED = 9300
# the lazy sums the new kernels hold, as their comments state them (poly.hip)
BOUNDS = {"bsgs_inner128": 1 << 124,                   # bsgs_inner_kernel: at most 16 products of canonical words per row and launch, "below 2^124"
          "giant_inner": LT.BOUNDS["inner"],           # hoist_sum_kernel: a MacAcc sum over the digits
          "giant_sum64": 1 << 64,                      # hoist_sum_kernel: at most 16 reduced inner sums per launch, "below 2^64"
          "giant_base64": 1 << 64}                     # bsgs_base_kernel: at most 16 canonical words per launch, in 64 bits
LAUNCH = 16


def table_of(S, n2, n1, absent=(), seed=PLAIN_SEED):
    """an n2 x n1 table of synthetic key-level plaintexts [K][N]; the pairs (i, j) of `absent` are None"""
    pts = LT.plains_of(S, n2 * n1, seed).reshape(n2, n1, S.K, S.N)
    return [[None if (i, j) in absent else pts[i, j] for j in range(n1)] for i in range(n2)]


def to_device(table):
    return [[None if p is None else api.DeviceBuffer.from_numpy(p) for p in row] for row in table]


def used(babies, giants, table):
    """the elements a present plaintext uses"""
    ub = {babies[j] for row in table for j, p in enumerate(row) if p is not None}
    ug = {giants[i] for i, row in enumerate(table) if any(p is not None for p in row)}
    return ub, ug


def bsgs(S, data, babies, giants, table, limit=0, rows_only=None, ct=None, bufs=None):
    """-> [batch][2][limbs][N] through the Python layer; only the keys of used elements are made"""
    ub, ug = used(babies, giants, table)
    for g in sorted(ub | ug):
        if g != 1:
            S.key(g, rows_only)
    out = S.ev.applyGaloisPlainSumBsgs(S.ct(data) if ct is None else ct, babies, giants, to_device(table) if bufs is None else bufs, S.gk, scratch_limit_words=limit)
    assert (out.size(), out.limbs, out.is_ntt_form, out.batch) == (2, data.shape[2], S.ntt, data.shape[0])
    return out.cpu()


# ---------------------------------------------------------------- the definition, in exact integers
def giant_model(S, us, Gs, keys, trace=None):
    """sum_i galois_{Gs[i]}(us[i]) with ONE mod-down: us[i] [2][dl][N] in the scheme's form, keys[i] [K-1][2][K][N] (not read for element 1) -> [2][dl][N]"""
    N, K, primes = S.N, S.K, S.primes
    dl = us[0].shape[1]
    qk = primes[K - 1]
    out_primes = primes[:dl] + [qk]
    key_limb = list(range(dl)) + [K - 1]
    coeffs = [[[oracle.ntt_standalone(N, primes[j], u[k, j], 3) if S.ntt else u[k, j] for j in range(dl)] for k in range(2)] for u in us]
    acc = np.zeros((2, dl + 1, N), dtype=object)
    launch = np.zeros((2, dl + 1, N), dtype=object)
    in_launch = 0
    for cf, g, key in zip(coeffs, Gs, keys):
        if g == 1:
            continue
        if in_launch == LAUNCH:
            launch[:] = 0
            in_launch = 0
        in_launch += 1
        d = cf[1]
        for i, p in enumerate(out_primes):
            inner = np.zeros((2, N), dtype=object)
            for j in range(dl):
                e = oracle.ntt_standalone(N, p, oracle.apply_galois(N, g, p, d[j] % np.uint64(p)), 1)
                for k in range(2):
                    inner[k] += obj(e) * obj(key[j, k, key_limb[i]])
            LT.note(trace, "giant_inner", inner)
            inner %= p
            acc[:, i] += inner
            launch[:, i] += inner
        LT.note(trace, "giant_sum64", launch)
    for i, p in enumerate(out_primes):
        acc[:, i] %= p
    # the base in the ciphertext's own form: sigma_G(u.c0), and u.c1 where G = 1 -- the automorphism in the coefficient domain
    base = np.zeros((2, dl, N), dtype=object)
    for j in range(dl):
        q = primes[j]
        launch = np.zeros((2, N), dtype=object)
        for r, (cf, g) in enumerate(zip(coeffs, Gs)):
            if r % LAUNCH == 0:
                launch[:] = 0
            rot = oracle.apply_galois(N, g, q, cf[0][j]) if g != 1 else cf[0][j]
            terms = [obj(oracle.ntt_standalone(N, q, rot, 1) if S.ntt else rot), obj(us[r][1, j]) if g == 1 else 0]
            for k in range(2):
                base[k, j] += terms[k]
                launch[k] += terms[k]
            LT.note(trace, "giant_base64", launch)
        base[:, j] %= q
    if all(g == 1 for g in Gs):
        return base.astype(np.uint64)
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


def model_item(S, ct, babies, giants, table, trace=None):
    """the definition for one ciphertext ct [2][dl][N]: stage 3 per used row by hoist_lt_cases.model_item, stage 4 by giant_model.  trace: the largest
    value of each lazy sum of the new kernels (BOUNDS); the row sums of bsgs_inner_kernel are hoist_lt_kernel<true>'s over the same pairs where the call
    has at most 16 babies other than 1 (one launch holds them all), which is where a trace is asked for"""
    bkeys = [S.host_keys.get(g) for g in babies]
    assert trace is None or sum(1 for g in babies if g != 1) <= LAUNCH
    us, Gs, gkeys = [], [], []
    for G, row in zip(giants, table):
        present = [j for j, p in enumerate(row) if p is not None]
        if not present:
            continue
        lt = None if trace is None else {}
        us.append(LT.model_item(S, ct, [babies[j] for j in present], [bkeys[j] for j in present], [row[j] for j in present], lt))
        for name, v in (lt or {}).items():
            assert v < LT.BOUNDS[name], (S.name, "the inputs break the documented bound of", name)
            if name == "outer128":
                LT.note(trace, "bsgs_inner128", [v])
        Gs.append(G)
        gkeys.append(S.host_keys.get(G))
    return giant_model(S, us, Gs, gkeys, trace)


def check_model(S, limbs, batch, babies, giants, table, seed, items=None, rows_only=None, limit=0, trace=None):
    """every limb of every output item (or of `items`) equals the model and is canonical"""
    data = S.inputs(limbs, batch, seed)
    got = bsgs(S, data, babies, giants, table, limit=limit, rows_only=rows_only)
    assert got.shape == (batch, 2, limbs, S.N)
    for b in (range(batch) if items is None else items):
        exp = model_item(S, data[b], babies, giants, table, trace)
        for name, v in (trace or {}).items():
            assert v < BOUNDS[name], (S.name, "the inputs break the documented bound of", name, v, BOUNDS[name])
        assert np.array_equal(got[b], exp), (S.name, limbs, "item", b, babies, giants)
        assert all((got[b, :, j] < np.uint64(S.primes[j])).all() for j in range(limbs))
    return got, data


def small_case(S, seed=PLAIN_SEED):
    """n1 = n2 = 3: one baby 1, one giant 1, one absent plaintext"""
    e = S.elts(5)
    return [e[0], 1, e[1]], [e[4], 1, e[0]], table_of(S, 3, 3, absent={(0, 2)}, seed=seed)


def check_small(S, limbs, seed):
    babies, giants, table = small_case(S, PLAIN_SEED + seed)
    for batch in (5, 1, 2):
        check_model(S, limbs, batch, babies, giants, table, seed + batch)


def check_identity_rows(S, limbs, seed):
    """a row whose only present baby is 1 (u is its base, among rows that take the mod-down) and a call whose babies and giants are all 1 (no key at all)"""
    babies, giants, _ = small_case(S)
    check_model(S, limbs, 3, babies, giants, table_of(S, 3, 3, absent={(2, 0), (2, 2), (1, 1)}, seed=PLAIN_SEED + seed), seed)
    lone = HC.Setup(S.name, S.cfg)
    check_model(lone, limbs, 2, [1, 1], [1, 1], table_of(lone, 2, 2, absent={(1, 0)}, seed=PLAIN_SEED + seed), seed + 1)
    assert not lone.host_keys and not lone.gk.keys


# ---------------------------------------------------------------- the identities with the two hoisted calls, byte for byte
def check_identities(S, limbs, batch, seed):
    data = S.inputs(limbs, batch, seed)
    e = S.elts(5)
    babies = [e[0], 1, e[1], e[4]]
    row = table_of(S, 1, 4, seed=PLAIN_SEED + seed)[0]
    u = LT.fused(S, data, babies, np.stack(row))
    assert np.array_equal(bsgs(S, data, babies, [1], [row]), u), "giants = [1] is the hoisted linear transform"
    G = e[1]
    assert np.array_equal(bsgs(S, data, babies, [G], [row]), S.hoisted(u, [G])[0]), "one giant is the hoisted rotation of the hoisted linear transform"
    # babies = [1]: the giant stage alone, u_i = pt[i][0] * ct
    giants = [e[0], 1, e[4]]
    col = table_of(S, 3, 1, seed=PLAIN_SEED + seed + 1)
    got = bsgs(S, data, [1], giants, col)
    for b in range(batch):
        us = [LT.model_item(S, data[b], [1], [None], [r[0]]) for r in col]
        assert np.array_equal(got[b], giant_model(S, us, giants, [S.host_keys.get(g) for g in giants])), (S.name, "giant stage alone, item", b)


# ---------------------------------------------------------------- chunk boundaries and the scratch plan
def scratch_words(S, limbs, items, rot_babies, rows, gc):
    """what Evaluator::galois_plain_sum_bsgs asks of the arena for a slab of `items` with `gc` rows per chunk (evaluator.cpp; include/troyhip.h documents it)"""
    N, dl, rl = S.N, limbs, limbs + 1
    ck = dl if S.ntt else 0
    per_item = rl * dl + ck + min(16, rot_babies) * 2 * rl + rows * 2 * rl + (0 if S.ntt else dl) + 2 * rl + 2 * dl
    per_row = 4 * dl + rl * dl + ck + 2 * dl + 4
    return items * N * (per_item + gc * per_row) + 32 * 16 + 128


def slabs():
    return capi.stat("bsgs_slabs", api.KernelProvider.lib())


def check_chunks(S, limbs, batch, seed, many_babies):
    """n1 = 17 (two baby chunks: the accumulate path of bsgs_inner_kernel) or n2 = 18 with 17 giants other than 1 and element 1 among them (the
    evaluator runs the giants other than 1 first, 16 rows per chunk under the default limit: a launch of hoist_sum_kernel over 16 giants and an
    accumulating one over the seventeenth) against the model.  Then the same limbs under a limit of five rows per chunk and the whole batch (n2 = 18:
    launches of 5, 5, 5 and 2 giants, three of them accumulating -- four giants per thread at batch 1, four items per thread at batch 5), and under a
    limit that forces one row per chunk and slabs of two items"""
    if many_babies:
        babies, giants = HC.many_elts(S, 17), [S.elts(2)[0], 1]
        absent = {(0, 3), (1, 16)}
    else:
        babies, giants = [S.elts(2)[0], 1], HC.many_elts(S, 17, one_at=5)
        assert sum(1 for g in giants if g != 1) == 17 and len(giants) == 18
        absent = {(2, 1), (17, 0)}
    table = table_of(S, len(giants), len(babies), absent=absent, seed=PLAIN_SEED + seed)
    rot_babies = sum(1 for g in babies if g != 1)
    s0 = slabs()
    got, data = check_model(S, limbs, batch, babies, giants, table, seed)
    assert slabs() - s0 == 1
    if not many_babies:
        limit = scratch_words(S, limbs, batch, rot_babies, len(giants), 5)
        assert limit < scratch_words(S, limbs, batch, rot_babies, len(giants), 6)
        s0 = slabs()
        assert np.array_equal(bsgs(S, data, babies, giants, table, limit=limit), got), (S.name, "five rows per chunk")
        assert slabs() - s0 == 1
    per_slab = 2 if batch > 2 else 1
    limit = scratch_words(S, limbs, per_slab, rot_babies, len(giants), 1)
    s0 = slabs()
    assert np.array_equal(bsgs(S, data, babies, giants, table, limit=limit), got), (S.name, "one row per chunk, slabs of", per_slab)
    assert slabs() - s0 == -(-batch // per_slab)
    if batch == 1:
        HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small", lambda: bsgs(S, data, babies, giants, table, limit=limit - 1))


# ---------------------------------------------------------------- independence
def check_independence(S, limbs, seed, batch=5):
    data = S.inputs(limbs, batch, seed)
    babies, giants, table = small_case(S, PLAIN_SEED + seed)
    ref = bsgs(S, data, babies, giants, table)
    # a dense operand (an odd batch is a strided one)
    assert np.array_equal(bsgs(S, data, babies, giants, table, ct=api.Ciphertext.from_numpy(S.ctx, data, S.ntt)), ref), "strided against dense"
    perm = [2, 0, 1]
    assert np.array_equal(bsgs(S, data, [babies[j] for j in perm], giants, [[row[j] for j in perm] for row in table]), ref), "babies permuted"
    assert np.array_equal(bsgs(S, data, babies, [giants[i] for i in perm], [table[i] for i in perm]), ref), "rows permuted"
    for b in range(batch):
        assert np.array_equal(bsgs(S, data[b:b + 1], babies, giants, table)[0], ref[b]), ("item alone", b)
    s0 = slabs()
    assert np.array_equal(bsgs(S, data, babies, giants, table, limit=scratch_words(S, limbs, 1, 2, 3, 1)), ref), "tight limit"
    assert slabs() - s0 == batch
    # one plaintext word changed: another result; the same word of an ABSENT pair's neighbour is not confused with it
    other = [list(row) for row in table]
    other[2][1] = other[2][1].copy()
    other[2][1][0, 5] = (other[2][1][0, 5] + np.uint64(1)) % np.uint64(S.primes[0])
    assert not np.array_equal(bsgs(S, data, babies, giants, other), ref)
    # a null entry is an absent term: the arithmetic is exact, so a zero plaintext in its place adds nothing before the mod-down
    zero = [list(row) for row in table]
    zero[0][2] = np.zeros_like(table[0][0])
    assert np.array_equal(bsgs(S, data, babies, giants, zero), ref), "absent against zero"


# ---------------------------------------------------------------- against the composition of existing calls, with real keys
BABY_STEPS, GIANT_STEPS = (0, 1, 2), (0, 3, 6)


def compose(S, a, rots, plain_mul, rotate):
    """the same BSGS from existing calls: hoisted baby rotations, plaintext multiply-accumulate per row, one rotation per giant, additions"""
    total = None
    for i, G in enumerate(GIANT_STEPS):
        inner = None
        for j in range(len(BABY_STEPS)):
            term = plain_mul(rots[j].copy(), i, j)
            if inner is None:
                inner = term
            else:
                S.ev.addInplace(inner, term)
        if G:
            inner = rotate(inner, G)
        if total is None:
            total = inner
        else:
            S.ev.addInplace(total, inner)
    return total


def check_composition_bfv_bgv(name, batch=2):
    S = HC.RealSetup(name, sorted(set(BABY_STEPS + GIANT_STEPS)))
    rng = np.random.default_rng(7)
    benc = api.BatchEncoder(S.ctx)
    K, N = S.ctx.key_limbs, S.N
    msgs = [rng.integers(0, S.t, N, dtype=np.uint64) for _ in range(batch)]
    diags = [[rng.integers(0, S.t, N, dtype=np.uint64) for _ in BABY_STEPS] for _ in GIANT_STEPS]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(benc.encode(m)) for m in msgs]))
    d_coeff = [[api.DeviceBuffer.from_numpy(benc.encode(d)) for d in row] for row in diags]
    d_ntt = [[S.ev.transformPlainToNtt(p, K) for p in row] for row in d_coeff]
    got = S.ev.rotateRowsPlainSumBsgs(a, BABY_STEPS, GIANT_STEPS, d_ntt, S.gk)
    assert (got.size(), got.limbs, got.is_ntt_form, got.batch, got.scale, got.correction_factor) == (2, a.limbs, False, batch, a.scale, a.correction_factor)
    rots = S.ev.rotateRowsHoisted(a, BABY_STEPS, S.gk)

    def plain_mul(term, i, j):
        S.ev.multiplyPlainNormalInplace(term, d_coeff[i][j])
        return term
    seq = compose(S, a, rots, plain_mul, lambda x, G: S.ev.rotateRows(x, G, S.gk))
    f, q = got.cpu(), seq.cpu()
    budgets = []
    for b in range(batch):
        df, ds = S.dec.decrypt(f[b]), S.dec.decrypt(q[b])
        assert np.array_equal(df, ds), (name, b)
        m = msgs[b].reshape(2, -1).astype(object)
        exp = sum(np.roll(sum(d.reshape(2, -1).astype(object) * np.roll(m, -s, axis=1) for s, d in zip(BABY_STEPS, row)), -G, axis=1)
                  for G, row in zip(GIANT_STEPS, diags)) % S.t
        assert np.array_equal(benc.decode(df).reshape(2, -1), exp.astype(np.uint64)), (name, b)
        bf, bq, fresh = S.dec.invariantNoiseBudget(f[b]), S.dec.invariantNoiseBudget(q[b]), S.dec.invariantNoiseBudget(a.cpu()[b])
        print(name, "item", b, "budget bsgs", bf, "composed", bq, "fresh", fresh)
        assert bq > 0 and bf >= bq - 2, (name, b, bf, bq)
        budgets.append((bf, bq))
    return budgets


def check_composition_ckks(name, batch=2, scale=2.0 ** 25):
    S = HC.RealSetup(name, sorted(set(BABY_STEPS + GIANT_STEPS)))
    rng = np.random.default_rng(8)
    cenc = api.CKKSEncoder(S.ctx)
    K, n = S.ctx.key_limbs, S.N // 2
    vals = [rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in range(batch)]
    diags = [[rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in BABY_STEPS] for _ in GIANT_STEPS]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(cenc.encode(v, scale)) for v in vals]), True, scale)
    plains_np = [[cenc.encode(d, scale, limbs=K) for d in row] for row in diags]
    got = S.ev.rotateVectorPlainSumBsgs(a, BABY_STEPS, GIANT_STEPS, to_device(plains_np), S.gk, plain_scale=scale)
    assert got.scale == a.scale * scale and got.is_ntt_form and (got.size(), got.limbs, got.batch) == (2, a.limbs, batch)
    rots = S.ev.rotateVectorHoisted(a, BABY_STEPS, S.gk)

    def plain_mul(term, i, j):
        S.ev.multiplyPlainInplace(term, api.DeviceBuffer.from_numpy(plains_np[i][j][:a.limbs]), scale)
        return term
    seq = compose(S, a, rots, plain_mul, lambda x, G: S.ev.rotateVector(x, G, S.gk))
    assert seq.scale == got.scale
    exact = [sum(np.roll(sum(d * np.roll(v, -s) for s, d in zip(BABY_STEPS, row)), -G) for G, row in zip(GIANT_STEPS, diags)) for v in vals]
    f, q = got.cpu(), seq.cpu()
    d_f = np.concatenate([np.abs(cenc.decode(S.dec.decrypt(f[b]), scale * scale) - exact[b]) for b in range(batch)])
    d_s = np.concatenate([np.abs(cenc.decode(S.dec.decrypt(q[b]), scale * scale) - exact[b]) for b in range(batch)])
    print(name, "max slot error bsgs", d_f.max(), "composed", d_s.max(), "medians", np.median(d_f), np.median(d_s))
    assert d_f.max() < 0.1 and d_s.max() < 0.1, (name, d_f.max(), d_s.max())
    assert np.median(d_f) <= 1.5 * np.median(d_s), (name, np.median(d_f), np.median(d_s))
    return d_f.max(), d_s.max(), np.median(d_f), np.median(d_s)


# ---------------------------------------------------------------- DiagonalMatvecBSGS
MATVEC_DIAGONALS = (0, 1, 3, 5, 13, 14)  # d = 16, baby_steps = 4: rows 0, 1 and 3; the giant row 2 (diagonals 8 .. 11) is zero


def matvec_matrix(rng, d, draw):
    k = np.arange(d)
    m = np.zeros((d, d), dtype=np.asarray(draw(1)).dtype)
    for r in MATVEC_DIAGONALS:
        m[k, (k + r) % d] = draw(d)
    return m


def check_matvec_bfv(name="bfv_n64_k3", d=16, batch=2):
    rng = np.random.default_rng(9)
    M = matvec_matrix(rng, d, lambda n: rng.integers(1, 1 << 9, n, dtype=np.uint64))
    cfg = HC.config(name)
    probe = api.SEALContext(cfg["scheme"], cfg["N"], api.CoeffModulus.Create(cfg["N"], cfg["bits"]), api.PlainModulus.Batching(cfg["N"], cfg["tbits"]))
    mv = app.DiagonalMatvecBSGS(probe, M, baby_steps=4)
    assert mv.steps == list(MATVEC_DIAGONALS) and mv.requiredSteps() == [1, 2, 3, 4, 12]
    assert app.DiagonalMatvecBSGS(probe, M).n1 == 8  # the default: the power of two nearest sqrt(6 d) = 9.8
    S = HC.RealSetup(name, mv.requiredSteps())  # a key set holding exactly those steps suffices
    mv = app.DiagonalMatvecBSGS(S.ctx, M, baby_steps=4)
    benc = api.BatchEncoder(S.ctx)
    table = mv.encodeDiagonals(benc)
    assert [[p is not None for p in row] for row in table] == [[True, True, False, True], [False, True, False, False], [False] * 4, [False, True, True, False]]
    xs = [rng.integers(0, S.t, d, dtype=np.uint64) for _ in range(batch)]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(benc.encode(np.tile(x, S.N // d))) for x in xs]))
    y = mv.apply(S.ev, a, S.gk).cpu()
    for b in range(batch):
        exp = (M.astype(object).dot(xs[b].astype(object)) % S.t).astype(np.uint64)
        assert np.array_equal(benc.decode(S.dec.decrypt(y[b])), np.tile(exp, S.N // d)), (name, b)


def check_matvec_ckks(name="ckks_n128_k6", d=16, batch=2, scale=2.0 ** 25):
    rng = np.random.default_rng(10)
    M = matvec_matrix(rng, d, lambda n: rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n))
    S = HC.RealSetup(name, sorted({1, 2, 3, 4, 12} | set(MATVEC_DIAGONALS)))
    mv, flat = app.DiagonalMatvecBSGS(S.ctx, M, baby_steps=4), app.DiagonalMatvec(S.ctx, M)
    assert mv.requiredSteps() == [1, 2, 3, 4, 12]
    cenc = api.CKKSEncoder(S.ctx)
    mv.encodeDiagonals(cenc, scale)
    flat.encodeDiagonals(cenc, scale)
    n = S.N // 2
    xs = [rng.uniform(-1, 1, d) + 1j * rng.uniform(-1, 1, d) for _ in range(batch)]
    a = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(cenc.encode(np.tile(x, n // d), scale)) for x in xs]), True, scale)
    got, ref = mv.apply(S.ev, a, S.gk), flat.apply(S.ev, a, S.gk)
    assert got.scale == scale * scale == ref.scale
    exact = [np.tile(M.dot(x), n // d) for x in xs]
    f, q = got.cpu(), ref.cpu()
    d_f = np.concatenate([np.abs(cenc.decode(S.dec.decrypt(f[b]), scale * scale) - exact[b]) for b in range(batch)])
    d_s = np.concatenate([np.abs(cenc.decode(S.dec.decrypt(q[b]), scale * scale) - exact[b]) for b in range(batch)])
    print(name, "matvec max slot error bsgs", d_f.max(), "DiagonalMatvec", d_s.max(), "medians", np.median(d_f), np.median(d_s))
    assert d_s.max() < 0.1 and d_f.max() < 0.1 and np.median(d_f) <= 1.5 * np.median(d_s), (name, np.median(d_f), np.median(d_s))


# ---------------------------------------------------------------- refusals and the layers
def raw_call(S, st_in, out_ptr, out_stride, babies, bkeys, giants, gkeys, pls, n1=None, n2=None, batch=1, limit=0, plain_scale=1.0, ctx=None):
    so = capi.CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    be, ge = (C.c_uint32 * max(len(babies), 1))(*babies), (C.c_uint32 * max(len(giants), 1))(*giants)
    bk, gk = (C.c_void_p * max(len(babies), 1))(*bkeys), (C.c_void_p * max(len(giants), 1))(*gkeys)
    p = (C.c_void_p * max(len(pls), 1))(*pls)
    rc = S.lib.troyhip_galois_plain_sum_bsgs(S.ctx.h if ctx is None else ctx.h, C.byref(st_in), C.byref(so), be, bk, len(babies) if n1 is None else n1,
                                             ge, gk, len(giants) if n2 is None else n2, p, C.c_double(plain_scale), C.c_uint64(limit), C.c_uint64(batch), None)
    return (rc, S.lib.troyhip_last_error().decode() if rc else "", so)


def check_refusals(S):
    inv = capi.INVALID_ARGUMENT
    limbs, N, K = S.ctx.first_limbs, S.N, S.K
    item = 2 * limbs * N
    g = S.ctx.galois_elt_from_step(1)
    S.key(g)
    kp = S.gk.keys[api.GaloisKeys.getIndex(g)].ptr
    pts = LT.plains_of(S, 2)
    pl = [api.DeviceBuffer.from_numpy(p) for p in pts]
    pp = pl[0].ptr
    data = S.inputs(limbs, 1, 5)
    a = S.ct(data)
    a3 = api.Ciphertext.from_numpy(S.ctx, synth.uniform_ct(6, S.primes[:limbs], 3, N, 1), S.ntt)
    out = api.DeviceBuffer(3 * item)
    st = a.struct()
    call = lambda *args, **kw: raw_call(S, *args, **kw)[:2]
    at_least, at_most = "takes at least one baby and one giant element", "takes at most 64 baby and 64 giant elements"
    assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], n1=0)[1].endswith(at_least)
    assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], n2=0) == (inv, "baby-step / giant-step transform " + at_least)
    assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], n1=-1)[0] == inv
    assert call(st, out.ptr, item, [g] * 65, [kp] * 65, [1], [None], [pp] * 65) == (inv, "baby-step / giant-step transform " + at_most)
    assert call(st, out.ptr, item, [1], [None], [g] * 65, [kp] * 65, [pp] * 65) == (inv, "baby-step / giant-step transform " + at_most)
    assert call(st, out.ptr, item, [g, 1], [kp, None], [g], [kp], [None, None]) == (inv, "baby-step / giant-step transform takes at least one plaintext")
    assert call(st, out.ptr, item, [2], [kp], [g], [kp], [pp]) == (inv, "Galois element is not valid")
    assert call(st, out.ptr, item, [g], [kp], [2 * N + 1], [kp], [pp]) == (inv, "Galois element is not valid")
    assert call(st, out.ptr, item, [g], [None], [1], [None], [pp]) == (inv, "Galois key not present")
    assert call(st, out.ptr, item, [1], [None], [g], [None], [pp]) == (inv, "Galois key not present")
    # ... but an element no present plaintext uses needs no key
    assert call(st, out.ptr, item, [1, g], [None, None], [1, g], [None, None], [pp, None, None, None])[0] == capi.OK
    assert call(a3.struct(), out.ptr, item, [g], [kp], [g], [kp], [pp]) == (inv, "encrypted size must be 2")
    wrong = a.struct()
    wrong.is_ntt_form = 0 if S.ntt else 1
    msg = {BFV: "BFV encrypted cannot be in NTT form", BGV: "BGV encrypted cannot be in NTT form", CKKS: "CKKS encrypted must be in NTT form"}[S.scheme]
    assert call(wrong, out.ptr, item, [g], [kp], [g], [kp], [pp]) == (inv, msg)
    # a host-only context and one with a single prime.  (A key made under ANOTHER context is refused where keys carry their parameters: troyn::Evaluator,
    # tests/cpp/test_troyn_bsgs.cpp; the C ABI and this layer take raw device pointers.  "more than 63 digits" cannot be reached: a context takes at
    # most 64 key primes, so a ciphertext has at most 63 limbs; the check guards the 64-bit digit masks of the kernels, as in the two hoisted calls.)
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    rc, text = call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], ctx=host)
    assert rc == capi.LOGIC_ERROR and "host-only" in text
    single = api.SEALContext(S.scheme, N, S.primes[:1], S.t)
    one = api.Ciphertext.from_numpy(single, synth.uniform_ct(7, S.primes[:1], 2, N, 1), S.ntt)
    assert call(one.struct(), out.ptr, 2 * N, [g], [kp], [g], [kp], [pp], ctx=single) == (capi.LOGIC_ERROR, "keyswitching is not supported by the context")
    # the destination: overlapping the operand, missing, too narrow
    assert call(st, a.buf.ptr, item, [g], [kp], [g], [kp], [pp]) == (inv, "baby-step / giant-step transform: destination must be a distinct buffer")
    assert call(st, None, item, [g], [kp], [g], [kp], [pp])[0] == inv
    assert call(st, out.ptr, item - 1, [g], [kp], [g], [kp], [pp]) == (inv, "destination batch stride too small for the result size")
    if S.scheme == CKKS:
        assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], plain_scale=2.0 ** 400) == (inv, "scale out of bounds")
    rc, text = call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], limit=scratch_words(S, limbs, 1, 1, 1, 1) - 1)
    assert rc == inv and text.startswith("scratch_limit_words is too small")
    assert call(st, out.ptr, item, [g], [kp], [g], [kp], [pp], limit=scratch_words(S, limbs, 1, 1, 1, 1))[0] == capi.OK
    # elements 1 alone need no key; the call fills in the descriptor, the scale is the product
    rc, _, so = raw_call(S, st, out.ptr, item, [1], [None], [1], [None], [pp], plain_scale=4.0)
    assert rc == capi.OK and (so.size, so.limbs, bool(so.is_ntt_form), so.scale, so.correction_factor) == (2, limbs, S.ntt, 4.0 * a.scale, a.correction_factor)
    assert np.array_equal(out.to_numpy(item).reshape(2, limbs, N), LT.model_item(S, data[0], [1], [None], pts[:1]))
    # the Python layer: the same refusals as exceptions
    gk = S.gk
    HC.with_raises(capi.InvalidArgument, "Galois key not present", lambda: S.ev.applyGaloisPlainSumBsgs(a, [1, g], [1], [pl], api.GaloisKeys(S.ctx)))
    HC.with_raises(capi.InvalidArgument, "at least one baby", lambda: S.ev.applyGaloisPlainSumBsgs(a, [], [1], [[]], gk))
    HC.with_raises(capi.InvalidArgument, "at least one baby", lambda: S.ev.applyGaloisPlainSumBsgs(a, [g], [], [], gk))
    HC.with_raises(capi.InvalidArgument, "one row of plaintexts per giant", lambda: S.ev.applyGaloisPlainSumBsgs(a, [g, 1], [1], [pl[:1]], gk))
    HC.with_raises(capi.InvalidArgument, "at least one plaintext", lambda: S.ev.applyGaloisPlainSumBsgs(a, [g, 1], [1], [[None, None]], gk))
    HC.with_raises(capi.InvalidArgument, "at most 64", lambda: S.ev.applyGaloisPlainSumBsgs(a, [1] * 65, [1], [[pl[0]] * 65], gk))
    HC.with_raises(capi.InvalidArgument, r"\[K\]\[N\] words", lambda: S.ev.applyGaloisPlainSumBsgs(a, [g], [1], [[api.DeviceBuffer((K - 1) * N)]], gk))
    HC.with_raises(capi.InvalidArgument, "encrypted size must be 2", lambda: S.ev.applyGaloisPlainSumBsgs(a3, [g], [1], [pl[:1]], gk))
    HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small", lambda: S.ev.applyGaloisPlainSumBsgs(a, [g], [1], [pl[:1]], gk, scratch_limit_words=1000))
    HC.with_raises(capi.LogicError, "unsupported scheme", lambda: (S.ev.rotateRowsPlainSumBsgs if S.ntt else S.ev.rotateVectorPlainSumBsgs)(a, [1], [1], [pl[:1]], gk))
    if S.scheme != CKKS:
        ntt_in = api.Ciphertext.from_numpy(S.ctx, data, True)
        HC.with_raises(capi.InvalidArgument, "cannot be in NTT form", lambda: S.ev.applyGaloisPlainSumBsgs(ntt_in, [g], [1], [pl[:1]], gk))


def check_python_layer(S):
    """rotate*PlainSumBsgs map steps through galois_elt_from_step, step 0 to element 1, and equal applyGaloisPlainSumBsgs"""
    limbs = S.ctx.first_limbs
    data = S.inputs(limbs, 3, 21)
    bsteps, gsteps = [1, 0, -1], [0, 2]
    elt = lambda s: S.ctx.galois_elt_from_step(s) if s else 1
    table = table_of(S, 2, 3, absent={(1, 1)})
    ref = bsgs(S, data, [elt(s) for s in bsteps], [elt(s) for s in gsteps], table)
    fn = S.ev.rotateVectorPlainSumBsgs if S.ntt else S.ev.rotateRowsPlainSumBsgs
    got = fn(S.ct(data), bsteps, gsteps, to_device(table), S.gk, plain_scale=2.0)
    assert isinstance(got, api.Ciphertext) and got.scale == 2.0
    assert np.array_equal(got.cpu(), ref)


# ---------------------------------------------------------------- the routes only large launches take
def check_large_route(S, limbs, batch, babies, giants, table, seed, rows_only=None, limit=0, model_items=None):
    """ONE call of `batch` items: three items against the model, EVERY item bit-for-bit against the same call at batch 1 -> the path-counter deltas"""
    data = S.inputs(limbs, batch, seed)
    ub, ug = used(babies, giants, table)
    for g in sorted(ub | ug):
        if g != 1:
            S.key(g, rows_only)
    bufs = to_device(table)
    s0 = HC.route_stats()
    got = bsgs(S, data, babies, giants, table, limit=limit, rows_only=rows_only, bufs=bufs)
    big = HC.delta(HC.route_stats(), s0)
    one = None
    for b in range(batch):
        s0 = HC.route_stats()
        alone = bsgs(S, data[b:b + 1], babies, giants, table, rows_only=rows_only, bufs=bufs)[0]
        one = one or HC.delta(HC.route_stats(), s0)
        assert np.array_equal(alone, got[b]), (S.name, "item", b, "differs from the same call at batch 1")
    for b in sorted({0, batch // 2, batch - 1} if model_items is None else model_items):
        assert np.array_equal(got[b], model_item(S, data[b], babies, giants, table)), (S.name, limbs, "item", b)
    print(S.name, "batch", batch, "counters of the large call", big, "of the call at batch 1", one)
    return big, one


# ---------------------------------------------------------------- residues at the ends of their range
def check_edge_pattern(scheme, bits, pattern, N=128, batches=(1, 5), seed=1900):
    """n1 = n2 = 16 elements other than 1 on the edge pattern applied to the ciphertext, the keys and the plaintexts together: sixteen terms in every lazy
    sum of a launch.  The model's own accumulators are held against the bounds the kernels' comments state before any limb is compared.
    -> the largest values the model saw, as fractions of their bounds"""
    S = HC.Setup(*HC.adhoc(HC.SCHEMES[scheme], N, bits, 40 if bits[0] == 60 and N == 128 else None), patterns=(pattern,) * 3)
    elts = HC.many_elts(S, 32)
    babies, giants = elts[:16], elts[16:]
    table = table_of(S, 16, 16, seed=PLAIN_SEED + seed)
    trace = {}
    for batch in batches:
        check_model(S, S.ctx.first_limbs, batch, babies, giants, table, seed + batch, items=[batch - 1], trace=trace)
    return {n: trace[n] / BOUNDS[n] for n in trace}
