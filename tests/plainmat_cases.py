"""Shared checks of the plaintext matrix times ciphertext vector (troyhip_multiply_plain_matrix) and of the PIR client and server
built on it (troy_amd/app.py).  Every step is exact arithmetic modulo p_l on canonical residues, so every comparison here is np.array_equal: against the
exact model in integers, against the multiplyPlainAccumulate + add composition of existing calls, of the call against itself on single items, single
columns, permuted rows and other strides, and of decryptions under real keys against the records.
Used by tests/test_device_plainmat.py (emulator build) and tests/test_gpu_plainmat.py (MI355X)."""
import ctypes as C

import numpy as np

import hoist_cases as HC
from troy_amd import api, app, capi, synth
from troy_amd.capi import BFV, CKKS

SYMBOL = "troyhip_multiply_plain_matrix"
COUNTER = "plainmat_launches"
SETS = ["bfv_n64_k3", "bgv_n128_k4", "ckks_n128_k6"]
NARROW = "nar_bfv_n4096_k3"        # primes below 2^33
ROWS = [1, 3, 63, 64, 130]         # a run of the lazy sums closes after 63 products: one run, a run and one product, more than two runs
COLS = [1, 4, 5]                   # a full tile of four columns, a ragged one; in the batched instance (tiles of two) one, two and two and a half tiles
BATCHES = [1, 2, 5]                # 1: the single-ciphertext instance; 2, 5: the batched one; 5: a strided operand and a ragged tile of left rows
ANCHOR_ROWS = [3, 16, 17, 40]
POOL = (130, 5, 5)                 # rows, batch, columns of the operands every smaller case is a corner of


def stat(name=COUNTER):
    return capi.stat(name, api.KernelProvider.lib())


def check_symbol(lib, header_text):
    assert hasattr(lib, SYMBOL) and SYMBOL in capi.SYMBOLS and "int %s(" % SYMBOL in header_text
    assert capi.stat(COUNTER, lib) >= 0 and capi.stat("plainmat_workgroups", lib) >= 0


# ---------------------------------------------------------------- the definition, in exact integers
def model(primes, ins, pls):
    """ins [R][B][size][limbs][N], pls [R][C][limbs][N] -> [C][B][size][limbs][N]: sum_r ins[r] * pls[r][c] mod p_l.  The operands are cut into
    21-bit pieces whose products, summed over the rows in 64-bit words, cannot overflow (rows * 2^42 < 2^64); the nine partial sums are put
    together and reduced in Python integers."""
    R = ins.shape[0]
    assert R < (1 << 22) and all(p < (1 << 63) for p in primes)
    mask = np.uint64((1 << 21) - 1)
    cut = lambda a: [(a >> np.uint64(21 * i)) & mask if i < 2 else a >> np.uint64(42) for i in range(3)]  # noqa: E731
    a, b = cut(ins), cut(pls)
    total = 0
    for i in range(3):
        for j in range(3):
            part = np.einsum("rbkln,rcln->cbkln", a[i], b[j])
            total = total + (part.astype(object) << (21 * (i + j)))
    out = np.empty(total.shape, dtype=np.uint64)
    for l, p in enumerate(primes):
        out[:, :, :, l] = (total[:, :, :, l] % p).astype(np.uint64)
    return out


def spot_check_model(primes, ins, pls, exp, seed=1, words=24):
    """a few words of the model against the definition written out in plain Python integers"""
    rng = np.random.default_rng(seed)
    R, B, size, limbs, N = ins.shape
    for _ in range(words):
        c, b, k, l, n = (int(rng.integers(0, d)) for d in (pls.shape[1], B, size, limbs, N))
        v = sum(int(ins[r, b, k, l, n]) * int(pls[r, c, l, n]) for r in range(R)) % primes[l]
        assert v == int(exp[c, b, k, l, n])


def canonical(primes, got):
    return all((got[..., l, :] < np.uint64(p)).all() for l, p in enumerate(primes))


# ---------------------------------------------------------------- operands
def pool(S, limbs, seed=9300):
    """the operands of one level, made once and left unchanged: (ins [130][5][3][limbs][N], pls [130][5][limbs][N]) in the setup's patterns"""
    cache = S.__dict__.setdefault("_plainmat_pool", {})
    if limbs not in cache:
        R, B, Cn = POOL
        q = S.primes[:limbs]
        ins = synth.edge_rows(S.ct_pattern, seed + limbs, q, R * B * 3 * limbs, S.N).reshape(R, B, 3, limbs, S.N)
        pls = synth.edge_rows(S.pt_pattern, seed + 50 + limbs, q, R * Cn * limbs, S.N).reshape(R, Cn, limbs, S.N)
        ins.setflags(write=False)
        pls.setflags(write=False)
        cache[limbs] = (ins, pls)
    return cache[limbs]


def operand(S, ins, scale=1.0, cf=1):
    """ins [R][B][size][limbs][N] -> ONE Ciphertext of R * B items, row after row.  As Setup.ct, an odd batch of size-2 items leaves room for a third
    polynomial per item: the operand is then a strided batch"""
    R, B, size, limbs, N = ins.shape
    return api.Ciphertext.from_numpy(S.ctx, ins.reshape(R * B, size, limbs, N), True, scale, cf, capacity=3 if B % 2 and size == 2 else None)


def run(S, ins, pls, plain_scale=1.0, **strides):
    """multiplyPlainMatrix through the Python layer -> [C][B][size][limbs][N]; checks the metadata of every column"""
    R, B, size, limbs, N = ins.shape
    Cn = pls.shape[1]
    a = operand(S, ins)
    out = S.ev.multiplyPlainMatrix(a, api.DeviceBuffer.from_numpy(pls), R, Cn, plain_scale, **strides)
    assert len(out) == Cn
    for o in out:
        assert (o.size(), o.limbs, o.batch, o.is_ntt_form, o.scale, o.correction_factor) == (size, limbs, B, True, a.scale * plain_scale, a.correction_factor)
    return np.stack([o.cpu() for o in out])


# ---------------------------------------------------------------- check 2: the model
def check_model(S, limbs, rows, cols, batch, size=2, spot=False):
    """every limb equals the model and is canonical; one launch"""
    ins, pls = pool(S, limbs)
    ins, pls = np.ascontiguousarray(ins[:rows, :batch, :size]), np.ascontiguousarray(pls[:rows, :cols])
    exp = model(S.primes[:limbs], ins, pls)
    if spot:
        spot_check_model(S.primes[:limbs], ins, pls, exp)
    n0 = stat()
    got = run(S, ins, pls, 2.0 ** 10 if S.scheme == CKKS else 1.0)
    assert stat() - n0 == 1
    assert np.array_equal(got, exp), (S.name, limbs, "rows", rows, "cols", cols, "batch", batch, "size", size)
    assert canonical(S.primes[:limbs], got)


# ---------------------------------------------------------------- check 3: the composition of existing calls
def composition(S, a, plains, rows, cols, limbs, batch, plain_scale=1.0):
    """what a caller could do before: per column ceil(rows / 16) multiplyPlainAccumulate calls and the adds between them (existing code, not the code
    under test).  a: the operand of `operand`; plains: DeviceBuffer [rows][cols][limbs][N] -> [cols][batch][size][limbs][N]"""
    pw = limbs * S.N
    item = a.bstride
    cts = []
    for r in range(rows):
        ct = api.Ciphertext(S.ctx, batch, a.size(), limbs, True, a.scale, a.correction_factor, a.capacity, buf=api._BufferWindow(a.buf, r * batch * item, batch * item))
        cts.append(ct)
    out = []
    for c in range(cols):
        acc = None
        for r0 in range(0, rows, 16):
            rr = range(r0, min(r0 + 16, rows))
            part = S.ev.multiplyPlainAccumulate([cts[r] for r in rr], [api._BufferWindow(plains, (r * cols + c) * pw, pw) for r in rr], plain_scale)
            acc = part if acc is None else S.ev.add(acc, part)
        out.append(acc.cpu())
    return np.stack(out)


def check_anchor(S, limbs, rows, batch, cols=3):
    ins, pls = pool(S, limbs)
    ins, pls = np.ascontiguousarray(ins[:rows, :batch, :2]), np.ascontiguousarray(pls[:rows, :cols])
    scale = 2.0 ** 10 if S.scheme == CKKS else 1.0
    got = run(S, ins, pls, scale)
    exp = composition(S, operand(S, ins), api.DeviceBuffer.from_numpy(pls), rows, cols, limbs, batch, scale)
    assert np.array_equal(got, exp), (S.name, limbs, "rows", rows, "batch", batch)
    assert got.any()


# ---------------------------------------------------------------- check 4: the lazy sums at their bound
def check_lazy_bound(name="bgv_n128_k4", rows=130, batch=2, cols=5):
    """plaintexts of p - 1 throughout with ciphertexts of p - 1 throughout and with the delta pattern: every product is the largest there is, in runs
    of 63.  An accumulator that overflows cannot pass."""
    for ct_pattern in ("max", "delta"):
        S = HC.Setup(name, patterns=(ct_pattern, "uniform", "max"))
        limbs = S.ctx.first_limbs
        ins, pls = pool(S, limbs)
        assert rows > 2 * 63 and (pls == np.array(S.primes[:limbs], dtype=np.uint64)[:, None] - np.uint64(1)).all()
        check_model(S, limbs, rows, cols, batch)
        check_model(S, limbs, rows, 1, 1, size=3)


def check_lazy_bound_rows_4096(name="bfv_n64_k3"):
    """rows = 4096, the most the call takes: 66 runs, every operand p - 1"""
    S = HC.Setup(name, patterns=("max", "uniform", "max"))
    limbs, N = S.ctx.first_limbs, S.N
    q = S.primes[:limbs]
    ins = synth.edge_rows("max", 1, q, 4096 * 2 * limbs, N).reshape(4096, 1, 2, limbs, N)
    pls = synth.edge_rows("max", 2, q, 4096 * limbs, N).reshape(4096, 1, limbs, N)
    exp = model(q, ins, pls)
    assert all(int(exp[0, 0, 0, l, 0]) == 4096 % p for l, p in enumerate(q))  # (p - 1)^2 = 1 (mod p), 4096 times
    assert np.array_equal(run(S, ins, pls), exp)
    ins = np.ascontiguousarray(ins)
    ins[1::2] = 1  # every other row the unit: the sum is no multiple of one word
    exp = model(q, ins, pls)
    spot_check_model(q, ins, pls, exp, words=4)
    assert np.array_equal(run(S, ins, pls), exp)


WIDE_BITS = [60, 60, 60]           # the widest primes the library creates (bfv_n32768_l14 and linear_n4096 use 58 - 60 bits)
WIDE_ROWS = [300, 4096]


def check_lazy_bound_wide_primes(rows, N=64):
    """the run length at the primes where it binds.  With primes below 2^41 (every set above) the high words of the operands are below 2^9 and neither a
    MacAcc word nor the 128-bit total can overflow in 4096 products, so those sets do not show whether runs are closed at all.  At 60 bits the high
    words are just below 2^28 and their products just below 2^56: the 64-bit word that sums them wraps after 256 products of p - 1, and rows (p - 1)^2,
    just below rows * 2^120, passes 2^128 from 257 rows on.  rows = 300 and 4096 with every operand p - 1 (and with the delta and uniform patterns) equal
    the model only if a run is closed in time and the closed runs are combined exactly; both kernel instances (batch 1, batch 2), sizes 2 and 3."""
    for ct_pattern, pt_pattern in (("max", "max"), ("delta", "max"), ("uniform", "uniform")):
        S = HC.Setup(*HC.adhoc(BFV, N, WIDE_BITS), patterns=(ct_pattern, "uniform", pt_pattern))
        limbs = S.ctx.first_limbs
        q = S.primes[:limbs]
        assert all(p.bit_length() == 60 for p in q) and rows > 256
        ins = synth.edge_rows(ct_pattern, 11 + rows, q, rows * 2 * 3 * limbs, N).reshape(rows, 2, 3, limbs, N)
        pls = synth.edge_rows(pt_pattern, 12 + rows, q, rows * 2 * limbs, N).reshape(rows, 2, limbs, N)
        if ct_pattern == "max":
            assert rows * (q[0] - 1) ** 2 >= 1 << 128 and 257 * ((q[0] - 1) >> 32) ** 2 >= 1 << 64  # the total and one word, were no run closed
        for batch, size, cols in ((1, 2, 2), (2, 2, 1), (1, 3, 1)):
            a, b = np.ascontiguousarray(ins[:, :batch, :size]), np.ascontiguousarray(pls[:, :cols])
            exp = model(q, a, b)
            spot_check_model(q, a, b, exp, words=3)
            got = run(S, a, b)
            assert np.array_equal(got, exp), ("60-bit primes", ct_pattern, "rows", rows, "batch", batch, "size", size)
            assert canonical(q, got)


# ---------------------------------------------------------------- check 5: independence
def raw_call(S, in_st, in_rs, rows, pl_ptr, pl_rs, pl_cs, cols, out_ptr, out_bs, out_cs, batch=1, plain_scale=1.0, ctx=None, out_desc=True):
    """in_st None: a null operand descriptor; out_desc False: a null destination descriptor"""
    so = capi.CtStruct(out_ptr, out_bs, 0, 0, 0, 0.0, 0)
    rc = S.lib.troyhip_multiply_plain_matrix((ctx or S.ctx).h, C.byref(in_st) if in_st is not None else None, C.c_uint64(in_rs), rows, C.c_void_p(pl_ptr), C.c_uint64(pl_rs),
                                             C.c_uint64(pl_cs), cols, C.c_double(plain_scale), C.byref(so) if out_desc else None, C.c_uint64(out_cs), C.c_uint64(batch), None)
    return rc, S.lib.troyhip_last_error().decode() if rc else "", so


def check_independence(S, limbs, rows=7, batch=5, cols=5):
    """the same bytes for every item alone, every column alone, permuted rows, and other strides of all three arrays"""
    N = S.N
    ins, pls = pool(S, limbs)
    ins, pls = np.ascontiguousarray(ins[:rows, :batch, :2]), np.ascontiguousarray(pls[:rows, :cols])
    full = run(S, ins, pls)
    assert np.array_equal(full, model(S.primes[:limbs], ins, pls))
    for b in range(batch):
        assert np.array_equal(run(S, ins[:, b:b + 1], pls)[:, 0], full[:, b]), (S.name, limbs, "item alone", b)
    for c in range(cols):
        assert np.array_equal(run(S, ins, pls[:, c:c + 1])[0], full[c]), (S.name, limbs, "column alone", c)
    perm = [3, 0, 6, 1, 5, 2, 4]
    assert np.array_equal(run(S, ins[perm], pls[perm]), full), (S.name, limbs, "permuted rows")
    # the operand as a list of windows of a buffer shaped like expandCoefficients' result, with rows the call does not read between the ones it does
    pw, item = limbs * N, 2 * limbs * N
    wide = np.zeros((2 * rows, batch, 2, limbs, N), dtype=np.uint64)
    wide[::2] = ins
    wide[1::2] = 7
    buf = api.DeviceBuffer.from_numpy(wide)
    wins = [api.Ciphertext(S.ctx, batch, 2, limbs, True, buf=api._BufferWindow(buf, 2 * r * batch * item, batch * item)) for r in range(rows)]
    # plaintexts with padded row and column strides
    pad = np.full((rows, cols + 2, limbs + 1, N), 5, dtype=np.uint64)
    pad[:, :cols, :limbs] = pls
    pbuf = api.DeviceBuffer.from_numpy(pad)
    ocs = batch * item + 2 * N
    got = S.ev.multiplyPlainMatrix(wins, pbuf, rows, cols, plain_row_stride=(cols + 2) * (limbs + 1) * N, plain_col_stride=(limbs + 1) * N, out_col_stride=ocs)
    assert np.array_equal(np.stack([o.cpu() for o in got]), full), (S.name, limbs, "strides")
    assert got[1].buf.ptr - got[0].buf.ptr == 8 * ocs
    HC.with_raises(capi.InvalidArgument, "common stride", lambda: S.ev.multiplyPlainMatrix([wins[0], wins[1], wins[3]], pbuf, 3, 1))
    HC.with_raises(capi.InvalidArgument, "common stride", lambda: S.ev.multiplyPlainMatrix([wins[1], wins[0]], pbuf, 2, 1))
    # a padded destination through the C ABI: items with room for a third polynomial, columns with two rows between them; the padding keeps its bytes
    obs, ocs = 3 * pw, batch * 3 * pw + 2 * N
    out = api.DeviceBuffer.from_numpy(np.full(cols * ocs, 9, dtype=np.uint64))
    rc, msg, so = raw_call(S, wins[0].struct(), 2 * batch * item, rows, pbuf.ptr, (cols + 2) * (limbs + 1) * N, (limbs + 1) * N, cols, out.ptr, obs, ocs, batch)
    assert rc == capi.OK, msg
    o = out.to_numpy().reshape(cols, ocs)
    items = o[:, :batch * obs].reshape(cols, batch, 3, limbs, N)
    assert np.array_equal(items[:, :, :2], full) and (items[:, :, 2] == 9).all() and (o[:, batch * obs:] == 9).all()


def check_stride_loop(S, monkeypatch, rows=3, batch=3, cols=5):
    """probe builds only: a grid capped at seven workgroups walks the rest with a stride"""
    limbs = S.ctx.first_limbs
    ins, pls = pool(S, limbs)
    ins, pls = np.ascontiguousarray(ins[:rows, :batch, :2]), np.ascontiguousarray(pls[:rows, :cols])
    exp = model(S.primes[:limbs], ins, pls)
    g0 = stat("plainmat_workgroups")
    assert np.array_equal(run(S, ins, pls), exp)
    whole = stat("plainmat_workgroups") - g0
    assert whole > 7, whole  # the grid the call launches by itself: one workgroup per block of the order
    monkeypatch.setenv("TROYHIP_PLAINMAT_MAX_BLOCKS", "7")
    g0 = stat("plainmat_workgroups")
    assert np.array_equal(run(S, ins, pls), exp)
    assert stat("plainmat_workgroups") - g0 == 7  # the cap took effect: seven workgroups walked all `whole` blocks
    monkeypatch.setenv("TROYHIP_PLAINMAT_XCDS", "1")  # ... and in the order as it comes
    assert np.array_equal(run(S, ins, pls), exp)


# ---------------------------------------------------------------- check 6: the grid limit
def check_grid_limit(S, cols=65537):
    """more columns than a grid dimension other than x holds, one row: the columns at both ends and around 65535 equal the call on those columns alone and
    the model, at batch 1 and at batch 2 (batch * cols past 65535 as well)"""
    limbs, N = S.ctx.first_limbs, S.N
    q = S.primes[:limbs]
    rng = np.random.default_rng(cols)
    pls = np.stack([rng.integers(0, p, (1, cols, N), dtype=np.uint64) for p in q], axis=2)
    pbuf = api.DeviceBuffer.from_numpy(pls)
    pick = [0, 1, cols - 2, cols - 1]
    few = np.ascontiguousarray(pls[:, pick])
    for batch in (1, 2):
        ins = synth.uniform_ct(77 + batch, q, 2, N, batch)[None]
        a = operand(S, ins)
        big = S.ev.multiplyPlainMatrix(a, pbuf, 1, cols)
        alone = run(S, ins, few)
        exp = model(q, ins, few)
        for i, c in enumerate(pick):
            got = big[c].cpu()
            assert np.array_equal(got, alone[i]) and np.array_equal(got, exp[i]), ("column", c, "batch", batch)
        del big


# ---------------------------------------------------------------- check 7: refusals
def check_refusals(S):
    inv, logic = capi.INVALID_ARGUMENT, capi.LOGIC_ERROR
    limbs, N = S.ctx.first_limbs, S.N
    pw = limbs * N
    item = 2 * pw
    rows, cols, batch = 3, 2, 2
    ins, pls = pool(S, limbs)
    ins, pls = np.ascontiguousarray(ins[:rows, :batch, :2]), np.ascontiguousarray(pls[:rows, :cols])
    a = operand(S, ins)
    p = api.DeviceBuffer.from_numpy(np.concatenate([pls.reshape(-1), np.zeros(64, dtype=np.uint64)]))  # room behind both arrays: a stride or a pointer that is
    st = a.struct()                                                                                     # a little too large stays inside its own buffer
    words = cols * batch * item
    out = api.DeviceBuffer(words + 64)
    out.zero()
    good = dict(in_rs=batch * item, rows=rows, pl_ptr=p.ptr, pl_rs=cols * pw, pl_cs=pw, cols=cols, out_ptr=out.ptr, out_bs=item, out_cs=batch * item, batch=batch)

    def call(in_st=st, **kw):
        return raw_call(S, in_st, **dict(good, **kw))

    def refused(rc_msg, code, text=None):
        rc, msg = rc_msg[:2]
        assert rc == code and (text is None or text in msg), (rc, msg, text)
        assert not out.to_numpy().any()  # the destination is untouched

    coeff = a.struct()
    coeff.is_ntt_form = 0
    refused(call(coeff), inv, "encrypted_ntt is not in NTT form")
    refused(call(None), inv, "null ciphertext")
    refused(call(out_desc=False), inv, "null ciphertext")
    nul = a.struct()
    nul.data = None
    refused(call(nul), inv, "encrypted is not valid for encryption parameters")
    refused(call(pl_ptr=None), inv, "plain_ntt is not valid for encryption parameters")
    refused(call(out_ptr=None), inv, "destination batch stride too small for the result size")
    for size in (1, 4):
        bad = a.struct()
        bad.size = size
        bad.batch_stride = 4 * pw
        refused(call(bad), inv, "encrypted size must be 2 or 3")
    for lv in (0, S.ctx.first_limbs + 1, 70):
        bad = a.struct()
        bad.limbs = lv
        refused(call(bad), inv, "encrypted is not valid for encryption parameters")
    small = a.struct()
    small.batch_stride = item - 2
    refused(call(small), inv, "batch stride is smaller than one ciphertext")
    refused(call(in_rs=item - 2), inv, "row stride is smaller than one ciphertext")
    refused(call(pl_rs=pw - 2), inv, "plaintext stride is smaller than one plaintext")
    refused(call(pl_cs=pw - 2), inv, "plaintext stride is smaller than one plaintext")
    refused(call(out_bs=item - 2), inv, "destination batch stride too small for the result size")
    refused(call(out_cs=item - 2), inv, "column stride is smaller than one ciphertext")
    refused(call(out_cs=item), inv, "the results of the destination overlap")  # column 1 would lie on item 1 of column 0
    refused(call(out_cs=batch * item + 1), inv, "strides must be even")
    refused(call(pl_ptr=p.ptr + 8), inv, "16-byte aligned")
    refused(call(in_rs=1 << 41), inv, "stride out of range")
    refused(call(in_rs=(1 << 36) + 2), inv, "stride out of range")
    wide = a.struct()
    wide.batch_stride = 1 << 36  # accepted for two items, not for 2^27: batch * stride would pass 2^56 words
    refused(call(wide, batch=1 << 27), inv, "stride out of range")
    refused(call(out_bs=1 << 36, out_cs=1 << 36, batch=1 << 27), inv, "stride out of range")
    for r in (0, 4097, -1):
        refused(call(rows=r), inv, "multiply_plain_matrix takes 1 to 4096 rows")
    for c in (0, (1 << 20) + 1, -1):
        refused(call(cols=c), inv, "multiply_plain_matrix takes 1 to 2^20 columns")
    # a destination that shares words with the operand or the plaintexts
    big = api.DeviceBuffer(rows * batch * item + words)
    big.copy_from(a.buf, rows * batch * item)
    ali = capi.CtStruct(big.ptr, item, 2, limbs, 1, 1.0, 1)
    for off in (0, pw, rows * batch * item - 2):
        rc, msg, _ = call(ali, out_ptr=big.ptr + 8 * off)
        assert rc == inv and "destination must be a distinct buffer" in msg, (rc, msg)
    assert np.array_equal(big.to_numpy(rows * batch * item), a.buf.to_numpy(rows * batch * item))
    pbig = api.DeviceBuffer(rows * cols * pw + words)
    pbig.copy_from(p, rows * cols * pw)
    rc, msg, _ = call(pl_ptr=pbig.ptr, out_ptr=pbig.ptr + 8 * (rows * cols * pw - 2))
    assert rc == inv and "destination must be a distinct buffer" in msg, (rc, msg)
    assert np.array_equal(pbig.to_numpy(rows * cols * pw), pls.reshape(-1))
    # a host-only context; a context of another ring, for which these strides address less than an item
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    rc, msg, _ = call(ctx=host)
    assert rc == logic and "host-only" in msg, (rc, msg)
    refused((rc, ""), logic)
    other = HC.Setup(*HC.adhoc(S.scheme, 2 * N, [40] * S.K, tbits=14))
    refused(call(ctx=other.ctx), inv, "batch stride is smaller than one ciphertext")
    deep = HC.Setup(*HC.adhoc(S.scheme, N, [40, 40]))  # one data limb: the operand's level does not exist there
    if limbs > 1:
        refused(call(ctx=deep.ctx), inv, "encrypted is not valid for encryption parameters")
    if S.scheme == CKKS:
        refused(call(plain_scale=2.0 ** 400), inv, "scale out of bounds")
        refused(call(plain_scale=-1.0), inv, "scale out of bounds")
        HC.with_raises(capi.InvalidArgument, "scale out of bounds", lambda: S.ev.multiplyPlainMatrix(a, p, rows, cols, 2.0 ** 400))
    # an empty batch does nothing; a good call fills in the descriptor
    rc, msg, so = call(batch=0)
    assert rc == capi.OK and not out.to_numpy(words).any(), msg
    n0 = stat()
    rc, msg, so = call(plain_scale=4.0)
    assert rc == capi.OK and stat() - n0 == 1, msg
    assert (so.size, so.limbs, so.is_ntt_form, so.scale, so.correction_factor) == (2, limbs, 1, a.scale * 4.0, a.correction_factor)
    assert np.array_equal(out.to_numpy(words).reshape(cols, batch, 2, limbs, N), model(S.primes[:limbs], ins, pls))
    # the Python layer
    HC.with_raises(capi.InvalidArgument, "one operand per row", lambda: S.ev.multiplyPlainMatrix([a], p, 2, 1))
    HC.with_raises(capi.InvalidArgument, "rows of one batch", lambda: S.ev.multiplyPlainMatrix(a, p, 4, 1))
    HC.with_raises(capi.InvalidArgument, "smaller than rows x cols plaintexts", lambda: S.ev.multiplyPlainMatrix(a, p, rows, cols + 1))
    HC.with_raises(capi.InvalidArgument, "at least one column", lambda: S.ev.multiplyPlainMatrix(a, p, rows, 0))


# ---------------------------------------------------------------- check 8: real keys, the PIR round trip
def real_context(scheme, N, bits, tbits):
    primes = api.CoeffModulus.Create(N, list(bits))
    t = int(api.PlainModulus.Batching(N, tbits))
    return api.SEALContext(scheme, N, primes, t), t


def check_pir(scheme, N, bits, tbits, D0, d, clients=3):
    """fresh keys from the generators; records uniform mod t; recover(answer(query(i))) == record i for the first, the last and two indices in between;
    answerBatch of three clients; positive noise budgets, printed; the scan stage alone decrypts to row r*'s records"""
    ctx, t = real_context(scheme, N, bits, tbits)
    kg = api.KeyGenerator(ctx, seed=(71, 72))
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(21, 43))
    dec = api.Decryptor(ctx, kg.secretKey())
    client = app.PIRClient(ctx, kg, enc, dec, D0, d)
    count = D0 << d
    rng = np.random.default_rng(N + D0)
    records = rng.integers(0, t, (count, N), dtype=np.uint64)
    server = app.PIRServer(ctx, records, D0)
    gk = client.galoisKeys()
    picks = [0, count - 1, count // 3, (2 * count) // 3 + 1]
    budgets = []
    for i in picks:
        query, sels = client.query(i)
        ans = server.answer(query, sels, gk)
        assert ans.batch == 1 and ans.size() == 2 and not ans.is_ntt_form
        assert np.array_equal(client.recover(ans), records[i]), (scheme, N, "index", i)
        budgets.append(client.noiseBudget(ans))
        assert budgets[-1] > 0, (scheme, N, i, budgets)
    print("scheme", scheme, "N", N, "D0", D0, "d", d, "PIR answer noise budgets", budgets)
    # the scan stage alone: sum_r db[r][c] * delta(r, r*) = the records of row r*
    i = picks[2]
    r_star = i % D0
    query, _ = client.query(i)
    cols = server.scan(query, gk)
    assert len(cols) == 1 << d
    for j, c in enumerate(cols):
        assert np.array_equal(client.recover(c), records[r_star + D0 * j]), (scheme, N, "scan column", j)
    print("scheme", scheme, "N", N, "scan noise budget", client.noiseBudget(cols[0]), "fresh", client.noiseBudget(query))
    # three clients in one scan
    ids = picks[:clients]
    qs = [client.query(i) for i in ids]
    answers = server.answerBatch([q for q, _ in qs], [s for _, s in qs], gk)
    assert len(answers) == clients
    for i, ans in zip(ids, answers):
        assert np.array_equal(client.recover(ans), records[i]), (scheme, N, "batched index", i)
        b = client.noiseBudget(ans)
        assert b > 0, (scheme, N, i, b)
        budgets.append(b)
    print("scheme", scheme, "N", N, "answerBatch noise budgets", budgets[len(picks):])
    return budgets
