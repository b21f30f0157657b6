"""The large-base matrix-core BEHZ kernels (behz2_extend_kernel / behz2_floor_sk_kernel) at every limb count that changes their shape, shared by
tests/test_device_behz_rows.py (emulator build) and tests/test_gpu_behz_rows.py (MI355X).

The extension sums the m~ residue in 32-bit arithmetic, one partial per wave through LDS, and the floor evaluates the m_sk row in one wave per
sub-tile and hands the digits of alpha to the others through LDS as limb nB of the stage-2 operand.  What can go wrong there depends on where the
limbs fall: which wave owns a limb (l mod 4), how many k-blocks the operands have, and where the extra input (r at limb L, alpha at limb nB) sits in
the last k-block.  L in {9, 12, 13, 14, 15} covers both k-block counts of the large-base kernels (3 and 4), every L mod 4, and the extra input in
each position of the last k-block.

The widths are the headline's, [60] + [58] * (L - 1) + [60]: with them the library's auxiliary base has t q / B >= 1 at every L (asserted), so a negative
Shenoy-Kumaresan quotient is reachable, as it is in production, and its sign-extended digits take the route through LDS.

BFV, N = 4096 (the smallest size the fused tensor pass takes), ONE call of batch 3 against constant second operands (behz_cases: the product is then
coefficient-wise and every coefficient carries its own case):
  item 0   uniform residues, with built coefficients at seeded positions: r = -sum q^-1 mod 2^32 at 0, 2^31 - 1, 2^31 and 2^32 - 1 (both sides of the
           centring), alpha at 0, +1 and "top", u_o and out_l at 0 and p - 1.  "top" is the largest quotient the builder's 64 candidates per prime
           reach (behz_cases.build_floor_multiples), NOT the base's bound |B|: that needs a floored value near -B |B|
  item 1   polynomial 0 all-zero residues, polynomial 1 every residue at p_l - 1
  item 2   uniform residues against a constant near q / 2 (behz_cases.wide_constant), with built coefficients whose quotient is exactly -1, -2 and -3:
           the floored value V = k B + d has alpha = floor(S(d) / B) - k, S(d) the conversion's sum of the residue d, so candidates around k B for
           every k up to |B| + 1 are run through the model and the first that shows each value is kept
Every item is compared byte for byte with the oracle's multiply and with behz_cases.Model, whose intermediates show on the CPU that each built
coefficient, after placement, meets the boundary it was built for; a boundary nobody meets fails the case, and nothing is named unreachable."""
import math

import numpy as np

import behz_cases as BC
import round_cases as RC
from troy_amd import synth
from troy_amd.capi import BFV

LIMBS = (9, 12, 13, 14, 15)
MT = BC.MT


def bits_for(L):
    return [60] + [58] * (L - 1) + [60]  # L data limbs and the special prime: the headline's widths


NEGATIVE = (-1, -2, -3)


def build_negative(M, seed):
    """coefficients of item 2 whose Shenoy-Kumaresan quotient is exactly -1, -2, -3, against the constant near q / 2"""
    assert M.tq_over_B >= 4 * (M.nB + 2), ("t q / B = 2^%.1f: the floored values k B, k <= |B| + 1, are out of reach" % math.log2(M.tq_over_B))
    Bn = BC.Built(M, BC.wide_constant(M, seed), seed)
    cand = []
    for k in range(1, M.nB + 2):
        centre = ((2 * k * M.PB + M.L) * M.Q) // (2 * M.t * Bn.c)
        cand += [(centre + d) % M.Q for d in range(-4, 4)] + [(-centre + d) % M.Q for d in range(-4, 4)]
    BC.pick(Bn, [("alpha=%d" % v, None, v) for v in NEGATIVE], cand, "alpha")
    return Bn


def build(cache, L, N, seed):
    S = RC.setup_in(cache, BFV, N, tuple(bits_for(L)), 20)
    M = BC.Model(S, S.K - 1)
    assert M.L == L and BC.variant_of(M) == dict(ext_small=False, floor_small=False, f2_fast=True), (L, BC.variant_of(M))
    assert ((M.L + 1 + 3) // 4, (M.nB + 1 + 3) // 4) in ((3, 3), (4, 4)), (M.L, M.nB)  # the k-block counts of the instances
    key = ("rows", L, N, seed)
    if key not in cache:
        Bd = BC.Built(M, BC.constant_for(M, seed), seed)
        BC.build_centred_r(Bd)
        BC.build_floor_multiples(Bd)
        a0, where = BC.place(Bd, N, seed + 1, items=1)
        a1 = np.zeros_like(a0)
        a1[0, 1] = BC.u64([p - 1 for p in M.q])[:, None]
        Bn = build_negative(M, seed + 2)
        a2, where2 = BC.place(Bn, N, seed + 3, items=1)
        cs = [Bd.c, Bd.c, Bn.c]
        a = np.concatenate([a0, a1, a2])
        b = np.concatenate([BC.constant_ct(M, c, N, 1) for c in cs])
        exp, I = BC.model_items(M, a, cs)
        for i in range(3):
            ref = BC.oracle_multiply(S, a[i], b[i])
            assert np.array_equal(ref, exp[i]), (L, "the model against the oracle, item", i, np.argwhere(ref != exp[i])[:4])
        for arr in (a, b, exp):
            arr.setflags(write=False)
        cache[key] = (Bd, Bn, a, b, exp, I)
    return (S, M) + cache[key]


def hits(M, Bd, Bn, I, N):
    """the boundaries of the module docstring, looked up in the model's intermediates of the placed input (flat index (item, polynomial, n))"""
    H = RC.Hits()
    for name in Bd.dropped + Bn.dropped:
        H.look(name, False)
    for name, r in (("r=0", 0), ("r=2^31-1", (MT >> 1) - 1), ("r=2^31", MT >> 1), ("r=2^32-1", MT - 1)):
        H.look(name, I["r"] == r)
    for name, v in (("alpha=0", 0), ("alpha=1", 1), ("alpha=top", Bd.alpha_top)) + tuple(("alpha=%d" % v, v) for v in NEGATIVE):
        H.look(name, I["alpha"] == v)
    zero_poly = slice(2 * N, 3 * N)  # item 1, polynomial 0
    top_poly = slice(3 * N, 4 * N)   # item 1, polynomial 1
    H.look("x=0", np.all(I["y"][:, zero_poly] == 0))
    H.look("x=p-1", np.all(I["y"][:, top_poly] == np.array([(p - 1) * M.ext_pre[l] % p for l, p in enumerate(M.q)], dtype=object)[:, None]))
    for l, p in enumerate(M.q):
        H.look("out%d=0" % l, I["out"][l] == 0)
        H.look("out%d=p-1" % l, I["out"][l] == p - 1)
    for o, p in enumerate(M.bsk):
        H.look("u%d=0" % o, I["u"][o] == 0)
        H.look("u%d=p-1" % o, I["u"][o] == p - 1)
    return H


def check(cache, L, N=4096, seed=5000):
    """-> the record of the case"""
    S, M, Bd, Bn, a, b, exp, I = build(cache, L, N, seed)
    kernels = RC.Kernels(S)
    with kernels:
        got = BC.run_family(S, "mfma", lambda: S.ev.multiply(S.ct(a), S.ct(b)).cpu())
    assert got.shape == (3, 3, L, N)
    for j in range(L):
        high = np.argwhere(got[:, :, j] >= np.uint64(S.primes[j]))
        assert not len(high), (L, "words not below their prime, limb", j, "at (item, polynomial, n)", high[:4])
    for i in range(3):
        assert got[i].tobytes() == exp[i].tobytes(), (L, "item", i, np.argwhere(got[i] != exp[i])[:4])
    if kernels.on:  # the names the launches carry (the emulator build records none)
        kb, kb2 = (M.L + 1 + 3) // 4, (M.nB + 1 + 3) // 4
        assert RC.calls_of(kernels.calls, "behz2_extend_kernel<%d>" % kb) > 0 and RC.calls_of(kernels.calls, "behz2s_") == 0, kernels.calls
        assert RC.calls_of(kernels.calls, "behz2_floor_sk_kernel<%d, %d, true>" % ((M.L + 3) // 4, kb2)) > 0, kernels.calls
    H = hits(M, Bd, Bn, I, N)
    count = H.check(cannot=(), what="L = %d" % L)
    rec = dict(L=L, nB=M.nB, N=N, xl_ext=L % 4, xl_floor=M.nB % 4, log2_tq_over_B=round(math.log2(M.tq_over_B), 1), alpha_min=int(I["alpha"].min()), alpha_top=Bd.alpha_top,
               built=len(Bd.cols) + len(Bn.cols), boundaries=count)
    print("behz rows", rec)
    return rec
