#!/usr/bin/env python3
"""The baby-step / giant-step linear transform with grouped keys (troyhip_galois_plain_sum_bsgs_grouped) at the bench shapes, one
JSON line per (shape, special primes, batch, split).  Real keys of both forms from the device generator, real encryptions brought to dl = K - alpha limbs
by the modulus switches.  Three forms of sum_r d_r * rot(x, r), r = 0 .. R - 1, R = n1 x n2, each ONE call through the Python layer on the same operand:

  grouped_bsgs_ms         (a) troyhip_galois_plain_sum_bsgs_grouped, baby steps 0 .. n1 - 1, giant steps 0, n1, .. (n2 - 1) n1, grouped keys
  per_prime_bsgs_ms       (b) troyhip_galois_plain_sum_bsgs with the per-prime keys, the same split and table
  grouped_hoisted_ms      (c) troyhip_galois_plain_sum_hoisted_grouped over all R elements (R - 1 grouped keys)

A sample is `--reps` back-to-back calls between two device events, divided by reps; after a warm-up of every form the three ALTERNATE `--rounds` times.
The figure is the median over the rounds, *_spread_ms is max - min over them.

  vs_per_prime, vs_hoisted                     (b) / (a) and (c) / (a)
  faster_than_per_prime, faster_than_hoisted   "yes" / "no": (a) is faster by more than the two spreads together
  *_key_bytes             the keys each form reads: n1 + n2 - 2 grouped, n1 + n2 - 2 per-prime, R - 1 grouped
  slabs                   slabs (a) ran in under the default scratch limit
  verified                the first and the last item of every form decrypt to the expected plaintext; CKKS: within slot_tolerance = 1e-3 sqrt(R / 16)
                          (max_slot_error: the largest slot error seen)
  kernels                 with --kernels: the library's per-launch events over ONE call of (a) and of (b), microseconds by kernel
  refused                 instead of the figures: the library's message where it does not accept alpha for the shape's primes

Usage: python tools/grouped_bsgs_bench.py [--shapes a,b] [--alphas 3] [--batches 1,8] [--splits 16x4,32x8] [--rounds 5] [--reps 3] [--kernels]
                                          [--out profiles/grouped_bsgs_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from encrypt_bench import Timer  # noqa: E402
from grouped_hoist_bench import alternate, kernel_split  # noqa: E402
from grouped_ks_bench import SHAPES  # noqa: E402
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import CKKS  # noqa: E402

FORMS = ("grouped_bsgs", "per_prime_bsgs", "grouped_hoisted")


def bench_shape(name, cfg, alphas, batches, splits, rounds, reps, kernels):
    lib = api.KernelProvider.lib()
    N, scheme = cfg["N"], cfg["scheme"]
    ckks = scheme == CKKS
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = int(api.PlainModulus.Batching(N, cfg["tbits"])) if cfg["tbits"] else 0
    ctx = api.SEALContext(scheme, N, primes, t)
    K = ctx.key_limbs
    kg = api.KeyGenerator(ctx, seed=(0x6B5, 18))
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(43, 44))
    dec = api.Decryptor(ctx, kg.secretKey())
    ev = api.Evaluator(ctx)
    coder = api.CKKSEncoder(ctx) if ckks else api.BatchEncoder(ctx)
    rmax = max(n1 * n2 for n1, n2 in splits)
    elt = lambda s: ctx.galois_elt_from_step(s) if s else 1
    split_steps = sorted({s for n1, n2 in splits for s in list(range(1, n1)) + [i * n1 for i in range(1, n2)]})
    gk0 = kg.createGaloisKeys([elt(s) for s in split_steps], device=True)  # the per-prime keys of the splits' steps only
    rng = np.random.default_rng(12)
    scale, pscale = 2.0 ** 40, 2.0 ** 20
    timer = Timer(lib)
    bsgs_p, bsgs_g, lt_g = (ev.rotateVectorPlainSumBsgs, ev.rotateVectorPlainSumBsgsGrouped, ev.rotateVectorPlainSumHoistedGrouped) if ckks else \
        (ev.rotateRowsPlainSumBsgs, ev.rotateRowsPlainSumBsgsGrouped, ev.rotateRowsPlainSumHoistedGrouped)
    diags = rng.uniform(-1, 1, (rmax, N // 2)) + 1j * rng.uniform(-1, 1, (rmax, N // 2)) if ckks else rng.integers(0, t, (rmax, N), dtype=np.uint64)

    def rolled(v, s):
        return np.roll(v, -s) if ckks else np.roll(v.reshape(2, -1), -s, axis=1).reshape(-1)

    def key_plain(d):  # a diagonal at the key level in NTT form
        return api.DeviceBuffer.from_numpy(coder.encode(d, pscale, limbs=K)) if ckks else ev.transformPlainToNtt(api.DeviceBuffer.from_numpy(coder.encode(d)), K)

    flat = [key_plain(d) for d in diags]  # (c): diagonal r against rot(x, r)
    # (a), (b): pt[i][j] = the encoding of rot(d_{i n1 + j}, -i n1)
    tables = {(n1, n2): [[key_plain(rolled(diags[i * n1 + j], -i * n1)) for j in range(n1)] for i in range(n2)] for n1, n2 in splits}
    out = []
    for alpha in alphas:
        try:
            digits, lmax, key_words = ctx.grouped_key_shape(alpha)
            gkg = kg.createGaloisKeys([elt(s) for s in range(1, rmax)], device=True, special_primes=alpha)  # every step: (c) reads them all
        except capi.TroyHipError as e:
            res = dict(shape=name, N=N, K=K, special_primes=alpha, refused=str(e.args[-1]))
            out.append(res)
            print(json.dumps(res), flush=True)
            continue
        for B in batches:
            if ckks:
                vals = rng.uniform(-1, 1, (B, N // 2)) + 1j * rng.uniform(-1, 1, (B, N // 2))
                a = api.Ciphertext.from_numpy(ctx, np.stack([enc.encrypt(coder.encode(v, scale)) for v in vals]), True, scale)
            else:
                vals = rng.integers(0, t, (B, N), dtype=np.uint64)
                a = api.Ciphertext.from_numpy(ctx, np.stack([enc.encrypt(coder.encode(v)) for v in vals]))
            a = ev.modSwitchTo(a, lmax) if a.limbs > lmax else a
            for n1, n2 in splits:
                R = n1 * n2
                table = tables[n1, n2]
                bsteps, gsteps = list(range(n1)), [i * n1 for i in range(n2)]
                ps = pscale if ckks else 1.0
                fns = {"grouped_bsgs": lambda: bsgs_g(a, bsteps, gsteps, table, gkg, ps),
                       "per_prime_bsgs": lambda: bsgs_p(a, bsteps, gsteps, table, gk0, ps),
                       "grouped_hoisted": lambda: lt_g(a, list(range(R)), flat[:R], gkg, ps)}
                s0 = capi.stat("grouped_bsgs_slabs", lib)
                got = {k: f() for k, f in fns.items()}
                slabs = capi.stat("grouped_bsgs_slabs", lib) - s0
                ok, worst = True, 0.0
                tol = 1e-3 * max(1.0, (R / 16) ** 0.5)  # grouped_hoist_bench.py's 1e-3 at R = 16; the errors of R independent terms add in quadrature
                for b in sorted({0, B - 1}):
                    if ckks:
                        want = sum(diags[r] * rolled(vals[b], r) for r in range(R))
                    else:
                        want = sum(diags[r] * rolled(vals[b], r) % np.uint64(t) for r in range(R)) % np.uint64(t)  # t < 2^20: nothing wraps in 64 bits
                    for k in FORMS:
                        h = got[k].cpu()[b]
                        if ckks:
                            e = float(np.abs(coder.decode(dec.decrypt(h), scale * pscale) - want).max())
                            worst, ok = max(worst, e), ok and e < tol
                        else:
                            ok = bool(np.array_equal(coder.decode(dec.decrypt(h, correction_factor=got[k].correction_factor)), want)) and ok
                del got
                ms = alternate(timer, fns, rounds, reps)
                (ta, sa), (tb, sb), (tc, sc) = (ms[k] for k in FORMS)
                res = dict(shape=name, N=N, K=K, special_primes=alpha, batch=B, R=R, n1=n1, n2=n2, limbs=lmax, digits=-(-lmax // alpha), per_prime_digits=lmax)
                for k in FORMS:
                    res[k + "_ms"], res[k + "_spread_ms"] = round(ms[k][0], 4), round(ms[k][1], 4)
                res.update(vs_per_prime=round(tb / ta, 3), vs_hoisted=round(tc / ta, 3), faster_than_per_prime="yes" if tb - ta > sa + sb else "no",
                           faster_than_hoisted="yes" if tc - ta > sa + sc else "no", slabs=slabs, grouped_bsgs_key_bytes=(n1 + n2 - 2) * key_words * 8,
                           per_prime_bsgs_key_bytes=(n1 + n2 - 2) * (K - 1) * 2 * K * N * 8, grouped_hoisted_key_bytes=(R - 1) * key_words * 8, verified=ok,
                           **({"max_slot_error": worst, "slot_tolerance": tol} if ckks else {}), rounds=rounds, reps=reps, build_id=capi.build_id(lib))
                if kernels:
                    res["kernels"] = {k: kernel_split(lib, fns[k]) for k in FORMS[:2]}
                out.append(res)
                print(json.dumps(res), flush=True)
            del a
        del gkg
    capi.check(lib, lib.troyhip_timer_destroy(timer.h))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bfv_n32768_l14,ckks_n32768_chain,bgv_n65536_relin_rot")
    ap.add_argument("--alphas", default="3")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--splits", default="16x4,32x8")  # R = 64 and R = 256 at the best splits of DESIGN.md section 4.12
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)  # 5 - 500 ms per call
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (a second run with other --alphas)")
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",") if v]
    splits = [tuple(int(v) for v in s.split("x")) for s in a.splits.split(",") if s]
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    if a.out and a.append and os.path.exists(a.out):
        with open(a.out) as f:
            lines = [json.loads(l) for l in f if l.strip()]
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], ints(a.alphas), ints(a.batches), splits, a.rounds, a.reps, a.kernels)
        lines += r
        ok = ok and all(v.get("verified", True) for v in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for v in lines:
                    f.write(json.dumps(v) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
