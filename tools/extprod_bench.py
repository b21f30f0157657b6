#!/usr/bin/env python3
"""The external product sum in one call (troyhip_external_product_sum) against what a caller could compose before it, one JSON
line per (shape, batch, terms).  Real keys, real RGSW ciphertexts from the device generator (createRGSWBatch: the selector bits of a fold, RGSW r
encrypting delta_{r, r*}), real encryptions of random polynomials: R batches of B ciphertexts are folded into one batch.  One process, both forms on the
same inputs, wall-clock around the call and a stream synchronisation, after a warm-up, ALTERNATING the forms `--rounds` times:

  fused_ms      (a)  Evaluator.externalProductSum: the digits of c0 and c1 of every term are written and read back (2 rl dl N words per term and item),
                     one inner product over all 2 R dl digits, ONE second half
  composed_ms   (b)  2 R troyhip_switch_key calls accumulating onto one zeroed ciphertext, target c_h of term r, key half h of RGSW r: the fused front
                     half, which never writes its digits, and 2 R second halves.  Existing code; its limbs are NOT those of (a) (2 R roundings)
                (each: the median over the rounds; *_spread_ms: max - min over the rounds)
  speedup       composed_ms / fused_ms
  faster        "yes" / "no": (a) is faster than (b) by more than the two spreads together
  slabs, chunks the counter deltas of one fused call (extprod_slabs, extprod_chunks)
  budget_a, budget_b   the smallest invariant noise budget over the items, in bits
  verified      (a) and (b) both decrypt to the selected message, for every item

Usage: python tools/extprod_bench.py [--shapes a,b] [--batches 1,8] [--terms 1,4,16] [--rounds N] [--out profiles/extprod_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from troy_amd import api, capi  # noqa: E402
from lwe_pack_bench import SHAPES, wall  # noqa: E402

COUNTERS = ("extprod_slabs", "extprod_chunks")


def composed(ctx, lib, cts, rgsws):
    """(b): 2 R key switches onto one zeroed ciphertext -> Ciphertext"""
    a0 = cts[0]
    K, N, pw = ctx.key_limbs, ctx.N, a0.limbs * ctx.N
    out = api.Ciphertext(ctx, a0.batch, 2, a0.limbs, a0.is_ntt_form, a0.scale, a0.correction_factor)
    out.buf.zero()
    st = out.struct()
    half = (K - 1) * 2 * K * N
    for a, g in zip(cts, rgsws):
        for h in range(2):
            capi.check(lib, lib.troyhip_switch_key(ctx.h, C.byref(st), C.c_void_p(a.buf.ptr + 8 * h * pw), C.c_uint64(a.bstride), C.c_void_p(g.buf.ptr + 8 * h * half),
                                                   C.c_uint64(a.batch), None))
    return out


def bench_shape(name, cfg, batches, terms, rounds, lib=None):
    lib = lib or api.KernelProvider.lib()
    N, scheme = cfg["N"], cfg["scheme"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = cfg.get("t") or api.PlainModulus.Batching(N, cfg["tbits"])
    ctx = api.SEALContext(scheme, N, primes, t)
    limbs = ctx.first_limbs
    kg = api.KeyGenerator(ctx, seed=(0x6E5, 7))
    sk_dev = api.DeviceBuffer.from_numpy(kg.secretKey())
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(25, 26))
    ev = api.Evaluator(ctx)
    rng = np.random.default_rng(10)
    Rmax, Bmax = max(terms), max(batches)
    star = Rmax // 3  # the selected term where it exists, else the last one
    msgs = rng.integers(0, t, (Rmax, Bmax, N), dtype=np.uint64)
    host = [np.stack([enc.encrypt(msgs[r, b]) for b in range(Bmax)]) for r in range(Rmax)]
    one, zero = np.ones(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    out = []
    for R in terms:
        sel = min(star, R - 1)
        G = kg.createRGSWBatch([one if r == sel else zero for r in range(R)])
        for B in batches:
            cts = [api.Ciphertext.from_numpy(ctx, host[r][:B]) for r in range(R)]
            forms = (lambda: ev.externalProductSum(cts, G), lambda: composed(ctx, lib, cts, G))
            c0 = [capi.stat(n, lib) for n in COUNTERS]
            _, ra = wall(lib, forms[0])  # the warm-up of both forms gives the results that are verified
            deltas = [capi.stat(n, lib) - v for n, v in zip(COUNTERS, c0)]
            _, rb = wall(lib, forms[1])
            times = ([], [])
            for _ in range(rounds):
                for f, ts in zip(forms, times):
                    ts.append(wall(lib, f)[0])
            ok_a = np.array_equal(ev.decrypt(ra, sk_dev), msgs[sel, :B])
            ok_b = np.array_equal(ev.decrypt(rb, sk_dev), msgs[sel, :B])
            ba, bb = int(ev.invariantNoiseBudget(ra, sk_dev).min()), int(ev.invariantNoiseBudget(rb, sk_dev).min())
            med = [float(np.median(ts)) for ts in times]
            spr = [max(ts) - min(ts) for ts in times]
            res = dict(shape=name, N=N, limbs=limbs, batch=B, terms=R, fused_ms=round(med[0], 3), fused_spread_ms=round(spr[0], 3), composed_ms=round(med[1], 3),
                       composed_spread_ms=round(spr[1], 3), speedup=round(med[1] / med[0], 2), faster="yes" if med[1] - med[0] > spr[0] + spr[1] else "no",
                       slabs=deltas[0], chunks=deltas[1], budget_a=ba, budget_b=bb, verified_a=bool(ok_a), verified_b=bool(ok_b),
                       verified=bool(ok_a and ok_b and ba > 0), rounds=rounds, build_id=capi.build_id(lib))
            out.append(res)
            print(json.dumps(res), flush=True)
            del ra, rb, cts
        del G
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="linear_n4096,linear_n8192,bfv_n8192_l4,bfv_n32768_l14")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--terms", default="1,4,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], [int(v) for v in a.batches.split(",")], [int(v) for v in a.terms.split(",")], a.rounds)
        lines += r
        ok = ok and all(v["verified"] for v in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for v in lines:
                    f.write(json.dumps(v) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
