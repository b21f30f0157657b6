#!/usr/bin/env python3
"""Blind rotation in one call (troyhip_blind_rotate) against what a caller could compose before it, one JSON line per
(shape, batch, n).  Real keys: a random ternary LWE secret of n digits, its BlindRotationKey from the device generator (T = 2), samples built in integers
modulo 2N for a chosen phase, a random table scaled as BFV scales a plaintext.  One process, both forms on the same inputs, wall-clock around the call
and a stream synchronisation, after a warm-up, ALTERNATING the forms `--rounds` times:

  fused_ms      (a)  Evaluator.blindRotate: per step one pre-kernel, one digit expansion, one inner product, one second half; the shifts are read
                     from device memory
  composed_ms   (b)  the same chain through the Python layer: per step negacyclicShift and sub per term and one externalProductSum(base=acc).  ALL ITEMS
                     ARE GIVEN THE SAME SHIFTS so that (b) can run as ONE batch -- negacyclicShift takes one shift per call -- which is the form most
                     favourable to (b); with shifts of their own the items of (b) would run one by one.  The limbs of (a) and (b) are equal
                (each: the median over the rounds; *_spread_ms: max - min over the rounds)
  speedup       composed_ms / fused_ms
  faster        "yes" / "no": (a) is faster than (b) by more than the two spreads together
  slabs, steps  the counter deltas of one fused call (blindrot_slabs, blindrot_steps)
  budget        the smallest invariant noise budget over the items, in bits
  verified      (a) and (b) hold the same limbs and decrypt to table x^phase, for every item

A shape the context refuses is reported as a line with "skipped".
Usage: python tools/blindrot_bench.py [--shapes a,b] [--batches 1,8,64] [--dims 64,512] [--rounds N] [--out profiles/blindrot_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import BFV  # noqa: E402
from lwe_pack_bench import SHAPES as _SHAPES, wall  # noqa: E402

SHAPES = dict(_SHAPES, bfv_n2048_l2=dict(scheme=BFV, N=2048, bits=[36, 36, 40], tbits=16))
COUNTERS = ("blindrot_slabs", "blindrot_steps")


def composed(ev, ctx, tv, row, n, rgsws, batch, limbs):
    """(b): the chain through the Python layer on a batch whose items share their shifts -> Ciphertext"""
    N = ctx.N
    data = np.zeros((batch, 2, limbs, N), dtype=np.uint64)
    data[:, 0] = tv
    acc = ev.negacyclicShift(api.Ciphertext.from_numpy(ctx, data), int(row[n]))
    for i in range(n):
        a = int(row[i])
        ops = [ev.sub(ev.negacyclicShift(acc, u), acc) for u in (a, (2 * N - a) % (2 * N))]
        acc = ev.externalProductSum(ops, rgsws[i], base=acc)
    return acc


def bench_shape(name, cfg, batches, dims, rounds, lib=None):
    lib = lib or api.KernelProvider.lib()
    N, scheme = cfg["N"], cfg["scheme"]
    try:
        primes = api.CoeffModulus.Create(N, cfg["bits"])
        t = int(cfg.get("t") or api.PlainModulus.Batching(N, cfg["tbits"]))
        ctx = api.SEALContext(scheme, N, primes, t)
    except capi.TroyHipError as e:
        res = dict(shape=name, N=N, skipped="the context refuses these parameters: %s" % e)
        print(json.dumps(res), flush=True)
        return [res]
    limbs, K = ctx.first_limbs, ctx.key_limbs
    kg = api.KeyGenerator(ctx, seed=(0xB11D, 7))
    sk_dev = api.DeviceBuffer.from_numpy(kg.secretKey())
    ev = api.Evaluator(ctx)
    rng = np.random.default_rng(12)
    f = rng.integers(0, t, N, dtype=np.uint64)
    q = 1
    for p in primes[:limbs]:
        q *= int(p)
    vals = [(q * int(v) + t // 2) // t for v in f]
    tv = np.array([[v % int(p) for v in vals] for p in primes[:limbs]], dtype=np.uint64)
    gw = 2 * (K - 1) * 2 * K * N
    out = []
    for n in dims:
        secret = rng.integers(-1, 2, n)
        key = kg.createBlindRotationKey(secret, ternary=True)
        rgsws = [[api.RGSWCiphertext(ctx, api._BufferWindow(key.buf, (i * 2 + tt) * gw, gw)) for tt in range(2)] for i in range(n)]
        phi = int(rng.integers(0, 2 * N))
        row = rng.integers(0, 2 * N, n + 1, dtype=np.uint64)
        row[n] = (phi - sum(int(a) * int(s) for a, s in zip(row[:n], secret))) % (2 * N)
        mono = np.zeros(N, dtype=np.int64)
        mono[phi % N] = -1 if phi >= N else 1
        full = np.zeros(2 * N, dtype=object)
        for i in np.flatnonzero(mono):
            full[i:i + N] += int(mono[i]) * f.astype(object)
        expect = ((full[:N] - full[N:]) % t).astype(np.uint64)
        for B in batches:
            lwe = api.DeviceBuffer.from_numpy(np.tile(row, (B, 1)))
            tvd = api.DeviceBuffer.from_numpy(tv)
            forms = (lambda: ev.blindRotate(lwe, key, tvd, limbs=limbs), lambda: composed(ev, ctx, tv, row, n, rgsws, B, limbs))
            c0 = [capi.stat(c, lib) for c in COUNTERS]
            _, ra = wall(lib, forms[0])  # the warm-up of both forms gives the results that are verified
            deltas = [capi.stat(c, lib) - v for c, v in zip(COUNTERS, c0)]
            _, rb = wall(lib, forms[1])
            times = ([], [])
            for _ in range(rounds):
                for fn, ts in zip(forms, times):
                    ts.append(wall(lib, fn)[0])
            same = np.array_equal(ra.cpu(), rb.cpu())
            ok_a = all(np.array_equal(m, expect) for m in ev.decrypt(ra, sk_dev))
            ok_b = all(np.array_equal(m, expect) for m in ev.decrypt(rb, sk_dev))
            budget = int(ev.invariantNoiseBudget(ra, sk_dev).min())
            med = [float(np.median(ts)) for ts in times]
            spr = [max(ts) - min(ts) for ts in times]
            res = dict(shape=name, N=N, limbs=limbs, batch=B, n=n, T=2, fused_ms=round(med[0], 3), fused_spread_ms=round(spr[0], 3), composed_ms=round(med[1], 3),
                       composed_spread_ms=round(spr[1], 3), speedup=round(med[1] / med[0], 2), faster="yes" if med[1] - med[0] > spr[0] + spr[1] else "no",
                       slabs=deltas[0], steps=deltas[1], budget=budget, same_limbs=bool(same), verified_a=bool(ok_a), verified_b=bool(ok_b),
                       verified=bool(same and ok_a and ok_b and budget > 0), rounds=rounds, build_id=capi.build_id(lib))
            out.append(res)
            print(json.dumps(res), flush=True)
            del ra, rb
        del rgsws, key
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="linear_n4096,bfv_n8192_l4,bfv_n2048_l2")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--dims", default="64,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], [int(v) for v in a.batches.split(",")], [int(v) for v in a.dims.split(",")], a.rounds)
        lines += r
        ok = ok and all(v.get("verified", True) for v in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for v in lines:
                    f.write(json.dumps(v) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
