#!/usr/bin/env python3
"""Key switching with grouped digits (troyhip_relinearize_grouped / troyhip_apply_galois_grouped) against the per-prime calls on an
operand at the same level, one JSON line per (shape, call, batch, special primes).  Real keys of both forms from the device generator, real encryptions
brought to dl = K - alpha limbs by the modulus switches.  One process, both forms through the Python layer on the same operand; a sample is the wall-clock
of `--reps` back-to-back calls between two stream synchronisations, divided by reps; after a warm-up of both forms the two ALTERNATE `--rounds` times:

  grouped_ms, per_prime_ms    the median over the rounds; *_spread_ms: max - min over the rounds
  speedup                     per_prime_ms / grouped_ms
  faster                      "yes" / "no": grouped is faster than per-prime by more than the two spreads together
  grouped_key_bytes, per_prime_key_bytes    one key of each form
  verified                    BFV / BGV: both results decrypt to the same plaintext, which is the expected one; CKKS: both within 1e-3 of it (max_slot_error:
                              the larger of the two largest slot errors)
  refused                     instead of the figures: the library's message where it does not accept alpha for the shape's primes

Usage: python tools/grouped_ks_bench.py [--shapes a,b] [--batches 1,8] [--alphas 2,3,4] [--rounds 5] [--reps 1000] [--out profiles/grouped_ks_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import BFV, BGV, CKKS  # noqa: E402

SHAPES = {  # bench.py's workload parameters
    "bfv_n32768_l14": dict(scheme=BFV, N=32768, bits=[60] + [58] * 13 + [60], tbits=20),
    "ckks_n32768_chain": dict(scheme=CKKS, N=32768, bits=[60] + [40] * 13 + [60], tbits=0),
    "bgv_n65536_relin_rot": dict(scheme=BGV, N=65536, bits=[60] + [50] * 13 + [60], tbits=20),
    "bfv_n4096_k7": dict(scheme=BFV, N=4096, bits=[58] * 5 + [60, 60], tbits=20),  # a quick shape for trying the tool
}


def wall(lib, fn, reps):
    capi.check(lib, lib.troyhip_stream_synchronize(None))
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    capi.check(lib, lib.troyhip_stream_synchronize(None))
    return (time.perf_counter() - t0) * 1e3 / reps, r


def bench_shape(name, cfg, batches, alphas, rounds, reps):
    lib = api.KernelProvider.lib()
    N, scheme = cfg["N"], cfg["scheme"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = int(api.PlainModulus.Batching(N, cfg["tbits"])) if cfg["tbits"] else 0
    ctx = api.SEALContext(scheme, N, primes, t)
    K = ctx.key_limbs
    kg = api.KeyGenerator(ctx, seed=(0x6B5, 16))
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(41, 42))
    dec = api.Decryptor(ctx, kg.secretKey())
    ev = api.Evaluator(ctx)
    elt = ctx.galois_elt_from_step(1)
    rk0, gk0 = kg.createRelinKeys(device=True), kg.createGaloisKeys([elt], device=True)
    rng = np.random.default_rng(11)
    scale = 2.0 ** 40
    if scheme == CKKS:
        coder = api.CKKSEncoder(ctx)
    else:
        coder = api.BatchEncoder(ctx)
    out = []
    for alpha in alphas:
        try:
            digits, lmax, key_words = ctx.grouped_key_shape(alpha)
            rkg, gkg = kg.createRelinKeys(device=True, special_primes=alpha), kg.createGaloisKeys([elt], device=True, special_primes=alpha)
        except capi.TroyHipError as e:
            res = dict(shape=name, N=N, K=K, special_primes=alpha, refused=str(e.args[-1]))
            out.append(res)
            print(json.dumps(res), flush=True)
            continue
        for B in batches:
            if scheme == CKKS:
                vals = rng.uniform(-1, 1, (B, N // 2)) + 1j * rng.uniform(-1, 1, (B, N // 2))
                a = api.Ciphertext.from_numpy(ctx, np.stack([enc.encrypt(coder.encode(v, scale)) for v in vals]), True, scale)
            else:
                vals = rng.integers(0, t, (B, N), dtype=np.uint64)
                a = api.Ciphertext.from_numpy(ctx, np.stack([enc.encrypt(coder.encode(v)) for v in vals]))
            a = ev.modSwitchTo(a, lmax) if a.limbs > lmax else a
            prod = ev.multiply(a, a)
            calls = {"relinearize": (lambda: ev.relinearize(prod, rkg), lambda: ev.relinearize(prod, rk0)),
                     "applyGalois": (lambda: ev.applyGalois(a, elt, gkg), lambda: ev.applyGalois(a, elt, gk0))}
            for call, (grouped, per_prime) in calls.items():
                _, rg = wall(lib, grouped, 1)  # the warm-up of both forms gives the results that are verified
                _, rp = wall(lib, per_prime, 1)
                tg, tp = [], []
                for _ in range(rounds):
                    tg.append(wall(lib, grouped, reps)[0])
                    tp.append(wall(lib, per_prime, reps)[0])
                hg, hp = rg.cpu(), rp.cpu()
                ok, worst = True, 0.0
                for b in range(B):
                    if scheme == CKKS:
                        sc = rg.scale
                        want = vals[b] * vals[b] if call == "relinearize" else np.roll(vals[b], -1)
                        eg = np.abs(coder.decode(dec.decrypt(hg[b]), sc) - want).max()
                        ep = np.abs(coder.decode(dec.decrypt(hp[b]), sc) - want).max()
                        ok, worst = ok and eg < 1e-3 and ep < 1e-3, max(worst, float(eg), float(ep))
                    else:
                        mg = coder.decode(dec.decrypt(hg[b], correction_factor=rg.correction_factor))
                        mp = coder.decode(dec.decrypt(hp[b], correction_factor=rp.correction_factor))
                        want = vals[b] * vals[b] % np.uint64(t) if call == "relinearize" else np.roll(vals[b].reshape(2, -1), -1, axis=1).reshape(-1)
                        ok = ok and np.array_equal(mg, mp) and np.array_equal(mg, want)
                mg_, mp_ = float(np.median(tg)), float(np.median(tp))
                sg, sp = max(tg) - min(tg), max(tp) - min(tp)
                res = dict(shape=name, N=N, K=K, call=call, batch=B, special_primes=alpha, limbs=lmax, digits=-(-lmax // alpha), per_prime_digits=lmax,
                           grouped_ms=round(mg_, 4), grouped_spread_ms=round(sg, 4), per_prime_ms=round(mp_, 4), per_prime_spread_ms=round(sp, 4),
                           speedup=round(mp_ / mg_, 3), faster="yes" if mp_ - mg_ > sg + sp else "no", grouped_key_bytes=key_words * 8,
                           per_prime_key_bytes=(K - 1) * 2 * K * N * 8, verified=bool(ok), **({"max_slot_error": worst} if scheme == CKKS else {}), rounds=rounds, reps=reps, build_id=capi.build_id(lib))
                out.append(res)
                print(json.dumps(res), flush=True)
                del rg, rp
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bfv_n32768_l14,ckks_n32768_chain,bgv_n65536_relin_rot")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--alphas", default="2,3,4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1000)  # 0.1 - 1 ms per call: a sample is a window of 0.1 - 1 s
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], [int(v) for v in a.batches.split(",")], [int(v) for v in a.alphas.split(",")], a.rounds, a.reps)
        lines += r
        ok = ok and all(v.get("verified", True) for v in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for v in lines:
                    f.write(json.dumps(v) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
