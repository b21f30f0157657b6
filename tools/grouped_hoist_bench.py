#!/usr/bin/env python3
"""The hoisted calls with grouped keys (troyhip_apply_galois_hoisted_grouped / troyhip_galois_plain_sum_hoisted_grouped) at the
bench shapes, one JSON line per (shape, call, special primes, batch, R).  Real keys of both forms from the device generator, real encryptions brought to
dl = K - alpha limbs by the modulus switches, steps 1 .. R.  Three forms of the same R rotations (call "rotations") or of sum_r d_r * rot(x, r) (call
"linear_transform"), all through the Python layer on the same operand:

  grouped_hoisted_ms      (a) ONE hoisted call with the grouped keys
  per_prime_hoisted_ms    (b) ONE hoisted call with the per-prime keys
  sequential_grouped_ms   (c) R applyGalois calls with the grouped keys (linear transform: each followed by multiplyPlain and add)

A sample is `--reps` back-to-back calls between two device events, divided by reps; after a warm-up of every form the three ALTERNATE `--rounds` times.
The figure is the median over the rounds, *_spread_ms is max - min over them.

  vs_per_prime, vs_sequential    (b) / (a) and (c) / (a)
  faster_than_per_prime, faster_than_sequential    "yes" / "no": (a) is faster by more than the two spreads together
  slabs                   slabs (a) ran in under the default scratch limit
  verified                the first and the last item of every form decrypt to the expected plaintext (rotations: of the first and the last rotation);
                          CKKS: within 1e-3 of it (max_slot_error: the largest slot error seen)
  kernels                 with --kernels: the library's per-launch events over ONE call of (a) and of (b), microseconds by kernel
  refused                 instead of the figures: the library's message where it does not accept alpha for the shape's primes

Usage: python tools/grouped_hoist_bench.py [--shapes a,b] [--alphas 2,3,4] [--batches 1,8] [--rots 2,4,8,16] [--lt-rots 8,16] [--rounds 5] [--reps 100]
                                           [--kernels] [--out profiles/grouped_hoist_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from encrypt_bench import Timer  # noqa: E402
from grouped_ks_bench import SHAPES  # noqa: E402
from hoist_bench import ktime_report  # noqa: E402
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import CKKS  # noqa: E402

FORMS = ("grouped_hoisted", "per_prime_hoisted", "sequential_grouped")


def alternate(timer, fns, rounds, reps):
    """-> {form: (median ms, spread ms)} after one warm-up call of each"""
    for f in fns.values():
        f()
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            samples[k].append(timer.run(f, reps))
    return {k: (float(np.median(v)), max(v) - min(v)) for k, v in samples.items()}


def kernel_split(lib, fn):
    capi.check(lib, lib.troyhip_ktime_enable(1))
    fn()
    capi.check(lib, lib.troyhip_stream_synchronize(None))
    ks = ktime_report(lib)
    capi.check(lib, lib.troyhip_ktime_enable(0))
    return {x["name"].strip(): round(x["total_us"], 1) for x in ks}


def bench_shape(name, cfg, alphas, batches, rots, lt_rots, rounds, reps, kernels):
    lib = api.KernelProvider.lib()
    N, scheme = cfg["N"], cfg["scheme"]
    ckks = scheme == CKKS
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = int(api.PlainModulus.Batching(N, cfg["tbits"])) if cfg["tbits"] else 0
    ctx = api.SEALContext(scheme, N, primes, t)
    K = ctx.key_limbs
    kg = api.KeyGenerator(ctx, seed=(0x6B5, 17))
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(41, 42))
    dec = api.Decryptor(ctx, kg.secretKey())
    ev = api.Evaluator(ctx)
    coder = api.CKKSEncoder(ctx) if ckks else api.BatchEncoder(ctx)
    rmax = max(rots + lt_rots)
    steps = list(range(1, rmax + 1))
    elts = [ctx.galois_elt_from_step(s) for s in steps]
    gk0 = kg.createGaloisKeys(elts, device=True)
    rng = np.random.default_rng(11)
    scale, pscale = 2.0 ** 40, 2.0 ** 20
    timer = Timer(lib)
    rot_fn, lt_hoisted, lt_grouped = (ev.rotateVector, ev.rotateVectorPlainSumHoisted, ev.rotateVectorPlainSumHoistedGrouped) if ckks else \
        (ev.rotateRows, ev.rotateRowsPlainSumHoisted, ev.rotateRowsPlainSumHoistedGrouped)
    # the diagonals of the linear transform: at the key level in NTT form for the hoisted calls, at the operand's level for the composition
    if ckks:
        diags = rng.uniform(-1, 1, (rmax, N // 2)) + 1j * rng.uniform(-1, 1, (rmax, N // 2))
        d_np = [coder.encode(d, pscale, limbs=K) for d in diags]
        d_key = [api.DeviceBuffer.from_numpy(p) for p in d_np]
    else:
        diags = rng.integers(0, t, (rmax, N), dtype=np.uint64)
        d_coeff = [api.DeviceBuffer.from_numpy(coder.encode(d)) for d in diags]
        d_key = [ev.transformPlainToNtt(p, K) for p in d_coeff]

    def rolled(v, s):
        return np.roll(v, -s) if ckks else np.roll(v.reshape(2, -1), -s, axis=1).reshape(-1)

    out = []
    for alpha in alphas:
        try:
            digits, lmax, key_words = ctx.grouped_key_shape(alpha)
            gkg = kg.createGaloisKeys(elts, device=True, special_primes=alpha)
        except capi.TroyHipError as e:
            res = dict(shape=name, N=N, K=K, special_primes=alpha, refused=str(e.args[-1]))
            out.append(res)
            print(json.dumps(res), flush=True)
            continue
        d_level = [api.DeviceBuffer.from_numpy(p[:lmax]) for p in d_np] if ckks else None
        for B in batches:
            if ckks:
                vals = rng.uniform(-1, 1, (B, N // 2)) + 1j * rng.uniform(-1, 1, (B, N // 2))
                a = api.Ciphertext.from_numpy(ctx, np.stack([enc.encrypt(coder.encode(v, scale)) for v in vals]), True, scale)
            else:
                vals = rng.integers(0, t, (B, N), dtype=np.uint64)
                a = api.Ciphertext.from_numpy(ctx, np.stack([enc.encrypt(coder.encode(v)) for v in vals]))
            a = ev.modSwitchTo(a, lmax) if a.limbs > lmax else a
            items = sorted({0, B - 1})

            def plain_of(ct, b, sc):
                h = ct.cpu()[b]
                return coder.decode(dec.decrypt(h), sc) if ckks else coder.decode(dec.decrypt(h, correction_factor=ct.correction_factor))

            def check(ct, b, want, sc, worst):
                m = plain_of(ct, b, sc)
                if ckks:
                    e = float(np.abs(m - want).max())
                    worst[0] = max(worst[0], e)
                    return e < 1e-3
                return bool(np.array_equal(m, want))

            def line(call, R, fns, results, slabs, extra):
                ms = alternate(timer, fns, rounds, reps)
                (ta, sa), (tb, sb), (tc, sc_) = (ms[k] for k in FORMS)
                res = dict(shape=name, N=N, K=K, call=call, special_primes=alpha, batch=B, R=R, limbs=lmax, digits=-(-lmax // alpha), per_prime_digits=lmax)
                for k in FORMS:
                    res[k + "_ms"], res[k + "_spread_ms"] = round(ms[k][0], 4), round(ms[k][1], 4)
                res.update(vs_per_prime=round(tb / ta, 3), vs_sequential=round(tc / ta, 3), faster_than_per_prime="yes" if tb - ta > sa + sb else "no",
                           faster_than_sequential="yes" if tc - ta > sa + sc_ else "no", slabs=slabs, grouped_key_bytes=key_words * 8,
                           per_prime_key_bytes=(K - 1) * 2 * K * N * 8, **results, rounds=rounds, reps=reps, build_id=capi.build_id(lib))
                if kernels:
                    res["kernels"] = {k: kernel_split(lib, fns[k]) for k in FORMS[:2]}
                res.update(extra)
                out.append(res)
                print(json.dumps(res), flush=True)

            for R in rots:
                fns = {"grouped_hoisted": lambda: ev.applyGaloisHoistedGrouped(a, elts[:R], gkg),
                       "per_prime_hoisted": lambda: ev.applyGaloisHoisted(a, elts[:R], gk0),
                       "sequential_grouped": lambda: [ev.applyGalois(a, e, gkg) for e in elts[:R]]}
                s0 = capi.stat("grouped_hoist_slabs", lib)
                got = {k: f() for k, f in fns.items()}
                slabs = capi.stat("grouped_hoist_slabs", lib) - s0
                ok, worst = True, [0.0]
                for k in FORMS:
                    for r in sorted({0, R - 1}):
                        for b in items:
                            ok = check(got[k][r], b, rolled(vals[b], steps[r]), scale, worst) and ok
                del got
                line("rotations", R, fns, dict(verified=ok, **({"max_slot_error": worst[0]} if ckks else {})), slabs, {})

            for R in lt_rots:
                def composition():
                    seq = None
                    for r in range(R):
                        term = rot_fn(a, steps[r], gkg)
                        if ckks:
                            ev.multiplyPlainInplace(term, d_level[r], pscale)
                        else:
                            ev.multiplyPlainNormalInplace(term, d_coeff[r])
                        if seq is None:
                            seq = term
                        else:
                            ev.addInplace(seq, term)
                    return seq

                ps = pscale if ckks else 1.0
                fns = {"grouped_hoisted": lambda: lt_grouped(a, steps[:R], d_key[:R], gkg, ps),
                       "per_prime_hoisted": lambda: lt_hoisted(a, steps[:R], d_key[:R], gk0, ps),
                       "sequential_grouped": composition}
                s0 = capi.stat("grouped_hoist_lt_slabs", lib)
                got = {k: f() for k, f in fns.items()}
                slabs = capi.stat("grouped_hoist_lt_slabs", lib) - s0
                ok, worst = True, [0.0]
                for b in items:
                    if ckks:
                        want = sum(diags[r] * rolled(vals[b], steps[r]) for r in range(R))
                    else:
                        want = (sum(diags[r].astype(object) * rolled(vals[b], steps[r]).astype(object) for r in range(R)) % t).astype(np.uint64)
                    for k in FORMS:
                        ok = check(got[k], b, want, scale * pscale, worst) and ok
                del got
                line("linear_transform", R, fns, dict(verified=ok, **({"max_slot_error": worst[0]} if ckks else {})), slabs, {})
            del a
        del gkg
    capi.check(lib, lib.troyhip_timer_destroy(timer.h))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bfv_n32768_l14,ckks_n32768_chain,bgv_n65536_relin_rot")
    ap.add_argument("--alphas", default="2,3,4")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--rots", default="2,4,8,16")
    ap.add_argument("--lt-rots", default="8,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)  # 0.1 - 8 ms per call: a sample is a window of 0.01 - 0.8 s
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",") if v]
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], ints(a.alphas), ints(a.batches), ints(a.rots), ints(a.lt_rots), a.rounds, a.reps, a.kernels)
        lines += r
        ok = ok and all(v.get("verified", True) for v in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for v in lines:
                    f.write(json.dumps(v) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
