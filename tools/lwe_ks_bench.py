#!/usr/bin/env python3
"""LWE key switching to a smaller dimension (troyhip_lwe_key_switch), one JSON line per (shape, n, R), two measurements.
Real keys: a random ternary LWE secret z of n digits, createLWESwitchKey(z, base_bits), fresh BFV encryptions whose measured coefficients sit at the centres
of the four windows of LookupTable(t_bits = 2), brought to one limb and extracted.  Wall-clock around the call and a stream synchronisation, after a
warm-up; `--rounds` rounds, the two routes of the pipeline ALTERNATING.

 kind "call"      Evaluator.lweKeySwitch(to_2n=False) alone on R = count x batch extracted samples:
   call_ms, call_spread_ms   the median and max - min over the rounds
   key_mb, key_fraction      the key's bytes, and key bytes / call time as a fraction of the 8 TB/s peak (a bare copy reaches 0.73)
   splits, slabs             lwe_ks_splits and the lwe_ks_slabs delta of one call
   noise_bits, decrypted     the phase of every switched sample under z, out[n] + <out[:n], z>, against the phase of the operand under the RLWE secret:
                             the bit length of the largest difference, and how many samples still decrypt to their message coefficient,
                             round(t phase / q_0) mod t, at ONE limb (a 60-bit q_0 under t = 2^41 leaves 2^18 for it)
   verified                  every difference is within the bound of section 4.23, N l (2^w - 1) 21, and every operand decrypts to its message
 kind "pipeline"  LookupTable.apply on the same ciphertexts, both routes returning f(message):
   switch_ms   (a)  lwe_key=LK and createBlindRotationKey(z): n CMux steps
   full_ms     (b)  no switch key, createBlindRotationKey(kg.extractionSecret()): N steps.  Its key takes 2 N RGSW ciphertexts; where that passes
                    `--mem-gib` the line says so under "full_skipped" and carries (a) alone
   speedup, faster           full_ms / switch_ms; "yes" / "no": (a) is faster than (b) by more than the two spreads together
   verified                  every result's constant coefficient decrypts to f(window) on both routes, with a positive noise budget

Usage: python tools/lwe_ks_bench.py [--shapes a,b] [--dims 512,1024] [--samples 1,8,64,512] [--base-bits 8] [--rounds N] [--pipeline-samples 1,8]
                                    [--mem-gib G] [--out profiles/lwe_ks_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from troy_amd import api, app, capi  # noqa: E402
from blindrot_bench import SHAPES  # noqa: E402
from lwe_pack_bench import wall  # noqa: E402

PEAK_BYTES_PER_MS = 8e12 / 1e3


def table(t):
    return (t // 4, 3, t - 5, t // 8 + 1)


def encryptions(ctx, kg, t, N, batch, terms, rng):
    """`batch` fresh ciphertexts whose coefficients `terms` sit at the centres of the windows -> (Ciphertext, windows [count][batch], messages)"""
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(5, 6))
    msgs = rng.integers(0, t, (batch, N), dtype=np.uint64)
    ks = np.array([[(b + 2 * j + 1) % 4 for b in range(batch)] for j in range(len(terms))])
    W = N // 4
    for j, term in enumerate(terms):
        for b in range(batch):
            msgs[b, term] = (t * (2 * int(ks[j, b]) + 1) * W + 2 * N) // (4 * N)
    return api.Ciphertext.from_numpy(ctx, np.stack([enc.encrypt(m) for m in msgs])), ks, msgs


def bench_shape(name, cfg, dims, sample_counts, base_bits, rounds, pipeline_samples, mem_gib, lib=None):
    lib = lib or api.KernelProvider.lib()
    N, scheme = cfg["N"], cfg["scheme"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = int(cfg.get("t") or api.PlainModulus.Batching(N, cfg["tbits"]))
    ctx = api.SEALContext(scheme, N, primes, t)
    q0, K = int(primes[0]), ctx.key_limbs
    kg = api.KeyGenerator(ctx, seed=(0x15E, 9))
    sk_dev = api.DeviceBuffer.from_numpy(kg.secretKey())
    uu = kg.extractionSecret().astype(object)
    ev = api.Evaluator(ctx)
    rng = np.random.default_rng(14)
    f = table(t)
    lut = app.LookupTable(ctx, lambda k: f[k], 2)
    out = []
    full_words = 2 * N * 2 * (K - 1) * 2 * K * N
    full_key = None
    full_skipped = None
    if full_words * 8 > mem_gib * 2**30:
        full_skipped = "the n = N key takes %.1f GiB" % (full_words * 8 / 2**30)
    for n in dims:
        z = rng.integers(-1, 2, n)
        LK = kg.createLWESwitchKey(z, base_bits=base_bits)
        BK = None
        zz = z.astype(object)
        for R in sample_counts:
            batch = min(R, 8)
            terms = [int(v) for v in rng.choice(N, R // batch, replace=False)]
            cts, ks, msgs = encryptions(ctx, kg, t, N, batch, terms, rng)
            lwes = ev.extractLWEs(ev.modSwitchTo(cts, 1), terms)
            call = lambda: ev.lweKeySwitch(lwes, LK, to_2n=False)  # noqa: E731
            s0 = capi.stat("lwe_ks_slabs", lib)
            _, res = wall(lib, call)
            slabs, splits = capi.stat("lwe_ks_slabs", lib) - s0, capi.stat("lwe_ks_splits", lib)
            ts = [wall(lib, call)[0] for _ in range(rounds)]
            got = res.to_numpy().reshape(R, n + 1).astype(object)
            phase = (got[:, n] + (got[:, :n] * zz).sum(axis=1)) % q0
            before = (lwes.c0_cpu().reshape(R).astype(object) + (lwes.c1_cpu().reshape(R, N).astype(object) * uu).sum(axis=1)) % q0
            diff = [min(int(d), q0 - int(d)) for d in (phase - before) % q0]
            decrypt = lambda ph: [((t * int(p) + q0 // 2) // q0) % t for p in ph]  # noqa: E731
            want = [int(msgs[b, term]) for term in terms for b in range(batch)]
            good = sum(1 for a, b in zip(decrypt(phase), want) if a == b)
            sound = decrypt(before) == want and max(diff) <= N * LK.digits * ((1 << base_bits) - 1) * 21
            med, key_mb = float(np.median(ts)), LK.buf.words * 8 / 1e6
            line = dict(kind="call", shape=name, N=N, n=n, base_bits=base_bits, digits=LK.digits, samples=R, call_ms=round(med, 4), call_spread_ms=round(max(ts) - min(ts), 4),
                        key_mb=round(key_mb, 1), key_fraction=round(key_mb * 1e6 / med / PEAK_BYTES_PER_MS, 3), splits=splits, slabs=slabs, noise_bits=max(diff).bit_length(), decrypted="%d/%d" % (good, R), verified=bool(sound),
                        rounds=rounds, build_id=capi.build_id(lib))
            out.append(line)
            print(json.dumps(line), flush=True)
            if R not in pipeline_samples:
                continue
            if BK is None:
                BK = kg.createBlindRotationKey(z, ternary=True)
            if full_key is None and not full_skipped:
                full_key = kg.createBlindRotationKey(kg.extractionSecret(), ternary=True)
            forms = [lambda: lut.apply(ev, cts, terms, BK, lwe_key=LK)]
            if full_key is not None:
                forms.append(lambda: lut.apply(ev, cts, terms, full_key))
            results = [wall(lib, fn)[1] for fn in forms]  # the warm-up gives the results that are verified
            times = [[] for _ in forms]
            for _ in range(rounds):
                for fn, tt in zip(forms, times):
                    tt.append(wall(lib, fn)[0])
            ok, budget = True, None
            for rot, _ in results:
                plains = ev.decrypt(rot, sk_dev)
                ok = ok and all(int(plains[j * batch + b][0]) == f[int(ks[j, b])] for j in range(len(terms)) for b in range(batch))
                bits = int(ev.invariantNoiseBudget(rot, sk_dev).min())
                budget = bits if budget is None else min(budget, bits)
            med = [float(np.median(tt)) for tt in times]
            spr = [max(tt) - min(tt) for tt in times]
            line = dict(kind="pipeline", shape=name, N=N, n=n, base_bits=base_bits, samples=R, switch_ms=round(med[0], 3), switch_spread_ms=round(spr[0], 3), budget=budget,
                        verified=bool(ok and budget > 0), rounds=rounds, build_id=capi.build_id(lib))
            if full_key is not None:
                line.update(full_ms=round(med[1], 3), full_spread_ms=round(spr[1], 3), speedup=round(med[1] / med[0], 2),
                            faster="yes" if med[1] - med[0] > spr[0] + spr[1] else "no")
            else:
                line.update(full_skipped=full_skipped)
            out.append(line)
            print(json.dumps(line), flush=True)
            del results
        del LK, BK
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="linear_n4096,bfv_n8192_l4,bfv_n2048_l2")
    ap.add_argument("--dims", default="512,1024")
    ap.add_argument("--samples", default="1,8,64,512")
    ap.add_argument("--pipeline-samples", default="1,8")
    ap.add_argument("--base-bits", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mem-gib", type=float, default=32.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    ints = lambda s: [int(v) for v in s.split(",") if v]  # noqa: E731
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], ints(a.dims), ints(a.samples), a.base_bits, a.rounds, ints(a.pipeline_samples), a.mem_gib)
        lines += r
        ok = ok and all(v.get("verified", True) for v in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for v in lines:
                    f.write(json.dumps(v) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
