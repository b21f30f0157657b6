#!/usr/bin/env python3
"""LWE extraction and packing in one call each (troyhip_extract_lwes + troyhip_pack_lwes) against the host-level composition the
package had (extractLWE per term + packLWECiphertexts), one JSON line per (shape, batch, count).  Real keys from createAutomorphismKeys(device=True), real
encryptions; `count` coefficients (spread over the ring) of ONE batch of ciphertexts are extracted and packed back into one ciphertext per item -- the
flow of a coefficient-packed linear layer.  One process, both forms through the Python layer on the same inputs, wall-clock around the call and a stream
synchronisation (the composition's cost is largely host round trips, which device events between launches would not see), after a warm-up,
ALTERNATING the two forms `--rounds` times:

  fused_ms        (a) Evaluator.extractLWEs + Evaluator.packLWEs
  composed_ms     (b) [Evaluator.extractLWE(ct, t) for t in terms] + Evaluator.packLWECiphertexts
                  (each: the median over the rounds; *_spread_ms: max - min over the rounds)
  speedup         composed_ms / fused_ms
  faster          "yes" / "no": (a) is faster than (b) by more than the two spreads together
  key_switches, chunks    the counter deltas of one fused call (lwe_pack_key_switches, lwe_pack_chunks); composed_key_switches = n' - 1 + log2 N - l per item batch
  identical       the two results are the same bytes
  verified        coefficient i * (N >> l) of the decryption of BOTH results is coefficient terms[i] of the decrypted input, for every item and sample

Shapes: the parameters of the LinearHelper tests (tests/cpp/test_troyn_linear.cpp: three 60-bit primes, t = 2^41) at N = 4096 and 8192, bench.py's
bfv_n8192_l4 and bfv_n32768_l14.  A (count, batch) whose samples, nodes and composition would not fit `--mem-gib`, or that would start after `--budget-s`
seconds of the shape have passed, is written as a line with "skipped".

Usage: python tools/lwe_pack_bench.py [--shapes a,b] [--batches 1,8] [--counts 2,8,64,512,N] [--rounds N] [--mem-gib G] [--budget-s S] [--out profiles/lwe_pack_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import BFV  # noqa: E402

SHAPES = {
    "linear_n4096": dict(scheme=BFV, N=4096, bits=[60, 60, 60], t=1 << 41),   # tests/cpp/test_troyn_linear.cpp
    "linear_n8192": dict(scheme=BFV, N=8192, bits=[60, 60, 60], t=1 << 41),
    "bfv_n8192_l4": dict(scheme=BFV, N=8192, bits=[40, 36, 36, 36, 40], tbits=20),  # bench.py
    "bfv_n32768_l14": dict(scheme=BFV, N=32768, bits=[60] + [58] * 13 + [60], tbits=20),
}
COUNTERS = ("lwe_pack_key_switches", "lwe_pack_chunks")


def clog2(n):
    return (n - 1).bit_length()


def wall(lib, fn):
    capi.check(lib, lib.troyhip_stream_synchronize(None))
    t0 = time.perf_counter()
    r = fn()
    capi.check(lib, lib.troyhip_stream_synchronize(None))
    return (time.perf_counter() - t0) * 1e3, r


def bench_shape(name, cfg, batches, counts, rounds, mem_gib, budget_s, lib=None):
    lib = lib or api.KernelProvider.lib()
    N, scheme = cfg["N"], cfg["scheme"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = cfg.get("t") or api.PlainModulus.Batching(N, cfg["tbits"])
    ctx = api.SEALContext(scheme, N, primes, t)
    limbs, logn = ctx.first_limbs, N.bit_length() - 1
    kg = api.KeyGenerator(ctx, seed=(0x17E, 6))
    gk = kg.createAutomorphismKeys(device=True)
    sk_dev = api.DeviceBuffer.from_numpy(kg.secretKey())
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(23, 24))
    ev = api.Evaluator(ctx)
    rng = np.random.default_rng(9)
    started = time.perf_counter()
    out = []
    for B in batches:
        msgs = rng.integers(0, t, (B, N), dtype=np.uint64)
        x = api.Ciphertext.from_numpy(ctx, np.stack([enc.encrypt(msgs[b]) for b in range(B)]))
        plain_in = ev.decrypt(x, sk_dev)
        assert np.array_equal(plain_in, msgs)
        for count in counts:
            count = N if count in (0, "N") else int(count)
            l = clog2(count)
            head = dict(shape=name, N=N, limbs=limbs, batch=B, count=count, layers=l, trace_rounds=logn - l)
            # samples + nodes of (a), the 2^l assembled ciphertexts (capacity 3) and their temporaries of (b)
            words = count * B * limbs * N * 2 + (3 + 2) * (1 << l) * B * limbs * N
            if words * 8 > mem_gib * 2 ** 30 or time.perf_counter() - started > budget_s:
                res = dict(head, skipped="memory" if words * 8 > mem_gib * 2 ** 30 else "time budget")
                out.append(res)
                print(json.dumps(res), flush=True)
                continue
            terms = [(i * N) // count for i in range(count)]

            def fused():
                return ev.packLWEs(ev.extractLWEs(x, terms), gk)

            def composed():
                return ev.packLWECiphertexts([ev.extractLWE(x, tm) for tm in terms], gk)

            c0 = [capi.stat(n, lib) for n in COUNTERS]
            _, ra = wall(lib, fused)  # the warm-up of both forms gives the results that are verified
            deltas = [capi.stat(n, lib) - v for n, v in zip(COUNTERS, c0)]
            _, rb = wall(lib, composed)
            ta, tb = [], []
            for _ in range(rounds):
                ta.append(wall(lib, fused)[0])
                tb.append(wall(lib, composed)[0])
            ha, hb = ra.cpu(), rb.cpu()[:, :2]
            step = N >> l
            ok = {}
            for k, r in (("a", ra), ("b", rb)):
                pt = ev.decrypt(r, sk_dev)
                ok[k] = bool(all(np.array_equal(pt[b, ::step][:count], msgs[b, terms]) for b in range(B)))
            ma, mb = float(np.median(ta)), float(np.median(tb))
            sa, sb = max(ta) - min(ta), max(tb) - min(tb)
            res = dict(head, fused_ms=round(ma, 3), fused_spread_ms=round(sa, 3), composed_ms=round(mb, 3), composed_spread_ms=round(sb, 3), speedup=round(mb / ma, 2),
                       faster="yes" if mb - ma > sa + sb else "no", key_switches=deltas[0], chunks=deltas[1], composed_key_switches=(1 << l) - 1 + logn - l,
                       identical=bool(np.array_equal(ha, hb)), verified_a=ok["a"], verified_b=ok["b"], verified=ok["a"] and ok["b"], rounds=rounds,
                       build_id=capi.build_id(lib))
            out.append(res)
            print(json.dumps(res), flush=True)
            del ra, rb
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="linear_n4096,linear_n8192,bfv_n8192_l4,bfv_n32768_l14")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--counts", default="2,8,64,512,N")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mem-gib", type=float, default=96.0)
    ap.add_argument("--budget-s", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], [int(v) for v in a.batches.split(",")], a.counts.split(","), a.rounds, a.mem_gib, a.budget_s)
        lines += r
        ok = ok and all(v.get("verified", True) and v.get("identical", True) for v in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for v in lines:
                    f.write(json.dumps(v) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
