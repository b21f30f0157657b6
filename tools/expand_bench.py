#!/usr/bin/env python3
"""Oblivious expansion in one call (troyhip_expand_coefficients) against what a caller could compose before it, one JSON line per
(shape, batch, count).  Real keys from createAutomorphismKeys(device=True), real encryptions of random polynomials; ONE batch of ciphertexts is expanded
into `count` batches.  One process, the three forms through the Python layer on the same inputs, wall-clock around the call and a stream synchronisation
(the compositions' cost is partly host round trips, which device events between launches would not see), after a warm-up, ALTERNATING the forms
`--rounds` times:

  fused_ms        (a)  Evaluator.expandCoefficients
  composed_ms     (b)  the definition node by node: divideByPolyModulusDegreeInplace, then per node applyGalois, add, sub, negacyclicShift
  layered_ms      (b') the nodes of a layer kept in ONE batch by the caller: per layer one applyGalois, add, sub, negacyclicShift over all nodes and a
                       device-to-device gather of the present children -- every layer's key is streamed once, as in (a)
                  (each: the median over the rounds; *_spread_ms: max - min over the rounds)
  speedup, speedup_layered       composed_ms / fused_ms, layered_ms / fused_ms
  faster, faster_than_layered    "yes" / "no": (a) is faster than that form by more than the two spreads together
  key_switches, chunks    the counter deltas of one fused call (expand_key_switches, expand_chunks); composed_key_switches = m - 1, layered = l
  identical       (a), (b) and (b') are the same bytes
  verified        output r of (a) and of (b) decrypts to sum_k a_(r + k m) x^(k m) of the decrypted input, for every item and output

Shapes: those of tools/lwe_pack_bench.py.  The output alone is count * B * 2 * limbs * N words and the compositions hold several copies of a layer: a
(count, batch) whose buffers would not fit `--mem-gib`, or that would start after `--budget-s` seconds of the shape have passed, is written as a line with
"skipped".

Usage: python tools/expand_bench.py [--shapes a,b] [--batches 1,8] [--counts 2,8,64,512] [--rounds N] [--mem-gib G] [--budget-s S] [--out profiles/expand_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from troy_amd import api, capi  # noqa: E402
from lwe_pack_bench import SHAPES, clog2, wall  # noqa: E402

COUNTERS = ("expand_key_switches", "expand_chunks")


def composed(ev, N, x, count, gk):
    """(b): node by node -> list of `count` Ciphertext batches"""
    l = clog2(count)
    c = x.copy()
    ev.divideByPolyModulusDegreeInplace(c, N >> l)
    nodes = [c]
    for j in range(l):
        s, g = 1 << j, (N >> j) + 1
        nxt = [None] * min(count, 2 * s)
        for a in range(s):
            c = nodes[a]
            k = ev.applyGalois(c, g, gk)
            nxt[a] = ev.add(c, k)
            if a + s < count:
                d = ev.sub(c, k)
                ev.negacyclicShiftInplace(d, 2 * N - s)
                nxt[a + s] = d
        nodes = nxt
    return nodes


def layered(ev, N, x, count, gk):
    """(b'): the nodes of a layer in one batch, node a of item b at a * B + b -> one Ciphertext of count * B items"""
    ctx, B, limbs = x.context, x.batch, x.limbs
    item = 2 * limbs * N
    l = clog2(count)
    cur = api.Ciphertext(ctx, B, 2, limbs, x.is_ntt_form, x.scale, x.correction_factor)
    for b in range(B):  # a dense copy (the operand may be strided)
        cur.buf.copy_from(x.buf, item, b * x.bstride, b * item)
    ev.divideByPolyModulusDegreeInplace(cur, N >> l)
    for j in range(l):
        s, g = 1 << j, (N >> j) + 1
        odd = min(s, count - s)
        k = ev.applyGalois(cur, g, gk)
        d = ev.sub(cur, k)
        ev.negacyclicShiftInplace(d, 2 * N - s)
        ev.addInplace(cur, k)
        nxt = api.Ciphertext(ctx, (s + odd) * B, 2, limbs, x.is_ntt_form, x.scale, x.correction_factor)
        nxt.buf.copy_from(cur.buf, s * B * item)
        nxt.buf.copy_from(d.buf, odd * B * item, 0, s * B * item)
        cur = nxt
    return cur


def bench_shape(name, cfg, batches, counts, rounds, mem_gib, budget_s, lib=None):
    lib = lib or api.KernelProvider.lib()
    N, scheme = cfg["N"], cfg["scheme"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = cfg.get("t") or api.PlainModulus.Batching(N, cfg["tbits"])
    ctx = api.SEALContext(scheme, N, primes, t)
    limbs = ctx.first_limbs
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
        assert np.array_equal(ev.decrypt(x, sk_dev), msgs)
        for count in counts:
            count = N if count in (0, "N") else int(count)
            l = clog2(count)
            m = 1 << l
            head = dict(shape=name, N=N, limbs=limbs, batch=B, count=count, layers=l)
            # the three results at once, and the four layer-sized temporaries (b') holds while it gathers
            words = (3 + 4) * count * B * 2 * limbs * N
            if words * 8 > mem_gib * 2 ** 30 or time.perf_counter() - started > budget_s:
                res = dict(head, skipped="memory" if words * 8 > mem_gib * 2 ** 30 else "time budget")
                out.append(res)
                print(json.dumps(res), flush=True)
                continue
            forms = (lambda: ev.expandCoefficients(x, count, gk), lambda: composed(ev, N, x, count, gk), lambda: layered(ev, N, x, count, gk))
            c0 = [capi.stat(n, lib) for n in COUNTERS]
            _, ra = wall(lib, forms[0])  # the warm-up of every form gives the results that are verified
            deltas = [capi.stat(n, lib) - v for n, v in zip(COUNTERS, c0)]
            _, rb = wall(lib, forms[1])
            _, rl = wall(lib, forms[2])
            times = ([], [], [])
            for _ in range(rounds):
                for f, ts in zip(forms, times):
                    ts.append(wall(lib, f)[0])
            hl = rl.cpu().reshape(count, B, 2, limbs, N)
            same, ok_a, ok_b = True, True, True
            for r in range(count):
                ha, hb = ra[r].cpu(), rb[r].cpu()[:, :2]
                same = same and np.array_equal(ha, hb) and np.array_equal(ha, hl[r])
                exp = np.zeros((B, N), dtype=np.uint64)
                exp[:, 0::m] = msgs[:, r::m]
                ok_a = ok_a and np.array_equal(ev.decrypt(ra[r], sk_dev), exp)
                ok_b = ok_b and np.array_equal(ev.decrypt(rb[r], sk_dev), exp)
            med = [float(np.median(ts)) for ts in times]
            spr = [max(ts) - min(ts) for ts in times]
            res = dict(head, fused_ms=round(med[0], 3), fused_spread_ms=round(spr[0], 3), composed_ms=round(med[1], 3), composed_spread_ms=round(spr[1], 3),
                       layered_ms=round(med[2], 3), layered_spread_ms=round(spr[2], 3), speedup=round(med[1] / med[0], 2), speedup_layered=round(med[2] / med[0], 2),
                       faster="yes" if med[1] - med[0] > spr[0] + spr[1] else "no", faster_than_layered="yes" if med[2] - med[0] > spr[0] + spr[2] else "no",
                       key_switches=deltas[0], chunks=deltas[1], composed_key_switches=m - 1, layered_key_switches=l, identical=bool(same), verified_a=bool(ok_a),
                       verified_b=bool(ok_b), verified=bool(ok_a and ok_b), rounds=rounds, build_id=capi.build_id(lib))
            out.append(res)
            print(json.dumps(res), flush=True)
            del ra, rb, rl, hl
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="linear_n4096,linear_n8192,bfv_n8192_l4,bfv_n32768_l14")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--counts", default="2,8,64,512")
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
