#!/usr/bin/env python3
"""Polynomial evaluation in one call (troyhip_evaluate_polynomial) against what a caller composes from the calls the library
already had, at the bench shapes: one JSON line per (shape, batch, degree).  Dense random coefficients, real keys and encryptions, one process, all
forms through the Python layer on the same inputs, timed with device events after a warm-up, ALTERNATING the forms `--rounds` times:

  fused_ms        (a) ONE Evaluator.evaluatePolynomial call
  composed_ms     (b) the same Paterson-Stockmeyer schedule from the older public calls: multiply, relinearizeInplace, the level step, a multiplyPlain per
                  term with the constant ENCODED as a plaintext (encoded once, outside the timed region), addInplace, addPlain, a multiply and a size-3 add
                  per block, one relinearization
  horner_ms       (c) Horner: degree - 1 products, each relinearized (and level-stepped); run where the chain has the levels (BFV: up to degree 15)
                  (each: the median over the rounds; *_spread_ms: max - min over the rounds)
  speedup_b/_c    composed_ms / fused_ms, horner_ms / fused_ms
  faster_b/_c     "yes" / "no": (a) is faster than the other form by more than the two spreads together
  products, relins, scalar_sums   the counter deltas of one fused call
  scalar_sum_*    scalar_sum_kernel alone over one fused call (the library's per-launch events): its time, its compulsory bytes
                  sum over its launches of (count + 1) x size x limbs x N x 8 per item, the bytes per second and their share of the 8 TB/s HBM peak
                  (a bare copy reaches 0.73 of it on this part: profiles/r06_elementwise_ab.txt)
  verified        every form that ran decrypts to the polynomial of the slots: BFV / BGV exactly modulo t in every slot of every item; CKKS within 1e-3
                  (slots and coefficients in [-1, 1], scale 2^40); verified_a/_b/_c per form

Usage: python tools/poly_bench.py [--shapes a,b] [--batches 1,8] [--degrees 7,15,31] [--reps N] [--rounds N] [--out profiles/poly_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from encrypt_bench import SHAPES, Timer  # noqa: E402
from hoist_bench import ktime_report  # noqa: E402
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import BFV, BGV, CKKS  # noqa: E402

CKKS_SCALE = 2.0 ** 40
HBM_PEAK = 8.0e12
COUNTERS = ("poly_products", "poly_relins", "poly_scalar_sums")


def clog2(n):
    return (n - 1).bit_length()


def plan(degree, k=0):
    """(k, m, lb, P, depth) as troyhip_polynomial_depth states them (include/troyhip.h)"""
    if not k:
        k = 2
        while k * k < degree + 1:
            k *= 2
    m = -(-(degree + 1) // k)
    lb = clog2(min(degree, k - 1))
    P = lb if m == 1 else max(lb + 1, clog2(k) + clog2(m - 1))
    return k, m, lb, P, P + 1


class Forms:
    def __init__(self, ctx, ev, rlk, coder, primes):
        self.ctx, self.ev, self.rlk, self.coder, self.primes = ctx, ev, rlk, coder, primes
        self.scheme, self.N = ctx.scheme, ctx.N
        self.plains = {}

    def plain(self, c, scale, limbs):
        """the constant c as a plaintext on the device, encoded once"""
        key = (c, scale, limbs)
        if key not in self.plains:
            if self.scheme == CKKS:
                self.plains[key] = api.DeviceBuffer.from_numpy(self.coder.encode(np.full(self.N // 2, c), scale, limbs))
            else:
                self.plains[key] = api.DeviceBuffer.from_numpy(self.coder.encode(np.full(self.N, c, dtype=np.int64)))
        return self.plains[key]

    def down(self, a, limbs):
        while a.limbs > limbs:
            a = self.ev.modSwitchToNext(a)
        return a

    def step(self, a):
        if self.scheme == BFV:
            return a
        return self.ev.rescaleToNext(a) if self.scheme == CKKS else self.ev.modSwitchToNext(a)

    def mul(self, a, b):
        L = min(a.limbs, b.limbs)
        p = self.ev.multiply(self.down(a, L), self.down(b, L))
        self.ev.relinearizeInplace(p, self.rlk)
        return self.step(p)

    def times_const(self, a, c, target):
        a = a.copy()
        if self.scheme == CKKS:
            ps = target / a.scale
            self.ev.multiplyPlainInplace(a, self.plain(c, ps, a.limbs), ps)
        else:
            self.ev.multiplyPlainNormalInplace(a, self.plain(c, 0, 0))
        return a

    def plus_const(self, a, c):
        if self.scheme == CKKS:
            self.ev.addPlainInplace(a, self.plain(c, a.scale, a.limbs), plain_scale=a.scale)
        else:
            self.ev.addPlainInplace(a, self.plain(c, 0, 0))

    def fused(self, x, coeffs):
        return self.ev.evaluatePolynomial(x, coeffs, self.rlk)

    def composed(self, x, coeffs):
        ev, scheme = self.ev, self.scheme
        d = len(coeffs) - 1
        k, m, lb, P, _ = plan(d)
        L0 = x.limbs
        at = (lambda lv: L0) if scheme == BFV else (lambda lv: L0 - lv)
        pw = {1: x}
        for j in range(2, min(k, d) + 1):
            pw[j] = self.mul(pw[(j + 1) // 2], pw[j // 2])
        X = {1: pw.get(k)}
        for i in range(2, m):
            X[i] = self.mul(X[(i + 1) // 2], X[i // 2])

        def block(i, limbs, target):
            acc = None
            for j in range(1, k):
                if i * k + j > d:
                    break
                a = self.times_const(self.down(pw[j], limbs), coeffs[i * k + j], target)
                if acc is None:
                    acc = a
                else:
                    ev.addInplace(acc, a)
            self.plus_const(acc, coeffs[i * k])
            return acc

        S = x.scale * float(self.primes[at(P) - 1]) if scheme == CKKS else 0.0
        if m == 1:
            return self.step(block(0, at(lb), S))
        acc = None
        for i in range(1, m):
            Xi = self.down(X[i], at(P))
            target = S / Xi.scale * float(self.primes[at(P - 1) - 1]) if scheme == CKKS else 0.0
            p = ev.multiply(self.down(self.step(block(i, at(P - 1), target)), at(P)), Xi)
            if acc is None:
                acc = p
            else:
                ev.addInplace(acc, p)
        ev.relinearizeInplace(acc, self.rlk)
        ev.addInplace(acc, block(0, at(P), S))
        return self.step(acc)

    def horner(self, x, coeffs):
        d = len(coeffs) - 1
        target = x.scale * float(self.primes[x.limbs - 1]) if self.scheme == CKKS else 0.0
        acc = self.times_const(x, coeffs[d], target)
        if self.scheme == CKKS:
            acc = self.ev.rescaleToNext(acc)
        self.plus_const(acc, coeffs[d - 1])
        for j in range(d - 2, -1, -1):
            acc = self.mul(acc, x)
            self.plus_const(acc, coeffs[j])
        return acc


def scalar_sum_bytes(scheme, degree, L0, N, B):
    """the compulsory traffic of the scalar sums of one dense call: (count + 1) x size x limbs x N x 8 bytes per item and launch"""
    k, m, lb, P, _ = plan(degree)
    at = (lambda lv: L0) if scheme == BFV else (lambda lv: L0 - lv)
    total = 0
    for i in range(m):
        count = max(1, min(k - 1, degree - i * k))
        limbs = at(lb) if m == 1 else (at(P) if i == 0 else at(P - 1))
        total += (count + 1) * 2 * limbs * N * 8 * B
    return total


def bench_shape(name, cfg, batches, degrees, reps, rounds):
    lib = api.KernelProvider.lib()
    N, scheme = cfg["N"], cfg["scheme"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
    ctx = api.SEALContext(scheme, N, primes, t)
    limbs, ckks = ctx.first_limbs, scheme == CKKS
    kg = api.KeyGenerator(ctx, seed=(0x11F7, 5))
    rlk = kg.createRelinKeys(device=True)
    sk_dev = api.DeviceBuffer.from_numpy(kg.secretKey())
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(21, 22))
    ev = api.Evaluator(ctx)
    coder = api.CKKSEncoder(ctx) if ckks else api.BatchEncoder(ctx)
    F = Forms(ctx, ev, rlk, coder, [int(p) for p in primes])
    rng = np.random.default_rng(8)
    timer = Timer(lib)
    out = []
    for B in batches:
        if ckks:
            slots = rng.uniform(-1, 1, (B, N // 2))
            x = enc.encryptBatch(coder.encodeBatch(slots, CKKS_SCALE, limbs, device=True), CKKS_SCALE)
        else:
            slots = rng.integers(0, t, (B, N), dtype=np.uint64)
            x = enc.encryptBatch(coder.encodeBatch(slots, device=True))
        for degree in degrees:
            if ckks:
                coeffs = [float(v) for v in rng.uniform(-1, 1, degree + 1)]
                exact = np.polynomial.polynomial.polyval(slots, coeffs)
            else:
                coeffs = [int(v) for v in rng.integers(1, t, degree + 1)]
                exact = np.zeros_like(slots)
                for c in reversed(coeffs):  # t < 2^21: every product fits 64 bits
                    exact = (exact * slots + np.uint64(c)) % np.uint64(t)
            depth = 0 if scheme == BFV else plan(degree)[4]
            with_c = degree <= 15 if scheme == BFV else limbs - degree >= ctx.last_limbs
            forms = [("a", F.fused), ("b", F.composed)] + ([("c", F.horner)] if with_c else [])
            c0 = np.array([capi.stat(n, lib) for n in COUNTERS])
            res_ct = {"a": F.fused(x, coeffs)}
            counts = [int(v) for v in np.array([capi.stat(n, lib) for n in COUNTERS]) - c0]
            for k, fn in forms[1:]:
                res_ct[k] = fn(x, coeffs)
            times = {k: [] for k, _ in forms}
            for _ in range(rounds):
                for k, fn in forms:
                    times[k].append(timer.run(lambda: fn(x, coeffs), reps))
            capi.check(lib, lib.troyhip_stream_synchronize(None))
            ver, errs = {}, {}
            for k, _ in forms:
                ct = res_ct[k]
                dcr = ev.decrypt(ct, sk_dev)
                if ckks:
                    errs[k] = float(np.abs(coder.decodeBatch(dcr, ct.scale).real - exact).max())
                    ver[k] = errs[k] < 1e-3
                else:
                    ver[k] = bool(np.array_equal(coder.decodeBatch(dcr), exact))
            ver["a"] = ver["a"] and res_ct["a"].limbs == limbs - depth and (not ckks or res_ct["a"].scale == CKKS_SCALE)
            med = {k: float(np.median(v)) for k, v in times.items()}
            spr = {k: max(v) - min(v) for k, v in times.items()}
            res = dict(shape=name, N=N, limbs=limbs, batch=B, degree=degree, baby_steps=plan(degree)[0], depth=depth, fused_ms=round(med["a"], 4),
                       fused_spread_ms=round(spr["a"], 4), composed_ms=round(med["b"], 4), composed_spread_ms=round(spr["b"], 4),
                       speedup_b=round(med["b"] / med["a"], 3), faster_b="yes" if med["b"] - med["a"] > spr["a"] + spr["b"] else "no",
                       products=counts[0], relins=counts[1], scalar_sums=counts[2], rounds=rounds, reps=reps)
            if with_c:
                res.update(horner_ms=round(med["c"], 4), horner_spread_ms=round(spr["c"], 4), speedup_c=round(med["c"] / med["a"], 3),
                           faster_c="yes" if med["c"] - med["a"] > spr["a"] + spr["c"] else "no")
            for k, _ in forms:
                res["verified_" + k] = bool(ver[k])
            res["verified"] = bool(all(ver.values()))
            if ckks:
                res["max_err"] = errs
            capi.check(lib, lib.troyhip_ktime_enable(1))
            F.fused(x, coeffs)
            capi.check(lib, lib.troyhip_stream_synchronize(None))
            ks = ktime_report(lib)
            capi.check(lib, lib.troyhip_ktime_enable(0))
            us = sum(v["total_us"] for v in ks if "scalar_sum" in v["name"])
            if us:
                nbytes = scalar_sum_bytes(scheme, degree, limbs, N, B)
                res.update(scalar_sum_us=round(us, 1), scalar_sum_launches=sum(v["calls"] for v in ks if "scalar_sum" in v["name"]), scalar_sum_bytes=nbytes,
                           scalar_sum_tbps=round(nbytes / (us * 1e-6) / 1e12, 3), scalar_sum_of_hbm_peak=round(nbytes / (us * 1e-6) / HBM_PEAK, 3))
            res["build_id"] = capi.build_id(lib)
            out.append(res)
            print(json.dumps(res), flush=True)
    capi.check(lib, lib.troyhip_timer_destroy(timer.h))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bfv_n32768_l14,bgv_n65536_relin_rot,ckks_n32768_chain")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--degrees", default="7,15,31")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], [int(x) for x in a.batches.split(",")], [int(x) for x in a.degrees.split(",")], a.reps, a.rounds)
        lines += r
        ok = ok and all(x["verified_a"] and x["verified_b"] for x in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
