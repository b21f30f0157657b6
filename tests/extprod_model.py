"""The exact model of the external product sum in Python integers, in the pattern of hoist_cases.model_item and factored so that
the inner products -- the expensive part -- are formed once for a case that is checked with and without a base:

  1. e_h[r][i][j] = NTT_{p_i}(d_j mod p_i), d_j limb j of polynomial h of term r (coefficient form, canonical), i over the dl data primes and the special one;
  2. acc[k][i] = sum_r sum_h sum_j e_h[r][i][j] * G_r[h][j][k][limb(i)] mod p_i;
  3. the scheme's mod-down by the special prime, added to the base (or to zero).

The transforms are the oracle's (oracle.ntt_standalone); everything else is Python integers.  `S` is a hoist_cases.Setup (N, K, primes, t, scheme)."""
import numpy as np

from oracle import oracle
from troy_amd.capi import BFV, BGV


def obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


def inner_products(S, cts, rgsws):
    """cts: R arrays [2][dl][N] (one item of every term); rgsws: R arrays [2][K-1][2][K][N] -> acc [2][dl + 1][N], Python integers below p_i"""
    N, K, primes = S.N, S.K, S.primes
    dl = cts[0].shape[1]
    out_primes = primes[:dl] + [primes[K - 1]]
    key_limb = list(range(dl)) + [K - 1]
    acc = np.zeros((2, dl + 1, N), dtype=object)
    for i, p in enumerate(out_primes):
        for ct, G in zip(cts, rgsws):
            for h in range(2):
                for j in range(dl):
                    e = obj(oracle.ntt_standalone(N, p, ct[h, j] % np.uint64(p), 1))
                    for k in range(2):
                        acc[k, i] += e * obj(G[h, j, k, key_limb[i]])
        acc[:, i] %= p
    return acc


def mod_down(S, acc, base=None):
    """step 3: acc [2][dl + 1][N] (NTT form) and base [2][dl][N] or None -> uint64 [2][dl][N], every limb canonical"""
    N, K, primes = S.N, S.K, S.primes
    dl = acc.shape[1] - 1
    qk = primes[K - 1]
    half = qk >> 1
    out_primes = primes[:dl] + [qk]
    out = np.zeros((2, dl, N), dtype=np.uint64)
    for k in range(2):
        coeff = [obj(oracle.ntt_standalone(N, p, acc[k, i].astype(np.uint64), 3)) for i, p in enumerate(out_primes)]
        last = coeff[dl]
        for j in range(dl):
            q = primes[j]
            inv = pow(qk, -1, q)
            if S.scheme == BFV:
                tl = (last + half) % qk
                v = (coeff[j] - tl % q + half % q) * inv
            else:
                assert S.scheme == BGV
                kt = (-last) % S.t * pow(qk, -1, S.t) % S.t
                v = (coeff[j] - kt % q * (qk % q) - last % q) * inv
            b = obj(base[k, j]) if base is not None else 0
            out[k, j] = ((b + v) % q).astype(np.uint64)
    return out


def model_item(S, cts, rgsws, base=None):
    return mod_down(S, inner_products(S, cts, rgsws), base)


def negacyclic_product(a, b, t):
    """a * b in Z_t[x] / (x^N + 1), coefficients as signed representatives or residues -> uint64 [N] below t"""
    N = len(a)
    assert t < 1 << 25 and N <= 1 << 13  # N t^2 fits 63 bits
    a = np.asarray(a).astype(np.int64) % t
    b = np.asarray(b).astype(np.int64) % t
    full = np.zeros(2 * N, dtype=np.int64)
    for i in np.flatnonzero(a):
        full[i:i + N] += a[i] * b
    return ((full[:N] - full[N:]) % t).astype(np.uint64)
