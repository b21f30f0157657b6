"""The helpers of tests/test_gpu_grid_limits.py on the host: the boundary set, the refusal of limb counts that divide 65535, the exact references
against the oracle.  No emulator case: ew_kernel at N = 2 past 65535 rows takes 33 s on the emulator build, too long for the CPU suite."""
import numpy as np
import pytest

import grid_cases as G
from grid_cases import BFV, CKKS, LIMIT

BITS4 = {BFV: [45, 40, 40, 40, 45], CKKS: [50, 40, 40, 40, 50]}


def test_grid_boundary_set_straddles_every_multiple():
    for r, batch in ((4, 16402), (8, 8201), (2, 65605), (3, 65605), (16, 4101)):
        items = G.boundary_items(batch, (r,))
        rows = batch * r
        assert {0, 1, batch - 1} <= set(items) and all(0 <= b < batch for b in items) and len(items) >= 8
        m = 1
        while m * LIMIT < rows:
            b = m * LIMIT // r  # the item that holds row m * 65535, the first row of the next stride
            assert b * r <= m * LIMIT < (b + 1) * r
            assert {b - 1, b, b + 1} & set(range(batch)) <= set(items), (r, batch, m)
            m += 1
        assert m > 1
    assert {65534, 65535, 65536} <= set(G.boundary_items(65605))
    assert {65532, 65533, 65534} <= set(G.boundary_items(65535))
    assert G.boundary_items(65605) == G.boundary_items(65605)  # a fixed seed
    assert G.batch_past(4) * 4 > LIMIT >= (G.batch_past(4, 1) - 1) * 4


def test_grid_limb_counts_that_divide_the_limit_are_refused():
    for bad in (1, 3, 5, 15, 17, 51, 255, 257):
        with pytest.raises(AssertionError):
            G.require_counts(bad)
    G.require_counts(2, 4, 8, 16, 6)


def test_grid_numpy_references_agree_with_the_oracle(oracle_lib):
    """the exact references of the element-wise cases against the oracle's own operations on a tiny batch at N = 16"""
    from oracle import ref as R
    from troy_amd import synth
    N, limbs, batch = G.N, 4, 3
    primes = oracle_lib.coeff_modulus_create(N, BITS4[CKKS])
    O = oracle_lib.Oracle(CKKS, N, primes, 0)
    q = primes[:limbs]
    xa, xb, xc = (synth.uniform_ct(11 + i, q, 2, N, batch) for i in range(3))
    xa[batch - 1] = G.extremes(q, (2, limbs, N), "alt")[0]
    xb[batch - 1] = G.extremes(q, (2, limbs, N), "alt")[1]
    pls = [synth.uniform_rows(21 + i, q, limbs, N) for i in range(3)]
    elt = O.elt_from_step(1)
    for b in range(batch):
        a, c = R.Ct(xa[b], True), R.Ct(xb[b], True)
        assert np.array_equal(G.ref_ew("add", xa[b], xb[b], q), O.eval(R.OP_ADD, a, c).data)
        assert np.array_equal(G.ref_ew("sub", xa[b], xb[b], q), O.eval(R.OP_SUB, a, c).data)
        assert np.array_equal(G.ref_ew("negate", xa[b], None, q), O.eval(R.OP_NEGATE, a).data)
        assert np.array_equal(G.ref_dyadic(xa[b], pls[0], q), O.eval(R.OP_MULTIPLY_PLAIN_NTT, a, pls[0]).data)
        # a scalar product is the dyadic product with a constant row
        sc = [pow(N, -1, p) * 12345 % p for p in q]
        const = np.array(sc, dtype=np.uint64)[:, None] * np.ones(N, dtype=np.uint64)
        assert np.array_equal(G.ref_scalar(xa[b], sc, q), O.eval(R.OP_MULTIPLY_PLAIN_NTT, a, const).data)
        acc = None
        for x, pl in zip((xa, xb, xc), pls):
            term = O.eval(R.OP_MULTIPLY_PLAIN_NTT, R.Ct(x[b], True), pl)
            acc = term if acc is None else O.eval(R.OP_ADD, acc, term)
        assert np.array_equal(G.ref_mul_plain_acc([xa[b], xb[b], xc[b]], pls, q), acc.data)
        for j in range(limbs):
            assert np.array_equal(G.ref_galois_ntt(xa[b, 0, j], elt, N), oracle_lib.apply_galois_ntt(N, elt, xa[b, 0, j]))


